"""Surface normals on the GPU (csrc/normals.hip, upnerf_viz_normals; upnerf_amd/normals.py).

upnerf_density_grad against the fp64 restatement of tests/normals_ref.py, per case (shape x band schedule, 257 seeded points):
err = max |g - g64| / max_i ||g64_i|| over the points whose ReLU margin in the reference is at least 1e-5.  The same figure is
measured for the route a user had before -- upnerf_field_fwd with everything stored, then upnerf_field_bwd with a unit seed on
d_sigma_s and need_dxyz, fp32 MFMA, called at the C ABI.  Gates: err <= 2 x the parent route's (same arithmetic class, another
summation order) and err <= 1e-4 (the project's parity gate); sigma is held to the same pair.  Both figures are printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import normals_ref as nr

pytestmark = pytest.mark.gpu

_CACHE = {}


def case(shape, band, head_bias=0.0, dense=False):
    """Module on the GPU, points, band weights and the fp64 reference of one case (computed once, shared, never written)."""
    key = (shape, band, head_bias, dense)
    if key not in _CACHE:
        W, D, skip = shape
        seed = nr.SEEDS[shape]
        sd, pts, wk = nr.make_field(W, D, skip, seed, head_bias, dense=dense), nr.make_points(seed), nr.band_weights(band)
        sigma, grad, margin, pre = nr.density(sd, pts, wk, D, skip)
        _CACHE[key] = dict(model=nr.build_module(W, D, skip, sd).cuda(), pts=pts.cuda(), wk=wk, sigma=sigma, grad=grad,
                           keep=margin >= nr.MARGIN_MIN, pre=pre)
    return _CACHE[key]


def fused(c, pts):
    from upnerf_amd import normals as nm
    s, g = nm.field_density_gradient(c["model"], pts, wk_xyz=c["wk"])
    return s, g


def parent_route(c, pts):
    """(sigma [M], dxyz [M, 3]) by upnerf_field_fwd (everything a training pass stores) + upnerf_field_bwd (unit seed, no heads)."""
    from upnerf_amd import _lib
    from upnerf_amd._lib import lib, ptr
    model = c["model"]
    pk, L = model.packer, model.packer.L
    W, D, M = pk.W, pk.D, pts.shape[0]
    dev = pts.device
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    P = model.packed().detach().contiguous()
    PF, PT = pk.frag_hip(P), pk.frag_t_hip(P)
    o, d, z = pts.contiguous(), torch.zeros(M, 3, device=dev), torch.zeros(M, 1, device=dev)  # o + 0 * 0 = the point itself
    sigma, x0, h = f(M), f(M, _lib.X0), f(D, M, W)
    hmask = torch.empty((D + 1) * ((M + 127) // 128) * 512, device=dev, dtype=torch.int64)
    fa = _lib.FieldFwdArgs(R=M, S=1, use_cand=0, use_rgb=0, rays_o=ptr(o), rays_d=ptr(d), z=ptr(z), wk_xyz=(C.c_float * 10)(*c["wk"]),
                           P=ptr(PF), sigma_s=ptr(sigma), x0=ptr(x0), h=ptr(h), hmask=ptr(hmask))
    assert lib.upnerf_field_fwd(C.byref(L), C.byref(fa), None) == 0
    ones, gz_h, gz_e, dpre, dxyz = torch.ones(M, device=dev), f(D, M, W), f(M, W), f(M), f(M, 3)
    fb = _lib.FieldBwdArgs(R=M, S=1, use_cand=0, use_rgb=0, need_dxyz=1, PT=ptr(PT), P=ptr(PF), d_sigma_s=ptr(ones),
                           sigma_s=ptr(sigma), x0=ptr(x0), h=ptr(h), hmask=ptr(hmask), gz_h=ptr(gz_h), gz_e=ptr(gz_e),
                           dpre_sig_s=ptr(dpre), dxyz=ptr(dxyz))
    assert lib.upnerf_field_bwd(C.byref(L), C.byref(fb), None) == 0
    return sigma, dxyz


def check_against_fp64(c, what, max_left_out=0.02):
    keep = c["keep"]
    assert (~keep).sum() <= max_left_out * len(keep)
    assert keep[0]  # the one-point case (M = 1, the point with a coordinate exactly 0) is measured, not skipped
    ps, pg = parent_route(c, c["pts"])
    ps, pg = ps.cpu().numpy(), pg.cpu().numpy()
    e_ps, e_pg = nr.rel_err(ps[keep], c["sigma"][keep]), nr.rel_err(pg[keep], c["grad"][keep])
    for M in nr.SIZES:
        k = keep[:M]
        s, g = fused(c, c["pts"][:M].contiguous())
        assert tuple(s.shape) == (M,) and tuple(g.shape) == (M, 3) and torch.isfinite(s).all() and torch.isfinite(g).all()
        # the error of the first M points on the scale of the whole case (one scale per case, whatever M)
        gs = np.sqrt((c["grad"][keep] ** 2).sum(1)).max()
        e_s = float(np.abs(s.cpu().numpy()[k] - c["sigma"][:M][k]).max() / np.abs(c["sigma"][keep]).max())
        e_g = float(np.abs(g.cpu().numpy()[k] - c["grad"][:M][k]).max() / gs)
        print(f"{what} M={M}: grad err {e_g:.3e} (parent route {e_pg:.3e}), sigma err {e_s:.3e} (parent route {e_ps:.3e}), "
              f"{int((~keep).sum())} points left out")
        assert e_g <= 2 * e_pg and e_g <= 1e-4, (M, e_g, e_pg)
        assert e_s <= 2 * e_ps and e_s <= 1e-4, (M, e_s, e_ps)


@pytest.mark.parametrize("band", nr.BANDS)
@pytest.mark.parametrize("shape", nr.SHAPES, ids=str)
def test_density_grad_matches_fp64(shape, band):
    check_against_fp64(case(shape, band), f"{shape} {band}")


def test_density_grad_on_the_linear_branch_of_the_softplus():
    shape, bias = nr.HEAD_BIAS_CASE
    c = case(shape, "ones", bias)
    assert c["pre"].min() > 20
    check_against_fp64(c, f"{shape} head bias {bias}")
    s, _ = fused(c, c["pts"])
    assert np.abs(s.cpu().numpy() - c["pre"]).max() <= 1e-4 * np.abs(c["pre"]).max()  # sigma = pre there


@pytest.mark.parametrize("band", nr.BANDS)
def test_dense_256x8_field_against_the_parent_route_and_fp64(band):
    """The 256 x 256 contractions with every weight and every mask position carrying data: a plain random (256, 8, 4) field.
    * sigma equals the parent route's bit for bit: the forward is the same arithmetic in the same order, so the ReLU decisions
      of the two routes agree at every point.
    * The gradients then differ only in softplus'(pre): sigmoid(pre) here, 1 - exp(-sigma) there, each within 2 eps of a value
      <= 1, an absolute difference of <= 4 eps = 2.4e-7.  The walk back is linear in it, so a point's gradient changes by that
      over its sigmoid, relatively: with the sigmoid >= 0.1 at every point of this field (asserted below) by <= 2.4e-6 of
      max ||g||, plus the roundings of a chain that now starts from another value.  Gate: 1e-5 of max ||g||, all 257 points.
    * fp64: the gates of the other cases (<= 2 x the parent route's error, <= 1e-4) on the points above the 1e-5 margin; a dense
      field of 2048 units leaves out 12 - 14 % of its points (32 - 35 of 257 at the committed seed; at most 15 % asserted)."""
    shape = (256, 8, 4)
    c = case(shape, band, dense=True)
    pts = c["pts"]
    ps, pg = parent_route(c, pts)
    s, g = fused(c, pts)
    assert torch.equal(s.view(torch.int32), ps.view(torch.int32))
    gmax = float(pg.norm(dim=1).max())
    assert (1.0 / (1.0 + np.exp(-c["pre"]))).min() >= 0.1
    d = float((g - pg).abs().max()) / gmax
    print(f"dense {shape} {band}: |fused - parent| / max||g|| = {d:.3e}; {int((~c['keep']).sum())} of {len(c['keep'])} points below "
          f"the margin")
    assert d <= 1e-5
    check_against_fp64(c, f"dense {shape} {band}", max_left_out=0.15)


@pytest.mark.parametrize("shape,dense", [((64, 8, 4), False), ((256, 8, 4), True)], ids=str)
def test_outputs_of_a_point_do_not_depend_on_the_batch(shape, dense):
    c = case(shape, "partial", dense=dense)
    pts = c["pts"]
    s, g = fused(c, pts)
    bits = lambda t: t.contiguous().view(torch.int32)
    for chunk in (1, 63, 100):  # another chunking: other tiles, other rows of the tile
        ss, gg = zip(*[fused(c, pts[i:i + chunk].contiguous()) for i in range(0, pts.shape[0], chunk)][:4])
        n = min(4 * chunk, pts.shape[0])
        assert torch.equal(bits(torch.cat(ss)), bits(s[:n])) and torch.equal(bits(torch.cat(gg)), bits(g[:n])), chunk
    perm = torch.randperm(pts.shape[0], generator=torch.Generator().manual_seed(3)).cuda()
    s2, g2 = fused(c, pts[perm].contiguous())
    assert torch.equal(bits(s2), bits(s[perm])) and torch.equal(bits(g2), bits(g[perm]))
    s3, g3 = fused(c, pts.flip(0).contiguous())
    assert torch.equal(bits(s3), bits(s.flip(0))) and torch.equal(bits(g3), bits(g.flip(0)))


def test_reuse_fragments_packs_once_and_never_outlives_its_block():
    from upnerf_amd import normals as nm
    c = case((64, 2, None), "ones")
    model, pts = c["model"], c["pts"][:65].contiguous()
    plain = fused(c, pts)
    with nm.reuse_fragments():
        a, b = fused(c, pts), fused(c, pts)
        assert len(nm._REUSE) == 1
    assert nm._REUSE is None
    for got in (a, b):
        assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
    w = model.share_sigma[0].weight
    old = w.detach().clone()
    try:
        w.data.mul_(2.0)  # (through .data: no version counter moves, as when the optimiser kernel writes)
        assert not torch.equal(fused(c, pts)[1], plain[1])  # outside a block every call packs the parameters as they are
    finally:
        w.data.copy_(old)
    assert torch.equal(fused(c, pts)[1], plain[1])


@pytest.mark.parametrize("S", [1, 32, 64, 192])
@pytest.mark.parametrize("R", [1, 3, 65])
def test_normal_composite_matches_numpy(R, S):
    from upnerf_amd.normals import normal_composite
    rng = np.random.default_rng(100 * R + S)
    g = rng.standard_normal((R, S, 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, (R, S, 1)).astype(np.float32)
    w = rng.random((R, S)).astype(np.float32) ** 4
    w[0] = 0                                   # all-zero weights
    if R > 1:
        g[1, ::2] = 0                          # zero gradients among the samples
        g[1, 0] = [np.nan, 1, 2]
        if S > 1:
            g[1, 1] = [np.inf, 0, 0]
    if R > 2:
        g[2], w[2] = [0, 0, 3], 0.25           # every sample points the same way: exactly unit length
    ref, tol = nr.composite_ref(g.reshape(-1, 3), w)
    got = normal_composite(torch.from_numpy(g).cuda().reshape(-1, 3), torch.from_numpy(w).cuda())
    assert tuple(got.shape) == (R, 3) and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any()
    assert np.array_equal(got[0], [0, 0, 0])
    if R > 2:
        assert np.array_equal(got[2], [0, 0, -1])
    assert (np.abs(got - ref).max(1) <= tol).all(), float((np.abs(got - ref).max(1) - tol).max())
    length = np.sqrt((got ** 2).sum(1))
    assert ((np.abs(length - 1) < 1e-6) | (length == 0)).all()
    again = normal_composite(torch.from_numpy(g).cuda(), torch.from_numpy(w).cuda())  # [R, S, 3] is accepted; same bits
    assert np.array_equal(again.cpu().numpy(), got.astype(np.float32))


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("rot", [False, True])
def test_viz_normals_matches_numpy_bit_for_bit(n, rot):
    from upnerf_amd.visualization import normal_image
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    x /= np.sqrt((x * x).sum(1, keepdims=True)).astype(np.float32)
    x[::7] = 0
    if n > 3:
        x[1], x[2], x[3] = [1, 0, 0], [np.nan, 0, 1], [0, -1, 2.5]
    r = None
    if rot:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        r = q.astype(np.float32)
    got = normal_image(torch.from_numpy(x).cuda(), (n, 1), rot=None if r is None else torch.from_numpy(r).cuda())
    assert tuple(got.shape) == (1, n, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy().reshape(n, 3), nr.viz_ref(x, r))
    assert np.array_equal(got.cpu().numpy().reshape(n, 3)[0], [128, 128, 128])


# ---- end to end ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def system():
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset, default_hparams
    hp = default_hparams(**{"nerf.N_samples": 32, "nerf.N_importance": 32, "max_steps": 1000})
    torch.manual_seed(11)
    s = NeRFSystem(hp, SyntheticDataset(6))
    s.setup()
    s.cuda()
    s.set_progress(0.8)  # sched_mult 1: the static colour exists
    return s


def render(system, rays, **kw):
    from upnerf_amd.rendering import render_rays
    hp = system.hparams
    with torch.no_grad():
        return render_rays(system.models, system.embeddings, rays, torch.zeros(rays.shape[0], dtype=torch.long, device="cuda"),
                           system.get_schedule_mult(system._host_progress), N_samples=hp["nerf.N_samples"],
                           N_importance=hp["nerf.N_importance"], use_disp=hp["nerf.use_disp"], perturb=0, encode_feat=True, **kw)


def some_rays(R=37):
    g = torch.Generator().manual_seed(4)
    o = (torch.rand(R, 3, generator=g) - 0.5) * 0.4
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, -1.0]), dim=1)
    return torch.cat([o, d, torch.tensor([0.1, 4.0]).expand(R, 2)], 1).cuda().contiguous()


def test_render_rays_with_normals_adds_one_key_and_changes_nothing_else(system):
    from upnerf_amd import normals as nm
    rays = some_rays()
    keep = {}
    plain, with_n = render(system, rays), render(system, rays, normals=True, keep=keep)
    assert set(with_n) == set(plain) | {"normal_fine"}
    for k in plain:
        assert torch.equal(plain[k], with_n[k]), k
    n = with_n["normal_fine"]
    pts = nm.sample_points(rays[:, :3], rays[:, 3:6], keep["z_fine"])
    _, grad = nm.density_gradient(system, pts, field="fine")
    assert torch.equal(n, nm.normal_composite(grad, with_n["s_weights_fine"]))
    length = n.norm(dim=1)
    assert tuple(n.shape) == (37, 3) and bool((((length - 1).abs() < 1e-5) | (length == 0)).all()) and float(length.max()) > 0
    # without a fine pass the coarse one carries the normal
    hp = system.hparams
    from upnerf_amd.rendering import render_rays
    with torch.no_grad():
        c = render_rays(system.models, system.embeddings, rays, torch.zeros(37, dtype=torch.long, device="cuda"), 1,
                        N_samples=hp["nerf.N_samples"], N_importance=0, perturb=0, encode_feat=True, normals=True)
    assert "normal_coarse" in c and "normal_fine" not in c


def test_render_path_normals_with_and_without_a_full_grid(system):
    from upnerf_amd import novel_view as nv
    from upnerf_amd.occupancy import OccupancyGrid
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2]],
                        [[np.cos(0.3), 0, np.sin(0.3), -0.2], [0, 1, 0, 0.1], [-np.sin(0.3), 0, np.cos(0.3), 0.0]]])
    path = nv.CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], 2, appearance=(1, 4), img_wh=(8, 8),
                                    K=torch.tensor([[7.5, 0, 3.6], [0, 7.0, 3.8], [0, 0, 1]]))
    a = nv.render_path(system, path, chunk=48, outputs=("rgb", "normal", "normal_float"))
    assert tuple(a["normal"].shape) == (2, 8, 8, 3) and a["normal"].dtype == torch.uint8
    assert tuple(a["normal_float"].shape) == (2, 64, 3)
    full = OccupancyGrid.from_cells(torch.ones(4, 4, 4, dtype=torch.bool).cuda(), ((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0)))
    b = nv.render_path(system, path, chunk=48, outputs=("rgb", "normal", "normal_float"), occupancy=full)
    assert nv.LAST_STATS == {"rays": 128, "hits": 128}
    assert torch.equal(a["normal_float"], b["normal_float"]) and torch.equal(a["normal"], b["normal"]) and torch.equal(a["rgb"], b["rgb"])
    empty = OccupancyGrid.from_cells(torch.zeros(4, 4, 4, dtype=torch.bool).cuda(), ((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0)))
    e = nv.render_path(system, path, chunk=48, outputs=("normal", "normal_float"), occupancy=empty)
    assert float(e["normal_float"].abs().max()) == 0 and bool((e["normal"] == 128).all())  # skipped rays: the zero normal, grey
    imgs = []
    nv.render_path(system, path, chunk=64, outputs=("normal",), sink=lambda tag, f, images: imgs.append(sorted(images)))
    assert imgs == [["normal"], ["normal"]]


def test_refine_normals_on_a_field_that_is_monotone_along_an_axis():
    """A one-layer field whose units all read x_1 (the identity block of the encoding, bands off) with positive weights, and a
    positive density head: sigma rises with y everywhere, so every normal is -y, within the gradient's gate (1e-4)."""
    from upnerf_amd import geometry
    W, D, skip = 64, 1, None
    sd = nr.make_field(W, D, skip, 3)
    w = torch.zeros(W, 63)
    w[:, 1] = sd["xyz_encoding_1.0.weight"][:, 1].abs() + 0.1
    sd["xyz_encoding_1.0.weight"] = w
    sd["xyz_encoding_1.0.bias"] = sd["xyz_encoding_1.0.bias"].abs() + 0.5  # (above max w: every unit is on over [-1, 1])
    sd["share_sigma.0.weight"] = sd["share_sigma.0.weight"].abs() + 0.01
    model = nr.build_module(W, D, skip, sd).cuda()
    model.set_progress(0.0)  # before the coarse-to-fine window: every band weight is zero
    system = type("S", (), {"models": {"nerf_fine": model}})()
    g = torch.Generator().manual_seed(2)
    v = (torch.rand(70, 3, generator=g) * 2 - 1).cuda()
    grid_n = torch.nn.functional.normalize(torch.randn(70, 3, generator=g), dim=1).cuda()
    mesh = geometry.Mesh(v, grid_n, torch.zeros(0, 3, dtype=torch.int32).cuda())
    out = geometry.refine_normals(system, mesh)
    assert out.vertices is mesh.vertices and out.faces is mesh.faces
    want = torch.tensor([0.0, -1.0, 0.0]).cuda().expand(70, 3)
    assert float((out.normals - want).abs().max()) <= 1e-4
    # where the field is flat (every unit off: a large negative bias) the grid normal is kept
    sd["xyz_encoding_1.0.bias"] = torch.full((W,), -100.0)
    system.models["nerf_fine"] = nr.build_module(W, D, skip, sd).cuda()
    system.models["nerf_fine"].set_progress(0.0)
    assert torch.equal(geometry.refine_normals(system, mesh).normals, grid_n)
