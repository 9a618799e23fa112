"""Depth-map fusion on the GPU (csrc/tsdf.hip, geometry.TsdfVolume / fuse_views) against the fp64 restatement in tests/tsdf_ref.py,
and the mesher's observed-only option (UPNERF_MTET_SKIP_NONFINITE) against a restatement of its rule written out below.

Inputs (tsdf_ref.scene): a 24 x 20 x 17 grid over [-1, 1]^3 -- 8160 voxels, no multiple of the 256-thread block, three different
axes --, trunc 0.25, three 40 x 30 cameras at distance 2.5 round a sphere of radius 0.8 whose depth maps are exact in fp64 and
rounded to fp32 (NaN off the sphere).  Every way out of the rule is taken by some voxels (asserted).

Gates.  A voxel is compared unless fp32 and fp64 may legitimately DECIDE differently for it: in some view its u + 0.5 or v + 0.5
lies within 1e-4 px of an integer (the fp32 projection spends about ten roundings on |u| <= 40: 2.4e-5 px), or its sdf lies
within 1e-5 of -trunc.  At most 1 % of the voxels may be left out (the reference leaves out 12 of 8160).  On all others:
  weight  equal, bit for bit: both sides add the same fp32 view weights in the same order.
  tsdf    r = |p - c| costs at most 6 roundings (three differences, three squares and two sums, the root; the first three act
          on values <= 3.5) on a result <= 4.3: 6 x 2^-24 x 4.3 = 1.5e-6, and the same bounds sdf = d - r (d is an input).
          Divided by trunc = 0.25: 6e-6.  Each fold T += (val - T)(w / Wn) adds four roundings on values <= 2, 5e-7, and
          averages what the earlier folds left rather than amplifying it: 1.5e-6 over three views.  8e-6 in all; the gate is
          2e-5 absolute.
  colour  inputs in [0, 1]; a fold is a difference, a quotient, a product and a sum, four roundings of <= 6e-8 on values <= 1,
          three folds: 7e-7 < 1e-6 absolute, the gate.
Mesh positions: the gate test_hip_mesh.py derives, 1e-6 of (the largest coordinate + the longest cell edge)."""
import itertools

import numpy as np
import pytest
import torch

import tsdf_ref as tr

pytestmark = pytest.mark.gpu

INTR = (tr.FX, tr.FY, tr.CX, tr.CY)
N = tr.RES[0] * tr.RES[1] * tr.RES[2]
RGB0 = 0.25  # what the colour volume holds before anything is fused (the module's own start is 0: any value must survive)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(views, colour=True, calls=None, rgb0=None, **kw):
    """A TsdfVolume of the shared grid with `views` (tsdf_ref dicts) folded in: all in one integrate() call, or cut into calls
    of the given lengths."""
    from upnerf_amd.geometry import TsdfVolume
    vol = TsdfVolume(tr.BOUNDS, tr.RES, tr.TRUNC, colour=colour)
    if rgb0 is not None:
        vol.rgb.fill_(rgb0)
    i = 0
    for n in calls or [len(views)]:
        part = views[i:i + n]
        vol.integrate([dev(v["depth"]) for v in part], np.stack([v["c2w"] for v in part]), INTR, tr.IMG_WH,
                      rgb=[dev(v["rgb"]) for v in part], opacity=[dev(v["opacity"]) for v in part], **kw)
        i += n
    assert i == len(views) and vol.n_views == i
    return vol


_REF = {}


def reference(kind):
    """(state, report, compared [N] bool) of the fp64 restatement, computed once per kind and never changed."""
    if kind not in _REF:
        views, P = tr.scene()
        st = tr.new_state(N, rgb0=RGB0)
        if kind == "count":
            rep = tr.integrate_points(P, st, [tr.without(v, "opacity") for v in views], tr.TRUNC)
        elif kind == "opacity":
            rep = tr.integrate_points(P, st, views, tr.TRUNC, min_opacity=0.5, weight_mode="opacity")
        left_out = np.zeros(N, bool)
        for r in rep:
            left_out |= r["near_pixel_edge"] | r["near_band_edge"]
            assert not (np.abs(r["sdf"] - tr.TRUNC) < 1e-5).any()  # (no colour decision of these inputs is in doubt either)
        assert left_out.mean() <= 0.01, left_out.mean()
        _REF[kind] = (st, rep, ~left_out)
    return _REF[kind]


def compare(vol, kind, tag):
    st, _, keep = reference(kind)
    flat = lambda t: t.reshape(N, -1).squeeze(-1).cpu().numpy()
    w, T, c, cw = flat(vol.weight), flat(vol.tsdf), flat(vol.rgb), flat(vol.rgb_weight)
    err_t = np.abs(T.astype(np.float64) - st["tsdf"])[keep].max()
    err_c = np.abs(c.astype(np.float64) - st["rgb"])[keep].max()
    print(f"{tag}: {int((~keep).sum())} of {N} voxels left out; max |tsdf| error {err_t:.2e} (gate 2e-5), colour {err_c:.2e} (gate 1e-6); "
          f"weights differ on {int((w != st['weight'])[keep].sum())}, colour weights on {int((cw != st['rgb_weight'])[keep].sum())}")
    assert torch.equal(torch.from_numpy(w[keep]), torch.from_numpy(st["weight"][keep]))
    assert torch.equal(torch.from_numpy(cw[keep]), torch.from_numpy(st["rgb_weight"][keep]))
    assert err_t <= 2e-5 and err_c <= 1e-6, (err_t, err_c)
    never = keep & (st["weight"] == 0)
    assert never.any() and (w[never] == 0).all() and (T[never] == 1.0).all()  # never observed: the initial volume
    assert (cw[never] == 0).all() and (c[never] == np.float32(RGB0)).all()


def test_the_inputs_take_every_way_out_of_the_rule():
    _, rep, keep = reference("count")
    seen = np.zeros(N, bool)
    for r in rep:
        b = r["branch"]
        share = lambda code: float((b == code).mean())
        assert 0.005 < share(tr.OUTSIDE) < 0.05 and 0.3 < share(tr.NO_DEPTH) < 0.6 and 0.3 < share(tr.BEHIND_BAND) < 0.6
        assert 0.05 < share(tr.UPDATED) < 0.2 and share(tr.BEHIND) == 0
        upd = b == tr.UPDATED
        assert (upd & (r["sdf"] > tr.TRUNC)).sum() > 50 and (upd & (np.abs(r["sdf"]) < tr.TRUNC)).sum() > 50  # clamped and in the band
        assert (upd & ~r["coloured"]).sum() > 50 and r["coloured"].sum() > 50
        seen |= upd
    assert 0.15 < seen.mean() < 0.35 and keep.mean() >= 0.99
    _, rep_o, _ = reference("opacity")
    assert all((r["branch"] == tr.LOW_OPACITY).sum() > 50 for r in rep_o)


def test_volume_matches_the_fp64_restatement():
    views, _ = tr.scene()
    compare(fuse([tr.without(v, "opacity") for v in views], rgb0=RGB0), "count", "three views, one launch")


def same_volume(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("tsdf", "weight", "rgb", "rgb_weight"))


def test_the_bits_do_not_depend_on_the_split_into_launches():
    views, _ = tr.scene()
    one = fuse(views, min_opacity=0.5, weight_mode="opacity")
    assert same_volume(one, fuse(views, calls=[1, 1, 1], min_opacity=0.5, weight_mode="opacity"))
    assert same_volume(one, fuse(views, calls=[2, 1], min_opacity=0.5, weight_mode="opacity"))
    assert not same_volume(one, fuse(views[::-1], min_opacity=0.5, weight_mode="opacity"))  # (the order of the views does matter)


def test_more_views_than_a_launch_holds():
    """Nine views in one call are cut into launches of TSDF_MAX_VIEWS = 8 and 1: the same bits as three calls of three."""
    from upnerf_amd import _lib
    views = [tr.without(v, "opacity") for v in tr.scene()[0]] * 3
    assert len(views) == _lib.TSDF_MAX_VIEWS + 1
    a, b = fuse(views), fuse(views, calls=[3, 3, 3])
    assert same_volume(a, b) and float(a.weight.max()) == 9.0


def test_opacity_as_the_weight():
    compare(fuse(tr.scene()[0], rgb0=RGB0, min_opacity=0.5, weight_mode="opacity"), "opacity", "opacity weights")
    with pytest.raises(RuntimeError):  # the weights of a view without its map: refused by the library
        fuse([tr.without(v, "opacity") for v in tr.scene()[0]], weight_mode="opacity")


def test_min_opacity_drops_exactly_the_pixels_below_it():
    views, _ = tr.scene()
    masked = []
    for v in views:
        low = v["opacity"] < np.float32(0.5)
        assert 0.1 < low.mean() < 0.5
        masked.append(dict(tr.without(v, "opacity"), depth=np.where(low, np.float32(np.nan), v["depth"])))
    got = fuse(views, min_opacity=0.5)
    assert same_volume(got, fuse(masked))                    # as if those pixels had no depth, and nothing else
    assert not same_volume(got, fuse(views, min_opacity=0.0))
    assert same_volume(fuse(views, min_opacity=0.0), fuse([tr.without(v, "opacity") for v in views]))


def test_colour_is_untouched_beyond_the_truncation():
    views, _ = tr.scene()
    _, rep, keep = reference("count")
    vol = fuse([tr.without(v, "opacity") for v in views], rgb0=RGB0)
    updated = np.zeros(N, bool)
    coloured = np.zeros(N, bool)
    for r in rep:
        updated |= r["branch"] == tr.UPDATED
        coloured |= r["coloured"]
    far = torch.from_numpy(keep & updated & ~coloured).cuda()  # seen, in every view that saw it from more than trunc in front
    assert int(far.sum()) > 100
    assert bool((vol.weight.reshape(-1)[far] > 0).all()) and bool((vol.tsdf.reshape(-1)[far] == 1.0).all())
    assert bool((vol.rgb_weight.reshape(-1)[far] == 0).all()) and bool((vol.rgb.reshape(-1, 3)[far] == RGB0).all())
    plain = fuse([tr.without(v, "opacity", "rgb") for v in views], colour=False)  # and a volume without colour is the same distance
    assert plain.rgb is None and torch.equal(plain.tsdf, vol.tsdf) and torch.equal(plain.weight, vol.weight)


def test_colour_samples_leave_out_corners_without_weight():
    from upnerf_amd.geometry import TsdfVolume
    vol = TsdfVolume(((0, 0, 0), (1, 2, 4)), (2, 2, 2), 0.5)
    corner = torch.arange(8, dtype=torch.float32).cuda().reshape(2, 2, 2)  # [z][y][x]: corner c = x + 2 y + 4 z has colour c / 16
    vol.rgb.copy_((corner / 16)[..., None].expand(2, 2, 2, 3))
    vol.rgb_weight.fill_(1.0)
    vol.rgb_weight[1, 1, 1] = 0  # corner 7
    pts = torch.tensor([[0.5, 1.0, 2.0], [0.25, 0.5, 3.0], [1.0, 2.0, 4.0], [0.0, 0.0, 0.0], [-3.0, 0.0, 9.0], [float("nan"), 0, 0]]).cuda()
    got = vol.sample_colour(pts).cpu().double()
    fx, fy, fz = 0.25, 0.25, 0.75
    wts = np.array([(fx if c & 1 else 1 - fx) * (fy if c & 2 else 1 - fy) * (fz if c & 4 else 1 - fz) for c in range(8)])
    want = [np.arange(7).sum() / 16 / 7,                      # the centre: the mean of the seven corners that count
            (wts[:7] * np.arange(7) / 16).sum() / wts[:7].sum(),
            0.5,                                              # ON corner 7: nothing with weight there, mid-grey
            0.0, 4 / 16,                                      # corner 0; outside the box: clamped, onto corner 4
            0.5]                                              # a NaN
    assert torch.allclose(got, torch.tensor(want).double()[:, None].expand(6, 3), atol=1e-6, rtol=0), (got[:, 0], want)
    vol.rgb_weight.zero_()
    assert bool((vol.sample_colour(pts) == 0.5).all())


# ---- the mesher's observed-only option: its rule restated, with tables derived here ---------------------------------------------

SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]  # edge slot of a grid point -> the far end
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]                               # tet edge -> its two tet vertices


def kuhn_split():
    """Six tetrahedra from corner 0 to corner 7, one per order of the axes; odd orders swap two vertices (positive orientation)."""
    tets = []
    for p in itertools.permutations((0, 1, 2)):
        a, b = 1 << p[0], (1 << p[0]) | (1 << p[1])
        odd = sum(p[i] > p[j] for i in range(3) for j in range(i + 1, 3)) % 2
        tets.append((0, b, a, 7) if odd else (0, a, b, 7))
    return tets


def triangles_of(case):
    """Triangles (as tet edges) of a case = sum of (vertex i inside) << i, normal from the inside to the outside vertices."""
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    eid = lambda a, b: PAIRS.index((min(a, b), max(a, b)))
    mid = lambda e: (X[PAIRS[e][0]] + X[PAIRS[e][1]]) / 2
    ins = [i for i in range(4) if (case >> i) & 1]
    out = [i for i in range(4) if not (case >> i) & 1]
    if len(ins) in (1, 3):
        a = (ins if len(ins) == 1 else out)[0]
        tris = [tuple(sorted(eid(a, b) for b in range(4) if b != a))]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        q = [eid(a, c), eid(a, d), eid(b, d), eid(b, c)]
        tris = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    else:
        return []
    flip = lambda t: np.cross(mid(t[1]) - mid(t[0]), mid(t[2]) - mid(t[0])) @ (X[out].mean(0) - X[ins].mean(0)) <= 0
    return [(t[0], t[2], t[1]) if flip(t) else t for t in tris]


def mesh_rule(G, bounds, level, observed_only):
    """(vertices [V, 3] fp64, faces [F, 3]): a grid point is inside when finite and >= level.  Vertices are the crossed edges in
    (point, slot) order -- with observed_only an edge is crossed only between two finite samples --, faces come in (cell,
    tetrahedron, triangle) order -- with observed_only only from tetrahedra whose four corners are finite."""
    G = np.asarray(G, np.float32)
    Nz, Ny, Nx = G.shape
    fin = np.isfinite(G)
    with np.errstate(invalid="ignore"):
        ins = fin & (G >= np.float32(level))
    axes = [tr.axis_coords(bounds[0][k], bounds[1][k], n) for k, n in enumerate((Nx, Ny, Nz))]
    vid, verts = {}, []
    for z, y, x in itertools.product(range(Nz), range(Ny), range(Nx)):
        for s, (dx, dy, dz) in enumerate(SLOTS):
            x1, y1, z1 = x + dx, y + dy, z + dz
            if x1 >= Nx or y1 >= Ny or z1 >= Nz or ins[z, y, x] == ins[z1, y1, x1]:
                continue
            both = fin[z, y, x] and fin[z1, y1, x1]
            if observed_only and not both:
                continue
            v0, v1 = float(G[z, y, x]), float(G[z1, y1, x1])
            t = (float(np.float32(level)) - v0) / (v1 - v0) if both else 0.5
            p0 = np.array([axes[0][x], axes[1][y], axes[2][z]])
            p1 = np.array([axes[0][x1], axes[1][y1], axes[2][z1]])
            vid[(x, y, z, s)] = len(verts)
            verts.append(p0 + t * (p1 - p0))
    faces = []
    tets = kuhn_split()
    for z, y, x in itertools.product(range(Nz - 1), range(Ny - 1), range(Nx - 1)):
        at = lambda c: (z + (c >> 2), y + ((c >> 1) & 1), x + (c & 1))
        for tet in tets:
            if observed_only and not all(fin[at(c)] for c in tet):
                continue
            case = sum(int(ins[at(c)]) << i for i, c in enumerate(tet))
            for tri in triangles_of(case):
                f = []
                for e in tri:
                    ca, cb = tet[PAIRS[e][0]], tet[PAIRS[e][1]]
                    lo_c, d = ca & cb, ca ^ cb
                    s = SLOTS.index((d & 1, (d >> 1) & 1, d >> 2))
                    oz, oy, ox = at(lo_c)
                    f.append(vid[(ox, oy, oz, s)])  # (a KeyError here: a triangle on an edge that emitted no vertex)
                faces.append(f)
    return np.array(verts).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)


HAND_RES, HAND_BOUNDS, HAND_LEVEL = (5, 4, 3), ((-1.0, 0.0, 0.5), (1.0, 0.9, 1.3)), -0.05


def hand_grid():
    """5 x 4 x 3 samples of a tilted plane that crosses the level between x = 2 and x = 4 (slanted: at x = 3 the samples with
    0.07 y + 0.05 z >= 0.25 are inside), with ONE sample nobody observed, next to the crossing: (2, 2, 1) would be 0.29, inside,
    and its +x neighbour is -0.11, outside."""
    z, y, x = np.meshgrid(np.arange(3), np.arange(4), np.arange(5), indexing="ij")
    G = (0.9 - 0.4 * x + 0.07 * y + 0.05 * z).astype(np.float32)
    G[1, 2, 2] = np.nan
    return G


def test_observed_only_meshes_equal_the_restated_rule():
    from upnerf_amd.geometry import extract_surface
    G = hand_grid()
    grid = torch.from_numpy(G).cuda()
    edge = np.sqrt(sum(((h - l) / (n - 1)) ** 2 for l, h, n in zip(HAND_BOUNDS[0], HAND_BOUNDS[1], HAND_RES)))
    gate = 1e-6 * (max(abs(v) for b in HAND_BOUNDS for v in b) + edge)
    sizes = {}
    for observed_only in (True, False):
        verts, faces = mesh_rule(G, HAND_BOUNDS, HAND_LEVEL, observed_only)
        mesh = extract_surface(grid, HAND_BOUNDS, HAND_LEVEL, observed_only=observed_only)
        V, F = len(verts), len(faces)
        sizes[observed_only] = (V, F)
        assert F > 0 and tuple(mesh.vertices.shape) == (V, 3) and tuple(mesh.normals.shape) == (V, 3)
        assert torch.equal(mesh.faces.cpu(), torch.from_numpy(faces.astype(np.int32)))
        assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V
        err = np.abs(mesh.vertices.cpu().numpy().astype(np.float64) - verts).max()
        print(f"observed_only={observed_only}: V {V} F {F}, max position error {err:.2e} (gate {gate:.2e})")
        assert err <= gate
        assert torch.isfinite(mesh.vertices).all() and torch.isfinite(mesh.normals).all()
    assert sizes[True][0] < sizes[False][0] and sizes[True][1] < sizes[False][1]  # the wall round the unobserved sample is gone
    clean = np.where(np.isnan(G), np.float32(0.9 - 0.8 + 0.14 + 0.05), G)
    assert sizes[True][1] < len(mesh_rule(clean, HAND_BOUNDS, HAND_LEVEL, True)[1])  # and so is the surface through its cells


def test_without_the_flag_the_mesh_is_the_one_of_a_call_that_passes_none():
    from upnerf_amd.geometry import extract_surface
    for G, bounds, level in ((hand_grid(), HAND_BOUNDS, HAND_LEVEL),):
        grid = torch.from_numpy(G).cuda()
        a = extract_surface(grid, bounds, level)
        b = extract_surface(grid, bounds, level, observed_only=False)
        assert a.faces.shape[0] > 0 and torch.equal(a.faces, b.faces)
        assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
        assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
    finite = torch.from_numpy(np.nan_to_num(hand_grid(), nan=0.19)).cuda()  # nothing unobserved: the flag changes nothing
    a, b = extract_surface(finite, HAND_BOUNDS, HAND_LEVEL), extract_surface(finite, HAND_BOUNDS, HAND_LEVEL, observed_only=True)
    assert torch.equal(a.faces, b.faces) and torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))


# ---- end to end -----------------------------------------------------------------------------------------------------------

COLOUR = (0.2, 0.6, 0.9)


def test_fused_views_mesh_the_sphere_they_saw():
    from upnerf_amd.geometry import extract_surface
    views = [dict(tr.without(v, "opacity"), rgb=np.tile(np.float32(COLOUR), (len(v["depth"]), 1))) for v in tr.scene()[0]]
    vol = fuse(views)
    mesh = vol.extract()
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    cell = float(np.sqrt(sum(((h - l) / (n - 1)) ** 2 for l, h, n in zip(tr.BOUNDS[0], tr.BOUNDS[1], tr.RES))))
    off = (mesh.vertices.double().norm(dim=1) - tr.RADIUS).abs()
    print(f"end to end: V {V} F {F}; | |v| - {tr.RADIUS} | max {float(off.max()):.4f}, mean {float(off.mean()):.4f} (bound {tr.TRUNC + cell:.4f})")
    assert V > 0 and F > 0 and int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V
    assert float(off.max()) <= tr.TRUNC + cell  # a zero crossing exists only inside an observed band
    grid = vol.surface_grid()
    assert bool(torch.isnan(grid).any()) and torch.equal(torch.isnan(grid), vol.weight < 1.0)
    assert torch.equal(grid[vol.weight >= 1.0], -vol.tsdf[vol.weight >= 1.0])
    walls = extract_surface(grid, tr.BOUNDS, 0.0, observed_only=False)
    assert walls.faces.shape[0] > F  # where the band meets what nobody saw
    assert tuple(mesh.colours.shape) == (V, 3)
    assert float((mesh.colours - torch.tensor(COLOUR).cuda()).abs().max()) <= 1e-6
    outward = (mesh.normals * torch.nn.functional.normalize(mesh.vertices, dim=1)).sum(1)  # towards the cameras: away from the centre
    has_normal = mesh.normals.norm(dim=1) > 0
    assert bool(has_normal.any()) and float(outward[has_normal].median()) > 0  # (the sign convention, not every noisy border vertex)
    two = vol.extract(min_weight=2.0)  # fewer voxels qualify when two views must agree
    assert 0 < two.faces.shape[0] < F


def make_system():
    from upnerf_amd import synth
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset, default_hparams
    hp = default_hparams(**{"nerf.N_samples": 32, "nerf.N_importance": 32, "max_steps": 1000})
    torch.manual_seed(11)
    s = NeRFSystem(hp, SyntheticDataset(6))
    s.setup()
    sd = {}
    for typ in ("coarse", "fine"):  # "trained-like" fields (synth.nerf_state): densities up to ~10 round the origin, so rays end
        st = synth.nerf_state(typ, D=8, W=256, seed=3, sigma_bias=-2.0, sigma_gain=30.0, trunk_gain=2.5)
        sd.update({f"nerf_{typ}.{k}": v for k, v in st.items()})
    missing, unexpected = s.load_state_dict(sd, strict=False)
    assert not unexpected and all(not k.startswith("nerf_") for k in missing)
    with torch.no_grad():
        for emb in s.embeddings.values():
            emb.weight.copy_(torch.randn(emb.weight.shape))
        s.se3_refine.weight.copy_(0.02 * torch.randn(s.se3_refine.weight.shape))
    ds = s.train_dataset
    ang = torch.linspace(-0.5, 0.5, 6)
    ds.poses = torch.zeros(6, 3, 4)
    ds.poses[:, 0, 0] = ds.poses[:, 2, 2] = torch.cos(ang)
    ds.poses[:, 0, 2], ds.poses[:, 2, 0], ds.poses[:, 1, 1] = torch.sin(ang), -torch.sin(ang), 1.0
    ds.poses[:, :, 3] = 1.5 * ds.poses[:, :, 2]  # on a circle round the origin, looking at it
    ds.nears, ds.fars = [0.1 + 0.01 * i for i in range(6)], [3.0 - 0.1 * i for i in range(6)]
    ds.Ks = [np.array([[14.0 + i, 0, 7.5], [0, 13.5 + i, 5.5], [0, 0, 1]]) for i in range(6)]
    ds.all_imgs_wh = torch.tensor([[16, 12]] * 6)
    s.cuda()
    s.set_progress(0.8)
    return s


def test_fuse_views_is_render_rays_and_integrate_on_the_training_views():
    from upnerf_amd.geometry import TsdfVolume, fuse_views
    from upnerf_amd.novel_view import path_rays
    from upnerf_amd.pose_align import refined_poses
    from upnerf_amd.rendering import render_rays
    s = make_system()
    assert s.get_schedule_mult(s._host_progress) == 1
    ds, hp = s.train_dataset, s.hparams
    bounds, res, ids = ((-1.0, -0.8, -1.0), (1.0, 0.8, 1.0)), (16, 16, 16), [4, 1]
    vol = fuse_views(s, bounds, res, img_ids=ids, chunk=100)
    cell = float(np.sqrt(sum(((h - l) / 15) ** 2 for l, h in zip(*bounds))))
    assert vol.n_views == 2 and abs(vol.trunc - 3 * cell) < 1e-12 and vol.resolution == res
    poses = refined_poses(s.se3_refine.weight.detach(), ds.poses)
    assert not torch.equal(poses.cpu(), ds.poses)  # the REFINED poses
    manual = TsdfVolume(bounds, res, 3 * cell)
    for i in ids:
        K = ds.Ks[i]
        intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        nf = torch.tensor([[ds.nears[i], ds.fars[i]]], dtype=torch.float32).cuda()
        rays, _ = path_rays(poses[i:i + 1].cuda().contiguous(), nf, (16, 12), intr, 0, 192)
        rows = {k: s.embeddings[k].weight.detach()[i].expand(192, -1).contiguous() for k in ("coarse_a", "fine_a")}
        with torch.no_grad():
            out = render_rays(s.models, s.embeddings, rays, None, 1, sched_phase=2, N_samples=hp["nerf.N_samples"],
                              N_importance=hp["nerf.N_importance"], use_disp=hp["nerf.use_disp"], perturb=0, encode_feat=True,
                              validation=True, embed_rows=rows)
        manual.integrate(out["s_depth_fine"], poses[i], intr, (16, 12), rgb=out["s_rgb_fine"], opacity=out["s_weights_fine"].sum(1),
                         min_opacity=0.5)
    print(f"fuse_views: {int((vol.weight > 0).sum())} of {vol.weight.numel()} voxels observed, {int((vol.rgb_weight > 0).sum())} coloured")
    assert int((vol.weight > 0).sum()) > 100 and int((vol.rgb_weight > 0).sum()) > 100  # (the comparison is about something)
    assert same_volume(vol, manual)
    assert same_volume(vol, fuse_views(s, bounds, res, img_ids=ids))  # one chunk per frame: the same volume
    half = fuse_views(s, bounds, res, img_ids=ids, downscale=2, trunc=0.4)
    assert half.trunc == 0.4 and half.n_views == 2
    with pytest.raises(ValueError):
        fuse_views(s, bounds, res, img_ids=[6])
    s.set_progress(0.05)
    assert s.get_schedule_mult(s._host_progress) == 0
    with pytest.raises(ValueError):
        fuse_views(s, bounds, res, img_ids=ids)
