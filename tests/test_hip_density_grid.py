"""The density pass of the mesh extraction on the GPU (upnerf_amd/geometry.py: grid_columns, density_grid, colour_vertices) and
the whole chain down to a PLY file, on a W = 256, D = 8 system with the synthetic weights of upnerf_amd/synth.py.

Gate of density_grid against the oracle (oracle/upnerf_oracle.py nerf_field, evaluated in fp64 at the same fp32 points): the
project's parity gate, 1e-4 relative, per sample, with an absolute floor of 1e-6 where the softplus output is near zero -- in
the default f16x3 mode and in the f32 mode alike.  Everything else here is bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))

BOUNDS = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9))
PROGRESS = 0.3  # inside the coarse-to-fine window (0.1, 0.5): some bands of the encoding are partly on
N_IMG = 6


@pytest.fixture(scope="module")
def system():
    from upnerf_amd import synth
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset, default_hparams
    hp = default_hparams(**{"nerf.N_samples": 32, "nerf.N_importance": 32, "max_steps": 1000, "val.chunk_size": 4096})
    torch.manual_seed(5)
    s = NeRFSystem(hp, SyntheticDataset(N_IMG))
    s.setup()
    sd = {}
    for typ in ("coarse", "fine"):
        # "trained-like" statistics (synth.nerf_state): densities from ~1e-9 (where the gate's floor applies) to ~10 over BOUNDS
        st = synth.nerf_state(typ, D=8, W=256, seed=3, sigma_bias=-2.0, sigma_gain=30.0, trunk_gain=2.5)
        sd.update({f"nerf_{typ}.{k}": v for k, v in st.items()})
    missing, unexpected = s.load_state_dict(sd, strict=False)
    assert not unexpected and all(not k.startswith("nerf_") for k in missing)
    s.cuda()
    s.set_progress(PROGRESS)
    return s


def axis(lo, hi, n):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return (lo + np.arange(n, dtype=np.float64) * ((hi - lo) / (n - 1))).astype(np.float32) if n > 1 else np.array([lo], np.float32)


def oracle_sigma(system, res, field="fine"):
    """[Nz, Ny, Nx] fp64 shared density of the oracle's field at the fp32 grid points."""
    import upnerf_oracle as orc
    Nx, Ny, Nz = res
    model = system.models[f"nerf_{field}"]
    p = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    hp = system.hparams
    cfg = orc.NerfCfg(typ=field, D=8, W=256, xyz_L=hp["nerf.N_emb_xyz"], dir_L=hp["nerf.N_emb_dir"], c2f=hp["pose.c2f"])
    x, y, z = (axis(BOUNDS[0][k], BOUNDS[1][k], n) for k, n in enumerate(res))
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    xyz = torch.from_numpy(np.stack([X, Y, Z], -1).reshape(-1, 3)).double()
    M = xyz.shape[0]
    progress = float(np.float32(PROGRESS))
    with torch.no_grad():
        out = orc.nerf_field(p, cfg, xyz, torch.zeros(M, 3, dtype=torch.float64), torch.zeros(M, 48, dtype=torch.float64), None,
                             1.0, progress)
    return out["s_sigma"].reshape(Nz, Ny, Nx).numpy()


_ORACLE = {}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("res", [(5, 6, 32), (4, 3, 33), (6, 5, 7)], ids=lambda r: "x".join(map(str, r)))
def test_density_grid_matches_the_oracle(system, res, mode, monkeypatch):
    from upnerf_amd import rendering
    from upnerf_amd.geometry import density_grid
    monkeypatch.setattr(rendering, "FIELD_MODE", mode)
    got = density_grid(system, BOUNDS, res, chunk=7)  # 30, 12 and 30 columns: the last chunk is shorter
    assert tuple(got.shape) == (res[2], res[1], res[0]) and got.dtype == torch.float32 and got.is_cuda
    if res not in _ORACLE:
        _ORACLE[res] = oracle_sigma(system, res)
    ref = _ORACLE[res]
    g = got.cpu().numpy().astype(np.float64)
    err = np.abs(g - ref)
    worst = float((err / np.maximum(1e-4 * np.abs(ref), 1e-6)).max())
    print(f"{mode} {res}: sigma in [{ref.min():.3e}, {ref.max():.3e}], max abs err {err.max():.2e}, "
          f"max rel err {float((err / np.abs(ref)).max()):.2e}, worst err / gate {worst:.3f}")
    assert ref.min() > 0 and ref.max() > 2 * ref.min()  # a field with some range
    assert worst <= 1.0
    # the coarse field is another network
    if res == (6, 5, 7) and mode == "f16x3":
        other = density_grid(system, BOUNDS, res, field="coarse")
        assert not torch.equal(other, got)
        ref_c = oracle_sigma(system, res, "coarse")
        assert float((np.abs(other.cpu().numpy() - ref_c) / np.maximum(1e-4 * np.abs(ref_c), 1e-6)).max()) <= 1.0


def test_density_grid_does_not_depend_on_the_chunk(system):
    from upnerf_amd.geometry import density_grid
    res = (5, 6, 33)
    whole = density_grid(system, BOUNDS, res)
    for chunk in (1, 7, 30, 1000):
        assert torch.equal(density_grid(system, BOUNDS, res, chunk=chunk), whole), chunk
    with pytest.raises(ValueError):
        density_grid(system, BOUNDS, res, chunk=0)
    with pytest.raises(ValueError):
        density_grid(system, BOUNDS, res, field="transient")


def test_grid_columns_match_numpy_bit_for_bit(system):
    from upnerf_amd.geometry import grid_columns
    res = (5, 6, 7)
    x, y, z = (axis(BOUNDS[0][k], BOUNDS[1][k], n) for k, n in enumerate(res))
    col0, count, S = 3, 11, 32  # starts in the middle of the first row of columns, ends in the third
    o, d, zz = grid_columns(BOUNDS, res, col0, count)
    assert tuple(o.shape) == (count, 3) and tuple(d.shape) == (count, 3) and tuple(zz.shape) == (count, S)
    cols = np.arange(col0, col0 + count)
    ref_o = np.stack([x[cols % 5], y[cols // 5], np.zeros(count, np.float32)], 1)
    ref_z = np.concatenate([z, np.full(S - 7, z[-1], np.float32)])
    assert np.array_equal(o.cpu().numpy().view(np.int32), ref_o.view(np.int32))
    assert np.array_equal(d.cpu().numpy(), np.tile(np.array([0, 0, 1], np.float32), (count, 1)))
    assert np.array_equal(zz.cpu().numpy().view(np.int32), np.tile(ref_z, (count, 1)).view(np.int32))
    # a column longer than the minimum is not padded; any split gives the same rows
    o2, _, z2 = grid_columns(BOUNDS, (5, 6, 40), 0, 30)
    assert tuple(z2.shape) == (30, 40) and np.array_equal(z2[7].cpu().numpy(), axis(BOUNDS[0][2], BOUNDS[1][2], 40))
    o3, _, _ = grid_columns(BOUNDS, (5, 6, 40), 13, 4)
    assert torch.equal(o3, o2[13:17])
    with pytest.raises(RuntimeError):
        grid_columns(BOUNDS, res, 25, 6)  # past the last column


def hand_mesh():
    from upnerf_amd.geometry import Mesh
    g = torch.Generator().manual_seed(2)
    v = (torch.rand(37, 3, generator=g) - 0.5).cuda()
    n = torch.nn.functional.normalize(torch.randn(37, 3, generator=g), dim=1).cuda()
    n[5] = 0  # a vertex without a normal
    return Mesh(v, n, torch.zeros(0, 3, dtype=torch.int32).cuda())


def test_colour_vertices_is_render_rays_on_the_vertex_rays(system):
    from upnerf_amd.geometry import colour_vertices
    from upnerf_amd.rendering import render_rays
    system.set_progress(0.8)
    try:
        mesh, slab, img = hand_mesh(), 0.05, 4
        got = colour_vertices(system, mesh, img, slab, chunk=10)
        p, n = mesh.vertices, mesh.normals
        d = -n
        d[5] = torch.tensor([0.0, 0.0, 1.0])
        rays = torch.cat([p + slab * n, d, torch.tensor([0.0, 2 * slab]).cuda().expand(37, 2)], 1).contiguous()
        assert torch.equal(rays[5, :3], p[5])
        hp = system.hparams
        rows = {k: system.embeddings[k].weight.detach()[img].expand(37, -1).contiguous() for k in ("coarse_a", "fine_a")}
        with torch.no_grad():
            ref = render_rays(system.models, system.embeddings, rays, None, 1, N_samples=hp["nerf.N_samples"],
                              N_importance=hp["nerf.N_importance"], use_disp=hp["nerf.use_disp"], perturb=0, encode_feat=True,
                              embed_rows=rows)["s_rgb_fine"]
        assert tuple(got.shape) == (37, 3) and torch.equal(got, ref)
        assert torch.isfinite(got).all() and float(got.min()) >= 0 and float(got.max()) <= 1
        assert torch.equal(colour_vertices(system, mesh, img, slab), got)  # one chunk
        assert not torch.equal(colour_vertices(system, mesh, 1, slab), got)  # another photograph's appearance
        with pytest.raises(ValueError):
            colour_vertices(system, mesh, N_IMG, slab)
    finally:
        system.set_progress(PROGRESS)


def test_grid_to_ply_end_to_end(system, tmp_path):
    from upnerf_amd.geometry import colour_vertices, density_grid, extract_surface, read_ply
    res = (12, 11, 32)
    grid = density_grid(system, BOUNDS, res)
    level = float(grid.median())
    mesh = extract_surface(grid, BOUNDS, level)
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    print(f"end to end: level {level:.4f}, V {V}, F {F}")
    assert V > 0 and F > 0 and tuple(mesh.normals.shape) == (V, 3)
    assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < V
    lo, hi = (torch.tensor(b).cuda() for b in BOUNDS)
    assert bool((mesh.vertices >= lo - 1e-6).all()) and bool((mesh.vertices <= hi + 1e-6).all())
    system.set_progress(0.8)
    try:
        mesh.colours = colour_vertices(system, mesh, 2, slab=0.05)
    finally:
        system.set_progress(PROGRESS)
    assert tuple(mesh.colours.shape) == (V, 3)
    path = str(tmp_path / "scene.ply")
    mesh.write_ply(path)
    back = read_ply(path)
    assert torch.equal(back.vertices, mesh.vertices.cpu()) and torch.equal(back.normals, mesh.normals.cpu())
    assert torch.equal(back.faces, mesh.faces.cpu()) and tuple(back.colours.shape) == (V, 3)
    assert torch.equal(back.colours, (mesh.colours.cpu() * 255.0).clamp(0, 255).to(torch.uint8))
    with pytest.raises(RuntimeError):
        density_grid(type("S", (), {"models": {"nerf_fine": torch.nn.Linear(2, 2)}})(), BOUNDS, res)  # a field on the CPU
