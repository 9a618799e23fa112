"""The occupancy grid on the GPU (csrc/occupancy.hip, upnerf_amd/occupancy.py, the `occupancy` keyword of render_path).

Reference: tests/occupancy_ref.py -- fp64 numpy, brute force over every occupied cell, nothing of the kernel's traversal.
Gates.  Bits, indices, compacted rows and scattered results are exact (`torch.equal`).  Spans of random rays: rays that graze
a cell (its status differs between the cell shrunk and grown by 1e-3 of its edge; at most 3 % of the rays, asserted on the CPU
in test_occupancy_cpu.py) are left out, all others agree on `hit` exactly and on t0, t1 within
3 x (5 x 2^-24 x M / min_k |d_k|), M = the largest |plane| + |o_k| of the case: five fp32 roundings with a margin of 3.
Axis-parallel rays through cell centres: 4 ulp."""
import numpy as np
import pytest
import torch

import occupancy_ref as ref

pytestmark = pytest.mark.gpu

B = ref.BOUNDS


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- 1. build ---------------------------------------------------------------------------------------------------------------------

def cells_of_grid(grid, level):
    ins = np.isfinite(grid) & (grid >= level)
    c = np.zeros(tuple(n - 1 for n in grid.shape), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c |= ins[dz:dz + c.shape[0], dy:dy + c.shape[1], dx:dx + c.shape[2]]
    return c


def dilated(c, rounds):
    for _ in range(rounds):
        p = np.pad(c, 1)
        out = np.zeros_like(c)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= p[dz:dz + c.shape[0], dy:dy + c.shape[1], dx:dx + c.shape[2]]
        c = out
    return c


def bricks_of(c):
    pad = [(0, -n % 8) for n in c.shape]
    p = np.pad(c, pad)
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8, p.shape[2] // 8, 8).any(axis=(1, 3, 5))


def random_grid(shape, seed):
    rng = np.random.RandomState(seed)
    g = rng.randn(*shape).astype(np.float32)
    flat = g.reshape(-1)
    flat[rng.permutation(flat.size)[:flat.size // 25]] = np.nan
    flat[rng.permutation(flat.size)[:flat.size // 200 + 1]] = np.inf
    flat[rng.permutation(flat.size)[:flat.size // 50]] = -np.inf
    level = float(np.sort(flat[np.isfinite(flat)])[int(0.995 * np.isfinite(flat).sum())])  # an exact sample value
    assert (flat == level).any()
    return g, level


@pytest.mark.parametrize("shape", [(10, 11, 13), (10, 2, 13), (9, 9, 70)])  # [Nz, Ny, Nx] points; (9, 9, 70): 69 cells, 9 bricks
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_build_from_density_equals_the_numpy_restatement(shape, dilate):
    from upnerf_amd.occupancy import OccupancyGrid
    grid, level = random_grid(shape, seed=sum(shape))
    want = dilated(cells_of_grid(grid, level), dilate)
    occ = OccupancyGrid.from_density(dev(grid), B, level, dilate=dilate)
    assert occ.dims == (shape[2] - 1, shape[1] - 1, shape[0] - 1)
    got = occ.cells()
    assert got.dtype == torch.bool and tuple(got.shape) == want.shape
    print(f"{shape} dilate {dilate}: occupied {want.mean():.3f}")
    assert want.any() and not want.all()
    assert torch.equal(got, dev(want))
    assert torch.equal(occ.bricks(), dev(bricks_of(want)))
    assert abs(occ.fraction - want.mean()) < 1e-6
    # unused high bits are zero, and a second build gives the same words
    for last, n in ((occ.fine_words - 1, occ.n_cells), (-1, int(np.prod(occ.brick_dims)))):
        if n % 32:
            assert (int(occ.words[last]) & 0xFFFFFFFF) >> (n % 32) == 0
    again = OccupancyGrid.from_density(dev(grid), B, level, dilate=dilate)
    assert torch.equal(again.words, occ.words)
    # the same cells handed over as an array give the same words
    assert torch.equal(OccupancyGrid.from_cells(dev(cells_of_grid(grid, level)), B, dilate=dilate).words, occ.words)
    assert torch.equal(OccupancyGrid.from_cells(dev(want.astype(np.uint8) * 7), B).words, occ.words)


def test_wrappers_refuse_wrong_dtypes_and_shapes():
    from upnerf_amd import occupancy as oc
    with pytest.raises(ValueError):
        oc.OccupancyGrid.from_density(torch.zeros(3, 3, 3, dtype=torch.float64).cuda(), B, 0.5)
    with pytest.raises(ValueError):
        oc.OccupancyGrid.from_density(torch.zeros(3, 3).cuda(), B, 0.5)
    with pytest.raises(ValueError):
        oc.OccupancyGrid.from_density(torch.zeros(3, 1, 3).cuda(), B, 0.5)  # an axis without a cell
    with pytest.raises(ValueError):
        oc.OccupancyGrid.from_density(torch.zeros(3, 3, 3).cuda(), B, 0.5, dilate=-1)
    with pytest.raises(ValueError):
        oc.OccupancyGrid.from_cells(torch.zeros(3, 3, 3).cuda(), B)
    occ = oc.OccupancyGrid.from_cells(torch.ones(3, 3, 3, dtype=torch.bool).cuda(), B)
    with pytest.raises(ValueError):
        oc.ray_spans(occ, torch.zeros(4, 7).cuda())
    with pytest.raises(ValueError):
        oc.ray_spans(occ, torch.zeros(4, 8, dtype=torch.float64).cuda())
    rays = torch.zeros(4, 8).cuda()
    with pytest.raises(ValueError):
        oc.compact_rays(occ, rays, rows=[torch.zeros(3, 16).cuda()])
    with pytest.raises(ValueError):
        oc.compact_rays(occ, rays, rows=[torch.zeros(4, 16).cuda()] * 5)
    with pytest.raises(ValueError):
        oc.scatter_results(torch.zeros(2, dtype=torch.int64).cuda(), rays, torch.zeros(2, 3).cuda())


# ---- 2. the mesh lies in occupied cells ------------------------------------------------------------------------------------------------

def test_every_vertex_of_the_mesh_lies_in_an_occupied_cell():
    from upnerf_amd.geometry import extract_surface
    from upnerf_amd.occupancy import OccupancyGrid
    N = (21, 18, 16)  # points (Nx, Ny, Nz)
    lo, hi = ref.bounds64(B)
    ax = [np.linspace(lo[k], hi[k], N[k]) for k in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    g = lambda c, s: np.exp(-((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) / (2 * s * s))
    grid = (g((-0.3, 0.1, 0.1), 0.3) + 0.8 * g((0.45, -0.2, 0.2), 0.22)).astype(np.float32)
    level = 0.5
    mesh = extract_surface(dev(grid), B, level)
    occ = OccupancyGrid.from_density(dev(grid), B, level, dilate=0)
    cells = occ.cells().cpu().numpy()
    v = mesh.vertices.cpu().numpy().astype(np.float64)
    assert v.shape[0] > 100 and 0 < cells.mean() < 0.5
    C = np.array(occ.dims)
    u = (v - lo) / ((hi - lo) / C)  # in cells; a vertex on a cell's boundary belongs to both neighbours (1e-4 of a cell: fp32)
    ok = np.zeros(v.shape[0], bool)
    for sx in (-1e-4, 1e-4):
        for sy in (-1e-4, 1e-4):
            for sz in (-1e-4, 1e-4):
                i = np.clip(np.floor(u + np.array([sx, sy, sz])).astype(int), 0, C - 1)
                ok |= cells[i[:, 2], i[:, 1], i[:, 0]]
    assert ok.all(), int((~ok).sum())


# ---- 3. spans of random rays -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,share,seed", ref.SPAN_CASES)
def test_spans_of_random_rays_match_brute_force(dims, share, seed):
    from upnerf_amd.occupancy import OccupancyGrid, ray_spans
    cells, rays = ref.random_cells(dims, share, seed), ref.random_rays(B, seed)
    occ = OccupancyGrid.from_cells(dev(cells), B)
    t0, t1, hit = (x.cpu().numpy() for x in ray_spans(occ, dev(rays)))
    r0, r1, rh = ref.spans_ref(cells, B, rays)
    keep = ~ref.grazing(cells, B, rays)
    tol = ref.span_tolerance(dims, B, rays)
    e0, e1 = np.abs(t0 - r0), np.abs(t1 - r1)
    both = keep & rh & (hit == 1)
    print(f"{dims} at {share}: grazing {1 - keep.mean():.4f}, hits {rh[keep].mean():.3f}, wrong hit flags {(hit[keep] != rh[keep]).sum()}, "
          f"max err t0 {e0[both].max():.2e} t1 {e1[both].max():.2e}, smallest gate {tol.min():.2e}, "
          f"worst err / gate {max((e0[both] / tol[both]).max(), (e1[both] / tol[both]).max()):.3f}")
    assert 1 - keep.mean() <= 0.03
    assert 0.15 <= rh[keep].mean() <= 0.85
    assert np.array_equal(hit[keep] == 1, rh[keep])
    assert (e0[both] <= tol[both]).all() and (e1[both] <= tol[both]).all()
    # on every ray, grazing or not: a hit has near <= t0 < t1 <= far, a miss t0 = t1 = far
    h = hit == 1
    assert (t0[h] >= rays[h, 6]).all() and (t1[h] <= rays[h, 7]).all() and (t1[h] > t0[h]).all()
    assert np.array_equal(t0[~h], rays[~h, 7]) and np.array_equal(t1[~h], rays[~h, 7])


# ---- 4. spans, deterministic -------------------------------------------------------------------------------------------------------------

def centres(dims):
    lo, hi = ref.bounds64(B)
    return [lo[k] + (np.arange(dims[k]) + 0.5) * (hi[k] - lo[k]) / dims[k] for k in range(3)]


def axis_rays(dims, axis, sign, scale=1.0):
    """One ray per cell column along `axis` through the cell centres, from 1 outside the box; fp32 [n, 8]."""
    lo, hi = ref.bounds64(B)
    c = centres(dims)
    others = [k for k in range(3) if k != axis]
    a, b = np.meshgrid(c[others[0]], c[others[1]], indexing="ij")
    n = a.size
    rays = np.zeros((n, 8))
    rays[:, others[0]], rays[:, others[1]] = a.ravel(), b.ravel()
    rays[:, axis] = lo[axis] - 1.0 if sign > 0 else hi[axis] + 1.0
    rays[:, 3 + axis] = sign * scale
    rays[:, 6], rays[:, 7] = 0.25 / scale, 6.0 / scale
    return rays.astype(np.float32)


def ulps(a, b):
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_axis_parallel_rays_through_cell_centres(axis, sign):
    from upnerf_amd.occupancy import OccupancyGrid, ray_spans
    dims = (12, 10, 9)
    cells = ref.random_cells(dims, 0.15, 5)
    occ = OccupancyGrid.from_cells(dev(cells), B)
    rays = axis_rays(dims, axis, sign)
    t0, t1, hit = (x.cpu().numpy() for x in ray_spans(occ, dev(rays)))
    r0, r1, rh = ref.spans_ref(cells, B, rays)
    assert not ref.grazing(cells, B, rays).any() and 0 < rh.mean() < 1
    assert np.array_equal(hit == 1, rh)
    u = max(ulps(t0[rh], r0[rh]).max(), ulps(t1[rh], r1[rh]).max())
    print(f"axis {axis} sign {sign}: {rh.sum()} of {rh.size} columns hit, max {u:.2f} ulp")
    assert u <= 4
    # d scaled by 2 (near and far with it): every t is halved exactly
    s0, s1, sh = (x.cpu().numpy() for x in ray_spans(occ, dev(axis_rays(dims, axis, sign, scale=2.0))))
    assert np.array_equal(sh, hit) and np.array_equal(s0 * 2, t0) and np.array_equal(s1 * 2, t1)
    # the same rays moved outside the slab of an axis they do not move along: all miss
    out = rays.copy()
    other = (axis + 1) % 3
    out[:, other] = ref.bounds64(B)[1][other] + 0.01
    assert int(ray_spans(OccupancyGrid.from_cells(dev(np.ones_like(cells)), B), dev(out))[2].sum()) == 0
    out[:, other] = ref.bounds64(B)[0][other] - 0.01
    assert int(ray_spans(OccupancyGrid.from_cells(dev(np.ones_like(cells)), B), dev(out))[2].sum()) == 0


def test_empty_and_full_grids():
    from upnerf_amd.occupancy import OccupancyGrid, ray_spans
    dims = (12, 10, 9)
    rays = np.concatenate([ref.random_rays(B, 7, 1024), axis_rays(dims, 0, 1), axis_rays(dims, 2, -1)])
    empty = OccupancyGrid.from_cells(dev(np.zeros(dims[::-1], bool)), B)
    t0, t1, hit = ray_spans(empty, dev(rays))
    assert int(hit.sum()) == 0 and torch.equal(t0, dev(rays[:, 7])) and torch.equal(t1, dev(rays[:, 7]))
    assert empty.fraction == 0.0
    full = OccupancyGrid.from_cells(dev(np.ones(dims[::-1], bool)), B)
    assert full.fraction == 1.0
    t0, t1, hit = (x.cpu().numpy() for x in ray_spans(full, dev(rays)))
    # the box clipped to [near, far], by the slab test in fp64
    lo, hi = ref.bounds64(B)
    r = rays.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - r[:, :3]) / r[:, 3:6], (hi - r[:, :3]) / r[:, 3:6]
    zero = r[:, 3:6] == 0
    ta, tb = np.where(zero, -np.inf, ta), np.where(zero, np.inf, tb)  # (the axis-parallel rays here are inside their slabs)
    te = np.maximum(r[:, 6], np.minimum(ta, tb).max(1))
    tx = np.minimum(r[:, 7], np.maximum(ta, tb).min(1))
    rh = tx > te
    sure = np.abs(tx - te) > 1e-4
    assert 0.15 < rh.mean() < 1 and np.array_equal(hit[sure] == 1, rh[sure])
    both = rh & (hit == 1)
    with np.errstate(divide="ignore"):
        tol = ref.span_tolerance(dims, B, rays)
    tol = np.where(np.isfinite(tol), tol, 4 * np.spacing(np.float32(4.0)))  # axis-parallel: 4 ulp of the largest t there
    assert (np.abs(t0 - te)[both] <= tol[both]).all() and (np.abs(t1 - tx)[both] <= tol[both]).all()


def test_a_long_grid_skips_bricks_and_finds_the_cells_at_its_ends():
    from upnerf_amd.occupancy import OccupancyGrid, ray_spans
    dims = (70, 3, 2)  # nine bricks along x, the last one six cells wide
    lo, hi = ref.bounds64(B)
    step = (hi - lo) / np.array(dims)
    c = centres(dims)
    for xs in ([69], [0], [66], [0, 69], [7, 8], [63, 64]):
        cells = np.zeros(dims[::-1], bool)
        cells[1, 2, xs] = True
        occ = OccupancyGrid.from_cells(dev(cells), B)
        assert int(occ.bricks().sum()) == len({x // 8 for x in xs})
        rays = []
        for sign in (1, -1):  # along the row of cells, both ways, and diagonally through it
            o = [lo[0] - 0.5 if sign > 0 else hi[0] + 0.5, c[1][2], c[2][1]]
            rays.append(o + [sign, 0, 0, 0.0, 4.0])
            d = np.array([sign, 0.02, 0.01])
            d /= np.linalg.norm(d)
            rays.append([o[0], o[1] - d[1] / d[0] * (c[0][xs[0]] - o[0]), o[2] - d[2] / d[0] * (c[0][xs[0]] - o[0])] + list(d) + [0.0, 4.0])
        o = [lo[0] - 0.5, c[1][0], c[2][1]]  # the row beside it: a miss
        rays.append(o + [1, 0, 0, 0.0, 4.0])
        rays = np.array(rays, np.float32)
        t0, t1, hit = (x.cpu().numpy() for x in ray_spans(occ, dev(rays)))
        r0, r1, rh = ref.spans_ref(cells, B, rays)
        assert not ref.grazing(cells, B, rays).any()
        assert rh.tolist() == [True, True, True, True, False] and np.array_equal(hit == 1, rh), (xs, hit, rh)
        assert np.abs(t0 - r0).max() <= 1e-6 and np.abs(t1 - r1).max() <= 1e-6, (xs, t0, r0, t1, r1)
        assert abs((t1[0] - t0[0]) - (xs[-1] - xs[0] + 1) * step[0]) <= 1e-6


# ---- 5. compact and scatter --------------------------------------------------------------------------------------------------------------

PATTERNS = {"none": lambda r: r < 0, "all": lambda r: r >= 0, "alternating": lambda r: r % 2 == 1, "last": lambda r: r == r.max(),
            "random": lambda r: np.random.RandomState(3).rand(r.size) < 0.3}


@pytest.mark.parametrize("R", [1000, 2500])  # 2500: more than one block of the scan (1024 rows each)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_compact_and_scatter(R, pattern):
    from upnerf_amd.occupancy import compact_hits, scatter_results
    g = torch.Generator().manual_seed(R)
    rays = torch.randn(R, 8, generator=g).cuda()
    t0, t1 = torch.rand(R, generator=g).cuda(), (1 + torch.rand(R, generator=g)).cuda()
    tabs = [torch.randn(R, 48, generator=g).cuda(), torch.randn(R, 16, generator=g).cuda()]
    hit = dev(PATTERNS[pattern](np.arange(R)).astype(np.uint8))
    want = torch.nonzero(hit).reshape(-1)
    rays_c, rows_c, index, n = compact_hits(rays, t0, t1, hit, tabs)
    assert n == want.numel() and index.dtype == torch.int32 and torch.equal(index.long(), want)
    assert tuple(rays_c.shape) == (n, 8) and [tuple(r.shape) for r in rows_c] == [(n, 48), (n, 16)]
    assert torch.equal(rays_c[:, :6], rays[want][:, :6])
    assert torch.equal(rays_c[:, 6], t0[want]) and torch.equal(rays_c[:, 7], t1[want])
    for got, tab in zip(rows_c, tabs):
        assert torch.equal(got, tab[want])
    # without tables, a bool mask, and buffers that are not 16-byte aligned: the same rows
    odd = torch.zeros(R * 8 + 1, device="cuda")
    odd[1:] = rays.reshape(-1)
    again = compact_hits(odd[1:].view(R, 8), t0, t1, hit.bool())
    assert again[3] == n and torch.equal(again[0], rays_c) and again[1] == [] and torch.equal(again[2], index)
    # scatter: the inverse of the gather, the background and the ray's far on every other row
    rgb_c, depth_c = torch.rand(n, 3, generator=g).cuda(), torch.rand(n, generator=g).cuda()
    for bg in (0.0, 1.0):
        rgb, depth = scatter_results(index, rays, rgb_c if n else None, depth_c if n else None, background=bg, want_depth=True)
        want_rgb = torch.full((R, 3), bg, device="cuda")
        want_rgb[want] = rgb_c
        want_depth = rays[:, 7].clone()
        want_depth[want] = depth_c
        assert torch.equal(rgb, want_rgb) and torch.equal(depth, want_depth)
    rgb, depth = scatter_results(index, rays, rgb_c if n else None)
    assert depth is None and torch.equal(rgb[want], rgb_c)


# ---- 6. through render_path --------------------------------------------------------------------------------------------------------------

ID0, ID1 = 1, 4
SCENE = ((-2.5, -2.5, -5.5), (2.5, 2.5, 0.5))  # the box in front of the cameras of two_key_path (they look down -z)


def make_system(progress):
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset, default_hparams
    hp = default_hparams(**{"nerf.N_samples": 32, "nerf.N_importance": 32, "max_steps": 1000})
    torch.manual_seed(11)
    s = NeRFSystem(hp, SyntheticDataset(6))
    s.setup()
    with torch.no_grad():
        for emb in s.embeddings.values():
            emb.weight.copy_(torch.randn(emb.weight.shape))
    s.cuda()
    s.set_progress(progress)
    return s


@pytest.fixture(scope="module")
def system():
    return make_system(0.3)  # sched_mult 0.5: four embedding tables


def render(system, rays, **kw):
    from upnerf_amd.rendering import render_rays
    hp = system.hparams
    with torch.no_grad():
        return render_rays(system.models, system.embeddings, rays, sched_mult=system.get_schedule_mult(system._host_progress),
                           N_samples=hp["nerf.N_samples"], N_importance=hp["nerf.N_importance"], use_disp=hp["nerf.use_disp"],
                           perturb=0, encode_feat=True, **kw)


def two_key_path(n_frames=3, wh=(8, 6)):
    from upnerf_amd.novel_view import CameraPath
    c = np.cos(0.3), np.sin(0.3)
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2]],
                        [[c[0], 0, c[1], -0.2], [0, 1, 0, 0.1], [-c[1], 0, c[0], 0.0]]])
    K = torch.tensor([[7.5, 0, 3.6], [0, 7.0, 2.8], [0, 0, 1]])
    return CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], n_frames, appearance=(ID0, ID1), img_wh=wh, K=K)


def frame_rays_and_rows(system, path, f):
    """The rays of frame f and its blended embedding rows, as render_path makes them."""
    from upnerf_amd import novel_view as nv
    from upnerf_amd.static_scene import static_keys
    c2w, nf = nv.path_poses(path.key_c2w.cuda(), path.key_near_far.cuda(), path.u.cuda(), path.mode)
    n = path.img_wh[0] * path.img_wh[1]
    keys = static_keys(system, system.get_schedule_mult(system._host_progress))
    tables = [(system.embeddings[k].weight.detach().contiguous(), None) for k in keys]
    rays, rows = nv.path_rays(c2w, nf, path.img_wh, path.K, f * n, n, tables=tables, i0=path.i0.cuda(), i1=path.i1.cuda(),
                              t=path.t.cuda())
    return rays, dict(zip(keys, rows))


def test_render_path_with_an_empty_grid_renders_nothing(system):
    from upnerf_amd import novel_view as nv
    from upnerf_amd.occupancy import OccupancyGrid
    from upnerf_amd.ops import TIMER
    occ = OccupancyGrid.from_cells(torch.zeros(4, 4, 4, dtype=torch.bool).cuda(), SCENE)
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, None
    try:
        out = nv.render_path(system, two_key_path(), chunk=16, outputs=("rgb_float", "rgb"), occupancy=occ)
        kern = TIMER.summary()
    finally:
        TIMER.enabled = False
        TIMER.reset()
    assert nv.LAST_STATS == {"rays": 144, "hits": 0}
    assert set(kern) == {"path_rays", "occ_spans", "occ_compact", "occ_scatter"}, sorted(kern)  # no field, no composite
    assert kern["occ_spans"]["launches"] == 9
    assert float(out["rgb_float"].abs().max()) == 0.0 and int(out["rgb"].max()) == 0  # the background (white_back is off)


def test_render_path_with_a_grid_renders_the_hit_rays_over_their_spans(system):
    from upnerf_amd import novel_view as nv
    from upnerf_amd.occupancy import OccupancyGrid, ray_spans
    path = two_key_path()
    cells = dev(ref.random_cells((6, 6, 6), 0.1, 8))
    occ = OccupancyGrid.from_cells(cells, SCENE)
    out = nv.render_path(system, path, chunk=48, outputs=("rgb_float",), occupancy=occ)["rgb_float"]  # a chunk = a frame
    assert set(nv.LAST_WORKSPACE) == {"rays", "coarse_a", "fine_a", "coarse_c", "fine_c", "occ_t0", "occ_t1", "occ_hit", "occ_index",
                                      "occ_count", "occ_rays_c", "occ_scan", "occ_rgb", "occ_coarse_a", "occ_fine_a", "occ_coarse_c",
                                      "occ_fine_c"}
    assert nv.LAST_WORKSPACE["occ_rays_c"] == (48, 8) and nv.LAST_WORKSPACE["occ_fine_a"] == (48, 48)
    hits = 0
    for f in range(3):
        rays, rows = frame_rays_and_rows(system, path, f)
        t0, t1, hit = ray_spans(occ, rays)
        idx = torch.nonzero(hit).reshape(-1)
        miss = torch.nonzero(hit == 0).reshape(-1)
        assert idx.numel() >= 5 and miss.numel() >= 5, (f, idx.numel())
        hits += idx.numel()
        tight = torch.cat([rays[idx][:, :6], t0[idx, None], t1[idx, None]], 1).contiguous()
        direct = render(system, tight, img_idx=None, embed_rows={k: v[idx].contiguous() for k, v in rows.items()})["s_rgb_fine"]
        assert torch.equal(out[f][idx], direct), f
        assert float(out[f][miss].abs().max()) == 0.0
        full = render(system, rays, img_idx=None, embed_rows=rows)["s_rgb_fine"]
        assert not torch.equal(out[f][idx], full[idx])  # the tightened span moves the samples: not the full render's bits
    assert nv.LAST_STATS == {"rays": 144, "hits": hits}
    # chunks that straddle frames give the same frames
    again = nv.render_path(system, path, chunk=16, outputs=("rgb_float", "depth"), depth_range=(0.1, 5.0), occupancy=occ)
    assert torch.equal(again["rgb_float"], out) and nv.LAST_STATS == {"rays": 144, "hits": hits}
    assert tuple(again["depth"].shape) == (3, 6, 8, 3) and nv.LAST_WORKSPACE["occ_depth"] == (16,)


def test_render_path_without_a_grid_is_what_it_was(system):
    from upnerf_amd import novel_view as nv
    path = two_key_path()
    out = nv.render_path(system, path, chunk=16, outputs=("rgb_float",))["rgb_float"]
    assert nv.LAST_WORKSPACE == {"rays": (16, 8), "coarse_a": (16, 48), "fine_a": (16, 48), "coarse_c": (16, 16), "fine_c": (16, 16)}
    assert nv.LAST_STATS == {}
    for f in range(3):
        rays, rows = frame_rays_and_rows(system, path, f)
        assert torch.equal(out[f], render(system, rays, img_idx=None, embed_rows=rows)["s_rgb_fine"]), f
    assert torch.equal(nv.render_path(system, path, chunk=16, outputs=("rgb_float",), occupancy=None)["rgb_float"], out)
