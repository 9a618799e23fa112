"""The sparse baked scene on the GPU (csrc/brick.hip, upnerf_baked_sparse_render in csrc/baked.hip, upnerf_amd/baked.py;
DESIGN.md 2.33).

Nothing here has a tolerance.  Table, gather, scatter and the bits from the pool are integer and byte work and are held to the
numpy restatement tests/baked_sparse_ref.py byte for byte; the sparse marcher is held to the dense marcher with torch.equal (the
dense marcher is held to fp64 by tests/test_hip_baked.py and tests/test_hip_baked_sh.py); the sparse bake is held to the dense
bake's sparsify() bit for bit, which rests on a field row's output depending on its own o, d, z, direction and appearance only.
That holds at the shapes of this test on an MI355X (2026-10-20).  It is not true of every shape: at 128^3 points, degree 2 and 48
directions 2 of 2 985 984 pool records differed by one fp16 step, because the f16 field kernels scale a tile of samples by the
tile's own largest magnitude and a sample's last bit depends on its tile-mates (tools/bench_baked.py --sparse
reports the count)."""
import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
import baked_sh_ref as sh
import baked_sparse_ref as sr
from baked_cases import dev

pytestmark = pytest.mark.gpu

CELLS = [(8, 8, 8), (9, 17, 5), (20, 12, 33)]  # one brick; 2 x 3 x 1 bricks, ragged on every axis; 3 x 2 x 5 bricks


def host_words(words):
    return words.cpu().numpy().view(np.uint32)


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("rgb", "depth", "opacity"))


def pattern(cells, kind):
    Cx, Cy, Cz = cells
    if kind == "clear":
        return np.zeros((Cz, Cy, Cx), bool)
    if kind == "set":
        return np.ones((Cz, Cy, Cx), bool)
    if kind == "last":  # one cell, in the last (ragged) brick
        c = np.zeros((Cz, Cy, Cx), bool)
        c[-1, -1, -1] = True
        return c
    return np.random.RandomState(Cx + Cy).uniform(size=(Cz, Cy, Cx)) < 0.3


@pytest.mark.parametrize("kind", ["clear", "set", "last", "seeded"])
@pytest.mark.parametrize("cells", CELLS)
def test_table_gather_scatter_and_bits_are_the_restatements_byte_for_byte(cells, kind):
    from upnerf_amd import baked
    from upnerf_amd.occupancy import OccupancyGrid
    Cx, Cy, Cz = cells
    res = (Cx + 1, Cy + 1, Cz + 1)
    cell = pattern(cells, kind)
    occ = OccupancyGrid.from_cells(dev(cell), br.BOUNDS)
    assert (host_words(occ.words) == sr.words(cell)).all()  # (the restatement packs as upnerf_occ_build does)
    slots, bricks, n = baked.brick_table(occ.words, cells)
    want_slots, want_bricks = sr.table(sr.brick_bits(cell))
    assert n == len(want_bricks) and slots.dtype == bricks.dtype == torch.int32
    assert (slots.cpu().numpy() == want_slots).all() and (bricks.cpu().numpy() == want_bricks).all()
    s2, b2, n2 = baked.brick_table(occ.words, cells)  # a second run
    assert n2 == n and torch.equal(s2, slots) and torch.equal(b2, bricks)
    B = sr.brick_dims(cells)
    assert n == {"clear": 0, "set": B[0] * B[1] * B[2], "last": 1}.get(kind, n)
    rng = np.random.RandomState(n + Cx)
    for E, at in ((4, 0), (16, 12), (32, 24), (64, 56)):
        grid = rng.randint(0, 256, (Cz + 1, Cy + 1, Cx + 1, E)).astype(np.uint8)
        pool = baked.brick_gather(dev(grid), bricks)
        want = sr.gather(grid, want_bricks)
        assert tuple(pool.shape) == (n, 9, 9, 9, E) and (pool.cpu().numpy() == want).all(), E
        if E == 16:  # fp32 points come back as fp32 points
            assert baked.brick_gather(dev(grid).view(torch.float32), bricks).dtype == torch.float32
        fill = rng.randint(0, 256, want.shape).astype(np.uint8)  # any pool, not only a gathered one: the owners alone store
        back = baked.brick_scatter(dev(fill), bricks, res)
        assert tuple(back.shape) == grid.shape and (back.cpu().numpy() == sr.scatter(fill, want_bricks, res)).all(), E
        # the bits of a pool of random bytes: its sigmas are any fp32, NaN and infinities and negative numbers among them
        sigma = np.ascontiguousarray(fill[..., at:at + 4]).view(np.float32)[..., 0]
        store = baked._aligned(fill.size, E, torch.device("cuda"))
        if n:
            store[:fill.size].copy_(dev(fill).view(-1))
        words = baked.brick_words(store, slots, n, res, E, at)
        assert (host_words(words) == sr.words(sr.cell_bits(sigma, want_slots, cells))).all(), E
    if kind == "clear":  # no brick: nothing is launched over the pool, and a render is all misses
        scene = baked.BakedScene.from_grids(torch.zeros(Cz + 1, Cy + 1, Cx + 1).cuda(), None, br.BOUNDS, 0.0).sparsify()
        assert scene.sparse and scene.n_bricks == 0 and scene.pool.shape[0] == 0 and int(scene.occupancy.words.abs().sum()) == 0
        rays = br.make_rays()
        out = scene.render(dev(rays), 0.05, background=0.25)
        assert float(out["opacity"].abs().max()) == 0 and bool((out["rgb"] == 0.25).all())
        assert torch.equal(out["depth"], dev(rays[:, 7]))


def dense_scene(name, degree):
    """A test grid of baked_ref as a dense scene of the degree (the SH records are baked_sh_ref's), built once."""
    return cases.scene_of((__name__, name, degree), lambda: cases.build(*(sh.GRIDS[name]() if degree == 0 else sh.sh_grid(name, degree)), degree))


@pytest.mark.parametrize("name", ["blob", "corners"])
def test_the_bits_from_the_pool_are_the_dense_scenes_words(name):
    from upnerf_amd.occupancy import OccupancyGrid
    rgbs, _ = sh.GRIDS[name]()
    for degree in (0, 1, 2):
        scene = dense_scene(name, degree)
        sp = scene.sparsify()
        assert sp.sparse and not scene.sparse and sp.sh_degree == degree and sp.resolution == scene.resolution
        words = OccupancyGrid.from_density(dev(rgbs[..., 3]), br.BOUNDS, level=sr.TINY, dilate=0).words
        assert torch.equal(sp.occupancy.words, words) and torch.equal(scene.occupancy.words, words)
        assert (host_words(words) == sr.words(sr.dense_cell_bits(rgbs[..., 3]))).all()
        assert sp.n_bricks == scene.n_bricks == (2 if name == "corners" else 4) and sp.fraction == scene.fraction
        assert torch.equal(sp.slots.cpu(), torch.from_numpy(sr.table(sr.brick_bits(sr.dense_cell_bits(rgbs[..., 3])))[0]))


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", ["blob", "corners"])
def test_the_sparse_marcher_is_the_dense_marcher_bit_for_bit(name, degree):
    scene = dense_scene(name, degree)
    sp = scene.sparsify()
    assert sp.grid is sp.pool and sp.device == scene.device
    assert sp.nbytes < scene.nbytes or name == "blob"  # (every brick of the blob is occupied: 4 x 729 points for its 990)
    rays = dev(br.make_rays())
    cell = br.cell_size(sh.GRIDS[name]()[0])
    hits = 0
    for step in (float(np.float32(cell)), float(np.float32(cell / 10))):
        for background in (0.0, 1.0):
            for stop in (0.0, 1e-3):
                want = scene.render(rays, step, background=background, stop=stop)
                got = sp.render(rays, step, background=background, stop=stop)
                for k in ("rgb", "depth", "opacity"):
                    assert torch.equal(got[k], want[k]), (k, step, background, stop, int((got[k] != want[k]).sum()))
                assert same(sp.render(rays, step, background=background, stop=stop), want)  # a second run
                a, b = sp.render(rays[:33], step, background=background, stop=stop), sp.render(rays[33:], step, background=background, stop=stop)
                assert same({k: torch.cat([a[k], b[k]]) for k in a}, want)  # a launch cut at ray 33
                hits = max(hits, int((want["opacity"] > 0).sum()))
    assert hits >= 20  # the comparison looked at rays that met the volume


def test_a_grid_the_dense_layout_would_not_want():
    """257^3 points (32^3 bricks), a slab round a tilted plane over the middle of the box: a few hundred bricks of 32 768."""
    from upnerf_amd.baked import BakedScene
    N = 257
    i = torch.arange(N, device="cuda", dtype=torch.float32)
    z, y, x = i[:, None, None], i[None, :, None], i[None, None, :]
    on = ((z - (128.0 + 0.2 * (x - 128.0) + 0.1 * (y - 128.0))).abs() <= 0.6) & ((x - 128.0).abs() <= 64) & ((y - 128.0).abs() <= 64)
    sigma = torch.where(on, torch.full((), 60.0, device="cuda"), torch.zeros((), device="cuda"))
    rgb = torch.stack([(x / 256).expand(N, N, N), (y / 256).expand(N, N, N), (z / 256).expand(N, N, N)], -1).contiguous()
    dense = BakedScene.from_grids(sigma, rgb, br.BOUNDS, 1.0)
    del rgb, sigma, on
    sp = dense.sparsify()
    n = sp.n_bricks
    print(f"257^3: {n} of 32768 bricks occupied, sparse {sp.nbytes} bytes, dense {dense.nbytes} bytes ({dense.nbytes / sp.nbytes:.1f} x)")
    assert 0 < n <= 1024 and n == dense.n_bricks
    lo, hi = br.bounds64(br.BOUNDS)
    rng = np.random.RandomState(2)
    rows = []
    for _ in range(64):  # rays through a point of the slab
        gx, gy = rng.uniform(70, 186, 2)
        p = lo + np.array([gx, gy, 128.0 + 0.2 * (gx - 128.0) + 0.1 * (gy - 128.0)]) / 256 * (hi - lo)
        d = rng.randn(3)
        d /= np.linalg.norm(d)
        rows.append(list(p - 1.5 * d) + list(d) + [0.0, 3.0])
    rays = dev(np.concatenate([np.asarray(rows, np.float32), br.make_rays()[[2, 5, 6]]]))  # and the miss cases: outside, a NaN, far <= near
    step = float(np.float32(((hi - lo) / (N - 1)).min() / 2))  # half a cell
    want, got = dense.render(rays, step, background=0.5), sp.render(rays, step, background=0.5)
    assert same(got, want)
    assert int((want["opacity"][:64] > 0.01).sum()) >= 48 and float(want["opacity"][64:].abs().max()) == 0
    table = (sp.slots.numel() + sp.bricks.numel()) * 4
    assert sp.slots.numel() == 32 ** 3 and sp.nbytes == n * 729 * 16 + table + sp.occupancy.words.numel() * 4
    assert sp.nbytes * 20 < dense.nbytes


# ---- the bake of a field ------------------------------------------------------------------------------------------------------------

BOX = ((-0.7, -0.5, -0.6), (0.8, 0.6, 0.9))  # the seeded system and the box of tests/test_hip_baked.py
RES = (20, 12, 33)  # 19 x 11 x 32 cells: 3 x 2 x 4 bricks, ragged in x and y
IMG = 4


@pytest.fixture(scope="module")
def system():
    return cases.make_system()


def test_the_sparse_bake_is_the_dense_bake_sparsified_bit_for_bit(system):
    from upnerf_amd.baked import BakedScene, sphere_directions
    from upnerf_amd.geometry import density_grid
    sigma = density_grid(system, BOX, RES).cpu().numpy()
    # a brick is occupied iff one of the grid points it stores is kept: the level is the median of the bricks' largest sigmas, so
    # that some bricks are occupied and some are not whatever the scale of these random weights (a quantile of the sigma, found
    # by looking at it)
    Bx, By, Bz = sr.brick_dims(tuple(n - 1 for n in RES))
    top = np.sort([sigma[8 * bz:8 * bz + 9, 8 * by:8 * by + 9, 8 * bx:8 * bx + 9].max() for bz in range(Bz) for by in range(By) for bx in range(Bx)])
    level = float(top[len(top) // 2])
    assert top[0] < level and level > 0 and np.isfinite(sigma).all()
    print(f"sigma in [{sigma.min():.4f}, {sigma.max():.4f}]; level {level:.4f} is its {float((sigma < level).mean()):.4f} quantile")
    for degree, kw in ((0, {}), (2, dict(sh_degree=2, dirs=sphere_directions(12)))):
        dense = BakedScene.build(system, BOX, RES, level, img_id=IMG, **kw)
        want = dense.sparsify()
        got = BakedScene.build(system, BOX, RES, level, img_id=IMG, sparse=True, chunk=100, **kw)  # lines in chunks of 100: they straddle bricks
        n = got.n_bricks
        print(f"degree {degree}: {n} of {Bx * By * Bz} bricks occupied (f_b = {got.brick_fraction:.3f}), {int((want.pool.view(-1) != 0).sum())} bytes of the pool set")
        assert 0 < n < Bx * By * Bz and got.sparse and got.sh_degree == degree and got.resolution == RES
        assert torch.equal(got.bricks, want.bricks) and torch.equal(got.slots, want.slots)
        diff = got.pool != want.pool
        if bool(diff.any()):  # which points differ, and by how much
            idx = diff.reshape(diff.shape[0], 9, 9, 9, -1).any(-1).nonzero()
            a, b = got.pool, want.pool
            print(f"degree {degree}: {idx.shape[0]} pool points differ, the first {idx[:8].tolist()}; largest difference "
                  f"{float((a.float() - b.float()).abs().max()):.3e}")
        assert torch.equal(got.pool, want.pool)
        assert torch.equal(got.occupancy.words, want.occupancy.words) and torch.equal(got.occupancy.words, dense.occupancy.words)
        other = BakedScene.build(system, BOX, RES, level, img_id=IMG, sparse=True, **kw)  # one chunk
        assert torch.equal(other.pool, got.pool)


# ---- round trips ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [0, 2])
@pytest.mark.parametrize("name", ["blob", "corners"])
def test_round_trips_through_the_dense_layout_and_a_file(tmp_path, name, degree):
    from upnerf_amd.baked import BakedScene
    scene = dense_scene(name, degree)
    sp = scene.sparsify()
    back = sp.densify()
    assert not back.sparse and back.sh_degree == degree and torch.equal(back.grid, scene.grid)
    assert torch.equal(back.occupancy.words, scene.occupancy.words)
    assert sp.sparsify() is sp and scene.densify() is scene
    path = str(tmp_path / "sparse.npz")
    sp.save(path)
    again = BakedScene.load(path, "cuda")
    assert again.sparse and again.sh_degree == degree and again.resolution == sp.resolution and again.n_bricks == sp.n_bricks
    assert torch.equal(again.pool, sp.pool) and torch.equal(again.bricks, sp.bricks) and torch.equal(again.slots, sp.slots)
    assert torch.equal(again.occupancy.words, sp.occupancy.words) and again.bounds == sp.bounds and again.level == sp.level
    rays = dev(br.make_rays())
    assert same(again.render(rays, 0.05, background=0.5), scene.render(rays, 0.05, background=0.5))
    made = BakedScene.from_bricks(sp.pool.clone(), sp.bricks.clone(), sp.resolution, sp.bounds, sp.level, degree)
    assert torch.equal(made.slots, sp.slots) and same(made.render(rays, 0.05), scene.render(rays, 0.05))
    scene.save(path)  # a dense scene's file still loads as a dense scene
    assert not BakedScene.load(path, "cuda").sparse


SCENE = ((-0.9, -0.8, -4.0), (0.7, 0.9, -1.5))  # a box in front of the cameras of the path below (tests/test_hip_baked.py)


def test_render_path_with_a_sparse_scene_is_its_render_on_the_path_rays(system):
    from upnerf_amd import novel_view as nv
    from upnerf_amd.baked import BakedScene
    rgbs, level = br.blob_grid()
    dense = BakedScene.from_grids(dev(rgbs[..., 3] * 0.1), dev(rgbs[..., :3]), SCENE, level * 0.1)
    scene = BakedScene.from_grids(dev(rgbs[..., 3] * 0.1), dev(rgbs[..., :3]), SCENE, level * 0.1, sparse=True)
    assert scene.sparse and torch.equal(scene.pool, dense.sparsify().pool)
    c = np.cos(0.3), np.sin(0.3)
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2]], [[c[0], 0, c[1], -0.2], [0, 1, 0, 0.1], [-c[1], 0, c[0], 0.0]]])
    K = torch.tensor([[22.0, 0, 11.6], [0, 21.0, 7.8], [0, 0, 1]])
    path = nv.CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], 2, appearance=(1, 4), img_wh=(24, 16), K=K)
    dt = 0.04
    out = nv.render_path(system, path, chunk=100, outputs=("rgb_float",), baked=scene, baked_step=dt)
    poses, nf = nv.path_poses(path.key_c2w.cuda(), path.key_near_far.cuda(), path.u.cuda(), path.mode)
    for f in range(2):
        rays, _ = nv.path_rays(poses, nf, path.img_wh, path.K, f * 384, 384)
        direct = scene.render(rays, dt, background=0.0)
        assert int((direct["opacity"] > 0.05).sum()) > 20 and int((direct["opacity"] == 0).sum()) > 20
        assert torch.equal(out["rgb_float"][f], direct["rgb"]) and same(direct, dense.render(rays, dt, background=0.0)), f
