"""A sparse baked scene without a GPU: the invariants of the layout's numpy restatement (tests/baked_sparse_ref.py), every host
refusal of the six entry points (non-null, never-dereferenced pointers, as tests/test_abi_cpu.py has them), the refusals of
BakedScene.from_bricks, and the files (save_bricks / load_bricks beside save_arrays / load_arrays, whose key sets stay apart)."""
import ctypes

import numpy as np
import pytest
import torch

import baked_ref as br
import baked_sparse_ref as sr

EINVAL, EUNSUP = -1, -2
ONE = ctypes.c_void_p(64)  # (non-null, aligned to every record size, never dereferenced on the host)
ODD = ctypes.c_void_p(72)  # aligned to 8 only
CASES = [((8, 8, 8), "one brick"), ((9, 17, 5), "ragged on every axis"), ((20, 12, 33), "five bricks along z")]


def random_cells(cells, share, seed):
    Cx, Cy, Cz = cells
    return np.random.RandomState(seed).uniform(size=(Cz, Cy, Cx)) < share


@pytest.mark.parametrize("cells", [c for c, _ in CASES])
@pytest.mark.parametrize("E", [4, 16, 64])
def test_gather_then_scatter_is_the_identity_and_the_pool_is_what_the_layout_says(cells, E):
    Cx, Cy, Cz = cells
    rng = np.random.RandomState(E + Cx)
    bits = sr.brick_bits(random_cells(cells, 0.02, 3))
    slots, bricks = sr.table(bits)
    Bx, By, Bz = sr.brick_dims(cells)
    assert 0 < len(bricks) and slots.shape == (Bz, By, Bx) and (np.diff(bricks) > 0).all()
    assert (slots.reshape(-1)[bricks] == np.arange(len(bricks))).all() and (slots >= 0).sum() == len(bricks)
    grid = sr.zero_outside(rng.randint(1, 256, (Cz + 1, Cy + 1, Cx + 1, E)).astype(np.uint8), bits)
    pool = sr.gather(grid, bricks)
    assert pool.shape == (len(bricks), 9, 9, 9, E)
    assert (sr.scatter(pool, bricks, (Cx + 1, Cy + 1, Cz + 1)) == grid).all()
    for s, b in enumerate(bricks):
        bx, by, bz = b % Bx, (b // Bx) % By, b // (Bx * By)
        # ragged bricks are zero outside the grid, and hold the grid's bytes (none of them zero where the owner is occupied) inside
        inside = np.ix_(np.arange(9) + 8 * bz <= Cz, np.arange(9) + 8 * by <= Cy, np.arange(9) + 8 * bx <= Cx)
        mask = np.zeros((9, 9, 9), bool)
        mask[inside] = True
        assert (pool[s][~mask] == 0).all()
        # faces that bricks share are stored once per brick with identical bytes
        if bx + 1 < Bx and slots[bz, by, bx + 1] >= 0:
            assert (pool[s][:, :, 8] == pool[slots[bz, by, bx + 1]][:, :, 0]).all()
        if by + 1 < By and slots[bz, by + 1, bx] >= 0:
            assert (pool[s][:, 8] == pool[slots[bz, by + 1, bx]][:, 0]).all()
        if bz + 1 < Bz and slots[bz + 1, by, bx] >= 0:
            assert (pool[s][8] == pool[slots[bz + 1, by, bx]][0]).all()


@pytest.mark.parametrize("name", ["blob", "corners"])
def test_the_bits_from_the_pool_are_the_bits_of_the_dense_sigma(name):
    rgbs, _ = {"blob": br.blob_grid, "corners": br.corner_grid}[name]()
    sigma = rgbs[..., 3]
    cells = sr.dense_cell_bits(sigma)
    assert (cells == br.occupied_cells(rgbs)).all() and 0 < cells.mean() < 1
    slots, bricks = sr.table(sr.brick_bits(cells))
    pool = sr.gather(rgbs, bricks)
    assert (sr.cell_bits(pool[..., 3], slots, cells.shape[::-1]) == cells).all()
    # no kept point is lost: the dense grid comes back whole
    assert (sr.scatter(pool, bricks, sigma.shape[::-1]) == rgbs).all()
    w = sr.words(cells)
    assert w.dtype == np.uint32 and w.size == (cells.size + 31) // 32 + (np.prod(sr.brick_dims(cells.shape[::-1])) + 31) // 32


# ---- host refusals --------------------------------------------------------------------------------------------------------------

def _table(**kw):
    from upnerf_amd import _lib
    return _lib.BrickTableArgs(**{**dict(Cx=9, Cy=17, Cz=5, words=ONE, slots=ONE, bricks=ONE, count=ONE, scratch=ONE), **kw})


def _copy(cls, **kw):
    return cls(**{**dict(Cx=9, Cy=17, Cz=5, n_bricks=3, E=16, bricks=ONE, grid=ONE, pool=ONE), **kw})


def _occ(**kw):
    from upnerf_amd import _lib
    return _lib.BrickOccArgs(**{**dict(Cx=9, Cy=17, Cz=5, n_bricks=3, E=16, sigma_offset=12, slots=ONE, pool=ONE, words=ONE), **kw})


def _columns(**kw):
    from upnerf_amd import _lib
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    return _lib.BrickColumnsArgs(**{**dict(Nx=10, Ny=18, Nz=6, S=32, lo=f3(0, 0, 0), hi=f3(1, 1, 1), line0=0, count=81, n_bricks=3,
                                           bricks=ONE, o=ONE, d=ONE, z=ONE), **kw})


def _render(**kw):
    from upnerf_amd import _lib
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    return _lib.BakedSparseRenderArgs(**{**dict(Cx=9, Cy=17, Cz=5, R=4, lo=f3(0, 0, 0), hi=f3(1, 1, 1), step=0.1, background=0.0,
                                                stop=0.0, degree=0, pool=ONE, slots=ONE, words=ONE, rays=ONE, rgb=ONE, depth=ONE,
                                                opacity=ONE), **kw})


def test_table_refusals():
    from upnerf_amd._lib import lib
    assert lib.upnerf_brick_table(None, None) == EINVAL
    for kw in (dict(Cx=0), dict(Cz=-1), dict(words=None), dict(slots=None), dict(bricks=None), dict(count=None), dict(scratch=None),
               dict(scratch=ODD)):
        assert lib.upnerf_brick_table(ctypes.byref(_table(**kw)), None) == EINVAL, kw
    assert lib.upnerf_brick_table_scratch(0, 4, 4) == EINVAL and lib.upnerf_brick_table_scratch(4, 4, -3) == EINVAL
    # a byte per brick and the levels of its scan, each rounded up to 16 bytes
    assert lib.upnerf_brick_table_scratch(9, 17, 5) == 16 + 16 and lib.upnerf_brick_table_scratch(256, 256, 256) == 32768 + 32 * 4 + 16


@pytest.mark.parametrize("which", ["gather", "scatter"])
def test_gather_and_scatter_refusals(which):
    from upnerf_amd import _lib
    fn, cls = ((_lib.lib.upnerf_brick_gather, _lib.BrickGatherArgs) if which == "gather" else
               (_lib.lib.upnerf_brick_scatter, _lib.BrickScatterArgs))
    assert fn(None, None) == EINVAL
    for kw in (dict(Cy=0), dict(E=0), dict(E=8), dict(E=12), dict(E=128), dict(n_bricks=0), dict(n_bricks=7),  # 2 x 3 x 1 = 6 bricks
               dict(bricks=None), dict(grid=None), dict(pool=None), dict(E=32, pool=ctypes.c_void_p(48)), dict(E=64, pool=ctypes.c_void_p(96)),
               dict(pool=ODD), dict(grid=ODD), dict(E=4, pool=ctypes.c_void_p(66))):
        assert fn(ctypes.byref(_copy(cls, **kw)), None) == EINVAL, kw


def test_occ_refusals():
    from upnerf_amd._lib import lib
    assert lib.upnerf_brick_occ(None, None) == EINVAL
    for kw in (dict(Cx=0), dict(E=8), dict(E=0), dict(sigma_offset=-4), dict(sigma_offset=13), dict(sigma_offset=16), dict(n_bricks=-1),
               dict(n_bricks=7), dict(slots=None), dict(words=None), dict(pool=None), dict(pool=ODD), dict(E=64, sigma_offset=56, pool=ctypes.c_void_p(96))):
        assert lib.upnerf_brick_occ(ctypes.byref(_occ(**kw)), None) == EINVAL, kw


def test_columns_refusals():
    from upnerf_amd._lib import lib
    assert lib.upnerf_brick_columns(None, None) == EINVAL
    nan = (ctypes.c_float * 3)(0, float("nan"), 0)
    for kw in (dict(Nx=1), dict(Nz=0), dict(S=31), dict(S=9), dict(count=0), dict(count=-5), dict(line0=-1), dict(n_bricks=0), dict(n_bricks=7),
               dict(line0=200, count=44), dict(bricks=None), dict(o=None), dict(d=None), dict(z=None), dict(lo=nan), dict(hi=nan)):
        assert lib.upnerf_brick_columns(ctypes.byref(_columns(**kw)), None) == EINVAL, kw


def test_sparse_render_refusals():
    from upnerf_amd._lib import lib
    assert lib.upnerf_baked_sparse_render(None, None) == EINVAL
    f3 = lambda *v: (ctypes.c_float * 3)(*v)
    for kw in (dict(degree=3), dict(degree=-1), dict(Cx=0), dict(R=0), dict(pool=None), dict(slots=None), dict(words=None), dict(rays=None),
               dict(rgb=None), dict(depth=None), dict(opacity=None), dict(pool=ODD), dict(degree=1, pool=ctypes.c_void_p(48)),
               dict(degree=2, pool=ctypes.c_void_p(96)), dict(rays=ODD), dict(step=0.0), dict(step=float("inf")), dict(stop=1.0),
               dict(background=float("nan")), dict(hi=f3(1, 0, 1))):
        assert lib.upnerf_baked_sparse_render(ctypes.byref(_render(**kw)), None) == EINVAL, kw


# ---- from_bricks and the files -------------------------------------------------------------------------------------------------

RES = (10, 18, 6)  # 9 x 17 x 5 cells: 2 x 3 x 1 bricks


def test_from_bricks_refuses_what_is_not_a_pool_and_its_table():
    from upnerf_amd.baked import BakedScene
    pool = torch.zeros(2, 9, 9, 9, 4)
    bricks = torch.tensor([1, 4], dtype=torch.int32)
    make = lambda p=pool, b=bricks, res=RES, deg=0: BakedScene.from_bricks(p, b, res, br.BOUNDS, 1.0, deg)
    rec = lambda E: torch.zeros(2, 9, 9, 9, E, dtype=torch.uint8)
    for kw in (dict(deg=3), dict(deg=-1), dict(deg=1.5),
               dict(p=pool.double()), dict(p=rec(16)), dict(p=pool[..., :3]), dict(p=pool[:, :8]), dict(p=pool.reshape(2, 729, 4)),
               dict(p=torch.zeros(2, 9, 9, 9, 8)[..., ::2]),                                   # not contiguous
               dict(p=rec(32), deg=2), dict(p=rec(64), deg=1), dict(p=pool, deg=1),
               dict(b=bricks.long()), dict(b=bricks[:1]), dict(b=torch.tensor([4, 1], dtype=torch.int32)),
               dict(b=torch.tensor([1, 1], dtype=torch.int32)), dict(b=torch.tensor([1, 6], dtype=torch.int32)),
               dict(b=torch.tensor([-1, 2], dtype=torch.int32)), dict(res=(10, 18, 1)), dict(res=(10, 18))):
        with pytest.raises(ValueError):
            make(**kw)
    for E, deg in ((16, 0), (32, 1), (64, 2)):  # a pool that is not aligned to its point
        spare = torch.zeros(2 * 729 * E + 2 * E, dtype=torch.uint8)
        off = -spare.data_ptr() % E + E // 2
        odd = spare[off:off + 2 * 729 * E].view(2, 9, 9, 9, E)
        assert odd.data_ptr() % E == E // 2
        with pytest.raises(ValueError, match="aligned"):
            make(p=odd.view(torch.float32) if deg == 0 else odd, deg=deg)
    with pytest.raises(RuntimeError):  # everything in order but the device: there is no CPU path
        make()


def _arrays(deg=0, n=2):
    rng = np.random.RandomState(deg)
    pool = rng.uniform(size=(n, 9, 9, 9, 4)).astype(np.float32) if deg == 0 else rng.randint(0, 256, (n, 9, 9, 9, 32 * deg)).astype(np.uint8)
    return pool, np.array([1, 4][:n], np.int32)


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_save_bricks_and_load_bricks_round_trip(tmp_path, deg):
    from upnerf_amd.baked import load_arrays, load_bricks, save_bricks
    pool, bricks = _arrays(deg)
    path = str(tmp_path / "sparse.npz")
    save_bricks(path, pool, bricks, RES, br.BOUNDS, 1.5, sh_degree=deg)
    with np.load(path) as f:
        assert set(f.files) == {"pool", "bricks", "resolution", "degree", "bounds", "level"}
    p, b, res, bounds, level, degree = load_bricks(path)
    assert p.dtype == pool.dtype and (p == pool).all() and b.dtype == np.int32 and (b == bricks).all()
    assert res == RES and bounds == br.BOUNDS and level == 1.5 and degree == deg
    with pytest.raises(ValueError):
        load_arrays(path)  # the dense loader keeps its two key sets
    save_bricks(path, pool[:0], bricks[:0], RES, br.BOUNDS, 1.5, sh_degree=deg)  # a scene without a brick is a scene
    assert load_bricks(path)[0].shape[0] == 0


def test_save_bricks_and_load_bricks_refuse_anything_else(tmp_path):
    from upnerf_amd.baked import load_bricks, save_arrays, save_bricks
    pool, bricks = _arrays(0)
    path = str(tmp_path / "x.npz")
    for kw in (dict(pool=pool.astype(np.float64)), dict(pool=pool[..., :3]), dict(pool=_arrays(1)[0]), dict(bricks=bricks.astype(np.int64)),
               dict(bricks=bricks[::-1]), dict(bricks=np.array([1, 1], np.int32)), dict(bricks=np.array([1, 6], np.int32)),
               dict(bricks=bricks[:1]), dict(resolution=(10, 18)), dict(resolution=(10, 1, 6)), dict(sh_degree=3), dict(sh_degree=1)):
        a = {**dict(pool=pool, bricks=bricks, resolution=RES, sh_degree=0), **kw}
        with pytest.raises(ValueError):
            save_bricks(path, a["pool"], a["bricks"], a["resolution"], br.BOUNDS, 1.0, sh_degree=a["sh_degree"])
    with pytest.raises(ValueError):
        save_bricks(path, pool, bricks, RES, ((0, 0, 0), (1, 0, 1)), 1.0)
    good = dict(pool=pool, bricks=bricks, resolution=np.asarray(RES, np.int64), degree=np.int64(0),
                bounds=np.asarray(br.BOUNDS, np.float64), level=np.float64(1.0))

    def write(**kw):
        with open(path, "wb") as fh:
            np.savez(fh, **kw)
    write(**good)
    assert load_bricks(path)[2] == RES
    for kw in (dict(degree=np.int64(3)), dict(degree=np.int64(1)), dict(resolution=np.asarray((10, 18, 7), np.int64)[:2]),
               dict(resolution=np.asarray((4, 4, 4), np.int64)),  # one brick: brick 4 is out of range
               dict(bounds=np.zeros((3, 2))), dict(bricks=bricks.astype(np.int64)), dict(pool=pool[:1]), dict(extra=np.zeros(1))):
        write(**{**good, **kw})
        with pytest.raises(ValueError):
            load_bricks(path)
    write(**{k: v for k, v in good.items() if k != "level"})
    with pytest.raises(ValueError):
        load_bricks(path)
    save_arrays(path, np.zeros((3, 3, 3, 4), np.float32), br.BOUNDS, 1.0)  # a dense scene's file is not a sparse scene's
    with pytest.raises(ValueError):
        load_bricks(path)
