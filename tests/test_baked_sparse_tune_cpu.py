"""Tuning a sparse baked scene on its pool, without a GPU: the numpy restatement of the face sum (tests/baked_sparse_tune_ref.py)
against the layout's own gather and scatter, a case written out by hand, and the refusals of the two new entry points and of the
Python layer, which are decided on the host (include/upnerf_hip.h; upnerf_amd/baked_sparse_tune.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import baked_sparse_ref as sr
import baked_sparse_tune_ref as ft

EINVAL, EUNSUP = -1, -2
CELLS = [(8, 8, 8), (9, 17, 5), (20, 12, 33)]  # those of tests/test_hip_baked_sparse.py


def _layout(cells, kind):
    Cx, Cy, Cz = cells
    bits = np.ones((Cz, Cy, Cx), bool) if kind == "set" else np.random.RandomState(Cx + Cy).uniform(size=(Cz, Cy, Cx)) < 0.3
    if kind == "holes":  # whole bricks missing: a shared point then has fewer copies than the geometry allows
        bits = ft.holes_bits(cells)
    return sr.table(sr.brick_bits(bits))


@pytest.mark.parametrize("kind", ["set", "seeded", "holes"])
@pytest.mark.parametrize("cells", CELLS)
def test_on_integers_the_face_sum_is_scatter_add_then_gather(cells, kind):
    """Integer-valued fp32 data sums exactly in any order: every copy becomes the sum over the copies, which is what gathering
    the grid of summed copies gives; a point with one copy and a pool point beyond the grid keep their bits."""
    slots, bricks = _layout(cells, kind)
    n = len(bricks)
    rng = np.random.RandomState(n)
    pool = rng.randint(-1000, 1000, (n, 9, 9, 9, 3)).astype(np.float32)
    got = ft.face_sum(pool, slots, cells)
    inside = ft.in_grid(bricks, cells)
    want = sr.gather(ft.scatter_add(pool, slots, cells), bricks).astype(np.float32)
    assert np.array_equal(got[inside], want[inside])
    assert np.array_equal(got[~inside].view(np.uint32), pool[~inside].view(np.uint32))
    shared = np.zeros(inside.shape, bool)
    groups = ft.copy_groups(slots, cells)
    for _, c in groups:
        assert 2 <= len(c) <= 8 and len(set(c)) == len(c)
        for at in c:
            shared[at] = True
    assert np.array_equal(got[~shared].view(np.uint32), pool[~shared].view(np.uint32))  # m = 1: unchanged
    assert not shared[:, 1:8, 1:8, 1:8].any()  # the 343 interior points of a brick are never shared
    if cells == (8, 8, 8):
        assert not groups  # one brick shares nothing
    else:
        assert groups and (got[shared] != pool[shared]).any()
    if kind == "set" and cells == (20, 12, 33):
        assert max(len(c) for _, c in groups) == 8  # a point all eight bricks round it hold
    if kind == "holes" and cells != (8, 8, 8):
        assert any(len(c) < ft.geometric_copies(x, y, z, cells) for (x, y, z), c in groups)


def test_two_bricks_by_hand():
    """16 x 8 x 8 cells: two bricks side by side in x.  Grid plane x = 8 is l = 8 of brick 0 and l = 0 of brick 1."""
    cells = (16, 8, 8)
    slots, bricks = sr.table(np.ones((1, 1, 2), bool))
    assert ft.holders(8, 16) == [(0, 8), (1, 0)] and ft.holders(16, 16) == [(1, 8)] and ft.holders(0, 16) == [(0, 0)] and ft.holders(3, 16) == [(0, 3)]
    assert ft.holders(8, 9) == [(0, 8), (1, 0)] and ft.holders(8, 8) == [(0, 8)]  # a last plane belongs to the last brick alone
    pool = np.zeros((2, 9, 9, 9, 1), np.float32)
    pool[0, :, :, 8, 0] = np.float32(1.0)
    pool[1, :, :, 0, 0] = np.float32(2.0 ** -24)  # 1 + 2^-24 rounds to 1 in fp32: the sum is formed in fp32
    pool[0, 4, 4, 8, 0], pool[1, 4, 4, 0, 0] = np.float32(0.1), np.float32(0.2)
    pool[0, 2, 2, 2, 0] = pool[1, 5, 5, 8, 0] = 7.0  # an interior point and the grid's end: one copy each
    got = ft.face_sum(pool, slots, cells)
    want = pool.copy()
    want[0, :, :, 8, 0] = want[1, :, :, 0, 0] = np.float32(1.0)
    want[0, 4, 4, 8, 0] = want[1, 4, 4, 0, 0] = np.float32(0.1) + np.float32(0.2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the order: three copies whose fp32 sum depends on the bracketing (2 x 2 x 1 bricks, the edge x = 8, y = 8)
    cells = (16, 16, 8)
    slots, bricks = sr.table(np.array([[[True, True], [True, False]]]))  # bricks 0, 1, 2; brick 3 is empty
    pool = np.zeros((3, 9, 9, 9, 1), np.float32)
    a, b, c = np.float32(1.0), np.float32(2.0 ** -24), np.float32(2.0 ** -24)
    pool[0, 3, 8, 8, 0], pool[1, 3, 8, 0, 0], pool[2, 3, 0, 8, 0] = b, c, a  # ascending bricks: (b + c) + a
    got = ft.face_sum(pool, slots, cells)
    assert got[0, 3, 8, 8, 0] == got[1, 3, 8, 0, 0] == got[2, 3, 0, 8, 0] == np.float32(np.float32(b + c) + a)
    assert np.float32(np.float32(b + c) + a) != np.float32(np.float32(a + b) + c)  # (the other bracketing loses both)


# ---- host refusals (the pattern of test_baked_tune_cpu.py: every pointer non-null and never dereferenced) -----------------------------

def _bwd_args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(64)
    a = _lib.BakedSparseRenderBwdArgs(Cx=8, Cy=9, Cz=10, R=67, lo=(ctypes.c_float * 3)(-0.7, -0.5, -0.6), hi=(ctypes.c_float * 3)(0.8, 0.6, 0.9),
                                      step=0.1, background=0.0, stop=0.0, degree=0, pool=one, slots=one, words=one, rays=one, g_rgb=one,
                                      g_depth=None, g_opacity=None, grad=one, grad_coef=one, grad_sigma=one)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BWD_REFUSALS = [
    (dict(slots=None), EINVAL),                                               # the sparse forward's own
    (dict(g_rgb=None), EINVAL), (dict(degree=3), EINVAL), (dict(degree=-1), EINVAL), (dict(step=0.0), EINVAL), (dict(step=-0.1), EINVAL),
    (dict(step=float("nan")), EINVAL), (dict(step=float("inf")), EINVAL), (dict(pool=None), EINVAL), (dict(words=None), EINVAL),
    (dict(rays=None), EINVAL), (dict(rays=ctypes.c_void_p(72)), EINVAL), (dict(R=0), EINVAL), (dict(Cx=0), EINVAL),
    (dict(background=float("nan")), EINVAL), (dict(stop=1.0), EINVAL), (dict(stop=-0.5), EINVAL),
    (dict(hi=(ctypes.c_float * 3)(0.8, -0.5, 0.9)), EINVAL),
    (dict(pool=ctypes.c_void_p(72)), EINVAL),                                 # degree 0: a point is 16 bytes
    (dict(degree=1, pool=ctypes.c_void_p(80)), EINVAL),                       # a record is aligned to its 32 bytes
    (dict(degree=2, pool=ctypes.c_void_p(96)), EINVAL),                       # ... or to its 64
    (dict(grad=None), EINVAL), (dict(degree=1, grad_coef=None), EINVAL), (dict(degree=2, grad_sigma=None), EINVAL),
]


@pytest.mark.parametrize("case,want", BWD_REFUSALS)
def test_sparse_render_bwd_refuses_before_launch(case, want):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_baked_sparse_render_bwd(ctypes.byref(_bwd_args(**case)), None) == want


def _sum_args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(64)
    a = _lib.BrickFaceSumArgs(Cx=9, Cy=17, Cz=5, n_bricks=3, F=4, slots=one, bricks=one, data=one)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


SUM_REFUSALS = [
    (dict(Cx=0), EINVAL), (dict(Cz=-3), EINVAL), (dict(n_bricks=0), EINVAL), (dict(n_bricks=7), EINVAL),  # 2 x 3 x 1 bricks
    (dict(F=0), EINVAL), (dict(F=-1), EINVAL), (dict(slots=None), EINVAL), (dict(bricks=None), EINVAL), (dict(data=None), EINVAL),
    (dict(data=ctypes.c_void_p(66)), EINVAL),
    (dict(Cx=1024, Cy=1024, Cz=1024, n_bricks=2 ** 21, F=2 ** 14), EUNSUP),   # more threads than a launch has
]


@pytest.mark.parametrize("case,want", SUM_REFUSALS)
def test_face_sum_refuses_before_launch(case, want):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_brick_face_sum(ctypes.byref(_sum_args(**case)), None) == want


def test_both_refuse_null():
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_baked_sparse_render_bwd(None, None) == EINVAL
    assert _lib.lib.upnerf_brick_face_sum(None, None) == EINVAL


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------

def test_a_dense_scene_is_refused_with_the_route():
    from upnerf_amd import baked_sparse_tune as st
    from upnerf_amd.baked import BakedScene
    scene = BakedScene.__new__(BakedScene)  # (no pool: a dense scene; nothing else of it is looked at)
    assert not scene.sparse
    for make in (lambda: st.PoolParams.of(scene), lambda: st.PoolTuner(scene, 1e-2), lambda: scene.tune_pool(1e-2),
                 lambda: st.distill(None, scene, [0, 1], 1, 1, 0.1), lambda: st.face_sum(None, scene)):
        with pytest.raises(ValueError) as e:
            make()
        assert "sparsify()" in str(e.value) and "baked_tune" in str(e.value)
    with pytest.raises(ValueError):
        st.PoolParams.of(object())
    with pytest.raises(ValueError):
        st.render(object(), None, 0.1)


def _render_path_tool():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import render_path
    return render_path


BASE = ["--config", "c.yaml", "--ckpt", "c.ckpt", "--images", "0", "1", "--frames", "2", "--out", "o"]
BAKED = ["--baked", "9", "9", "9", "--level", "1.0", "--step", "0.1"]


@pytest.mark.parametrize("extra", [[], ["--baked-sparse"], ["--baked-tune", "3"], ["--load-baked", "f.npz", "--step", "0.1"]])
def test_tune_pool_flag_needs_a_sparse_bake_that_is_tuned(extra):
    tool = _render_path_tool()
    argv = BASE + (extra if "--load-baked" in extra else BAKED + extra) + ["--baked-tune-pool"]
    with pytest.raises(SystemExit) as e:
        tool.check_args(tool.parser().parse_args(argv))
    assert "--baked-tune-pool" in str(e.value) and "--baked-sparse" in str(e.value) and "--baked-tune" in str(e.value)


def test_tune_pool_flag_is_accepted_with_both_and_off_by_default():
    tool = _render_path_tool()
    a = tool.check_args(tool.parser().parse_args(BASE + BAKED + ["--baked-sparse", "--baked-tune", "3", "--baked-tune-pool"]))
    assert a.baked_tune_pool is True
    b = tool.check_args(tool.parser().parse_args(BASE + BAKED + ["--baked-sparse", "--baked-tune", "3"]))
    assert b.baked_tune_pool is False
