"""Camera paths without a GPU: the host plan of a path (which frame sits where and blends which images), and the host-side
refusals of the two path entry points (nothing is launched)."""
import ctypes

import numpy as np
import pytest

ONE = ctypes.c_void_p(16)  # non-null, never dereferenced: every call below is refused on the host


@pytest.mark.parametrize("ids,n_frames,loop", [([3, 17, 42], 7, False), ([3, 17, 42], 120, False), ([5, 2], 4, False),
                                               ([3, 17, 42], 10, True), ([4, 1, 0, 2], 13, True)])
def test_plan_follows_the_keyframes(ids, n_frames, loop):
    from upnerf_amd.novel_view import plan_path
    u, i0, i1, t = (x.numpy() for x in plan_path(n_frames, img_ids=ids, loop=loop))
    keys = ids + ids[:1] if loop else ids
    K = len(keys)
    assert u.dtype == np.float32 and t.dtype == np.float32 and i0.dtype == np.int32 and i1.dtype == np.int32
    assert u.shape == i0.shape == i1.shape == t.shape == (n_frames,)
    assert u[0] == 0 and u[-1] == K - 1
    assert np.all(np.diff(u) > 0)
    np.testing.assert_allclose(np.diff(u.astype(np.float64)), (K - 1) / (n_frames - 1), rtol=0, atol=K * 2.0 ** -23)
    on_key = u == np.floor(u)
    assert on_key[0] and on_key[-1]
    for f in np.nonzero(on_key)[0]:
        assert t[f] == 0 and i0[f] == keys[int(u[f])]
    for f in range(n_frames):
        k = min(int(np.floor(u[f])), K - 1)
        assert i0[f] == keys[k] and i1[f] == keys[min(k + 1, K - 1)]
        assert t[f] == np.float32(np.float64(u[f]) - k) and 0 <= t[f] < 1
    if loop:
        assert i0[-1] == ids[0]


def test_plan_accepts_one_frame():
    from upnerf_amd.novel_view import plan_path
    u, i0, i1, t = plan_path(1, img_ids=[3, 17])
    assert u.tolist() == [0.0] and t.tolist() == [0.0] and i0.tolist() == [3]
    u, i0, i1, t = plan_path(1, n_keys=3, appearance=(4, 5))
    assert u.tolist() == [0.0] and t.tolist() == [0.0] and (i0.tolist(), i1.tolist()) == ([4], [5])


def test_plan_of_free_poses_blends_once_over_the_whole_path():
    from upnerf_amd.novel_view import plan_path
    u, i0, i1, t = (x.numpy() for x in plan_path(9, n_keys=4, appearance=(2, 5)))
    assert u[0] == 0 and u[-1] == 3
    assert np.all(i0 == 2) and np.all(i1 == 5)
    assert t[0] == 0 and t[-1] == 1
    np.testing.assert_array_equal(t, (np.arange(9) / 8).astype(np.float32))  # eighths are exact
    _, a0, a1, _ = plan_path(5, n_keys=2, appearance=(3, 3))
    assert a0.tolist() == a1.tolist() == [3] * 5


def test_plan_refuses_what_is_not_a_path():
    from upnerf_amd.novel_view import plan_path
    for kw in (dict(n_frames=0, img_ids=[1, 2]), dict(n_frames=3, img_ids=[1]), dict(n_frames=3),
               dict(n_frames=3, img_ids=[1, 2], appearance=(0, 1)), dict(n_frames=3, appearance=(0, 1)),
               dict(n_frames=3, n_keys=1, appearance=(0, 1))):
        with pytest.raises(ValueError):
            plan_path(**kw)


def test_camera_path_from_poses_holds_host_tensors():
    import torch
    from upnerf_amd.novel_view import CameraPath
    c2w = torch.eye(3, 4).repeat(3, 1, 1)
    p = CameraPath.from_poses(c2w, (0.1, 5.0), 5, appearance=(1, 2), img_wh=(8, 6), K=np.array([[7.0, 0, 4], [0, 9, 3], [0, 0, 1]]))
    assert p.n_frames == 5 and tuple(p.key_near_far.shape) == (3, 2) and p.img_wh == (8, 6) and p.mode == "catmull"
    assert not p.key_c2w.is_cuda and p.i0.dtype == torch.int32 and float(p.K[1, 1]) == 9.0
    with pytest.raises(ValueError):
        CameraPath.from_poses(c2w, (0.1, 5.0), 5, appearance=(1, 2), img_wh=(8, 6), K=np.eye(3), mode="bezier")


def _poses_args(**kw):
    from upnerf_amd import _lib
    a = _lib.PathPosesArgs(K=4, F=8, mode=_lib.PATH_CATMULL, key_c2w=ONE, key_nf=ONE, u=ONE, c2w=ONE, nf=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _rays_args(n_tables=2, dims=(48, 16), **kw):
    from upnerf_amd import _lib
    a = _lib.PathRaysArgs(F=3, H=5, W=7, n_tables=n_tables, row0=30, R=50, fx=9.0, fy=8.0, cx=3.3, cy=2.2, c2w=ONE, nf=ONE, i0=ONE,
                          i1=ONE, t=ONE, rays=ONE)
    for j in range(min(n_tables, _lib.PATH_MAX_TABLES)):
        a.tables[j] = _lib.PathTable(table=ONE, dim=dims[j % len(dims)], n_rows=6, out=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw", [dict(K=1), dict(K=0), dict(F=0), dict(mode=2), dict(mode=-1), dict(key_c2w=None), dict(key_nf=None),
                                dict(u=None), dict(c2w=None), dict(nf=None)])
def test_path_poses_refuses_before_launch(kw):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_path_poses(ctypes.byref(_poses_args(**kw)), None) == -1
    assert _lib.lib.upnerf_path_poses(None, None) == -1


@pytest.mark.parametrize("build", [
    lambda: _rays_args(n_tables=5), lambda: _rays_args(dims=(65, 16)), lambda: _rays_args(dims=(48, 0)), lambda: _rays_args(R=0),
    lambda: _rays_args(n_tables=-1), lambda: _rays_args(row0=-1), lambda: _rays_args(row0=56), lambda: _rays_args(F=0),
    lambda: _rays_args(H=0), lambda: _rays_args(W=0), lambda: _rays_args(fx=0.0), lambda: _rays_args(fy=float("nan")),
    lambda: _rays_args(rays=None), lambda: _rays_args(c2w=None), lambda: _rays_args(nf=None), lambda: _rays_args(i0=None),
    lambda: _rays_args(t=None),
])
def test_path_rays_refuses_before_launch(build):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_path_rays(ctypes.byref(build()), None) == -1
    assert _lib.lib.upnerf_path_rays(None, None) == -1


def test_path_rays_refuses_a_table_without_memory():
    from upnerf_amd import _lib
    a = _rays_args()
    a.tables[1].out = None
    assert _lib.lib.upnerf_path_rays(ctypes.byref(a), None) == -1
    a = _rays_args()
    a.tables[0].n_rows = 0
    assert _lib.lib.upnerf_path_rays(ctypes.byref(a), None) == -1


def test_render_rays_documents_the_embed_rows_keyword():
    from upnerf_amd import rendering
    assert 'kwargs["embed_rows"]' in rendering.render_rays.__doc__
