"""Depth-map fusion without a GPU: the host-side refusals of upnerf_tsdf_* and of the mesher's new flag (dummy non-null pointers,
never dereferenced: every case is refused before a launch), the
Python wrappers' refusal of CPU tensors, the command line of tools/extract_mesh.py, and the fp64 restatement (tests/tsdf_ref.py)
against the example its docstring works by hand."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import tsdf_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONE = C.c_void_p(16)


def integrate_args(views=1, view_kw=None, **kw):
    from upnerf_amd import _lib
    a = _lib.TsdfIntegrateArgs(Nx=4, Ny=5, Nz=6, n_views=views, lo=(C.c_float * 3)(-1, -1, -1), hi=(C.c_float * 3)(1, 1, 1),
                               trunc=0.25, min_opacity=0.5, weight_mode=0, tsdf=ONE, weight=ONE, rgb=ONE, rgb_weight=ONE)
    for k in range(min(max(views, 0), _lib.TSDF_MAX_VIEWS)):
        a.views[k] = _lib.TsdfView(fx=10, fy=10, cx=4, cy=3, W=8, H=6, depth=ONE, opacity=ONE, rgb=ONE)
    for k, v in (view_kw or {}).items():
        setattr(a.views[max(views, 1) - 1], k, v)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


INTEGRATE_REFUSALS = [
    dict(tsdf=None), dict(weight=None), dict(rgb_weight=None),                       # null pointers (rgb without its weight)
    dict(views=0), dict(views=-1), dict(views=9),                                    # n_views outside [1, MAX]
    dict(trunc=0.0), dict(trunc=-0.25), dict(trunc=float("inf")), dict(trunc=float("nan")),
    dict(min_opacity=float("nan")), dict(weight_mode=2), dict(weight_mode=-1),
    dict(Nx=1), dict(Ny=1), dict(Nz=1), dict(Nx=0),                                  # an axis < 2
    dict(Nx=2048, Ny=2048, Nz=512), dict(Nx=65536, Ny=65536, Nz=2),                  # Nx Ny Nz = 2^31, Nx Ny = 2^32
    dict(hi=(C.c_float * 3)(1, -1, 1)), dict(hi=(C.c_float * 3)(1, 1, -1.5)),        # hi <= lo
    dict(lo=(C.c_float * 3)(float("nan"), -1, -1)), dict(hi=(C.c_float * 3)(1, float("inf"), 1)),
    dict(view_kw=dict(depth=None)), dict(views=3, view_kw=dict(depth=None)),         # the last of three views without a map
    dict(view_kw=dict(W=0)), dict(view_kw=dict(H=0)), dict(view_kw=dict(W=65536, H=32768)),
    dict(weight_mode=1, view_kw=dict(opacity=None)),                                 # opacity weights without the map
]


@pytest.mark.parametrize("case", INTEGRATE_REFUSALS, ids=lambda c: ",".join(c))
def test_integrate_refuses_before_launch(case):
    from upnerf_amd import _lib
    assert _lib.TSDF_MAX_VIEWS == 8
    assert _lib.lib.upnerf_tsdf_integrate(C.byref(integrate_args(**case)), None) == EINVAL
    assert _lib.lib.upnerf_tsdf_integrate(None, None) == EINVAL


def test_surface_and_sample_refuse_before_launch():
    from upnerf_amd import _lib
    surf = lambda **kw: _lib.TsdfSurfaceArgs(**{**dict(n=100, min_weight=1.0, tsdf=ONE, weight=ONE, out=ONE), **kw})
    for kw in (dict(tsdf=None), dict(weight=None), dict(out=None), dict(n=0), dict(n=2 ** 31), dict(min_weight=float("nan"))):
        assert _lib.lib.upnerf_tsdf_surface(C.byref(surf(**kw)), None) == EINVAL, kw
    assert _lib.lib.upnerf_tsdf_surface(None, None) == EINVAL
    samp = lambda **kw: _lib.TsdfSampleArgs(**{**dict(Nx=4, Ny=5, Nz=6, V=3, lo=(C.c_float * 3)(-1, -1, -1), hi=(C.c_float * 3)(1, 1, 1),
                                                    rgb=ONE, rgb_weight=ONE, points=ONE, out=ONE), **kw})
    for kw in (dict(rgb=None), dict(rgb_weight=None), dict(points=None), dict(out=None), dict(V=0), dict(Nz=1),
               dict(Nx=2048, Ny=2048, Nz=512), dict(hi=(C.c_float * 3)(-1, 1, 1))):
        assert _lib.lib.upnerf_tsdf_sample(C.byref(samp(**kw)), None) == EINVAL, kw
    assert _lib.lib.upnerf_tsdf_sample(None, None) == EINVAL


def test_mesher_refuses_an_unknown_flag():
    from upnerf_amd import _lib, geometry
    assert _lib.MTET_SKIP_NONFINITE == 1
    a = _lib.MtetArgs(Nx=4, Ny=4, Nz=4, level=0.5, grid=ONE, tab=geometry._tables(), flags=2)
    assert _lib.lib.upnerf_mtet_count(C.byref(a), ONE, ONE, None) == EINVAL
    a.lo, a.hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    assert _lib.lib.upnerf_mtet_emit(C.byref(a), ONE, None) == EINVAL


def test_python_wrappers_refuse_cpu_tensors():
    from upnerf_amd import geometry
    box = ((0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError):
        geometry.TsdfVolume(box, (4, 4, 4), 0.1, device="cpu")
    with pytest.raises(RuntimeError):
        geometry.extract_surface(torch.zeros(2, 2, 2), box, 0.0, observed_only=True)
    vol = object.__new__(geometry.TsdfVolume)  # a volume cannot be made without a device: its fields by hand, on the CPU
    vol.bounds, vol.resolution, vol.trunc, vol.n_views = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (4, 4, 4), 0.1, 0
    vol.tsdf, vol.weight = torch.ones(4, 4, 4), torch.zeros(4, 4, 4)
    vol.rgb, vol.rgb_weight = torch.zeros(4, 4, 4, 3), torch.zeros(4, 4, 4)
    pose = torch.eye(4)[:3]
    with pytest.raises(RuntimeError):
        vol.integrate(torch.ones(12), pose, (2.0, 2.0, 1.5, 1.0), (4, 3))
    with pytest.raises(RuntimeError):
        vol.sample_colour(torch.zeros(5, 3))
    with pytest.raises(RuntimeError):
        vol.surface_grid()
    with pytest.raises(ValueError):
        vol.integrate(torch.ones(12), pose, (2.0, 2.0, 1.5, 1.0), (4, 3), weight_mode="mean")
    with pytest.raises(ValueError):
        geometry.TsdfVolume(box, (4, 1, 4), 0.1)  # (refused before the device is asked for)


def test_extract_mesh_takes_exactly_one_of_level_and_fuse_depth(tmp_path):
    spec = importlib.util.spec_from_file_location("extract_mesh_tool_tsdf", os.path.join(ROOT, "tools", "extract_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--ckpt", "x.ckpt", "--out", str(tmp_path / "o.ply"), "--bounds", "0", "0", "0", "1", "1", "1"]
    a = tool.parser().parse_args(base + ["--fuse-depth", "--images", "0", "3", "--trunc", "0.2", "--downscale", "4", "--min-weight", "2"])
    assert a.fuse_depth and a.level is None and a.images == [0, 3] and a.trunc == 0.2 and a.downscale == 4 and a.min_weight == 2.0
    d = tool.parser().parse_args(base + ["--fuse-depth"])
    assert d.images is None and d.trunc is None and d.downscale == 1 and d.min_weight == 1.0
    with pytest.raises(SystemExit):
        tool.parser().parse_args(base + ["--fuse-depth", "--level", "3"])
    with pytest.raises(SystemExit):
        tool.parser().parse_args(base)


def test_reference_reproduces_the_hand_worked_example():
    pose = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.0]])
    v1 = tr.make_view(pose, 2, 2, 1, 1, 3, 3, np.full(9, 1.5), rgb=np.tile([1, 0, 0.5], (9, 1)))
    v2 = tr.make_view(pose, 2, 2, 1, 1, 3, 3, np.full(9, 1.75), rgb=np.tile([0, 1, 0.5], (9, 1)))
    P = np.array([[0, 0, 0.5], [0, 0, 1.25], [0, 0, -0.25]])
    s = tr.new_state(3)
    rep = tr.integrate_points(P, s, [v1, v2], 0.5)
    assert s["tsdf"].tolist() == [0.25, 1.0, -1.0]
    assert s["weight"].tolist() == [2.0, 2.0, 1.0] and s["weight"].dtype == np.float32
    assert s["rgb"].tolist() == [[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.0, 1.0, 0.5]]
    assert s["rgb_weight"].tolist() == [2.0, 0.0, 1.0]
    assert rep[0]["branch"].tolist() == [tr.UPDATED, tr.UPDATED, tr.BEHIND_BAND] and rep[1]["branch"].tolist() == [tr.UPDATED] * 3
    assert rep[0]["sdf"].tolist() == [0.0, 0.75, -0.75] and rep[1]["coloured"].tolist() == [True, False, True]
    # the other ways out: a point behind the camera, one outside the image, a pixel without depth, one with too little opacity
    v3 = tr.make_view(pose, 2, 2, 1, 1, 3, 3, [1.5, np.nan, 1.5, 0.0, 1.5, 1.5, 1.5, 1.5, 1.5], opacity=[1, 1, 1, 1, 0.4, 1, 1, 1, 1])
    Q = np.array([[0, 0, 2.5], [3.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 0, 0.5]])  # pixels: -, outside, (1, 0), (0, 1), (1, 1)
    s = tr.new_state(5, colour=False)
    rep = tr.integrate_points(Q, s, [v3], 0.5)
    assert rep[0]["branch"].tolist() == [tr.BEHIND, tr.OUTSIDE, tr.NO_DEPTH, tr.NO_DEPTH, tr.LOW_OPACITY]
    assert s["weight"].tolist() == [0.0] * 5 and s["tsdf"].tolist() == [1.0] * 5
    # and the opacity as the weight: 0.75 then 0.25 -> T = 0 then 0 + (0.5 - 0) * 0.25 / 1 = 0.125
    o1 = dict(v1, opacity=np.full(9, 0.75, np.float32))
    o2 = dict(v2, opacity=np.full(9, 0.25, np.float32))
    s = tr.new_state(1)
    tr.integrate_points(P[:1], s, [o1, o2], 0.5, min_opacity=0.1, weight_mode="opacity")
    assert s["tsdf"].tolist() == [0.125] and s["weight"].tolist() == [1.0] and s["rgb"][0].tolist() == [0.75, 0.25, 0.5]
