"""The baked scene without a GPU: the fp64 restatement (tests/baked_ref.py) against closed forms, the host-side refusals of
upnerf_baked_render / upnerf_baked_pack and of the Python surface, and the arrays of
a saved scene."""
import ctypes
import os

import numpy as np
import pytest

import baked_ref as br



def constant_box(sigma, colour, shape=(6, 7, 8)):
    """rgbs of a grid that holds `sigma` and `colour` at EVERY point, the boundary included: a box of constant density."""
    s = np.full(shape, sigma, np.float32)
    c = np.broadcast_to(np.asarray(colour, np.float32), shape + (3,))
    return br.prune(s, c, 0.0)


@pytest.mark.parametrize("background", [0.0, 1.0])
@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_a_box_of_constant_density_has_a_closed_form(background, scale):
    sigma, colour, step = 1.7, (0.2, 0.5, 0.9), 0.013 / scale  # (the step is in units of t)
    rgbs = constant_box(sigma, colour)
    lo, hi = br.bounds64(br.BOUNDS)
    d = np.array([0.6, -0.3, 0.74]) * scale
    rays = np.array([list(((lo + hi) / 2) - 1.1 * d / scale) + list(d) + [0.0, 3.0 / scale],
                     [lo[0] - 0.4, 0.01, 0.02, scale, 0, 0, 0.1 / scale, 2.4 / scale]], np.float32)
    out = br.render(rgbs, br.BOUNDS, rays, step, background)
    length = np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1)
    n = out["inside"]
    assert (n > 50).all()
    want = 1 - np.exp(-float(np.float32(sigma)) * float(np.float32(step)) * length * n)
    assert np.abs(out["opacity"] - want).max() < 1e-12
    c = np.asarray(colour, np.float32).astype(np.float64)
    assert np.abs(out["rgb"] - (want[:, None] * c + (1 - want[:, None]) * background)).max() < 1e-12
    # the box is as long as the samples say: n step |d| within one step of the chord of the axis-parallel ray
    assert abs(n[1] * float(np.float32(step)) * length[1] - (hi[0] - lo[0])) <= float(np.float32(step)) * length[1]


def test_scaling_d_and_the_step_gives_the_same_picture():
    rgbs, _ = br.blob_grid()
    rays = br.make_rays()
    keep = np.isfinite(rays).all(1)
    step = 0.021
    a = br.render(rgbs, br.BOUNDS, rays[keep], step, 0.25)
    scaled = rays[keep].astype(np.float64)
    scaled[:, 3:6] *= 2.5
    scaled[:, 6:8] /= 2.5
    # (the scaled rows and step are fp64 numbers here: the reference's own arithmetic, not a second rounding to fp32)
    lo, hi = br.bounds64(br.BOUNDS)
    grid = rgbs.astype(np.float64)
    C = np.array(grid.shape[2::-1], np.float64) - 1
    compared = 0
    for r in range(scaled.shape[0]):
        c, dep, op, n, _, _ = br.render_ray(grid, lo, hi, C, scaled[r], float(np.float32(step)) / 2.5, 0.25, 0.0)
        if n != a["n"][r]:  # (K is a fp32 number: the last sample of a ray may come or go)
            continue
        compared += 1
        assert np.abs(c - a["rgb"][r]).max() < 1e-9 and abs(op - a["opacity"][r]) < 1e-9 and abs(dep * 2.5 - a["depth"][r]) < 1e-9
    assert compared >= 60
    assert (a["opacity"] > 0.5).sum() > 10 and (a["opacity"] < 1e-3).sum() >= 2


def test_misses_show_the_background_at_far_and_stop_ends_a_ray():
    rgbs, _ = br.blob_grid()
    rays = br.make_rays()
    out = br.render(rgbs, br.BOUNDS, rays, 0.05, 0.25)
    for r in (2, 5, 6):  # misses the box, a NaN, far <= near
        assert np.array_equal(out["rgb"][r], np.full(3, 0.25)) and out["opacity"][r] == 0 and out["n"][r] == 0
        assert out["depth"][r] == rays[r, 7] or np.isnan(rays[r]).any()
    stopped = br.render(rgbs, br.BOUNDS, rays, 0.05, 0.25, stop=1e-3)
    assert (stopped["n"] < out["n"]).any() and np.abs(stopped["rgb"] - out["rgb"]).max() <= 1e-3 * 1.25
    assert (stopped["n"] <= out["n"]).all()


def test_the_test_grids_are_what_their_docstrings_say():
    rgbs, _ = br.blob_grid()
    assert rgbs.shape == (11, 10, 9, 4)
    cells = br.occupied_cells(rgbs)
    assert cells.shape == (10, 9, 8) and cells.size % 32 and 0.2 < cells.mean() < 0.9
    corner, _ = br.corner_grid()
    bricks = br.occupied_cells(corner).reshape(2, 8, 2, 8, 2, 8).any(axis=(1, 3, 5))
    assert bricks.sum() == 2 and bricks[0, 0, 0] and bricks[1, 1, 1]
    for g in (rgbs, corner):  # zero on the outermost layer of points, and pruned points are exact zeros
        assert not g[[0, -1]].any() and not g[:, [0, -1]].any() and not g[:, :, [0, -1]].any()
        assert not g[g[..., 3] == 0].any()
    rays = br.make_rays()
    assert rays.shape == (67, 8) and (rays[0, 3:6] == 0).sum() == 2 and np.isnan(rays[5]).any() and rays[6, 7] <= rays[6, 6]
    assert abs(np.linalg.norm(rays[4, 3:6]) - 2.5) < 1e-6


# ---- host checks ---------------------------------------------------------------------------------------------------------------------

def _render_args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)  # (non-null, aligned, never dereferenced: every case below is refused on the host)
    a = _lib.BakedRenderArgs(Cx=8, Cy=9, Cz=10, R=5, lo=(ctypes.c_float * 3)(-1, -1, -1), hi=(ctypes.c_float * 3)(1, 1, 1), step=0.1,
                             background=0.0, stop=0.0, rgbs=one, words=one, rays=one, rgb=one, depth=one, opacity=one)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("case", [
    dict(R=0), dict(Cx=0), dict(Cz=-1), dict(Cx=70000, Cy=70000), dict(step=0.0), dict(step=-0.1), dict(step=float("nan")),
    dict(step=float("inf")), dict(background=float("nan")), dict(stop=-0.1), dict(stop=1.0), dict(stop=float("nan")),
    dict(rgbs=None), dict(words=None), dict(rays=None), dict(rgb=None), dict(depth=None), dict(opacity=None),
    dict(rgbs=ctypes.c_void_p(24)), dict(rays=ctypes.c_void_p(20)),  # not 16-byte aligned
    dict(hi=(ctypes.c_float * 3)(1, -1, 1)), dict(lo=(ctypes.c_float * 3)(float("nan"), -1, -1)),
    dict(hi=(ctypes.c_float * 3)(1, float("inf"), 1)),
])
def test_baked_render_refuses_before_launch(case):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_baked_render(ctypes.byref(_render_args(**case)), None) == -1
    assert _lib.lib.upnerf_baked_render(None, None) == -1


def test_baked_pack_refuses_before_launch():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    ok = dict(n=10, level=0.5, sigma=one, rgb=one, rgbs=one, kept=None)
    for bad in (dict(n=0), dict(sigma=None), dict(rgbs=None), dict(rgbs=ctypes.c_void_p(8)), dict(level=float("nan"))):
        assert _lib.lib.upnerf_baked_pack(ctypes.byref(_lib.BakedPackArgs(**{**ok, **bad})), None) == -1
    assert _lib.lib.upnerf_baked_pack(None, None) == -1


def test_the_python_surface_refuses_on_the_host():
    import torch
    from upnerf_amd import baked
    with pytest.raises(RuntimeError):  # no CPU path
        baked.BakedScene.from_grids(torch.zeros(3, 3, 3), None, br.BOUNDS)
    with pytest.raises(RuntimeError):
        baked.BakedScene(torch.zeros(3, 3, 3, 4), br.BOUNDS, 0.0)
    rays = torch.zeros(4, 8)
    for bad in (dict(step=0.0), dict(step=float("nan")), dict(background=float("inf")), dict(stop=1.0), dict(stop=-1e-3)):
        with pytest.raises(ValueError):
            baked._render_args(rays, **{**dict(step=0.1, background=0.0, stop=0.0), **bad})
    for bad in (torch.zeros(4, 7), torch.zeros(4, 8, dtype=torch.float64), torch.zeros(0, 8)):
        with pytest.raises(ValueError):
            baked._render_args(bad, 0.1, 0.0, 0.0)
    assert baked._render_args(rays, 0.1, 1, 0) == (0.1, 1.0, 0.0)
    assert np.float32(baked.TINY) > 0 and np.float32(baked.TINY) / np.float32(2) == 0  # the smallest positive fp32


def test_save_and_load_round_trip_the_arrays(tmp_path):
    from upnerf_amd import baked
    rgbs, level = br.blob_grid()
    path = str(tmp_path / "scene.npz")
    baked.save_arrays(path, rgbs, br.BOUNDS, level)
    assert os.path.exists(path)
    back, bounds, lv = baked.load_arrays(path)
    assert back.dtype == np.float32 and np.array_equal(back.view(np.int32), rgbs.view(np.int32))
    assert bounds == (tuple(float(x) for x in br.BOUNDS[0]), tuple(float(x) for x in br.BOUNDS[1])) and lv == level
    with pytest.raises(ValueError):
        baked.save_arrays(path, rgbs.astype(np.float64), br.BOUNDS, level)
    with pytest.raises(ValueError):
        baked.save_arrays(path, rgbs, ((0, 0, 0), (1, 0, 1)), level)
    other = str(tmp_path / "other.npz")
    np.savez(other, rgbs=rgbs)
    with pytest.raises(ValueError):
        baked.load_arrays(other)
