"""The restatement of the doubled resolution, tests/baked_upsample_ref.py, on the CPU: it is reproducible bit for
bit, it keeps what the definition says it keeps, and the fp64 render of the child's numbers stays within render_gate of the fp64
render of the parent's numbers on every ray -- the gate the GPU tests then use (level = the smallest positive fp32, stop = 0, the
rays and steps of tests/test_hip_baked_tune.py)."""
import numpy as np
import pytest

import baked_ref as br
import baked_sh_ref as sh
import baked_tune_ref as tr
import baked_tv_ref as tvr
import baked_upsample_ref as ur

_CACHE = {}


def rays_of(name):
    return np.concatenate([br.make_rays(), tr.extra_rays(tvr.GRIDS[name]()[0])])


def renders(name, degree, step):
    """(parent's fp64 render, child's fp64 render, the gate), computed once."""
    key = (name, degree, step)
    if key not in _CACHE:
        parent, _ = ur.parents(name, degree)
        child = ur.upsample(parent, degree, ur.TINY)
        rays = rays_of(name)
        dt = sh.steps(tvr.GRIDS[name]()[0])[step]
        _CACHE[key] = (tr.render64(ur.numbers(parent, degree), degree, br.BOUNDS, rays, dt),
                       tr.render64(ur.numbers(child, degree), degree, br.BOUNDS, rays, dt),
                       ur.render_gate(child, parent, degree, br.BOUNDS, rays, dt))
    return _CACHE[key]


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", list(tvr.GRIDS))
def test_restatement_is_reproducible_and_keeps_the_parents(name, degree):
    parent, level = ur.parents(name, degree)
    a, b = ur.upsample(parent, degree, level), ur.upsample(parent.copy(), degree, level)
    assert a.tobytes() == b.tobytes()
    Nz, Ny, Nx = parent.shape[:3]
    assert a.shape[:3] == (2 * Nz - 1, 2 * Ny - 1, 2 * Nx - 1) and a.shape[3:] == parent.shape[3:] and a.dtype == parent.dtype
    assert a[::2, ::2, ::2].tobytes() == parent.tobytes()  # an even index copies (a kept parent is kept again at its own level)
    s = ur.stored(a, degree)[..., -1]
    assert ((s == 0) | (s >= np.float32(level))).all() and (s > 0).any()  # no kept child below the level
    loose = ur.stored(ur.upsample(parent, degree, ur.TINY), degree)[..., -1]
    assert (loose > 0).sum() > (s > 0).sum() or name == "cell"  # the level prunes blends of kept and dropped parents


def test_blend_order_and_exact_halving():
    v = np.zeros((2, 2, 2, 1), np.float32)
    v[0, 0, 0], v[0, 0, 1], v[0, 1, 0], v[0, 1, 1] = 1.0, 2.0 ** -24, -1.0, 3.0
    out = ur.blend(v)
    x0, x1 = np.float32(0.5) * (np.float32(1.0) + np.float32(2.0 ** -24)), np.float32(0.5) * (np.float32(-1.0) + np.float32(3.0))
    assert out[0, 1, 1, 0] == np.float32(0.5) * (x0 + x1)  # x pairs first, then y
    assert out[0, 0, 1, 0] == x0 and out[0, 2, 1, 0] == x1
    assert ur.blend(np.full((3, 2, 4, 2), 0.7, np.float32)).tobytes() == np.full((5, 3, 7, 2), 0.7, np.float32).tobytes()


@pytest.mark.parametrize("step", ["cell", "tenth"])
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", ["blob", "big"])
def test_child_render_is_within_the_gate_of_the_parent_render(name, degree, step):
    (rgb_p, depth_p, op_p), (rgb_c, depth_c, op_c), (g_rgb, g_depth, g_op) = renders(name, degree, step)
    worst = 0.0
    for what, a, b, gate in (("rgb", rgb_c, rgb_p, g_rgb), ("depth", depth_c, depth_p, g_depth), ("opacity", op_c, op_p, g_op)):
        err = np.abs(a - b)
        noise = 1e-13 * np.maximum(1.0, np.abs(b))  # the two fp64 restatements' own roundings
        assert (err <= gate + noise).all(), (what, np.argwhere(err > gate + noise)[:5], float(err.max()))
        worst = max(worst, float((err / np.maximum(gate, 1e-300))[gate > 0].max(initial=0.0)))
    hit = op_p > 1e-3
    print(f"{name} degree {degree} {step}: {int(hit.sum())} rays hit, worst err / gate {worst:.3f}, largest gate {float(g_rgb.max()):.3e}")
    assert hit.sum() >= 30 and g_rgb.max() < 1e-2
