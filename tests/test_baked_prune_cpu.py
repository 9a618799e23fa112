"""Pruning a baked scene by visibility, without a GPU: the fp64 restatement tests/baked_prune_ref.py against closed
forms, the semantics of prune in numpy, the condition on the GPU test's rays, and tests/host/baked_vis_host.hip -- the per-ray
function the kernel calls, compiled for the host with a plain max as its recorder -- on the grids and ray families of
tests/walk_cases.py:

  * the visibility marched with the occupancy bits is bit for bit the one that visits every sample, in both layouts;
  * it is the same at degrees 0, 1 and 2 (only the sigma of a point is read);
  * the pool's, after a face max, is bit for bit the gathered dense one;
  * both lie inside the restatement's intervals;
  * the program is clean under AddressSanitizer and UndefinedBehaviorSanitizer (host side; on a machine without a GPU)."""
import os

import numpy as np
import pytest
import torch

import baked_prune_ref as pr
import baked_ref as br
import baked_sparse_ref as sr
import walk_cases as wc
from walk_checks import CONFIGS, REF_CONFIGS, host_build, run_clean

SANITIZE = not torch.cuda.is_available()  # sanitizer runs belong on a machine without a GPU
TN = pr.TINY_NORMAL
F32 = np.float32


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------

def one_cell(sigma=2.0):
    """A single cell (2 x 2 x 2 points) of constant sigma in the unit box."""
    return np.full((2, 2, 2), sigma, F32), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def test_one_cell_and_one_sample():
    sigma, bounds = one_cell(2.0)
    ray = np.asarray([[-1.0, 0.5, 0.5, 1.0, 0.0, 0.0, 1.0, 2.0]], F32)  # one sample at t = 1.5: the middle of the cell
    lo, hi = pr.visibility(sigma, bounds, ray, 1.0)
    w = 1.0 - np.exp(-2.0)
    assert (lo > 0).all() and np.allclose(lo, w, rtol=1e-6, atol=0) and np.allclose(hi, w, rtol=1e-6, atol=0)
    assert (lo <= w).all() and (w <= hi).all() and (hi - lo < 1e-6).all()
    # one dead corner: it receives nothing, the others are unchanged
    sigma[1, 0, 1] = 0.0
    lo2, hi2 = pr.visibility(sigma, bounds, ray, 1.0)
    assert lo2[1, 0, 1] == 0 and hi2[1, 0, 1] == 0 and (lo2 > 0).sum() == 7


def test_a_uniform_slab_gives_geometric_weights():
    # 8 cells on x, sigma 3 everywhere but the outermost layer of x: inside, w_k = (1 - a) a^k with a = exp(-3 step)
    sigma = np.zeros((2, 2, 9), F32)
    sigma[:, :, 1:8] = 3.0
    bounds = ((0.0, 0.0, 0.0), (8.0, 1.0, 1.0))
    step = 0.5
    ray = np.asarray([[-0.125, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0, 9.0]], F32)  # samples at x = 0.125 + 0.5 k: never on a face
    lo, hi = pr.visibility(sigma, bounds, ray, step)
    a = np.exp(-3.0 * step)
    # cell 2 (corners 2 and 3, both 3.0) holds samples k = 4, 5; before it cell 0 (sigma 3 x), cell 1 (sigma 3): T at its entry
    xs = 0.125 + 0.5 * np.arange(4)
    T = np.prod(np.exp(-step * np.interp(xs, [0, 1, 2], [0, 3, 3])))
    best = T * (1 - a)  # the first sample of the cell has the largest weight
    assert lo[0, 0, 0] == 0 and hi[0, 0, 0] == 0  # the dead outer layer
    # point 3 touches cells 2 and 3: the larger is cell 2's; point 2 touches cells 1 and 2: cell 1's first sample is larger
    # (the interval is the gate of baked_ref: a few units of fp32 roundoff per sample before it, on numbers below 1)
    assert lo[0, 0, 3] <= best <= hi[0, 0, 3] and hi[0, 0, 3] - lo[0, 0, 3] < 1e-5
    T1 = np.prod(np.exp(-step * np.interp(xs[:2], [0, 1, 2], [0, 3, 3])))
    assert lo[0, 0, 2] <= T1 * (1 - a) <= hi[0, 0, 2] and hi[0, 0, 2] - lo[0, 0, 2] < 1e-5
    # deeper cells see geometrically less: a cell holds two samples
    assert abs(hi[0, 0, 4] / hi[0, 0, 3] - a * a) < 1e-4
    assert pr.uncertain(lo, hi) == 0.0


def test_a_miss_sees_nothing():
    sigma, bounds = one_cell()
    rays = np.asarray([[-1.0, 2.5, 0.5, 1.0, 0.0, 0.0, 0.0, 3.0],      # passes beside the box
                       [-1.0, 0.5, 0.5, 1.0, 0.0, 0.0, 2.0, 2.0],      # far <= near
                       [np.nan, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0, 3.0]], F32)
    lo, hi = pr.visibility(sigma, bounds, rays, 0.25)
    assert (lo == 0).all() and (hi == 0).all()


def test_stop_ends_the_ray_and_an_opaque_sample_does_too():
    sigma = np.zeros((2, 2, 9), F32)
    sigma[:, :, 1:8] = 3.0
    bounds = ((0.0, 0.0, 0.0), (8.0, 1.0, 1.0))
    ray = np.asarray([[-0.125, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0, 9.0]], F32)
    lo0, hi0 = pr.visibility(sigma, bounds, ray, 0.5)
    lo1, hi1 = pr.visibility(sigma, bounds, ray, 0.5, stop=0.05)
    # T falls below 0.05 after ln(20) / 1.5 ~ 2 samples at full density: the deep points are seen without stop and not with it
    assert (hi0[0, 0, 6] > 0) and hi1[0, 0, 6] == 0 and lo1[0, 0, 6] == 0
    assert (lo1 <= lo0).all() and (hi1 <= hi0).all() and np.array_equal(lo1[0, 0, :3], lo0[0, 0, :3])
    # sigma 1000: alpha is 1 in fp32 at the first full sample, and nothing behind it is in any interval
    wall = np.zeros((2, 2, 9), F32)
    wall[:, :, 2:5] = 1000.0
    wall[:, :, 6] = 5.0
    lo, hi = pr.visibility(wall, bounds, ray, 0.5)
    assert (lo[0, 0, 2] > 0) and (hi[:, :, 3:] == 0).all()


def test_prune_semantics():
    rng = np.random.RandomState(3)
    pts = rng.randint(1, 255, (5, 4, 3, 32)).astype(np.uint8)
    vis = rng.uniform(0, 1, (5, 4, 3)).astype(F32)
    vis[0, 0, 0], vis[1, 1, 1], vis[2, 2, 2] = 0.0, np.nan, 0.25
    out, kept = pr.prune(pts, vis, 0.25)
    assert kept[2, 2, 2] == 1 and kept[0, 0, 0] == 0 and kept[1, 1, 1] == 0  # >= keeps, a NaN goes
    assert np.array_equal(out[kept == 1], pts[kept == 1]) and (out[kept == 0] == 0).all()
    assert np.array_equal(kept == 1, np.nan_to_num(vis, nan=-1.0) >= F32(0.25))
    # the default weight drops exactly what nothing sees
    out, kept = pr.prune(pts, vis, TN)
    assert np.array_equal(kept == 1, np.nan_to_num(vis, nan=0.0) > 0)
    # a face max in numpy: the copies of a point agree afterwards
    bricks = np.asarray([0, 1, 2], np.int32)
    pool = rng.uniform(0, 1, (3, 9, 9, 9)).astype(F32)
    m = pr.face_max(pool, bricks, (18, 9, 9))
    assert np.array_equal(m[0, :, :, 8], m[1, :, :, 0]) and np.array_equal(m[0, :, :, 8], np.maximum(pool[0, :, :, 8], pool[1, :, :, 0]))
    assert np.array_equal(m[2, :, :, 2:], pool[2, :, :, 2:])  # beyond the grid (x = 18 ..): not touched


# ---- the condition on the GPU test's rays ------------------------------------------------------------------------------------------

def gpu_cases():
    """(name, rgbs, rays, {step name: step}) of tests/test_hip_baked_prune.py's interval checks."""
    rays = br.make_rays()
    out = []
    for name, make in (("blob", br.blob_grid), ("corners", br.corner_grid), ("ragged", pr.ragged_grid)):
        rgbs, _ = make()
        cell = br.cell_size(rgbs)
        out.append((name, rgbs, rays, {"cell": float(F32(cell)), "tenth": float(F32(cell / 10))}))
    rgbs, _ = pr.wall_grid()
    wr, step = pr.wall_rays()
    out.append(("wall", rgbs, wr, {"half": step}))
    return out


@pytest.mark.parametrize("case", gpu_cases(), ids=lambda c: c[0])
def test_few_points_of_the_gpu_scenes_are_undecided(case):
    name, rgbs, rays, steps = case
    for step_name, step in steps.items():
        for stop in (0.0, 1e-3):
            lo, hi = pr.visibility(rgbs[..., 3], br.BOUNDS, rays, step, stop)
            share = pr.uncertain(lo, hi)
            print(f"{name} {step_name} stop {stop}: {int((hi > 0).sum())} points seen, undecided share {share:.4f}")
            assert (hi > 0).sum() > 50 and share <= 0.1 and (lo <= hi).all()
    if name == "wall":
        assert (hi[:, :, pr.WALL_X[1]:] == 0).all() and (lo[2:-2, 2:-2, pr.WALL_X[0]] > 0).all()  # nothing behind the first layer


# ---- the host program ------------------------------------------------------------------------------------------------------------

needs_hipcc = pytest.mark.skipif(host_build.hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vis_host"))
    built = {False: host_build.build(out, names=("baked_vis_host",))["baked_vis_host"]}
    if SANITIZE:
        built[True] = host_build.build(out, sanitize=True, names=("baked_vis_host",))["baked_vis_host"]
    return built


def run_vis(exe, directory, name, rays, step, stop):
    """baked_vis_host on a scene of walk_cases: (dense [3 degrees][2: every sample, bits][Nz, Ny, Nx], pool [3][2][n, 9, 9, 9])."""
    S = wc.scene(name)
    d = str(directory)
    lo, hi = (np.asarray(b, F32) for b in wc.BOUNDS)
    np.asarray(list(S["cells"]) + [len(rays), len(S["bricks"])], np.int32).tofile(os.path.join(d, "dims.bin"))
    np.concatenate([lo, hi, [step, 0.0, stop]]).astype(F32).tofile(os.path.join(d, "params.bin"))
    for degree in (0, 1, 2):
        np.ascontiguousarray(S["points"][degree]).tofile(os.path.join(d, f"points{degree}.bin"))
        np.ascontiguousarray(S["pool"][degree]).tofile(os.path.join(d, f"pool{degree}.bin"))
    S["slots"].astype(np.int32).tofile(os.path.join(d, "slots.bin"))
    S["words"].astype(np.uint32).tofile(os.path.join(d, "words.bin"))
    np.ascontiguousarray(rays, F32).tofile(os.path.join(d, "rays.bin"))
    run_clean(exe, d)
    shape = S["rgbs"].shape[:3]
    dense = np.fromfile(os.path.join(d, "vis_dense.bin"), np.uint32).reshape((3, 2) + shape)
    pool = np.fromfile(os.path.join(d, "vis_pool.bin"), np.uint32).reshape(3, 2, len(S["bricks"]), 9, 9, 9)
    return dense, pool


def check_exact(name, dense, pool):
    """The bit-for-bit claims on one run (the arrays are the floats' bits); returns the points seen."""
    S = wc.scene(name)
    for degree in (0, 1, 2):
        assert np.array_equal(dense[degree, 0], dense[degree, 1]), (name, degree, "dense: the bits change the visibility")
        assert np.array_equal(pool[degree, 0], pool[degree, 1]), (name, degree, "pool: the bits change the visibility")
        assert np.array_equal(dense[degree], dense[0]) and np.array_equal(pool[degree], pool[0]), (name, degree, "the degree is seen")
    d = dense[0, 1].view(F32)
    whole = pr.face_max(pool[0, 1].view(F32), S["bricks"], S["rgbs"].shape[2::-1])
    assert np.array_equal(whole.view(np.uint32), sr.gather(d[..., None], S["bricks"])[..., 0].view(np.uint32)), (name, "pool != dense")
    live = S["rgbs"][..., 3] != 0
    assert (d[~live] == 0).all() and np.isfinite(d).all() and ((d == 0) | (d >= F32(TN))).all() and (d <= 1).all()
    return int((d > 0).sum())


@needs_hipcc
@pytest.mark.parametrize("name", list(wc.GRIDS))
def test_the_host_visibility_is_exact_and_inside_the_intervals(programs, tmp_path, name):
    S = wc.scene(name)
    seen = 0
    for step_name, stop in CONFIGS:
        step = wc.steps(name)[step_name]
        rays, _ = wc.rays_of(40, 11, S["cells"], step, big=False)
        seen += check_exact(name, *run_vis(programs[False], tmp_path, name, rays, step, stop))
    if name != "one-cell":
        assert seen > 100
    for step_name, stop in REF_CONFIGS:
        step = wc.steps(name)[step_name]
        rays, _ = wc.rays_of(6, 12, S["cells"], step, ref=S["edge"], big=False)
        dense, pool = run_vis(programs[False], tmp_path, name, rays, step, stop)
        lo, hi = pr.visibility(S["rgbs"][..., 3], wc.BOUNDS, rays, step, stop)
        d = dense[0, 1].view(F32)
        ok = pr.within(d, lo, hi)
        assert ok.all(), (name, step_name, stop, np.argwhere(~ok)[:5], d[~ok][:5], lo[~ok][:5], hi[~ok][:5])
        whole = pr.face_max(pool[0, 1].view(F32), S["bricks"], S["rgbs"].shape[2::-1])
        lo_p, hi_p = (sr.gather(x[..., None], S["bricks"])[..., 0] for x in (lo, hi))
        assert pr.within(whole, lo_p, hi_p).all(), (name, step_name, stop, "pool")
        print(f"{name} {step_name} stop {stop}: {int((d > 0).sum())} points seen, undecided share {pr.uncertain(lo, hi):.3f}")


@needs_hipcc
@pytest.mark.skipif(not SANITIZE, reason="sanitizer runs belong on a machine without a GPU")
@pytest.mark.parametrize("name", list(wc.GRIDS))
def test_the_visibility_march_is_clean_under_the_sanitizers(programs, tmp_path, name):
    S = wc.scene(name)
    for step_name, stop in CONFIGS:
        step = wc.steps(name)[step_name]
        rays, _ = wc.rays_of(10, 13, S["cells"], step, big=False)
        check_exact(name, *run_vis(programs[True], tmp_path, name, rays, step, stop))
