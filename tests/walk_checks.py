"""What tests/test_walks_host_cpu.py (the host programs of tests/host/) and tests/test_hip_walk_edges.py (the entry points on the
GPU) share: the recipe of the host programs, loaded by path, how they are fed and read, and the functions that judge a march
and a set of spans -- the same for host and device.  The claims are stated in tests/test_walks_host_cpu.py's docstring."""
import importlib.util
import os

import numpy as np

import baked_ref as br
import baked_sh_ref as sh
import occupancy_ref as oref
import walk_cases as wc

_spec = importlib.util.spec_from_file_location("walk_host_build", os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "walk_host_build.py"))
host_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host_build)

N_PLAIN, N_SAN, N_SPAN = 720, 72, 100
N_REF = {True: 50, False: 20}  # rays per family of the fp64 comparison: on an edge grid the 2 % cap needs 50 to allow one
CONFIGS = [("cell", 0.0), ("tenth", 0.0), ("tenth", 1e-3), ("over", 0.0)]
REF_CONFIGS = [("cell", 0.0), ("tenth", 1e-3)]
BORDERLINE_CAP = 0.02
GRAZING_CAP = {"vertices": 0.53, "in-plane": 0.92, "shallow": 0.28, "faces-start": 0.14, "far-origin": 0.14, "caps": 0.07,
               "random-wide": 0.11}
BACKGROUND = 0.5


def run_clean(exe, directory):
    code, err = host_build.run(exe, directory)
    assert code == 0 and err == "", (exe, code, err[-2000:])


def run_march(exe, directory, name, rays, step, stop):
    """baked_host on a scene of walk_cases and rays [R, 8]: its outputs as arrays."""
    S = wc.scene(name)
    d = str(directory)
    lo, hi = (np.asarray(b, np.float32) for b in wc.BOUNDS)
    R = len(rays)
    np.asarray(list(S["cells"]) + [R, len(S["bricks"])], np.int32).tofile(os.path.join(d, "dims.bin"))
    np.concatenate([lo, hi, [step, BACKGROUND, stop]]).astype(np.float32).tofile(os.path.join(d, "params.bin"))
    for degree in (0, 1, 2):
        np.ascontiguousarray(S["points"][degree]).tofile(os.path.join(d, f"points{degree}.bin"))
        np.ascontiguousarray(S["pool"][degree]).tofile(os.path.join(d, f"pool{degree}.bin"))
    S["slots"].astype(np.int32).tofile(os.path.join(d, "slots.bin"))
    S["words"].astype(np.uint32).tofile(os.path.join(d, "words.bin"))
    np.ascontiguousarray(rays, np.float32).tofile(os.path.join(d, "rays.bin"))
    run_clean(exe, d)
    load = lambda f, t: np.fromfile(os.path.join(d, f), t)
    return dict(march=load("march.bin", np.uint32).reshape(12, R, 5), K=load("K.bin", np.int32), flags=load("flags.bin", np.uint8),
                brute=load("brute.bin", np.int32).reshape(12, R), count=load("count.bin", np.int32).reshape(12, R),
                visit=load("visit.bin", np.int32))


def check_exact(out, fam, stop, what):
    """The exact claims on one run; returns (rays, visited samples with the bits, without them)."""
    R = len(out["K"])
    K = out["K"].astype(np.int64)
    at = np.cumsum(K) - K
    ray_of = np.repeat(np.arange(R), K)
    name_of = lambda r: wc.FAMILIES[fam[r]]
    assert len(out["flags"]) == K.sum()
    ends = np.cumsum(out["count"].reshape(-1).astype(np.int64))
    seen = [0, 0]
    for c in range(12):
        degree, layout, bits = c >> 2, (c >> 1) & 1, c & 1
        need = ((1, 7), (9, 13))[layout][bits]  # 1 inside, 2 brick bit, 4 cell bit, 8 slot >= 0 (a sparse march reads the slot)
        idx = np.nonzero((out["flags"] & need) == need)[0]
        rid = ray_of[idx]
        cnt = np.bincount(rid, minlength=R)
        if stop == 0:
            assert np.array_equal(out["brute"][c], cnt), (what, c)
        assert (out["brute"][c] <= cnt).all()
        rank = np.arange(len(idx)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        keep = rank < out["brute"][c][rid]
        want_k, want_n = (idx - at[rid])[keep], np.minimum(cnt, out["brute"][c])
        bad = np.nonzero(out["count"][c] != want_n)[0]
        assert bad.size == 0, (what, f"degree {degree} layout {layout} bits {bits}", name_of(bad[0]), int(bad[0]),
                               int(out["count"][c][bad[0]]), int(want_n[bad[0]]))
        got_k = out["visit"][ends[c * R] - out["count"][c][0]:ends[c * R + R - 1]]
        if not np.array_equal(got_k, want_k):
            j = int(np.nonzero(got_k != want_k)[0][0])
            r = int(np.searchsorted(np.cumsum(want_n), j, side="right"))
            raise AssertionError((what, f"degree {degree} layout {layout} bits {bits}", name_of(r), r, int(got_k[j]), int(want_k[j])))
        seen[bits] += int(want_n.sum())
    m = out["march"]
    for degree in (0, 1, 2):
        for layout in (0, 1):
            c = (degree * 2 + layout) * 2
            bad = np.nonzero((m[c] != m[c + 1]).any(1))[0]  # (compared as bits: a NaN equals itself)
            assert bad.size == 0, (what, "skipping is not exact", degree, layout, name_of(bad[0]), int(bad[0]))
        bad = np.nonzero((m[degree * 4 + 1] != m[degree * 4 + 3]).any(1))[0]
        assert bad.size == 0, (what, "sparse is not dense", degree, name_of(bad[0]), int(bad[0]))
    return R, seen[1], seen[0]


_REF = {}


def _restate(name, degree, rays, step, stop):
    S = wc.scene(name)
    if degree == 0:
        return br.render(S["rgbs"], wc.BOUNDS, rays, step, BACKGROUND, stop)
    return sh.render(S["points"][degree], degree, wc.BOUNDS, rays, step, BACKGROUND, stop)


def restate_ahead(jobs):
    """The restatements of jobs [(name, degree, rays, step, stop)] computed side by side in fresh child processes (a CPU test's
    way to its time budget; never called by a test that has a device open) and kept for compare_fp64."""
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    jobs = [j for j in jobs if (j[0], j[1], j[3], j[4], j[2].tobytes()) not in _REF]
    if not jobs:
        return
    with ProcessPoolExecutor(min(len(jobs), os.cpu_count() or 1, 8), mp_context=multiprocessing.get_context("spawn")) as pool:
        for j, ref in zip(jobs, pool.map(_restate, *zip(*jobs))):
            _REF[(j[0], j[1], j[3], j[4], j[2].tobytes())] = ref


def compare_fp64(name, degree, rays, fam, step, stop, got):
    """got [R, 5] fp32 (rgb, depth, opacity) against the restatement's gates; returns (the worst err / gate, the share left out,
    the rays that hit, the restatement's dict, the rays that were compared)."""
    S = wc.scene(name)
    key = (name, degree, step, stop, rays.tobytes())
    if key not in _REF:  # computed once, shared by the tests that need it, never changed
        _REF[key] = _restate(name, degree, rays, step, stop)
    ref = _REF[key]
    want = np.concatenate([ref["rgb"], ref["depth"][:, None], ref["opacity"][:, None]], 1)
    gate = np.concatenate([ref["gate_rgb"], ref["gate_depth"][:, None], ref["gate_opacity"][:, None]], 1)
    keep = np.ones(len(rays), bool)
    if S["edge"]:
        keep = ~wc.borderline(S["cells"], rays, step)
        for f, fname in enumerate(wc.FAMILIES):
            left, n = int((~keep[fam == f]).sum()), int((fam == f).sum())
            assert left <= BORDERLINE_CAP * n + 1e-9, (name, fname, step, left, n)
    finite = np.isfinite(want).all(1)  # (a miss whose far is no number: the far comes back as it is)
    got64 = got.astype(np.float64)
    assert np.array_equal(got64[~finite], want[~finite], equal_nan=True)
    rows = keep & finite
    err = np.abs(got64[rows] - want[rows])
    bad = np.argwhere(err > gate[rows])
    assert bad.size == 0, (name, degree, step, stop, wc.FAMILIES[fam[rows][bad[0][0]]], bad[:4].tolist(), float(err.max()))
    return float((err / np.maximum(gate[rows], 1e-300)).max()), 1 - keep.mean(), int((ref["n"][rows] > 0).sum()), ref, rows


def run_spans(exe, directory, name, rays):
    S = wc.scene(name)
    d = str(directory)
    np.asarray(list(S["cells"]) + [len(rays)], np.int32).tofile(os.path.join(d, "dims.bin"))
    np.concatenate([np.asarray(b, np.float32) for b in wc.BOUNDS]).tofile(os.path.join(d, "bounds.bin"))
    S["words"].astype(np.uint32).tofile(os.path.join(d, "words.bin"))
    np.ascontiguousarray(rays, np.float32).tofile(os.path.join(d, "rays.bin"))
    run_clean(exe, d)
    return (np.fromfile(os.path.join(d, "t0.bin"), np.float32), np.fromfile(os.path.join(d, "t1.bin"), np.float32),
            np.fromfile(os.path.join(d, "hit.bin"), np.uint8))


def check_spans(name, rays, fam, t0, t1, hit):
    """The span claims (module docstring), family by family, for the host program and the kernel alike."""
    S = wc.scene(name)
    R = len(rays)
    r0, r1, rh, graze = np.zeros(R), np.zeros(R), np.zeros(R, bool), np.zeros(R, bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in range(0, R, 512):  # (brute force holds rays x occupied cells at once)
            r0[a:a + 512], r1[a:a + 512], rh[a:a + 512] = oref.spans_ref(S["bits"], wc.BOUNDS, rays[a:a + 512])
            graze[a:a + 512] = oref.grazing(S["bits"], wc.BOUNDS, rays[a:a + 512])
        d = np.abs(rays[:, 3:6].astype(np.float64))
        moved = rays.astype(np.float64)
        moved[:, 3:6] = np.where(d == 0, d.max(1, keepdims=True), d)  # the smallest NON-ZERO component divides
        # ray by ray: span_tolerance takes its M from the largest |o| it is given, and a far origin is no other ray's business
        tol = np.array([oref.span_tolerance(S["cells"], wc.BOUNDS, moved[r:r + 1])[0] for r in range(R)])
    h = hit == 1
    far = rays[:, 7]
    for f, fname in enumerate(wc.FAMILIES):
        rows = fam == f
        keep = rows & ~graze
        both = keep & rh & h & np.isfinite(tol)
        e0, e1 = np.abs(t0 - r0), np.abs(t1 - r1)
        print(f"spans {name} {fname}: grazing {graze[rows].mean():.4f}, hits {rh[keep].mean() if keep.any() else 0:.3f}, compared {both.sum()}, "
              f"worst err / gate {max((e0[both] / tol[both]).max(), (e1[both] / tol[both]).max()) if both.any() else 0:.3f}")
        assert graze[rows].mean() <= GRAZING_CAP[fname], (name, fname)
        want = rh & (r1.astype(np.float32) > r0.astype(np.float32))  # (hit is t1 > t0 IN FP32: include/upnerf_hip.h)
        assert np.array_equal(h[keep], want[keep]), (name, fname, np.nonzero(keep & (h != want))[0][:5])
        assert (e0[both] <= tol[both]).all() and (e1[both] <= tol[both]).all(), (name, fname)
    assert (t0[h] <= t1[h]).all() and (t1[h] <= far[h]).all() and (t0[h] >= rays[h, 6]).all()
    assert np.array_equal(t0[~h].view(np.uint32), far[~h].view(np.uint32)) and np.array_equal(t1[~h].view(np.uint32), far[~h].view(np.uint32))
    return int((rh & ~graze).sum())
