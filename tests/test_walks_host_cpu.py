"""The two walks on the host, against brute force: baked_walk / baked_march (csrc/baked.hip) and occ_walk (csrc/occupancy.hip) are
__host__ __device__, and tests/host/baked_host.hip and tests/host/occ_host.hip are stand-alone programs that include the kernel
sources unchanged and call them with no device (tests/host/build.py builds and runs them; skipped without hipcc).  Grids and
ray families are tests/walk_cases.py's.

The marcher checks are exact, without a tolerance and without an exclusion, on every ray, grid, degree {0, 1, 2} and layout
{dense, sparse}: the samples the walk hands to `visit` are brute force's (every k in [0, K) located, its bits and slot looked up,
nothing skipped), with the bits and without; the march with the bits is the march without them, bit for bit; the sparse march
is the dense march, bit for bit.  N_PLAIN rays per family and configuration: 7 families x 4 configurations (step, stop) x 720 =
20 160 rays per (grid, layout, degree); the sanitizer build (AddressSanitizer + UBSan on the host side, only where there is no
GPU) runs 2 016, must exit 0 and write nothing to stderr.

The fp64 restatements (baked_ref.render, baked_sh_ref.render; computed side by side in child processes) hold the host march to
their own derived gates on N_REF rays per family, grid and degree: 20 on `blob` and `corners`, with the families as the exact
checks draw them and no ray left out; 50 on the grids with density on their outermost layer (`edge`: faces, ragged, one-cell).
There the families are drawn with ref=True, and that parametrisation gives up what the family is named for: `in-plane` uses no
lo or hi face, `faces-start` is 0.05 to 0.45 of a step from the face instead of ulps, `far-origin` stands 10 and 100 diagonals
away, `vertices` starts from interior lattice points.  So on the edge grids the comparison with fp64 does NOT see those cases
(the exact checks do, on every grid); a ray with a sample within its dg of a face is left out (walk_cases.borderline), and the
share left out is capped at BORDERLINE_CAP = 2 % per family and grid.  On `one-cell` next to no ray meets the cell: the
comparison there is of misses.

The span walk is held to occupancy_ref.spans_ref: `hit` is equal on every ray `grazing` does not flag; t0 and t1 are within
span_tolerance, evaluated with the smallest NON-ZERO |d_k| (a zero component produces no t; for `shallow` this divides by the
tiny component and the gate is then loose, which is what five roundings of a t of that size come to); the tolerance is taken
ray by ray, so that its M is the ray's own |o| (worst err / gate measured: 0.06).  `vertices` and `in-plane` rays that are not
grazing touch no occupied cell: for them the check is of the hit flag and of t0 = t1 = far.  The grazing share per
family is printed and capped at GRAZING_CAP[family]: the largest share the reference alone gives over the five grids and the two
ray sets of this file (vertices 0.472 and in-plane 0.870 -- such rays run along cell faces and edges by construction -- shallow
0.230, faces-start 0.083, far-origin 0.090, caps 0.020, random-wide 0.056) plus a margin of 0.05.  On every ray, grazing or not:
t0 <= t1 <= far, and t0 = t1 = far on a miss.

Which of the branches these rays reach was counted once, with counters in a scratch copy of the two kernel files (host side):
baked_propose's K - 1 clamp 90 940 times in 10.2 M proposals, the K cap, the box jump taken 448 k times and refused 4.5 M, the
brick jump taken 538 k and the cell jump 592 k times, refused 1.6 M; in occ_walk 199 ties of tx.  NOT reached by any of these
rays: the correction of occ_cell_of (either way), a NaN at its cast, and the end of the walk's budget."""
import time

import numpy as np
import pytest
import torch

import walk_cases as wc
from walk_checks import CONFIGS, N_PLAIN, N_REF, N_SAN, N_SPAN, REF_CONFIGS, check_exact, check_spans, compare_fp64, host_build, restate_ahead, run_march, run_spans

SANITIZE = not torch.cuda.is_available()  # sanitizer runs belong on a machine without a GPU

pytestmark = pytest.mark.skipif(host_build.hipcc() is None, reason="hipcc is not installed")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("walk_host"))
    t = time.time()
    from concurrent.futures import ThreadPoolExecutor
    jobs = [(san, name) for san in ((False, True) if SANITIZE else (False,)) for name in host_build.PROGRAMS]
    with ThreadPoolExecutor(len(jobs)) as pool:  # (the compilers are child processes: they run side by side)
        done = list(pool.map(lambda j: host_build.build(out, sanitize=j[0], names=(j[1],)), jobs))
    built = {}
    for (san, name), exe in zip(jobs, done):
        built.setdefault(san, {}).update(exe)
    print(f"host programs built in {time.time() - t:.1f} s")
    return built


def exact_runs(exe, tmp_path, name, n, seed):
    S = wc.scene(name)
    total = [0, 0, 0]
    for step_name, stop in CONFIGS:
        step = wc.steps(name)[step_name]
        rays, fam = wc.rays_of(n, seed, S["cells"], step)
        out = run_march(exe, tmp_path, name, rays, step, stop)
        got = check_exact(out, fam, stop, (name, step_name, stop))
        total = [a + b for a, b in zip(total, got)]
        if step_name == "tenth" and stop == 0:
            big = out["K"] == 4194304
            assert big.sum() == 2 and (out["count"][0, big] > 0).all()  # the K cap is reached, on rays that cross the box
            jumped = (out["count"][1] < out["count"][0]) & (out["count"][0] > 0)
            assert jumped.mean() > 0.2  # the bits do skip samples that the march without them visits
    print(f"{name}: {total[0]} rays per (layout, degree); samples visited with the bits {total[1]}, without {total[2]}")
    return total


@pytest.mark.parametrize("name", list(wc.GRIDS))
def test_the_walk_visits_brute_forces_samples_and_the_marches_agree_bit_for_bit(programs, tmp_path, name):
    t = time.time()
    total = exact_runs(programs[False]["baked_host"], tmp_path, name, N_PLAIN, 1)
    print(f"{name}: {time.time() - t:.1f} s")
    assert total[0] >= 20000 and total[1] > 0 and total[2] > total[1]


@pytest.mark.skipif(not SANITIZE, reason="sanitizer runs belong on a machine without a GPU")
@pytest.mark.parametrize("name", list(wc.GRIDS))
def test_the_marcher_is_clean_under_the_sanitizers(programs, tmp_path, name):
    total = exact_runs(programs[True]["baked_host"], tmp_path, name, N_SAN, 2)
    assert total[0] >= 2000


@pytest.mark.parametrize("name", list(wc.GRIDS))
def test_the_host_march_is_within_the_fp64_restatements_gates(programs, tmp_path, name):
    S = wc.scene(name)
    hits = 0
    cases = []
    for step_name, stop in REF_CONFIGS:
        step = wc.steps(name)[step_name]
        cases.append((step_name, step, stop) + wc.rays_of(N_REF[S["edge"]], 3, S["cells"], step, ref=S["edge"], big=False))
    restate_ahead([(name, degree, rays, step, stop) for _, step, stop, rays, _ in cases for degree in (0, 1, 2)])
    for step_name, step, stop, rays, fam in cases:
        out = run_march(programs[False]["baked_host"], tmp_path, name, rays, step, stop)
        for degree in (0, 1, 2):
            worst, left, n = compare_fp64(name, degree, rays, fam, step, stop, out["march"][degree * 4 + 1].view(np.float32))[:3]
            hits = max(hits, n)
            print(f"{name} {step_name} stop {stop} degree {degree}: worst err / gate {worst:.3f}, left out {left:.4f}, {n} rays hit")
    if name != "one-cell":  # (a single cell in a far corner is seldom met: there the comparison is of misses)
        assert hits >= 20


@pytest.mark.parametrize("name", list(wc.GRIDS))
def test_the_span_walk_gives_brute_forces_spans(programs, tmp_path, name):
    S = wc.scene(name)
    rays, fam = wc.rays_of(N_SPAN, 4, S["cells"], wc.steps(name)["cell"], big=False)
    t0, t1, hit = run_spans(programs[False]["occ_host"], tmp_path, name, rays)
    hits = check_spans(name, rays, fam, t0, t1, hit)
    if name != "one-cell":  # (a single cell is seldom hit: its spans are misses, and the one-cell rays of the marcher's exact checks hit it)
        assert hits >= 50
    if SANITIZE:
        small, fam2 = wc.rays_of(N_SAN, 5, S["cells"], wc.steps(name)["cell"], big=False)
        check_spans(name, small, fam2, *run_spans(programs[True]["occ_host"], tmp_path, name, small))
