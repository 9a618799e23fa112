"""tests/prologue_ref.py on the CPU: the fp32 restatements are pinned bit for bit to the oracle and to tests/kernel_space.py, the
Philox restatement to the published known-answer vectors, and every case list of tests/test_hip_prologue.py is generated here
with the conditions that test relies on asserted -- margins of the random inputs from every branch point, exactly representable
planted values, monotone coarse-depth rows inside [near, far] -- together with e32 = |fp32 - fp64| of each list."""
import numpy as np
import pytest
import torch

import kernel_space as ks
import prologue_ref as pr
from golden_util import orc

F32, F64 = torch.float32, torch.float64


def _gen(shape, seed, lo=-1.0, hi=1.0):  # test_hip_kernels.gen
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _exact32(x):
    return float(np.float32(x)) == float(x)


# ------------------------------------------------------------------------------------------ Philox
def test_philox_restatement_gives_the_published_known_answers():
    """Philox4x32-10 known-answer vectors of Salmon et al. (Random123's kat_vectors): counter, key -> output."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))
    for ctr, key, out in kat:
        got = pr.philox4x32_10(np.array([ctr], dtype=np.uint32), key)
        assert [int(v) for v in got[0]] == list(out), (ctr, key)


def test_philox_uniform_is_the_counter_layout_of_the_kernel():
    """Row r, column c = word c & 3 of the block with counter (row, c // 4, step, draw) and key (seed lo, seed hi), as
    (x >> 8) 2^-24: in [0, 1), 24 bits; a row depends on its GLOBAL number only, and the tail n % 4 != 0 cuts a block short."""
    seed, step, draw = (0xFFFFFFFF << 32) | 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF
    u = pr.philox_uniform(seed, step, [0xFFFFFFFF], 4, draw)  # the second known answer, through the wrapper (column block 0 ...
    assert u.dtype == np.float32 and u.shape == (1, 4)
    blk1 = pr.philox4x32_10(np.array([[0xFFFFFFFF, 1, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint32), (0xFFFFFFFF, 0xFFFFFFFF))[0]
    u7 = pr.philox_uniform(seed, step, [0xFFFFFFFF], 7, draw)  # ... and block 1 behind it)
    assert np.array_equal(u7[0, :4], u[0]) and [int(v) for v in (u7[0, 4:] * 2.0 ** 24)] == [int(v) >> 8 for v in blk1[:3]]
    zero = pr.philox_uniform(0, 0, [0], 4, 0)
    assert [int(v) for v in zero[0] * 2 ** 24] == [0x6627E8D5 >> 8, 0xE169C58D >> 8, 0xBC57AC4C >> 8, 0x9B00DBD8 >> 8]
    k = pr.UNIFORM_KEY
    assert k["seed"] >> 32 != 0 and k["row0"] + k["row_stride"] * (max(pr.UNIFORM_R) - 1) > 2 ** 16
    rows = k["row0"] + k["row_stride"] * np.arange(9)
    for n in pr.UNIFORM_N:
        a = pr.philox_uniform(k["seed"], k["step"], rows, n, 1)
        assert a.shape == (9, n) and a.min() >= 0.0 and a.max() < 1.0 and np.array_equal(a * 2.0 ** 24, np.round(a * 2.0 ** 24))
        assert np.array_equal(a, pr.philox_uniform(k["seed"], k["step"], rows, 132, 1)[:, :n])
        assert np.array_equal(a[3:5], pr.philox_uniform(k["seed"], k["step"], rows[3:5], n, 1))
    # every field of the key moves the draws
    base = pr.philox_uniform(k["seed"], k["step"], rows, 8, 0)
    for other in (pr.philox_uniform(k["seed"] ^ (1 << 32), k["step"], rows, 8, 0), pr.philox_uniform(k["seed"] ^ 1, k["step"], rows, 8, 0),
                  pr.philox_uniform(k["seed"], k["step"] + 1, rows, 8, 0), pr.philox_uniform(k["seed"], k["step"], rows + 1, 8, 0),
                  pr.philox_uniform(k["seed"], k["step"], rows, 8, 1)):
        assert not np.any(other == base)
    assert float(np.float32(pr.KEYED["step"])) == pr.KEYED["step"] == 2 ** 24 - 1  # the largest odd step fp32 holds: step_dev is exact
    assert pr.KEYED["seed"] >> 32 != 0 and pr.U_MAX == float(np.float32(pr.U_MAX)) and np.nextafter(np.float32(pr.U_MAX), np.float32(2)) == 1.0


# ------------------------------------------------------------------------------------------ coarse depths
@pytest.mark.parametrize("S,perturb,disp", [(64, 0.0, False), (64, 1.0, False), (48, 0.5, True), (128, 1.0, False)])
def test_coarse_restatement_in_fp32_is_the_oracle_bit_for_bit(S, perturb, disp):
    """On the inputs of test_hip_kernels.test_sample_coarse."""
    R = 33
    nf = torch.stack([_gen((R,), 7, 0.05, 0.3), _gen((R,), 8, 3.0, 6.0)], 1)
    u = _gen((R, S), 9, 0.0, 1.0)
    ref = orc.coarse_depths(nf[:, :1], nf[:, 1:], S, disp, perturb, u if perturb > 0 else None)
    got = pr.coarse_depths(nf, torch.linspace(0, 1, S), u, perturb, disp, F32)
    assert got.dtype == F32 and np.array_equal(got.numpy(), ref.numpy())


@pytest.mark.parametrize("R,S", pr.COARSE_SHAPES)
def test_coarse_cases_hold_what_the_gpu_test_relies_on(R, S):
    nf, steps, u = pr.coarse_case(R, S)
    K = len(pr.COARSE_PLANTED)
    assert R >= K + 3 and nf.dtype == steps.dtype == u.dtype == F32
    near, far = nf[:, :1], nf[:, 1:]
    # the only branch of the arithmetic is near < far: a margin for the random rows, exact values for the planted ones
    assert bool((far - near >= 1e-3)[:R - K].all()) and bool((near > 0).all())
    assert all(_exact32(v) for row in pr.COARSE_PLANTED for v in row) and nf[R - K:].tolist() == [list(r) for r in pr.COARSE_PLANTED]
    assert bool((1 / (1 / nf) == nf).all())  # column 0 / the last column of disparity mode are near / far themselves
    assert bool((u[0] == 0).all()) and bool((u[1] == np.float32(pr.U_MAX)).all()) and 0.0 <= float(u.min()) and float(u.max()) < 1.0
    assert bool((steps[1:] > steps[:-1]).all()) and float(steps[0]) == 0.0 and (S == 1 or float(steps[-1]) == 1.0)
    worst = 0.0
    for disp in (0, 1):
        for keyed in (False, True):
            for perturb in pr.PERTURBS:
                if keyed and perturb == 0:
                    continue
                z32, z64, lo32 = pr.coarse_refs(R, S, disp, perturb, keyed)
                assert z32.dtype == F32 and z64.dtype == F64 and z32.shape == (R, S)
                assert bool((z32[:, 1:] >= z32[:, :-1]).all()), (disp, perturb, keyed)
                assert bool((z32 >= near).all()) and bool((z32 <= far).all()), (disp, perturb, keyed)
                assert bool((z32[R - K] == 2.0).all())  # near == far: every depth is that value
                if perturb == 0:
                    assert torch.equal(z32[:, 0], nf[:, 0]) and (S == 1 or torch.equal(z32[:, -1], nf[:, 1]))
                    assert torch.equal(z32, lo32)
                elif not keyed:
                    assert torch.equal(z32[0], lo32[0])  # u = 0: the lower bin edge
                e32 = (z32.double() - z64).abs()
                worst = max(worst, float((e32 / z64.abs()).max()))
    assert worst < 16 * 2.0 ** -24  # e32 is rounding error, not another branch: a dozen operations of 2^-24 each
    print(f"coarse R={R} S={S}: max e32 / |z| = {worst / 2.0 ** -24:.2f} x 2^-24")


def test_keyed_coarse_draws_are_the_planted_key():
    k = pr.KEYED
    assert (k["row0"], k["row_stride"]) == (5, 3)
    u = pr.keyed_u(7, 65)
    assert u.shape == (7, 65) and torch.equal(u[2:3], torch.from_numpy(pr.philox_uniform(k["seed"], k["step"], [11], 65, 0)))


# ------------------------------------------------------------------------------------------ direction encoding
@pytest.mark.parametrize("R", pr.AUX_R)
def test_aux_restatement_and_cases(R):
    d, a = pr.aux_case(R)
    K = min(R, len(pr.AUX_PLANTED))
    assert d.dtype == a.dtype == F32 and d[R - K:].tolist() == [list(r) for r in pr.AUX_PLANTED[:K]]
    nrm = d[:R - K].double().norm(dim=1)
    assert bool(((nrm[0::2] - 1).abs() < 1e-6).all()) and bool((nrm[1::2] > 1.04).all()) and bool((nrm <= 4.0).all())
    if R > 100:
        assert float(nrm.max()) > 3.5
    worst = 0.0
    for wk in pr.AUX_WK:
        assert all(_exact32(w) for w in wk)
        for rows in (a, None):
            r32, r64 = pr.ray_aux(d, rows, wk, F32), pr.ray_aux(d, rows, wk, F64)
            assert r32.dtype == F32 and r64.dtype == F64 and r32.shape == (R, pr.AUXK) == (R, ks.AUXK)
            assert torch.equal(r32, ks.ray_aux(d, rows, list(wk)))  # tests/kernel_space.py stays the fp32 statement
            assert torch.equal(r32[:, :3], d) and float(r32[:, 75:].abs().max()) == 0.0
            assert torch.equal(r32[:, 27:75], a if rows is not None else torch.zeros(R, 48))
            for k in range(4):
                if wk[k] == 0:
                    cols = [3 + 8 * n + 4 * t + k for n in range(3) for t in range(2)]
                    assert float(r32[:, cols].abs().max()) == 0.0 and float(r64[:, cols].abs().max()) == 0.0
            # the arguments are the kernel's: an ulp of d fl32(pi) 2^k moves sine and cosine by at most |arg| 2^-24
            e32 = (r32.double() - r64).abs()
            bound = (d.double().abs() * (np.pi * 8) * 2.0 ** -24 + 2.0 ** -23).max()
            assert float(e32.max()) <= float(bound)
            worst = max(worst, float(e32.max()))
    # (0, 0, 0, 1) against its reverse: the two band orders differ on every row but the all-zero direction
    fwd, rev = pr.ray_aux(d, None, (0.0, 0.0, 0.0, 1.0), F64), pr.ray_aux(d, None, (1.0, 0.0, 0.0, 0.0), F64)
    differ = ((fwd - rev).abs().max(1)[0] > 0.5)
    assert bool(differ.all())  # cos(0) weighted by the wrong band is off by 1 on the zero direction too
    print(f"ray_aux R={R}: max e32 = {worst:.3e}")


# ------------------------------------------------------------------------------------------ ray gather
@pytest.mark.parametrize("h", pr.GATHER_H)
@pytest.mark.parametrize("C", pr.GATHER_C)
def test_gather_cases_and_the_vectorised_bilinear(C, h):
    bufs, n_planted = pr.gather_case(C, h)
    N = pr.GATHER_N
    assert bufs["feat_maps"].shape == (pr.GATHER_I, h, h, C) and n_planted <= 256 and n_planted % 3 == 0
    pxl = bufs["all_pxl_coords"]
    assert float(pxl.min()) >= 0.0 and float(pxl.max()) <= 1.0
    P = pr.planted_coords(h)
    want = {0.0, 1.0, float(np.nextafter(np.float32(0), np.float32(1))), float(np.nextafter(np.float32(1), np.float32(0)))}
    if h == 9:
        for k in range(1, 8):
            want |= {k / 8, float(np.nextafter(np.float32(k / 8), np.float32(0))), float(np.nextafter(np.float32(k / 8), np.float32(1)))}
    assert set(P.tolist()) == want
    n = P.numel()
    assert torch.equal(pxl[:n, 0], P) and torch.equal(pxl[n:2 * n, 0], P) and torch.equal(pxl[2 * n:3 * n, 1], P)
    assert set(pxl[:n, 1].tolist()) == want  # paired with a permutation of themselves
    # h - 1 is 0, 1 or 8: the product with a coordinate is exact in fp32, so fp32 and fp64 floor the same number
    prod32, prod64 = pxl * (h - 1), pxl.double() * (h - 1)
    assert torch.equal(prod32.double(), prod64)
    free = torch.ones(N, 2, dtype=torch.bool)
    free[:n], free[n:2 * n, 0], free[2 * n:3 * n, 1] = False, False, False
    if h > 1:
        assert float((prod64 - prod64.round()).abs()[free].min()) >= 1e-3
    assert float(bufs["all_ray_infos"][0, 2]) == pr.GATHER_I - 1 and float(bufs["all_ray_infos"][N - 1, 2]) == 0
    for R in pr.GATHER_R:
        idx = pr.gather_idx(R)
        assert idx.numel() == R and int(idx[0]) == N - 1 and (R < 2 or int(idx[1]) == 0) and (R < 4 or int(idx[2]) == int(idx[3]))
        ref, f32, f64 = pr.gather_refs(C, h, R)
        assert torch.equal(f32, ref["feats"])  # the independent vectorised statement is the oracle's loop, bit for bit
        e32 = (f32.double() - f64).abs()
        mag = pr.bilinear({**bufs, "feat_maps": bufs["feat_maps"].abs()}, idx, F64)  # the four products' magnitudes
        # three roundings in a weight, one in its product, one per addition: below 8 x 2^-24 of the summed magnitudes (and the
        # underflow of a product with a subnormal weight)
        assert bool((e32 <= 8 * 2.0 ** -24 * mag + 4e-45).all())
        last = (pxl[idx] == 1.0).any(1) if h > 1 else torch.ones(R, dtype=torch.bool)
        assert float(f64[last].abs().sum()) == 0.0 and float(f32[last].abs().sum()) == 0.0  # the reference's zero weights
        if h > 1 and int(last.sum()) < R:
            assert float(f64[~last].abs().sum(1).min()) > 0.0
    assert int(pr.gather_idx(261).max()) >= n_planted - 1
