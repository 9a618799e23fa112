"""The embedding kernels of csrc/rays.hip (upnerf_embed_bwd, upnerf_embed_bwd_grouped, upnerf_embed_fwd_grouped) and
upnerf_matvec / upnerf_matvec_rank1 (csrc/gemm.hip) through the C ABI.  tests/test_hip_kernels.py reaches the embedding kernels
only through ops.embed_rows at R <= 5000 (the grouped kernel: R <= 3000, one LDS trip of 4096 indices) and the matrix-vector
kernel at one shape, M = 128, K = 384, trans = 1.

Part 1, embedding backward (per-table and grouped).  Both kernels document a fixed order -- increasing ray index, no atomics --
so the first reference is the sequential fp32 sum in ray order on the CPU (np.add.at on float32) and has to match BIT FOR BIT;
the second is the fp64 sum with the gate count u sum |g| per element (count = that table row's number of hits, u = 2^-24: a
chain of count - 1 additions), which a row without a hit meets only with exact zeros.  R crosses the per-table kernel's 64-wide
trips and the grouped kernel's 4096-wide LDS trips (4095, 4096, 4097, 8193: a second and a third trip behind a barrier), N goes
below the four waves of a workgroup, dim crosses the 64-lane quarters.  Index families: uniform; every ray on one row; one row
never hit; one row hit only in the last 64 rays of the second LDS trip (R <= 4096: of the only trip); and indices -1, N, 2^31,
2^32 + 1 mixed in, which both kernels have to ignore -- row 1, which (int)(2^32 + 1) aliases, keeps its in-range sum.
The grouped kernel (ngroups 1, 2, 8, mixed dims) is bitwise the per-table kernel table by table.
Part 2, upnerf_embed_fwd_grouped: rows bitwise the table's; an index outside [0, N) gives an all-NaN row and touches nothing else.
Part 3, upnerf_matvec / upnerf_matvec_rank1 against fp64: y within L u (sum |a| |x| + |add|), L = M + 1 (trans = 1) or K + 1
(trans = 0); R within 2 u (|R0| + |x v|) (one product and one sum, or one fused operation); rank1's y bitwise matvec's.
Sentinel rows stand behind every output, NaN in the padding columns of A, sentinels in those of R.  Refusals return UPNERF_EINVAL.

Worst measured ratio error / gate on an MI355X (gate: <= 1):
    part 1  fp64 gate, per-table and grouped   0.50  (a row hit twice: one addition, rounded to half an ulp, against 2 u sum |g|;
                                                     the bit-for-bit comparison with the sequential fp32 sum is the stronger check)
    part 3  y, trans = 0                       0.062 (0.49 at K = 1: one product and one sum)
            y, trans = 1                       0.19  (0.77 at M = 1)
            R of upnerf_matvec_rank1           0.50
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dense_ref as dr

pytestmark = pytest.mark.gpu

SENT = -7.25
EINVAL = -1  # UPNERF_EINVAL (include/upnerf_hip.h)
WORST = {}
CHUNK = 4096  # csrc/rays.hip: EMB_CHUNK


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib
    return dict(L=_lib, lib=_lib.lib)


def note(part, r):
    """Keeps the worst ratio of a part and prints it (pytest -s shows the figures before the assertion)."""
    WORST[part] = r if math.isnan(r) else max(WORST.get(part, 0.0), r)
    print(f"[embed] {part}: ratio {r:.3f} (worst so far {WORST[part]:.3f})")
    return r


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def padded(rows, dim, extra=4):
    """A device buffer of rows + extra rows, all sentinel."""
    return torch.full((rows + extra, dim), SENT, device="cuda")


def body(buf, rows):
    c = buf.detach().cpu().numpy()
    assert (c[rows:] == SENT).all(), "sentinel rows overwritten"
    return c[:rows]


# ========================================================================================= 1. embedding backward, direct
# (R, N, dim): every value of R in {1, 63, 64, 65, 4095, 4096, 4097, 8193}, N in {1, 3, 4, 5, 97} and
# dim in {1, 2, 63, 64, 65, 128, 255, 256}
EMBED_SHAPES = [(1, 1, 1), (1, 97, 256), (63, 3, 2), (63, 5, 255), (64, 4, 63), (64, 97, 64), (65, 5, 65), (65, 1, 128),
                (4095, 3, 256), (4095, 97, 1), (4096, 4, 128), (4096, 5, 63), (4097, 5, 255), (4097, 1, 64), (4097, 97, 2),
                (8193, 1, 256), (8193, 1, 1), (8193, 3, 65), (8193, 4, 255), (8193, 97, 256), (8193, 5, 64)]
OUTSIDE = (-1, None, 2 ** 31, 2 ** 32 + 1)  # None: N itself
INDEX_FAMILIES = ("uniform", "one_row", "never", "late", "outside")


def indices(fam, R, N, seed):
    """int64 [R] of one index family (module docstring)."""
    g = np.random.default_rng(seed)
    idx = g.integers(0, N, R).astype(np.int64)
    if fam == "one_row":
        idx[:] = N - 1
    elif fam == "never":  # row N // 2 is never hit (N = 1: nobody is hit at all -- every index is outside)
        idx[idx == N // 2] = (N // 2 + 1) % N if N > 1 else -1
    elif fam == "late":  # row 0 only in the last 64 rays of the second LDS trip (of the only one when R <= 4096)
        end = min(R, 2 * CHUNK)
        lo = max(end - 64, CHUNK if R > CHUNK else 0)
        idx[idx == 0] = (1 % N) if N > 1 else -1
        idx[lo:end] = 0
    elif fam == "outside":
        for j in range(0, R, 3):
            o = OUTSIDE[(j // 3) % 4]
            idx[j] = N if o is None else o
    return idx


def embed_refs(idx, g, N):
    """(sequential fp32 sum in ray order, fp64 sum, gate count u sum |g|) of the rows with an index inside [0, N)."""
    ok = (idx >= 0) & (idx < N)
    seq = np.zeros((N, g.shape[1]), np.float32)
    np.add.at(seq, idx[ok], g[ok])
    ref = np.zeros((N, g.shape[1]), np.float64)
    np.add.at(ref, idx[ok], g[ok].astype(np.float64))
    mag = np.zeros_like(ref)
    np.add.at(mag, idx[ok], np.abs(g[ok]).astype(np.float64))
    count = np.bincount(idx[ok], minlength=N).astype(np.float64)
    return seq, ref, count[:, None] * dr.U * mag, count


def groups_of(L, cls, firsts, seconds, dims):
    arr = (cls * len(dims))()
    for j, (a, b, d) in enumerate(zip(firsts, seconds, dims)):
        arr[j] = cls(a.data_ptr(), b.data_ptr(), d)
    return arr


@pytest.mark.parametrize("R,N,dim", EMBED_SHAPES)
def test_embed_bwd_direct(hip, R, N, dim):
    L, lib = hip["L"], hip["lib"]
    rng = np.random.default_rng(R * 1000 + N * 10 + dim)
    g = rng.standard_normal((R, dim)).astype(np.float32)
    gd = torch.from_numpy(g).cuda()
    for k, fam in enumerate(INDEX_FAMILIES):
        idx = indices(fam, R, N, 31 * R + N + k)
        seq, ref, gate, count = embed_refs(idx, g, N)
        if fam == "never":
            assert count[N // 2] == 0
        if fam == "late" and R > CHUNK:
            hits = np.nonzero(idx == 0)[0]
            assert hits.min() >= CHUNK and hits.max() < 2 * CHUNK and hits.min() >= min(R, 2 * CHUNK) - 64
        if fam == "outside":
            assert set(OUTSIDE) - {None} <= set(idx.tolist()) or R < 12
        idxd = torch.from_numpy(idx).cuda()
        out1, out2 = padded(N, dim), padded(N, dim)
        assert lib.upnerf_embed_bwd(R, N, dim, idxd.data_ptr(), gd.data_ptr(), out1.data_ptr(), None) == 0
        arr = groups_of(L, L.EmbedGroup, [gd], [out2], [dim])
        assert lib.upnerf_embed_bwd_grouped(R, N, idxd.data_ptr(), arr, 1, None) == 0
        torch.cuda.synchronize()
        for name, out in (("per-table", body(out1, N)), ("grouped", body(out2, N))):
            assert np.array_equal(bits(out), bits(seq)), (name, fam, R, N, dim, "not the sequential fp32 sum in ray order")
            r = note(f"part 1 {name}", dr.ratio(torch.from_numpy(out), torch.from_numpy(ref), torch.from_numpy(gate)))
            assert r <= 1, (name, fam, R, N, dim, r)
            assert (out[count == 0] == 0).all()


@pytest.mark.parametrize("R,N", [(65, 3), (4097, 5), (8193, 1), (8193, 97)])
@pytest.mark.parametrize("dims", [(256, 1), (256, 1, 63, 64, 65, 128, 255, 2), (1, 255, 2, 256, 128, 65, 64, 63)], ids=["2", "8a", "8b"])
def test_embed_bwd_grouped_is_the_per_table_kernel(hip, R, N, dims):
    L, lib = hip["L"], hip["lib"]
    rng = np.random.default_rng(R + N + len(dims))
    gs = [rng.standard_normal((R, d)).astype(np.float32) for d in dims]
    gds = [torch.from_numpy(x).cuda() for x in gs]
    for fam in ("uniform", "late", "outside"):
        idx = indices(fam, R, N, R + 7 * N)
        idxd = torch.from_numpy(idx).cuda()
        outs = [padded(N, d) for d in dims]
        arr = groups_of(L, L.EmbedGroup, gds, outs, dims)
        assert lib.upnerf_embed_bwd_grouped(R, N, idxd.data_ptr(), arr, len(dims), None) == 0
        torch.cuda.synchronize()
        for j, d in enumerate(dims):
            single = padded(N, d)
            assert lib.upnerf_embed_bwd(R, N, d, idxd.data_ptr(), gds[j].data_ptr(), single.data_ptr(), None) == 0
            torch.cuda.synchronize()
            got, one = body(outs[j], N), body(single, N)
            assert np.array_equal(bits(got), bits(one)), (fam, R, N, j, d)
            seq, ref, gate, _ = embed_refs(idx, gs[j], N)
            assert np.array_equal(bits(got), bits(seq)), (fam, R, N, j, d)
            assert note("part 1 grouped", dr.ratio(torch.from_numpy(got), torch.from_numpy(ref), torch.from_numpy(gate))) <= 1


def test_embed_refusals(hip):
    L, lib = hip["L"], hip["lib"]
    R, N = 5, 3
    idx = torch.zeros(R, dtype=torch.int64, device="cuda")
    g, out, tab = torch.zeros(R, 256, device="cuda"), padded(N, 256), torch.zeros(N, 256, device="cuda")
    rows = padded(R, 256)
    for cls, fn, a, b in ((L.EmbedGroup, lib.upnerf_embed_bwd_grouped, g, out), (L.EmbedRowsGroup, lib.upnerf_embed_fwd_grouped, tab, rows)):
        nine = groups_of(L, cls, [a] * 9, [b] * 9, [4] * 9)
        assert fn(R, N, idx.data_ptr(), nine, 0, None) == EINVAL and fn(R, N, idx.data_ptr(), nine, 9, None) == EINVAL
        assert fn(R, N, idx.data_ptr(), nine, -1, None) == EINVAL and fn(R, N, idx.data_ptr(), None, 1, None) == EINVAL
        for dim in (0, 257, -1):
            two = groups_of(L, cls, [a, a], [b, b], [4, dim])
            assert fn(R, N, idx.data_ptr(), two, 2, None) == EINVAL, dim
        assert fn(0, N, idx.data_ptr(), nine, 1, None) == EINVAL and fn(R, 0, idx.data_ptr(), nine, 1, None) == EINVAL
        assert fn(R, N, None, nine, 1, None) == EINVAL
    for dim in (0, 257):
        assert lib.upnerf_embed_bwd(R, N, dim, idx.data_ptr(), g.data_ptr(), out.data_ptr(), None) == EINVAL
    assert lib.upnerf_embed_bwd(0, N, 4, idx.data_ptr(), g.data_ptr(), out.data_ptr(), None) == EINVAL
    assert lib.upnerf_embed_bwd(R, N, 4, None, g.data_ptr(), out.data_ptr(), None) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((rows == SENT).all()), "a refused call wrote something"


# =============================================================================================== 2. embedding forward, direct
@pytest.mark.parametrize("R", [1, 3, 4, 5, 777])
@pytest.mark.parametrize("N", [1, 5, 97])
def test_embed_fwd_grouped_direct(hip, R, N):
    L, lib = hip["L"], hip["lib"]
    rng = np.random.default_rng(R + N)
    for dims in ((1,), (256, 1), (1, 2, 63, 64, 65, 128, 255, 256)):
        tabs = [rng.standard_normal((N, d)).astype(np.float32) for d in dims]
        tds = [torch.from_numpy(t).cuda() for t in tabs]
        for fam in ("uniform", "outside"):
            idx = indices(fam, R, N, 5 * R + N)
            idxd = torch.from_numpy(idx).cuda()
            outs = [padded(R, d) for d in dims]
            arr = groups_of(L, L.EmbedRowsGroup, tds, outs, dims)
            assert lib.upnerf_embed_fwd_grouped(R, N, idxd.data_ptr(), arr, len(dims), None) == 0
            torch.cuda.synchronize()
            ok = (idx >= 0) & (idx < N)
            assert fam != "outside" or not ok[0]
            for t, o, d in zip(tabs, outs, dims):
                got = body(o, R)
                assert np.array_equal(bits(got[ok]), bits(t[idx[ok]])), (R, N, d, fam)
                assert np.isnan(got[~ok]).all(), (R, N, d, fam)


# ====================================================================================== 3. upnerf_matvec, upnerf_matvec_rank1
# every M in {1, 15, 16, 17, 127, 128, 129, 300} and K in {1, 15, 16, 17, 384}
MATVEC_SHAPES = [(1, 1), (1, 384), (15, 16), (15, 1), (16, 15), (16, 384), (17, 17), (127, 384), (127, 15), (128, 1), (128, 16),
                 (129, 17), (129, 384), (300, 384), (300, 15), (300, 1)]


@pytest.mark.parametrize("M,K", MATVEC_SHAPES)
def test_matvec_and_rank1(hip, M, K):
    lib = hip["lib"]
    for fam in ("flat", "rows12"):
        A = dr.flat((M, K), 900 + M + K)
        if fam == "rows12":
            A[sorted({0, M // 2, M - 1})] *= 4096.0
        lda = K + 3
        Aw = torch.full((M, lda), float("nan"))
        Aw[:, :K] = A
        Aw = Aw.cuda()
        ys = {}
        for trans in (0, 1):
            n_in, n_out = (M, K) if trans else (K, M)
            x, add = dr.flat((n_in,), 901 + M + K + trans), dr.flat((n_out,), 903 + M + K + trans) * 3.0
            Ad = A.double() if not trans else A.double().t()
            xd, addd = x.cuda(), add.cuda()
            for has_add in (False, True):
                ref = Ad @ x.double() + (add.double() if has_add else 0.0)
                S = Ad.abs() @ x.double().abs() + (add.double().abs() if has_add else 0.0)
                gate = dr.gate_fp32(n_in + 1, S)
                res = []
                for _ in range(2):
                    y = torch.full((n_out + 4,), SENT, device="cuda")
                    assert lib.upnerf_matvec(M, K, Aw.data_ptr(), lda, xd.data_ptr(), addd.data_ptr() if has_add else None,
                                             y.data_ptr(), trans, None) == 0
                    torch.cuda.synchronize()
                    res.append(y.cpu())
                assert torch.equal(res[0], res[1]) and bool((res[0][n_out:] == SENT).all())
                r = note(f"part 3 y trans={trans}" + (" (M or K = 1)" if n_in == 1 else ""), dr.ratio(res[0][:n_out], ref, gate))
                assert r <= 1, (fam, M, K, trans, has_add, r)
                ys[(trans, has_add)] = res[0][:n_out]
            if trans:  # rank1: the same y bit for bit, and R += x (x) v
                v, R0 = dr.flat((K,), 905 + M + K), dr.flat((M, K), 906 + M + K)
                ldr = K + 5
                Rw = torch.full((M + 2, ldr), SENT)
                Rw[:M, :K] = R0
                Rw = Rw.cuda()
                y = torch.full((K + 4,), SENT, device="cuda")
                vd = v.cuda()
                assert lib.upnerf_matvec_rank1(M, K, Aw.data_ptr(), lda, xd.data_ptr(), y.data_ptr(), Rw.data_ptr(), ldr, vd.data_ptr(),
                                               None) == 0
                torch.cuda.synchronize()
                y, Rw = y.cpu(), Rw.cpu()
                assert bool((y[K:] == SENT).all()) and bool((Rw[:M, K:] == SENT).all()) and bool((Rw[M:] == SENT).all())
                assert torch.equal(y[:K].view(torch.int32), ys[(1, False)].view(torch.int32)), (fam, M, K)
                xv = x.double()[:, None] * v.double()[None, :]
                r = note("part 3 R", dr.ratio(Rw[:M, :K], R0.double() + xv, 2 * dr.U * (R0.double().abs() + xv.abs())))
                assert r <= 1, (fam, M, K, r)


def test_matvec_refusals(hip):
    lib = hip["lib"]
    M, K = 5, 8
    A, x, v = torch.zeros(M, K, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    y, R = torch.full((12,), SENT, device="cuda"), torch.full((M, K), SENT, device="cuda")
    p = lambda t: t.data_ptr()
    for trans in (0, 1):
        assert lib.upnerf_matvec(M, K, p(A), K - 1, p(x), None, p(y), trans, None) == EINVAL
        assert lib.upnerf_matvec(0, K, p(A), K, p(x), None, p(y), trans, None) == EINVAL
        assert lib.upnerf_matvec(M, 0, p(A), K, p(x), None, p(y), trans, None) == EINVAL
        assert lib.upnerf_matvec(M, K, None, K, p(x), None, p(y), trans, None) == EINVAL
    assert lib.upnerf_matvec_rank1(M, K, p(A), K - 1, p(x), p(y), p(R), K, p(v), None) == EINVAL
    assert lib.upnerf_matvec_rank1(M, K, p(A), K, p(x), p(y), p(R), K - 1, p(v), None) == EINVAL
    assert lib.upnerf_matvec_rank1(M, K, p(A), K, p(x), p(y), None, K, p(v), None) == EINVAL
    assert lib.upnerf_matvec_rank1(M, K, p(A), K, p(x), p(y), p(R), K, None, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((R == SENT).all()), "a refused call wrote something"
