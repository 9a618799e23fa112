"""The dense kernels -- upnerf_wgrad, upnerf_wgrad16 on fp32 rows (planes 0 / 1 / 2, the riding head, n2), upnerf_vec_wgrad,
upnerf_linear, upnerf_frag16 and upnerf_adam -- through the C ABI against fp64 references, at the block-shape, split and exponent
edges that tests/test_hip_kernels.py reaches only through gates normalised by a tensor's maximum.

Every gate is a derived per-element bound computed on the CPU from the inputs, never from a kernel's output; the derivations
(the split constant c = 3 + 2^-8, the subnormal floor 2^-25 (1 + 2^-10) per operand, the M 2^-49 2^-(ea+eb) tail, planes = 0 =
the three-term split) are in the module docstring of tests/dense_ref.py, and tests/test_dense_ref_cpu.py proves on the CPU that
an emulation of the kernels' arithmetic is inside them and that one lost term or one lost ragged column is outside.  In short,
with u = 2^-24, S = |A|^T |B| (+ |bias|) in fp64 and L terms per sum:
    fp32 kernels            L u S                  (column sums, the riding head, vec_wgrad: L u sum |a|)
    planes 0 / 2 (f16x3)    (M u + c 2^-22) S + 2^-25 (1 + 2^-10) (2^-ea sum_m |B| + 2^-eb sum_m |A|) + M 2^-49 2^-(ea+eb)
    planes 1 (f16)          the same with 2^-10 + 2^-22 for c 2^-22
    linear with ReLU        the gate on the pre-activation; exactly 0 where the fp64 pre-activation is below minus the gate
    frag16                  |x - 2^-e (hi + lo)| <= max(2^-22 |x|, 2^-25 2^-e);  wnorm: cols u of the fp64 row 1-norm
    adam                    4 e32 + 2^-22 scale (e32: the formula of csrc/gemm.hip:adam_update in fp32 on the CPU against fp64)
M <= 512 everywhere: on the flat family (|a|, |b| in [0.5, 1]) one lost or duplicated term moves an element by >= S / (4 M),
more than ten times the fp32 and f16x3 gates.  Where a bound is 0 the result has to be exactly 0; a NaN anywhere fails; no
element is left out.  Input families: dense_ref.family (flat; columns of A at 2^0 .. 2^-20 and, every other one, in fp16's
subnormal range after scaling; three rows of both operands at 2^12; A = 0; maximum exactly 2^p and the float below, p in
{-3, 0, 5}; both operands at 2^-40 and at 2^-60 (ea + eb = 148: the unscale factor is a subnormal fp32 number); A at 2^40).

The row-norm kernel of upnerf_frag16 takes 8 consecutive rows per wave and every descriptor has a multiple of 32 rows (the entry
point refuses anything else), so an 8-row group cannot straddle two descriptors; what part 5 reaches is the flush at a
descriptor's last row with the next group starting the next descriptor, and workgroups (32 rows) that straddle.

Worst measured ratio error / gate on an MI355X (gate: <= 1).  At M = 1 a sum is ONE rounded product, so its error reaches the
bound by construction (u |a b|; planes 1: two operand roundings of 2^-11); the other figures leave the M = 1 cases out:
                                    M = 1    flat family, M >= 31    families 2-6 (M = 200 and 33)
    part 1  upnerf_wgrad            0.998    0.11                    0.25       (column sums db: 0.18 over everything)
            planes 0 / 2            0.61     0.07                    0.42
            planes 1                0.955    0.27                    0.68
    part 2  riding head, n2         0.16
    part 3  upnerf_vec_wgrad        0.967 at M = 1, 0.32 over M in {7, 33, 512}
    part 4  upnerf_linear           0.32
    part 5  upnerf_frag16           0.50     (decode and wnorm together)
    part 6  upnerf_adam             0.25
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dense_ref as dr

pytestmark = pytest.mark.gpu

SENT = -7.25  # sentinel of the padding columns
WORST = {}


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib, ops
    return dict(L=_lib, lib=_lib.lib, ops=ops)


def cpu(t):
    return t.detach().cpu()


def note(part, r):
    """Keeps the worst ratio of a part and prints it (pytest -s shows the figures before the assertion)."""
    WORST[part] = r if math.isnan(r) else max(WORST.get(part, 0.0), r)
    print(f"[dense] {part}: ratio {r:.3f} (worst so far {WORST[part]:.3f})")
    return r


def wide(x, pad_l, pad_r):
    """x as a column block of a wider CUDA tensor whose other columns are NaN: (tensor, element offset, row stride)."""
    M, n = x.shape
    w = torch.full((M, pad_l + n + pad_r), float("nan"))
    w[:, pad_l:pad_l + n] = x
    return w.cuda(), pad_l, pad_l + n + pad_r


def block_shape(N, K):
    """csrc/gemm.hip: wgrad_shape."""
    return (256 if N >= 256 else 128 if N > 64 else 64), (256 if K >= 256 else 128 if K > 64 else 64)


def wgrad_scratch(N, K, nsplit):
    """The comment above wgrad_shape: nsplit * (roundup(N) * roundup(K) + roundup(N)) floats, rounded to the block shape."""
    TN, TK = block_shape(N, K)
    rn, rk = (N + TN - 1) // TN * TN, (K + TK - 1) // TK * TK
    return nsplit * (rn * rk + rn)


# ========================================================================== 1. upnerf_wgrad / upnerf_wgrad16 on fp32 rows
# (N, K) pairs: every one of the nine block shapes, each also ragged; 260 = a second block of 4 live columns
SHAPES = [(64, 64), (64, 60), (64, 72), (64, 260), (68, 64), (128, 64), (132, 128), (132, 72), (128, 256), (132, 260), (260, 60),
          (256, 72), (256, 256), (260, 260)]
MS = (1, 31, 32, 33, 64, 65, 200, 512)
KERNELS = ("fp32", 0, 1, 2)
FAMILY_SHAPES = ((256, 256), (128, 64), (132, 72))


def run_wgrad(hip, kern, A, B, M, N, K, nsplit, with_db, expo=None, v=None, n2=0):
    """One call through the C ABI on column blocks of wider tensors, ldo > K with sentinel padding, run twice (bitwise equal).
    Returns dict(dW [N][K], db or None, dv, dbv) on the CPU."""
    L, lib = hip["L"], hip["lib"]
    Aw, ao, lda = A
    Bw, bo, ldb = B
    ldo = K + 4
    outs = []
    for _ in range(2):
        dW = torch.full((N, ldo), SENT, device="cuda")
        db = torch.full((N + 4,), SENT, device="cuda") if with_db else None
        dv = torch.full((K + 4,), SENT, device="cuda") if v is not None else None
        dbv = torch.full((4,), SENT, device="cuda") if v is not None else None
        if kern == "fp32":
            slabs = torch.full((wgrad_scratch(N, K, nsplit),), float("nan"), device="cuda")
            rc = lib.upnerf_wgrad(M, Aw.data_ptr() + 4 * ao, lda, N, Bw.data_ptr() + 4 * bo, ldb, K, dW.data_ptr(), ldo,
                                  db.data_ptr() if with_db else None, slabs.data_ptr(), nsplit, None)
        else:
            d = L.WgradDesc(M=M, N=N, K=K, planes=kern, A=L.WgradOperand(p=Aw.data_ptr() + 4 * ao, ld=lda, kind=L.WG_F32),
                            B=L.WgradOperand(p=Bw.data_ptr() + 4 * bo, ld=ldb, kind=L.WG_F32), expo_a=expo.data_ptr(),
                            expo_b=expo.data_ptr() + 4, dW=dW.data_ptr(), db=db.data_ptr() if with_db else None, ldo=ldo, nsplit=nsplit)
            if n2:
                d.n2, d.ldo2 = n2, ldo
                d.dW2 = dW.data_ptr() + 4 * n2 * ldo  # rows n2.. of the same image: one comparison covers both destinations
                d.db2 = db.data_ptr() + 4 * n2 if with_db else None
            if v is not None:
                d.v, d.dv, d.dbv = v.data_ptr(), dv.data_ptr(), dbv.data_ptr()
            need = lib.upnerf_wgrad16_scratch(C.byref(d))
            assert need >= wgrad_scratch(N, K, nsplit) and (v is not None or need == wgrad_scratch(N, K, nsplit))
            slabs = torch.full((need,), float("nan"), device="cuda")
            d.slabs = slabs.data_ptr()
            rc = lib.upnerf_wgrad16(C.byref(d), None, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append([None if t is None else cpu(t) for t in (dW, db, dv, dbv)])
    for a, b in zip(*outs):  # bitwise reproducible (NaN-free by the gate below; the sentinels compare equal)
        assert a is None or torch.equal(a, b), (kern, M, N, K, nsplit)
    dW, db, dv, dbv = outs[0]
    assert bool((dW[:, K:] == SENT).all()), "padding columns of dW overwritten"
    res = dict(dW=dW[:, :K])
    if with_db:
        assert bool((db[N:] == SENT).all())
        res["db"] = db[:N]
    if v is not None:
        assert bool((dv[K:] == SENT).all()) and bool((dbv[1:] == SENT).all())
        res["dv"], res["dbv"] = dv[:K], dbv[:1]
    return res


def check_wgrad(hip, fam, M, N, K, seed, nsplits, kernels=KERNELS):
    A, B = dr.family(fam, M, N, K, seed)
    ref = dr.wgrad_ref(A, B)
    Aw, Bw = wide(A, 4, 4), wide(B, 8, 4)
    expo = hip["ops"].scale_exponents(Aw[0][:, 4:4 + N], Bw[0][:, 8:8 + K])
    ea, eb = (int(x) for x in cpu(expo))
    assert (ea, eb) == (dr.host_exponent(A), dr.host_exponent(B)), (fam, ea, eb)
    worst = {}
    for i, ns in enumerate(nsplits):
        gots = {}
        for kern in kernels:
            with_db = (i + KERNELS.index(kern)) % 2 == 0
            got = gots[kern] = run_wgrad(hip, kern, Aw, Bw, M, N, K, ns, with_db, expo)
            gate = dr.gate_fp32(M, ref["S"]) if kern == "fp32" else dr.gate_f16(ref, M, ea, eb, kern)
            key = "fp32" if kern == "fp32" else "planes 1" if kern == 1 else "planes 0/2"
            r = dr.ratio(got["dW"], ref["dW"], gate)
            worst[key] = r if math.isnan(r) else max(worst.get(key, 0.0), r)
            if with_db:
                rb = dr.ratio(got["db"], ref["db"], dr.gate_fp32(M, ref["sa"]))
                worst["db"] = rb if math.isnan(rb) else max(worst.get("db", 0.0), rb)
            if fam == "zeroA":
                assert float(got["dW"].abs().max()) == 0.0 and (not with_db or float(got["db"].abs().max()) == 0.0)
            if fam == "tiny60":  # ea + eb = 148 > 126: neither flushed to zero nor inf
                assert bool(torch.isfinite(got["dW"]).all()) and float(got["dW"].abs().min()) > 0, (kern, M, N, K, ns)
        if 0 in gots and 2 in gots:  # planes 0 and 2 name one arithmetic: the same bits
            assert torch.equal(gots[0]["dW"], gots[2]["dW"]), (fam, M, N, K, ns)
    for k, r in worst.items():
        note(f"part 1 {k}", r)
    bad = {k: r for k, r in worst.items() if not r <= 1}
    assert not bad, (fam, M, N, K, bad)


def nsplits_for(M):
    return (1, 3, (M + 31) // 32 + 2)  # the last one leaves trailing splits without rows


@pytest.mark.parametrize("N,K", SHAPES)
def test_wgrad_flat_family_on_every_block_shape(hip, N, K):
    """All four kernels on the flat family: every M, nsplit in {1, 3, more than ceil(M / 32)}, db present and absent."""
    for j, M in enumerate(MS):
        check_wgrad(hip, "flat", M, N, K, 1000 + 17 * j + N + K, nsplits_for(M))


@pytest.mark.parametrize("fam", [f for f in dr.FAMILIES if f != "flat"])
@pytest.mark.parametrize("N,K", FAMILY_SHAPES)
def test_wgrad_exponent_families(hip, fam, N, K):
    """Families 2-6 on 256 x 256, 128 x 64 and a ragged shape; M = 200 (ragged last chunk) and M = 33."""
    check_wgrad(hip, fam, 200, N, K, 2000 + N, (3,))
    check_wgrad(hip, fam, 33, N, K, 2100 + K, (1, 4))


# ==================================================================================== 2. the riding head and n2, fp32 rows
@pytest.mark.parametrize("fam", ["cols", "rows12"])
def test_wgrad16_riding_head_and_row_split(hip, fam):
    M, N, K = 200, 256, 256
    A, B = dr.family(fam, M, N, K, 31)
    v = dr.family(fam, M, K, 4, 33)[1][:, 0].contiguous() if fam == "rows12" else dr.flat((M,), 33) * 2.0 ** -7
    ref = dr.wgrad_ref(A, B)
    Aw, Bw = wide(A, 4, 4), wide(B, 8, 4)
    expo = hip["ops"].scale_exponents(Aw[0][:, 4:4 + N], Bw[0][:, 8:8 + K])
    ea, eb = (int(x) for x in cpu(expo))
    assert (ea, eb) == (dr.host_exponent(A), dr.host_exponent(B))
    gate = dr.gate_f16(ref, M, ea, eb, 2)
    vd = v.double()
    ref_v, gate_v = vd @ B.double(), dr.gate_fp32(M, vd.abs() @ B.double().abs())
    plain = None
    for ns in (3, 9):  # 9 > ceil(200 / 32): empty trailing splits
        got = run_wgrad(hip, 2, Aw, Bw, M, N, K, ns, True, expo, v=v.cuda())
        rs = [dr.ratio(got["dW"], ref["dW"], gate), dr.ratio(got["db"], ref["db"], dr.gate_fp32(M, ref["sa"])),
              dr.ratio(got["dv"], ref_v, gate_v), dr.ratio(got["dbv"], vd.sum()[None], dr.gate_fp32(M, vd.abs().sum()[None]))]
        split = run_wgrad(hip, 2, Aw, Bw, M, N, K, ns, True, expo, n2=128)
        plain = run_wgrad(hip, 2, Aw, Bw, M, N, K, ns, True, expo)
        assert torch.equal(split["dW"], plain["dW"]) and torch.equal(split["db"], plain["db"])  # the same sums, two destinations
        assert torch.equal(got["dW"], plain["dW"]) and torch.equal(got["db"], plain["db"])      # the head changes nothing else
        r = note("part 2", max(rs) if not any(math.isnan(x) for x in rs) else dr.NAN)
        assert r <= 1, (fam, ns, rs)


# ====================================================================================================== 3. upnerf_vec_wgrad
@pytest.mark.parametrize("K", [32, 64, 128, 256])
def test_vec_wgrad(hip, K):
    lib = hip["lib"]
    for fam in ("flat", "rows12"):
        for M in (1, 7, 33, 512):
            V, X = dr.family(fam, M, 4, K, 300 + M + K)
            Xw, xo, ldx = wide(X, 4, 8)
            for nvec in (1, 2, 3):
                for ldv in (nvec, 4):
                    v = V[:, :ldv].contiguous().cuda()
                    vd = V[:, :nvec].double()
                    ref, S = vd.t() @ X.double(), vd.abs().t() @ X.double().abs()
                    for ns in (1, 3, M + 2):  # rows per split = ceil(M / ns): the last splits get none
                        res = []
                        for _ in range(2):
                            dw, dbv = torch.full((nvec * K + 4,), SENT, device="cuda"), torch.full((nvec + 1,), SENT, device="cuda")
                            ws = torch.full((ns * 4 * (K + 1),), float("nan"), device="cuda")
                            assert lib.upnerf_vec_wgrad(M, v.data_ptr(), ldv, nvec, Xw.data_ptr() + 4 * xo, ldx, K, dw.data_ptr(),
                                                        dbv.data_ptr(), ws.data_ptr(), ns, None) == 0
                            torch.cuda.synchronize()
                            res.append((cpu(dw), cpu(dbv)))
                        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
                        dw, dbv = res[0]
                        assert bool((dw[nvec * K:] == SENT).all()) and float(dbv[nvec]) == SENT
                        r = max(dr.ratio(dw[:nvec * K].view(nvec, K), ref, dr.gate_fp32(M, S)),
                                dr.ratio(dbv[:nvec], vd.sum(0), dr.gate_fp32(M, vd.abs().sum(0))))
                        assert note("part 3", r) <= 1, (fam, M, K, nvec, ldv, ns, r)


# ========================================================================================================= 4. upnerf_linear
LIN_M, LIN_N, LIN_K = (1, 63, 64, 65, 130), (1, 3, 5, 63, 64, 65, 132), (8, 56, 64, 72, 136)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_linear(hip, act):
    """C = act(x . w^T + bias): every (M, N, K), bias present and absent, lda > K, ldc > N with sentinel padding; act & 2 (w given
    as [K][N]) through the 16-byte path (ldb and N multiples of 4) and the element-wise path (odd ldb)."""
    lib = hip["lib"]
    refs = {}
    for fam in ("flat", "rows12"):
        for M in LIN_M:
            if fam == "rows12" and M not in (65, 130):
                continue
            for K in LIN_K:
                xs, _ = dr.family(fam, M, K, 4, 400 + M + K)
                xw, xo, lda = wide(xs, 4, 4)
                for N in LIN_N:
                    w = dr.flat((N, K), 500 + N + K)
                    bias_all = dr.flat((N,), 600 + N)
                    if act & 2:
                        ldbs = [N + 4, N + 1 + N % 2] if N % 4 == 0 else [N + (4 - N % 4) % 4 + 4, N + 1 + N % 2]  # ldb % 4 == 0 | odd
                        wt = w.t().contiguous()
                    else:
                        ldbs = [K + 4]
                    for ldb in ldbs:
                        src = wt if act & 2 else w
                        wb = torch.full((src.shape[0], ldb), float("nan"))
                        wb[:, :src.shape[1]] = src
                        wb = wb.cuda()
                        for has_bias in (True, False):
                            bias = bias_all if has_bias else None
                            key = (fam, M, K, N, has_bias)
                            if key not in refs:
                                refs[key] = dr.linear_ref(xs, w, bias)
                            pre, S = refs[key]
                            gate = dr.gate_fp32(K + int(has_bias), S)
                            ldc = N + 3
                            out = torch.full((M, ldc), SENT, device="cuda")
                            bd = bias.cuda() if has_bias else None
                            assert lib.upnerf_linear(M, N, K, xw.data_ptr() + 4 * xo, lda, wb.data_ptr(), ldb,
                                                     bd.data_ptr() if has_bias else None, out.data_ptr(), ldc, act, None) == 0
                            torch.cuda.synchronize()
                            out = cpu(out)
                            assert bool((out[:, N:] == SENT).all()), "padding columns of C overwritten"
                            got = out[:, :N]
                            want = pre.clamp_min(0.0) if act & 1 else pre  # (ReLU is 1-Lipschitz: the pre-activation's gate holds)
                            r = dr.ratio(got, want, gate)
                            if act & 1:
                                assert bool((got[pre < -gate] == 0).all()) and bool((got >= 0).all())
                            assert note("part 4", r) <= 1, (fam, M, N, K, act, ldb, has_bias, r)


# ========================================================================================================= 5. upnerf_frag16
def frag16_case():
    """Hand-built descriptors.  Forward set: 1280 + 1536 + 640 + 2304 + 3200 elements (+ five of 512), so the first 2048-element
    workgroup of the maxima kernel straddles ids 0 | 1, the second 1 | 1 | 2, the third 2 | 3, the fifth 3 | 5 | 6 | 7; the
    32-row descriptors end a row-norm workgroup and a wave's 8-row group at each boundary.  id 1: two descriptors, the transposed
    one holds the larger maximum.  Family 5 in full: maximum exactly 2^p and the float below, p in {-3, 0, 5} (ids 5 | 6, 7 | 1,
    0 | 8); family 6: 2^-40 (id 3, maximum in the last element), 2^-60 (id 9), 2^40 (id 4); family 4: id 2."""
    mats, off = [], 0

    def add(rows, cols, transpose, exp_id, vals, kp, k0=0):
        nonlocal off
        assert vals.shape == (rows, cols)
        ld = (rows if transpose else cols) + 3
        stored = vals.t() if transpose else vals
        buf = torch.full((stored.shape[0], ld), float("nan"))
        buf[:, :stored.shape[1]] = stored
        m = dict(rows=rows, cols=cols, transpose=transpose, exp_id=exp_id, vals=vals, src_off=off, src_ld=ld, buf=buf.reshape(-1),
                 dst_kp=kp, dst_k0=k0)
        off += buf.numel()
        mats.append(m)
        return m

    def topped(shape, seed, top, at):
        """Flat values scaled below `top`, and `top` itself planted at `at`."""
        x = dr.flat(shape, seed) * top
        lim = dr.below(abs(top))
        x = x.clamp(-lim, lim)
        x[at] = top
        return x

    a = topped((32, 40), 71, 32.0, (5, 7))                # family 5: maximum exactly 2^5
    b = dr.flat((64, 24), 72) * 0.7
    c = topped((32, 20), 73, -dr.below(1.0), (31, 19))    # the float below 2^0 sets the exponent both descriptors of id 1 share
    z = torch.zeros(32, 72)                               # family 4
    t = topped((64, 50), 74, 2.0 ** -40, (63, 49))        # family 6, the maximum in the last element
    h = dr.flat((32, 64), 75) * 2.0 ** 40                 # family 6 (backward set only), stored transposed
    fwd = [add(32, 40, 0, 0, a, 48), add(64, 24, 0, 1, b, 32), add(32, 20, 1, 1, c, 32), add(32, 72, 0, 2, z, 80),
           add(64, 50, 0, 3, t, 64)]
    for k, top in enumerate((2.0 ** -3, dr.below(2.0 ** -3), 1.0, dr.below(32.0), 2.0 ** -60)):
        fwd.append(add(32, 16, k % 2, 5 + k, topped((32, 16), 76 + k, top if k % 2 else -top, (k, 15 - k)), 16))
    bwd = [add(32, 64, 1, 4, h, 64), dict(fwd[0], dst_kp=64, dst_k0=16)]  # (the second one reads the same source matrix again)
    for group in (fwd, bwd):
        o = 0
        for m in group:
            m["dst_off"] = o
            o += m["rows"] * m["dst_kp"]
        group.append(o)  # floats of the set's image
    src = torch.cat([m["buf"] for m in mats])
    return src, fwd, bwd


def test_frag16_direct(hip):
    L, lib = hip["L"], hip["lib"]
    for perm_fwd, perm_bwd in ((0, 1), (1, 0)):
        src, fwd, bwd = frag16_case()
        nf, nb = fwd.pop(), bwd.pop()
        mk = lambda ms: (L.Frag16Desc * len(ms))(*[L.Frag16Desc(src_off=m["src_off"], src_ld=m["src_ld"], transpose=m["transpose"],
                                                                 rows=m["rows"], cols=m["cols"], dst_off=m["dst_off"], dst_kp=m["dst_kp"],
                                                                 dst_k0=m["dst_k0"], exp_id=m["exp_id"]) for m in ms])
        PAT = 0x7BFF  # 65504: the pattern of untouched fp16 slots
        dst_f = torch.full((nf * 2,), PAT, dtype=torch.int16).cuda()
        dst_b = torch.full((nb * 2,), PAT, dtype=torch.int16).cuda()
        amax = torch.full((16,), float("nan"), device="cuda")
        wexp = torch.full((16,), 77, dtype=torch.int32, device="cuda")
        wnorm = torch.full((64,), float("nan"), device="cuda")
        srcd = src.cuda()
        assert lib.upnerf_frag16(srcd.data_ptr(), dst_f.data_ptr(), dst_b.data_ptr(), mk(fwd), len(fwd), mk(bwd), len(bwd),
                                 amax.data_ptr(), wexp.data_ptr(), perm_fwd, perm_bwd, wnorm.data_ptr(), None) == 0
        torch.cuda.synchronize()
        wexp, wnorm = cpu(wexp), cpu(wnorm)
        mx = {}
        for m in fwd + bwd:
            mx[m["exp_id"]] = max(mx.get(m["exp_id"], 0.0), float(m["vals"].abs().max()))
        for i in range(16):
            assert int(wexp[i]) == dr.frag16_exponent(mx.get(i, 0.0)), (i, int(wexp[i]))
            if mx.get(i, 0.0) > 0:
                assert 2.0 ** 13 <= mx[i] * 2.0 ** int(wexp[i]) < 2.0 ** 14
        assert int(wexp[2]) == 0 and int(wexp[0]) == 14 - 6 and int(wexp[1]) == 14 and int(wexp[3]) == 14 + 39 and int(wexp[4]) == 14 - 40
        assert [int(wexp[i]) for i in range(5, 10)] == [16, 17, 13, 9, 73]
        worst = 0.0
        for base, group, dst, perm in ((0, fwd, dst_f, perm_fwd), (32, bwd, dst_b, perm_bwd)):
            raw = cpu(dst).view(torch.float16)
            touched = torch.zeros(raw.numel(), dtype=torch.bool)
            for j, m in enumerate(group):
                rows, cols, kp, k0, e = m["rows"], m["cols"], m["dst_kp"], m["dst_k0"], int(wexp[m["exp_id"]])
                idx = np.array([[[(m["dst_off"] * 4 + dr.frag16_byte(r, k0 + c, kp, pl, perm)) // 2 for c in range(cols)]
                                 for r in range(rows)] for pl in (0, 1)])
                idx = torch.from_numpy(idx)
                assert not bool(touched[idx.reshape(-1)].any())
                touched[idx.reshape(-1)] = True
                hi, lo = raw[idx[0]].double(), raw[idx[1]].double()
                x = m["vals"].double()
                bound = torch.maximum(2.0 ** -22 * x.abs(), torch.full_like(x, 2.0 ** -25 * 2.0 ** -e))
                worst = max(worst, note("part 5", dr.ratio((hi + lo) * 2.0 ** -e, x, bound)))
                if m["exp_id"] == 2:
                    assert float(hi.abs().max()) == 0.0 and float(lo.abs().max()) == 0.0
                assert float(hi.abs().max()) <= 2.0 ** 14
                norm = x.abs().sum(1).max()
                worst = max(worst, note("part 5", dr.ratio(wnorm[base + j][None], norm[None], cols * dr.U * norm[None])))
            assert bool((raw.view(torch.int16)[~touched] == PAT).all()), "padding columns of the fragment image overwritten"
            unused = torch.ones(32, dtype=torch.bool)
            unused[:len(group)] = False
            assert bool((wnorm[base:base + 32][unused] == 0).all())
        assert worst <= 1, worst


# =========================================================================================================== 6. upnerf_adam
@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
def test_adam(hip, step):
    lib = hip["lib"]
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    ss, bc2 = dr.adam_bias_scalars(lr, b1, b2, step)
    tp, tg, tm, tv = dr.adam_table(step)
    for n in (1, 255, 256, 257, None):
        if n is None:
            p, g, m, v = tp, tg, tm, tv
        else:
            p, g, m = dr.flat((n,), 800 + n), dr.flat((n,), 801 + n) * 1e-2, dr.flat((n,), 802 + n) * 1e-3
            v = dr.flat((n,), 803 + n).abs() * 1e-5
        r32 = dr.adam_formula(p, g, m, v, b1, b2, eps, ss, bc2, torch.float32)
        r64 = dr.adam_formula(p, g, m, v, b1, b2, eps, ss, bc2, torch.float64)
        outs = []
        for dyn in (False, True):
            pd, gd, md, vd = (torch.cat([t, torch.full((3,), SENT)]).cuda() for t in (p, g, m, v))
            dyn2 = torch.tensor([ss, bc2], dtype=torch.float32).cuda() if dyn else None
            args = (5.0, 7.0) if dyn else (ss, bc2)  # with dyn2 the by-value pair must be ignored
            assert lib.upnerf_adam(p.numel(), pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), b1, b2, eps, *args,
                                   dyn2.data_ptr() if dyn else None, None) == 0
            torch.cuda.synchronize()
            outs.append([cpu(t) for t in (pd, md, vd)])
            assert all(bool((t[-3:] == SENT).all()) for t in outs[-1]) and torch.equal(cpu(gd)[:-3], g)
        for a, b in zip(*outs):  # the device-scalar call is bitwise the by-value call (NaN-free: checked by the gate below)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        got = [t[:-3] for t in outs[0]]
        over = torch.isinf(r32[2])  # fp32 overflows (1 - beta2) g g: outside any gate; the outcome has to be torch's
        if n is None:
            t_p, t_m, t_v = dr.torch_adam(p, g, m, v, lr, b1, b2, eps, step)
            assert bool(over.any()) and bool((torch.isinf(t_v) == over).all())
            assert torch.equal(got[2][over], t_v[over]) and torch.equal(got[0][over], t_p[over]) and torch.equal(got[0][over], p[over])
            assert torch.equal(got[1][over], r32[1][over])
        else:
            assert not bool(over.any())
        ok = ~over
        for name, x, x32, x64, sc in zip("pmv", got, r32[:3], r64[:3], r64[3]):
            gate = 4 * (x32.double() - x64).abs() + 2.0 ** -22 * sc
            r = note("part 6", dr.ratio(x[ok], x64[ok], gate[ok]))
            assert r <= 1, (step, n, name, r)
