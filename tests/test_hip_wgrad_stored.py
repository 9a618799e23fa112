"""upnerf_wgrad16 on its fp16-STORED operand kinds (UPNERF_WG_F16_TILE, _F16_FRAG, _F24, _PLANES), upnerf_vec_wgrad_frag16 and
upnerf_wgrad_grouped through the C ABI against fp64 on the DECODED operands, at every block shape a kind supports, the row counts
around the 32- and 64-row exponent tiles, and the exponent edges -- where tests/test_hip_kernels.py has gates normalised by a tensor's
maximum.  Encoders, decoders, families, references and the derived per-element bounds: tests/wgrad_store_ref.py (derivations in its
docstring; tests/test_wgrad_store_ref_cpu.py proves them on the CPU and shows which slips they see).  In short, with u = 2^-24:
    one-plane kinds     M u T + floors: 2^-25 per element whose rescaled plane is a subnormal fp16 number, nothing otherwise
    fp32 B beside them  + 2^-11 S (its one rounding to fp16)
    f24, planes         (M + 2) u T + the same floors for both planes + |AL|^T |BL| (the dropped lo-lo term; c 2^-22 S for residues)
    db, dv, dbv, vec    L u sum |terms| in natural units (fp32 sums of exactly converted terms; the decode adds nothing)
    grouped             M u S (fp32 MFMA)
Outputs sit in wider buffers with sentinel padding (ldo > K, ldo2 != ldo), scratch is NaN-filled, every call runs twice and must
repeat bit for bit, every element is compared, a NaN anywhere fails, a bound of 0 asks for exactly 0.  Stored tensors are padded to
whole exponent tiles with fp16 NaN bits and arbitrary residual bytes (row-major kinds: NaN in the padding columns too).

Row splits: the launcher gives a split ceil(ceil(M / nsplit) / 32) * 32 rows (64 for planes).  For the 64-row-tile kinds nsplit is
chosen so that this is an odd multiple of 32 -- a workgroup then starts and ends inside an exponent tile; for fragments (32-row
tiles) and planes (whole 64-row tiles by construction) no such nsplit exists, they get a split count that leaves the last split
ragged or empty.

Family 6 (one tile 2^-10 .. 2^-40 below the tensor's maximum) decided the open question of the rescale: the bound that follows from
the header has no room for a clamp of the exponent difference at -24 (a tile 2^-25 below enters twice too large; with a column
that is small everywhere else that is far outside the per-element floor), and none for f24's old byte decode below 2^-19 (s = f / 32
rounded to zero).  The kernels now round v 2^d ONCE for every d (through fp32 below -24) and decode the byte before the rescale;
bits are unchanged for -19 <= d (f24) resp. -24 <= d (the others).

upnerf_vec_wgrad_frag16 multiplies the padded rows of its last tile by zero weights, so they must hold finite numbers (the
register-resident kernels write finite rows there); this module pads THAT tensor with fp16's largest finite value, not NaN.

Out of scope: the producer kernels writing these formats (tests/test_hip_parity.py, tests/test_hip_field_edges.py).  This module
pins the consumer to the header's statement of the format.

Worst measured ratio error / bound on an MI355X (bound: <= 1; findings, not gates):
    At M = 1 a one-plane sum is ONE exact product (error 0); beside a fp32 B it is one rounded operand, and for f24 two rounded
    additions of three products, so those reach their bounds by construction and are listed apart, as are the fp32 kernels at M = 1
    (one rounded product).  f24 "families 2-5" is 1.000 on the byte-carried family: there the error IS the dropped lo-lo term.
                                   both operands stored                    fp32 B beside the stored A (x0)
                                   flat M>1   M=1     fam 2-5   far tiles   flat M>1   M=1     fam 2-3   far tiles
        WG_F16_TILE                0.040      0.000   0.019     0.156       0.328      0.744   0.186     0.322
        WG_F16_FRAG (256 and 128)  0.044      0.000   0.042     0.235       0.328      0.744   0.263     0.258
        WG_F24                     0.072      0.800   1.000     0.177       0.057      0.515   0.028     0.214
        WG_PLANES                  0.026      -       0.019     0.115       -          -       -         -
        column sums db             0.014 over every kind, shape and family
        riding head, n2 = 128      0.055      chained run of two kinds: 0.179
        upnerf_vec_wgrad_frag16    0.038      (0.971 at M = 1)
        upnerf_wgrad_grouped       0.300      (0.999 at M = 1)
"""
import ctypes as C
import math

import pytest
import torch

import dense_ref as dr
import wgrad_store_ref as ws

pytestmark = pytest.mark.gpu

SENT = -7.25
WORST = {}
MS = (1, 31, 32, 33, 63, 64, 65, 200, 512)
MS_PLANES = (64, 128, 192, 512)


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib, ops
    return dict(L=_lib, lib=_lib.lib, ops=ops, kind={"tile": _lib.WG_F16_TILE, "frag": _lib.WG_F16_FRAG, "f24": _lib.WG_F24,
                                                     "planes": _lib.WG_PLANES})


def cpu(t):
    return t.detach().cpu()


def note(part, r):
    WORST[part] = r if math.isnan(r) else max(WORST.get(part, 0.0), r)
    print(f"[stored] {part}: ratio {r:.3f} (worst so far {WORST[part]:.3f})")
    return r


def nsplits_for(kind, M):
    """1 and a split count whose rows per split cut the exponent tiles (module docstring)."""
    if kind == "planes":
        return (1, 3)                      # 64-row chunks: M = 128 -> 64 + 64 + none, 192 -> 64 each, 512 -> 192 + 192 + 128
    t = ws.TILE[kind]
    for ns in range(2, 40):
        rows = ((M + ns - 1) // ns + 31) // 32 * 32
        if rows % t or M <= 32:
            return (1, ns)
    return (1, 3)                          # fragments: rows per split are whole 32-row tiles whatever nsplit is


class DevOp:
    """A stored operand (or fp32 rows inside a wider NaN-padded tensor) on the device, with its upnerf_wgrad_operand."""

    def __init__(self, hip, op):
        L = hip["L"]
        if isinstance(op, ws.Stored):
            img = ws.device_image(op, ld=None if op.kind == "planes" else op.W + 8)
            self.keep = [img["p"].cuda(), None if img["lo"] is None else img["lo"].cuda(), img["exp"].cuda()]
            self.c = L.WgradOperand(p=self.keep[0].data_ptr(), lo=None if self.keep[1] is None else self.keep[1].data_ptr(),
                                    exp=self.keep[2].data_ptr(), ld=img["ld"], kind=hip["kind"][op.kind])
        else:
            M, n = op.shape
            w = torch.full((M, n + 16), float("nan"))
            w[:, 8:8 + n] = op
            self.keep = [w.cuda()]
            self.c = L.WgradOperand(p=self.keep[0].data_ptr() + 32, ld=n + 16, kind=L.WG_F32)


def expo_for(hip, A, B, fa=None, fb=None):
    """Device int32 [2] from ops.scale_exponents on the decoded values (checked against the host formula) unless forced."""
    da = ws.decode(A).float() if isinstance(A, ws.Stored) else A
    db = ws.decode(B).float() if isinstance(B, ws.Stored) else B
    ex = hip["ops"].scale_exponents(da.cuda(), db.cuda())
    ea, eb = (int(x) for x in cpu(ex))
    assert (ea, eb) == (ws.tensor_exponent(A), ws.tensor_exponent(B))
    if fa is not None or fb is not None:
        ea, eb = (ea if fa is None else fa), (eb if fb is None else fb)
        ex = torch.tensor([ea, eb], dtype=torch.int32).cuda()
    return ex, ea, eb


def run(hip, dA, dB, M, N, K, ns, expo, with_db=True, v=None, n2=0, chain=None):
    """One upnerf_wgrad16 call, twice, bitwise equal; returns the results on the CPU.  chain: a list the (descriptor, outputs) are
    appended to instead of launching (see run_chain)."""
    L, lib = hip["L"], hip["lib"]
    ldo, ldo2 = K + 4, K + 12
    outs = []
    for _ in range(2):
        n1 = n2 if n2 else N
        dW = torch.full((n1, ldo), SENT, device="cuda")
        db = torch.full((n1 + 4,), SENT, device="cuda") if with_db else None
        dW2 = torch.full((N - n2, ldo2), SENT, device="cuda") if n2 else None
        db2 = torch.full((N - n2 + 4,), SENT, device="cuda") if (n2 and with_db) else None
        dv = torch.full((K + 4,), SENT, device="cuda") if v is not None else None
        dbv = torch.full((4,), SENT, device="cuda") if v is not None else None
        d = L.WgradDesc(M=M, N=N, K=K, planes=2, A=dA.c, B=dB.c, expo_a=expo.data_ptr(), expo_b=expo.data_ptr() + 4, dW=dW.data_ptr(),
                        db=db.data_ptr() if with_db else None, ldo=ldo, nsplit=ns)
        if n2:
            d.n2, d.dW2, d.ldo2, d.db2 = n2, dW2.data_ptr(), ldo2, (db2.data_ptr() if with_db else None)
        if v is not None:
            d.v, d.dv, d.dbv = v.data_ptr(), dv.data_ptr(), dbv.data_ptr()
        need = lib.upnerf_wgrad16_scratch(C.byref(d))
        assert need > 0
        slabs = torch.full((need,), float("nan"), device="cuda")
        d.slabs = slabs.data_ptr()
        bufs = (dW, db, dW2, db2, dv, dbv)
        if chain is not None:
            chain.append((d, bufs, slabs))
            return None
        rc = lib.upnerf_wgrad16(C.byref(d), None, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        outs.append([None if t is None else cpu(t) for t in bufs])
    for a, b in zip(*outs):
        assert a is None or torch.equal(a, b), (M, N, K, ns)
    return collect(outs[0], N, K, n2, with_db, v is not None)


def collect(bufs, N, K, n2, with_db, has_v):
    """Checks the sentinels and joins the two destinations of a split result."""
    dW, db, dW2, db2, dv, dbv = bufs
    n1 = n2 if n2 else N
    assert bool((dW[:, K:] == SENT).all()), "padding columns of dW overwritten"
    res = dict(dW=dW[:, :K])
    if with_db:
        assert bool((db[n1:] == SENT).all())
        res["db"] = db[:n1]
    if n2:
        assert bool((dW2[:, K:] == SENT).all()), "padding columns of dW2 overwritten"
        res["dW"] = torch.cat([res["dW"], dW2[:, :K]])
        if with_db:
            assert bool((db2[N - n2:] == SENT).all())
            res["db"] = torch.cat([res["db"], db2[:N - n2]])
    if has_v:
        assert bool((dv[K:] == SENT).all()) and bool((dbv[1:] == SENT).all())
        res["dv"], res["dbv"] = dv[:K], dbv[:1]
    return res


def check(hip, part, A, B, fa=None, fb=None, nsplits=None, tag=()):
    """Every nsplit of one operand pair against the reference; returns the last result."""
    M, N = A.M, A.W
    K = B.W if isinstance(B, ws.Stored) else B.shape[1]
    expo, ea, eb = expo_for(hip, A, B, fa, fb)
    ref = ws.reference(A, B, ea, eb)
    dA, dB = DevOp(hip, A), DevOp(hip, B)
    got = None
    for i, ns in enumerate(nsplits or nsplits_for(A.kind, M)):
        with_db = i % 2 == 0
        got = run(hip, dA, dB, M, N, K, ns, expo, with_db)
        r = note(part, dr.ratio(got["dW"], ref["dW"], ref["gate"]))
        assert r <= 1, (part, A.kind, M, N, K, ns, r) + tuple(tag)
        if with_db:
            rb = note(part + " db", dr.ratio(got["db"], ref["db"], ref["gate_db"]))
            assert rb <= 1, (part, A.kind, M, N, K, ns, "db", rb) + tuple(tag)
    return got, ref


def stored_pair(kind, fam, M, N, K, seed, b_fam=None, side="A", **kw):
    other = b_fam or ("flat" if fam in ("zero", "zerotile", "far") else fam)
    (X, fx), (Y, fy) = ws.family(kind, fam, M, N if side == "A" else K, seed, **kw), ws.family(kind, other, M, K if side == "A" else N, seed + 50)
    return (X, Y, fx, fy) if side == "A" else (Y, X, fy, fx)


# ============================================================================================ 1. every block shape, every M
SHAPES = [("tile", 256, 256), ("tile", 256, 64), ("frag", 256, 256), ("frag", 128, 128), ("frag", 256, 64), ("f24", 256, 256),
          ("f24", 256, 64), ("planes", 256, 256)]


@pytest.mark.parametrize("kind,N,K", SHAPES)
def test_flat_family_on_every_block_shape_and_row_count(hip, kind, N, K):
    """Family 1.  K = 64: fp32 B (the encoding x0) beside the stored A."""
    for j, M in enumerate(MS_PLANES if kind == "planes" else MS):
        A, _ = ws.family(kind, "flat", M, N, 1000 + 13 * j + N)
        B = dr.flat((M, K), 1001 + 13 * j + K) if K == 64 else ws.family(kind, "flat", M, K, 1002 + 13 * j + K)[0]
        part = f"1 {kind}" + (" x0" if K == 64 else "") + (" M=1" if M == 1 else "")
        check(hip, part, A, B, tag=("flat",))


# ======================================================================================================== 2. families 2 - 6
def fam_Ms(kind):
    return {"tile": (200, 65), "frag": (77, 33), "f24": (200, 65), "planes": (192, 128)}[kind]


@pytest.mark.parametrize("kind,fam", [(k, f) for k in ws.KINDS for f in ("tiles10", "zerotile", "zero", "peak", "resid")
                                      if f != "resid" or k in ws.TWO_PLANES])
def test_exponent_and_value_families(hip, kind, fam):
    """Families 2 - 5 on 256 x 256 (and, families 2 and 3, beside a fp32 B): tile exponents +-10 apart, an all-zero tile and A = 0
    (exactly 0 out), fp16's largest finite value at rescale factor 1 beside the smallest normal, the residual extremes."""
    for M in fam_Ms(kind):
        A, B, fa, fb = stored_pair(kind, fam, M, 256, 256, 2000 + M)
        got, _ = check(hip, f"2 {kind}", A, B, fa, fb, tag=(fam,))
        if fam == "zero":
            assert float(got["dW"].abs().max()) == 0.0
        if kind != "planes" and fam in ("tiles10", "zerotile", "zero"):
            got, _ = check(hip, f"2 {kind} x0", A, dr.flat((M, 64), 2001 + M), tag=(fam, "x0"))
            if fam == "zero":
                assert float(got["dW"].abs().max()) == 0.0


@pytest.mark.parametrize("far", ws.FAR)
@pytest.mark.parametrize("kind", ws.KINDS)
def test_a_tile_far_below_the_maximum(hip, kind, far):
    """Family 6: one tile's exponent exceeds the tensor-wide one by `far`, in A (last, ragged tile) and in B (first tile), plain and
    with a column that is small in every other tile; both operands far in the same tile; beside a fp32 B."""
    M = fam_Ms(kind)[0]
    for side, kw in (("A", {}), ("A", dict(small_col=5)), ("B", dict(small_col=5, far_tile=0)), ("A", dict(b_fam="far"))):
        A, B, fa, fb = stored_pair(kind, "far", M, 256, 256, 3000 + far, side=side, far=far, **kw)
        check(hip, f"6 {kind}", A, B, fa, fb, tag=("far", far, side, kw))
    if kind != "planes":
        A, _ = ws.family(kind, "far", M, 256, 3100 + far, far=far, small_col=5)
        check(hip, f"6 {kind} x0", A, dr.flat((M, 64), 3101 + far), tag=("far", far, "x0"))


# ====================================================================================== 3. the riding head, n2, a chained run
@pytest.mark.parametrize("fam", ["flat", "tiles10", "far"])
def test_riding_head_and_row_split_on_fragments(hip, fam):
    """Families 7 and 8: desc.v on fragment operands (dv, dbv in natural units), the result split at n2 = 128 -- the same sums."""
    for M in (77, 33, 512):
        A, B, fa, fb = stored_pair("frag", fam, M, 256, 256, 4000 + M, side="B" if fam == "far" else "A", **({"far": 25} if fam == "far" else {}))
        v = dr.flat((M,), 4001 + M) * 2.0 ** -7
        expo, ea, eb = expo_for(hip, A, B, fa, fb)
        ref, vref = ws.reference(A, B, ea, eb), ws.vec_reference(v[:, None], B, M)
        dA, dB = DevOp(hip, A), DevOp(hip, B)
        for ns in (1, 3):
            plain = run(hip, dA, dB, M, 256, 256, ns, expo)
            got = run(hip, dA, dB, M, 256, 256, ns, expo, v=v.cuda())
            split = run(hip, dA, dB, M, 256, 256, ns, expo, n2=128)
            assert torch.equal(split["dW"], plain["dW"]) and torch.equal(split["db"], plain["db"])
            assert torch.equal(got["dW"], plain["dW"]) and torch.equal(got["db"], plain["db"])
            rs = [dr.ratio(got["dW"], ref["dW"], ref["gate"]), dr.ratio(got["db"], ref["db"], ref["gate_db"]),
                  dr.ratio(got["dv"], vref["dw"][0], vref["gate"][0]), dr.ratio(got["dbv"], vref["dbv"], vref["gate_b"])]
            r = note("3 head, n2", dr.NAN if any(math.isnan(x) for x in rs) else max(rs))
            assert r <= 1, (fam, M, ns, rs)


def test_a_chained_run_of_two_kinds_is_the_unchained_one(hip):
    """Family 9: fragments 256 x 256 with n2, then tile rows beside a fp32 B, on one pending record, finished by
    upnerf_wgrad_finish: bitwise the unchained calls, and inside the bounds."""
    L, lib = hip["L"], hip["lib"]
    M = 200
    A1, B1, _, _ = stored_pair("frag", "tiles10", M, 256, 256, 5000)
    A2, B2 = ws.family("tile", "tiles10", M, 256, 5001)[0], dr.flat((M, 64), 5002)
    probs = []
    for A, B, n2 in ((A1, B1, 128), (A2, B2, 0)):
        K = B.W if isinstance(B, ws.Stored) else B.shape[1]
        expo, ea, eb = expo_for(hip, A, B)
        probs.append(dict(A=DevOp(hip, A), B=DevOp(hip, B), K=K, n2=n2, expo=expo, ref=ws.reference(A, B, ea, eb)))
    singles = [run(hip, p["A"], p["B"], M, 256, p["K"], 3, p["expo"], n2=p["n2"]) for p in probs]
    runs = []
    for _ in range(2):
        chain, pend = [], L.WgradPending()
        for p in probs:
            run(hip, p["A"], p["B"], M, 256, p["K"], 3, p["expo"], n2=p["n2"], chain=chain)
        for d, _, _ in chain:
            assert lib.upnerf_wgrad16(C.byref(d), C.byref(pend), None) == 0
        assert lib.upnerf_wgrad_finish(C.byref(pend), None) == 0 and pend.nsplit == 0
        torch.cuda.synchronize()
        runs.append([collect([None if t is None else cpu(t) for t in bufs], 256, p["K"], p["n2"], True, False)
                     for (_, bufs, _), p in zip(chain, probs)])
    for p, single, a, b in zip(probs, singles, *runs):
        assert torch.equal(a["dW"], b["dW"]) and torch.equal(a["db"], b["db"])
        assert torch.equal(a["dW"], single["dW"]) and torch.equal(a["db"], single["db"])
        r = note("3 chain", max(dr.ratio(a["dW"], p["ref"]["dW"], p["ref"]["gate"]), dr.ratio(a["db"], p["ref"]["db"], p["ref"]["gate_db"])))
        assert r <= 1


# =============================================================================================== 4. upnerf_vec_wgrad_frag16
@pytest.mark.parametrize("K", [128, 256])
def test_vec_wgrad_frag16(hip, K):
    lib = hip["lib"]
    for fam, kw in (("flat", {}), ("tiles10", {}), ("far", dict(far=25)), ("far", dict(far=40, far_tile=0))):
        for M in (1, 31, 33, 77, 512):
            X, _ = ws.family("frag", fam, M, K, 6000 + M + K, **kw)
            img = ws.device_image(X)
            p = img["p"].clone()
            pad = ws.from_frag(torch.arange(img["Mp"] * K), img["Mp"], K)[M:].reshape(-1)  # slots of the padded rows: finite (docstring)
            p[pad] = 0x7BFF
            x16, xexp = p.cuda(), img["exp"].cuda()
            for nvec in (1, 3):
                ldv = 4 if nvec == 3 else 1
                V = dr.flat((M, ldv), 6001 + M + nvec)
                ref = ws.vec_reference(V[:, :nvec], X, M)
                vd = V.cuda()
                for ns in (1, 3):
                    res = []
                    for _ in range(2):
                        dw, dbv = torch.full((nvec * K + 4,), SENT, device="cuda"), torch.full((nvec + 1,), SENT, device="cuda")
                        scr = torch.full((ns * 4 * (K + 1),), float("nan"), device="cuda")
                        assert lib.upnerf_vec_wgrad_frag16(M, vd.data_ptr(), ldv, nvec, x16.data_ptr(), xexp.data_ptr(), K, dw.data_ptr(),
                                                           dbv.data_ptr(), scr.data_ptr(), ns, None) == 0
                        torch.cuda.synchronize()
                        res.append((cpu(dw), cpu(dbv)))
                    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
                    dw, dbv = res[0]
                    assert bool((dw[nvec * K:] == SENT).all()) and float(dbv[nvec]) == SENT
                    r = max(dr.ratio(dw[:nvec * K].view(nvec, K), ref["dw"], ref["gate"]), dr.ratio(dbv[:nvec], ref["dbv"], ref["gate_b"]))
                    assert note("4 vec frag16" + (" M=1" if M == 1 else ""), r) <= 1, (fam, kw, M, K, nvec, ns, r)


# ================================================================================================== 5. upnerf_wgrad_grouped
GROUP_NK = [(4, 4), (124, 132), (128, 128), (260, 4), (4, 260)]
GROUP_M = [1, 33, 7, 64, 65, 200, 31, 96]


def grouped(hip, specs, nsplit):
    """specs: (M, N, K, with_db).  One launch, twice; every group against fp64 with M u S."""
    L, lib = hip["L"], hip["lib"]
    res = []
    data = []
    for j, (M, N, K, with_db) in enumerate(specs):
        A, B = dr.flat((M, N), 7000 + j), dr.flat((M, K), 7100 + j)
        data.append((A, B, DevOp(hip, A), DevOp(hip, B)))
    for _ in range(2):
        groups, outs = [], []
        for (M, N, K, with_db), (A, B, dA, dB) in zip(specs, data):
            ldo = K + 4
            dW = torch.full((N, ldo), SENT, device="cuda")
            db = torch.full((N + 4,), SENT, device="cuda") if with_db else None
            groups.append(L.WgradGroup(A=dA.c.p, B=dB.c.p, dW=dW.data_ptr(), db=db.data_ptr() if with_db else None, M=M, N=N, K=K,
                                       lda=dA.c.ld, ldb=dB.c.ld, ldo=ldo))
            outs.append((dW, db))
        arr = (L.WgradGroup * len(groups))(*groups)
        n = lib.upnerf_wgrad_grouped_scratch(arr, len(groups), nsplit)
        assert n > 0
        scr = torch.full((n,), float("nan"), device="cuda")
        assert lib.upnerf_wgrad_grouped(arr, len(groups), scr.data_ptr(), nsplit, None) == 0
        torch.cuda.synchronize()
        res.append([(cpu(w), None if b is None else cpu(b)) for w, b in outs])
    for (M, N, K, with_db), (A, B, _, _), (w0, b0), (w1, b1) in zip(specs, data, *res):
        assert torch.equal(w0, w1) and (b0 is None or torch.equal(b0, b1))
        assert bool((w0[:, K:] == SENT).all()) and (b0 is None or bool((b0[N:] == SENT).all()))
        ref = dr.wgrad_ref(A, B)
        r = dr.ratio(w0[:, :K], ref["dW"], dr.gate_fp32(M, ref["S"]))
        if with_db:
            r = max(r, dr.ratio(b0[:N], ref["db"], dr.gate_fp32(M, ref["sa"])))
        assert note("5 grouped" + (" M=1" if M == 1 else ""), r) <= 1, (M, N, K, with_db, r)


def test_wgrad_grouped_thirty_two_groups_and_one(hip):
    specs = [(GROUP_M[(j + j // 5) % len(GROUP_M)], *GROUP_NK[j % 5], j % 3 != 1) for j in range(32)]
    assert {s[0] for s in specs} >= {1, 33} and any(not s[3] for s in specs) and len(specs) == hip["L"].MAX_WGRAD_GROUPS
    grouped(hip, specs, 3)
    grouped(hip, [(33, 124, 132, True)], 2)
    grouped(hip, [(1, 260, 4, False)], 1)
