"""The fp16-STORED operand kinds of upnerf_wgrad16 (include/upnerf_hip.h, UPNERF_WG_F16_TILE / _F16_FRAG / _F24 / _PLANES), stated
on the CPU from the header alone: encoders, decoders, the fragment index map, seeded input families, fp64 references on the DECODED
operands and derived per-element error bounds.  tests/test_wgrad_store_ref_cpu.py proves the bounds on an emulation of the kernels'
arithmetic and shows that they see the listed slips; tests/test_hip_wgrad_stored.py holds the kernels to them.  No bound is computed
from a kernel's output.  Quantisation on the way INTO storage is not part of the budget: the reference contracts what the stored
bits mean.

Storage (x = the exponent of the row's tile; 64 rows per tile, 32 for fragments):
    tile, frag   value = hi 2^-x                          hi fp16
    f24          value = (hi + (byte - 128) / 32) 2^-x    byte uint8
    planes       value = (hi + lo) 2^-x                   lo fp16
Fragment order [32-row tile][k-block s][lane][j]: feature = 16 s + 8 (j / 4) + 4 (lane / 32) + j % 4, row = 32 tile + lane % 32.

Notation as in tests/dense_ref.py: u = 2^-24, S = |A|^T |B| in fp64, ea / eb the tensor-wide exponents, a' = 2^ea a the operand at the
tensor-wide scale, d = ea - x the power of two a stored plane is rescaled by (d <= 0 for a tile below the tensor's maximum).

The contract the bounds follow from (header): a stored plane is brought to the tensor-wide exponent "on load", in fp16, and the
planes are contracted with exact products and fp32 accumulation.  One fp16 rounding of p 2^d (p = hi or lo, a power-of-two scaling):
    exact while |p 2^d| >= 2^-14 (a normal fp16 number: 11 bits survive) and for p = 0;
    |error| <= 2^-25 below that (subnormal spacing 2^-24, round to nearest) -- the subnormal floor, PER ELEMENT.
There is no d for which more is allowed: a tile 2^-25 or 2^-40 below the tensor's maximum rounds towards zero like any other small
number.  (The kernels used to clamp d at -24, which multiplies such a tile by 2^(-24 - d) instead: outside this floor by up to
2^14; family "far" reaches it, test_wgrad_store_ref_cpu.py shows the clamped arithmetic outside the bound.)
Per operand element, in units of the tensor-wide scale:
    one plane (tile, frag)          D = 2^-25 [0 < |hi 2^d| < 2^-14]
    two planes (f24, planes)        D = 2^-25 ([0 < |hi 2^d| < 2^-14] + [0 < |lo 2^d| < 2^-14]),  |al| <= |lo 2^d| + its floor
    f24's byte decode               (byte - 128) / 32 is a multiple of 2^-5 of magnitude <= 4: exact in fp16 whether it is formed as
                                    v / 32 - 4 with two roundings or one (v / 32 <= 8 and the difference are 8-bit multiples of
                                    2^-5), so the decode adds NOTHING to D: the only rounding is the rescale of the decoded residual
    fp32 B beside one-plane A       one rounding to fp16:  D = 2^-11 |b'| (normal range), 2^-25 below it
    fp32 B beside f24               split on load as in dense_ref: D = 2^-22 |b'| + 2^-25,  |bl| <= 2^-11 (1 + 2^-11) |b'| + 2^-25
    sum_m |ah bh - a' b'| <= DA^T |B'| + |A'|^T DB + DA^T DB            (times 1 + 2^-10, dense_ref's slack for second-order terms)
The three-product kinds drop al bl: the bound adds |AL|^T |BL| computed from the stored lo planes -- for residues of a rounding
(|lo| <= 2^-11 |hi|) that is dense_ref's c 2^-22 S, for arbitrary bytes (family "resid") it is what the bytes say.
fp32 accumulation over M: L u T with T = (|AH| + |AL|)^T (|BH| + |BL|) >= the summed magnitudes of the terms and L = M for one
product per row, M + 2 for three (a 16-deep MFMA step rounds once: 3 ceil(M / 16) + the slab additions <= M + 2; dense_ref's
argument, with the two extra roundings that three products need at M = 1).
    gate = 2^-(ea+eb) [ L u T + (1 + 2^-10) (DA^T |B'| + |A'|^T DB + DA^T DB) + |AL|^T |BL| ]
Every term vanishes with the operand (indicator floors), so an all-zero A asks for exactly 0.
db, and dv / dbv of the riding head and upnerf_vec_wgrad_frag16, are fp32 sums in natural units of exactly converted terms
(fp16 -> fp32 and the power of two are exact):  L u sum |terms|,  L = M (2 M for the two-plane kinds: hi and lo are added apart).
The decode adds nothing there either.

On the flat family (|a|, |b| in [0.5, 1]) a lost row moves every element by >= 1/4; the CPU test asserts gate < 1/40 there for the
M it uses, and that each mutated restatement is more than 10 gates away.
"""
import math

import torch

import dense_ref as dr

U = dr.U
SLACK = 1.0 + 2.0 ** -10
KINDS = ("tile", "frag", "f24", "planes")
TILE = {"tile": 64, "frag": 32, "f24": 64, "planes": 64}
TWO_PLANES = ("f24", "planes")
NAN16 = 0x7E00
H_MAX = 65504.0
H_MIN = 2.0 ** -14


class Stored:
    """One stored operand in LOGICAL row-major order: hi fp16 [M][W], lo (None | uint8 [M][W] | fp16 [M][W]), exp int32 [tiles]."""

    def __init__(self, kind, hi, lo, exp):
        assert kind in KINDS and hi.dtype == torch.float16 and exp.dtype == torch.int32
        assert exp.numel() == (hi.shape[0] + TILE[kind] - 1) // TILE[kind]
        assert (lo is None) == (kind not in TWO_PLANES)
        assert lo is None or (lo.shape == hi.shape and lo.dtype == (torch.uint8 if kind == "f24" else torch.float16))
        assert bool(torch.isfinite(hi).all())
        self.kind, self.hi, self.lo, self.exp = kind, hi, lo, exp
        self.M, self.W = hi.shape

    def row_exp(self):
        return self.exp.long().repeat_interleave(TILE[self.kind])[:self.M]

    def lo_value(self, about=128):
        """The lo plane in the tile's units, fp64 (zeros for the one-plane kinds)."""
        if self.kind == "f24":
            return (self.lo.double() - about) / 32.0
        if self.kind == "planes":
            return self.lo.double()
        return torch.zeros(self.M, self.W, dtype=torch.float64)

    def rows(self, sl):
        """Rows [0, sl) as an operand of their own (whole leading tiles + a ragged one)."""
        nt = (sl + TILE[self.kind] - 1) // TILE[self.kind]
        return Stored(self.kind, self.hi[:sl].clone(), None if self.lo is None else self.lo[:sl].clone(), self.exp[:nt].clone())


def pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.as_tensor(e).double())


def decode(st):
    """fp64 value the stored bits mean."""
    return (st.hi.double() + st.lo_value()) * pow2(-st.row_exp())[:, None]


def encode(kind, X, exp):
    """What a producer stores for X [M][W] under the per-tile exponents exp: hi = fl16(X 2^x), the residual as the kind keeps it
    (f24: byte = round(32 lo) + 128 with |32 lo| clamped to 127, as the field kernels write it)."""
    exp = torch.as_tensor(exp).to(torch.int32)
    M = X.shape[0]
    sc = X.double() * pow2(exp.long().repeat_interleave(TILE[kind])[:M])[:, None]
    assert float(sc.abs().max()) <= H_MAX if sc.numel() else True
    hi = sc.float().half()
    lo = None
    if kind == "f24":
        lo = (torch.round(32.0 * (sc - hi.double())).clamp(-127, 127) + 128).to(torch.uint8)
    elif kind == "planes":
        lo = (sc - hi.double()).float().half()
    return Stored(kind, hi, lo, exp)


# ------------------------------------------------------------------------------------------------------ the fragment order
def frag_index(Mp, W):
    """[Mp][W] int64: position of element (row, feature) in the fragment image [tile][s][lane][j] (header: feature = 16 s +
    8 (j / 4) + 4 (lane / 32) + j % 4, row = 32 tile + lane % 32), built by walking the IMAGE and writing down where each slot's
    element lives -- the map as the header states it, not its inverse."""
    assert Mp % 32 == 0 and W % 16 == 0
    pos = torch.arange(Mp * W)
    j, lane = pos % 8, (pos // 8) % 64
    s, tile = (pos // 512) % (W // 16), pos // (512 * (W // 16))
    feature = 16 * s + 8 * (j // 4) + 4 * (lane // 32) + j % 4
    row = 32 * tile + lane % 32
    idx = torch.full((Mp, W), -1, dtype=torch.int64)
    idx[row, feature] = pos
    assert int(idx.min()) == 0 and idx.unique().numel() == Mp * W
    return idx


def to_frag(rows16):
    """[Mp][W] int16 bit patterns -> the flat fragment image."""
    Mp, W = rows16.shape
    out = torch.empty(Mp * W, dtype=rows16.dtype)
    out[frag_index(Mp, W).reshape(-1)] = rows16.reshape(-1)
    return out


def from_frag(image, Mp, W):
    return image.reshape(-1)[frag_index(Mp, W)]


def device_image(st, ld=None):
    """CPU tensors in the layout the kernels read: dict(p int16, lo uint8 | int16 | None, exp int32, ld).  The tensor is padded to
    whole exponent tiles; the padded rows hold fp16 NaN bits (and, row-major, NaN in the columns past W when ld > W) and arbitrary
    residual bytes: nothing of them may reach a result."""
    t = TILE[st.kind]
    Mp = (st.M + t - 1) // t * t
    ld = st.W if (ld is None or st.kind == "frag") else ld
    p = torch.full((Mp, ld), NAN16, dtype=torch.int16)
    p[:st.M, :st.W] = st.hi.view(torch.int16)
    lo = None
    if st.kind == "f24":
        lo = ((torch.arange(Mp * ld) * 7 + 3) % 256).to(torch.uint8).reshape(Mp, ld)
        lo[:st.M, :st.W] = st.lo
    elif st.kind == "planes":
        lo = torch.full((Mp, ld), NAN16, dtype=torch.int16)
        lo[:st.M, :st.W] = st.lo.view(torch.int16)
    if st.kind == "frag":
        p = to_frag(p)
    return dict(p=p.contiguous(), lo=lo, exp=st.exp.clone(), ld=ld, Mp=Mp)


# ---------------------------------------------------------------------------------------------------------------- families
FAMILIES = ("flat", "tiles10", "zerotile", "zero", "peak", "resid", "far")
FAR = (10, 23, 24, 25, 40)


def ulp16(h):
    """Spacing of fp16 at |h| (2^-24 in the subnormal range)."""
    e = torch.floor(torch.log2(h.double().abs().clamp_min(H_MIN)))
    return pow2(e - 10)


def family(kind, fam, M, W, seed, far=25, far_tile=None, small_col=None):
    """(Stored, forced tensor-wide exponent or None) of one input family (numbers as in the issue's list):
    flat      1  |value| in [0.5, 1], every tile exponent 14
    tiles10   2  tile t scaled by 2^k_t, k_t in [-10, 0] (first 0, last -10), exponent 14 - k_t
    zerotile  3  the middle tile all zero under an exponent (21) that no value backs;  zero: everything zero
    peak      4  one tile between 32752 and fp16's largest finite value 65504 (both signs planted), the others at +-2^-14, the
                 smallest normal; tensor-wide exponent FORCED to the tiles' 14: rescale factor 1
    resid     5  f24: hi small (|hi| in [1/16, 1/8]) under residual bytes 0 / 128 / 255 in turn: the bytes carry the value;
                 planes: lo = half an ulp of hi with the opposite sign, its largest magnitude
    far       6  tile far_tile 2^-far below the others (exponent 14 + far, planes as large as everywhere); small_col: that column
                 is 2^-26 of the rest in every OTHER tile, so S of its output row does not hide the far tile"""
    t = TILE[kind]
    nt = (M + t - 1) // t
    tile = torch.arange(M) // t
    X = dr.flat((M, W), seed).double()
    exp = torch.full((nt,), 14, dtype=torch.int32)
    if fam == "flat":
        pass
    elif fam == "tiles10":
        k = -torch.randint(0, 11, (nt,), generator=dr._gen(seed + 7))
        k[0] = 0
        if nt > 1:
            k[-1] = -10
        X = X * pow2(k[tile])[:, None]
        exp = (14 - k).to(torch.int32)
    elif fam == "zerotile":
        X[tile == nt // 2] = 0.0
        exp[nt // 2] = 21
    elif fam == "zero":
        X = X * 0.0
    elif fam == "peak":
        tp = nt // 2
        sgn = torch.sign(X)
        hi = torch.where((tile == tp)[:, None], X * H_MAX, sgn * H_MIN)
        r0 = int(torch.nonzero(tile == tp)[0])
        hi[r0, 1], hi[r0, W - 1] = H_MAX, -H_MAX
        hi = hi.float().half()
        lo = None
        if kind == "f24":
            lo = torch.randint(1, 256, (M, W), generator=dr._gen(seed + 3)).to(torch.uint8)
        elif kind == "planes":
            lo = ((torch.rand(M, W, generator=dr._gen(seed + 3)).double() - 0.5) * ulp16(hi)).float().half()
        return Stored(kind, hi, lo, exp), 14
    elif fam == "resid":
        assert kind in TWO_PLANES
        if kind == "f24":
            st = encode(kind, X * 2.0 ** -17, exp)
            r, c = torch.meshgrid(torch.arange(M), torch.arange(W), indexing="ij")
            st.lo = torch.tensor([0, 128, 255], dtype=torch.uint8)[(r + c) % 3]
            return st, None
        st = encode(kind, X, exp)
        st.lo = (-torch.sign(st.hi.double()) * ulp16(st.hi) / 2).float().half()
        return st, None
    elif fam == "far":
        ft = nt - 1 if far_tile is None else far_tile
        if small_col is not None:
            X[tile != ft, small_col] *= 2.0 ** -26
        X[tile == ft] *= 2.0 ** -far
        exp[ft] = 14 + far
    else:
        raise KeyError(fam)
    return encode(kind, X, exp), None


def tensor_exponent(st_or_rows):
    """dense_ref.host_exponent of the decoded values (= ops.scale_exponents; 113 for an all-zero tensor)."""
    x = decode(st_or_rows) if isinstance(st_or_rows, Stored) else st_or_rows
    return dr.host_exponent(x.double())


# -------------------------------------------------------------------------------------------------- references and bounds
def _terms(op, e, three):
    """Per-element pieces of one operand at the tensor-wide scale 2^e: P = |a'|, D = bound of |ah + al - a'|, L = bound of |al|,
    T = bound of |ah| + |al|, nat = summed magnitudes of its terms in natural units (for db), val = the fp64 value."""
    if isinstance(op, Stored):
        d = (e - op.row_exp()).double()
        f = pow2(d)[:, None]
        h, l = op.hi.double().abs() * f, op.lo_value().abs() * f
        sub = lambda p: ((p > 0) & (p < H_MIN)).double() * 2.0 ** -25
        D = sub(h) + sub(l)
        val = decode(op)
        assert float(h.max() if h.numel() else 0.0) <= H_MAX, "the tensor-wide exponent overflows fp16"
        nat = (op.hi.double().abs() + op.lo_value().abs()) * pow2(-op.row_exp())[:, None]
        return dict(P=(val * 2.0 ** e).abs(), D=D, L=l + sub(l), T=h + l + D, nat=nat, val=val)
    val = op.double()
    P = (val * 2.0 ** e).abs()
    nz = (P > 0).double()
    if three:
        D = (2.0 ** -22 * P + 2.0 ** -25) * nz
        L = (2.0 ** -11 * (1 + 2.0 ** -11) * P + 2.0 ** -25) * nz
    else:
        D = torch.where(P >= H_MIN, 2.0 ** -11 * P, torch.full_like(P, 2.0 ** -25)) * nz
        L = torch.zeros_like(P)
    return dict(P=P, D=D, L=L, T=P + D + L, nat=val.abs(), val=val)


def reference(A, B, ea, eb):
    """fp64 contraction of the decoded operands and the per-element gates: dict(dW, db, S, gate, gate_db, A, B (decoded))."""
    three = A.kind in TWO_PLANES
    M = A.M
    ta, tb = _terms(A, ea, three), _terms(B, eb, three)
    L = M + 2 if three else M
    g = L * U * (ta["T"].t() @ tb["T"]) + SLACK * (ta["D"].t() @ tb["P"] + ta["P"].t() @ tb["D"] + ta["D"].t() @ tb["D"])
    if three:
        g = g + ta["L"].t() @ tb["L"]
    a, b = ta["val"], tb["val"]
    Lb = 2 * M if three else M
    return dict(dW=a.t() @ b, db=a.sum(0), S=a.abs().t() @ b.abs(), gate=g * 2.0 ** -(ea + eb), gate_db=Lb * U * ta["nat"].sum(0), A=a, B=b)


def vec_reference(v, X, M):
    """upnerf_vec_wgrad_frag16 and the riding head: dw = v^T X, dbv = sum v on the decoded X, gates M u sum |v| |x| / M u sum |v|."""
    vd, x = v.double(), (decode(X) if isinstance(X, Stored) else X.double())
    return dict(dw=vd.t() @ x, dbv=vd.sum(0), gate=M * U * (vd.abs().t() @ x.abs()), gate_b=M * U * vd.abs().sum(0))


# -------------------------------------------------------------------------------------- emulation of the kernels' arithmetic
def _h(x):
    """One rounding to fp16 of fp64 numbers that fp32 holds exactly (11- or 8-bit significands times a power of two)."""
    return x.float().half().double()


MUTATIONS = ("last_row", "neighbour_exp", "drop_lo", "byte127", "lane_half", "col_block")


def _planes(op, e, three, legacy, mut, is_a):
    """(hi plane, lo plane) as the kernel hands them to the matrix cores, fp64 holding fp16 values."""
    if not isinstance(op, Stored):  # fp32 rows: scaled in fp32, rounded or split as the f16x3 kernel does
        x = op.float() * 2.0 ** e
        if mut == "col_block" and not is_a:
            x = x.clone()
            x[:, -8:] = 0
        hi, lo = dr.split16(x)
        return hi.double(), (lo.double() if three else torch.zeros_like(hi, dtype=torch.float64))
    x = op.row_exp()
    if mut == "neighbour_exp" and is_a:  # the last tile decoded under its neighbour's exponent
        t = TILE[op.kind]
        x = x.clone()
        x[(op.exp.numel() - 1) * t:] = int(op.exp[-2])
    d = e - x
    d = d.clamp(-24 if legacy else -10000, 15)
    f = pow2(d)[:, None]
    hi = _h(op.hi.double() * f)
    if op.kind == "f24":
        about = 127 if (mut == "byte127" and is_a) else 128
        if legacy:  # v * s + o in fp16 with s = f / 32 and o = -4 f rounded to fp16 first
            s, o = _h(f / 32.0), _h(-(about / 32.0) * f)
            lo = _h(_h(op.lo.double() * s) + o)
        else:       # (v / 32 - 4) is exact; one rounding at the rescale
            lo = _h(op.lo_value(about) * f)
    elif op.kind == "planes":
        lo = _h(op.lo.double() * f)
    else:
        lo = torch.zeros_like(hi)
    if mut == "drop_lo":
        lo = torch.zeros_like(hi)
    if mut == "last_row" and is_a:
        hi, lo = hi.clone(), lo.clone()
        hi[-1], lo[-1] = 0, 0
    if mut == "lane_half" and is_a:  # k-block 1 of the last tile: the lanes 32.. hold what lanes ..31 should (features c ^ 4)
        hi = hi.clone()
        r0 = (op.exp.numel() - 1) * TILE[op.kind]
        c = torch.arange(16, 32)
        hi[r0:, c] = hi[r0:, c ^ 4]
    if mut == "col_block" and not is_a:
        hi, lo = hi.clone(), lo.clone()
        hi[:, -8:], lo[:, -8:] = 0, 0
    return hi, lo


def emulate(A, B, ea, eb, legacy=False, mut=None):
    """upnerf_wgrad16's arithmetic on stored operands (the comments above wgrad_f16p_kernel / wgrad_planes_kernel): every plane
    rescaled by 2^(e_tensor - e_tile) with ONE fp16 rounding, exact products summed (here in fp64), unscaled, rounded to fp32; db
    from the planes in natural units.  legacy: the arithmetic before this module existed -- the exponent difference clamped to
    [-24, 15] and f24's residual decoded as v * s + o with s = f / 32, o = -4 f in fp16.  mut: one of MUTATIONS."""
    three = A.kind in TWO_PLANES
    ah, al = _planes(A, ea, three, legacy, mut, True)
    bh, bl = _planes(B, eb, three, legacy, mut, False)
    acc = ah.t() @ bh
    if three:
        acc = acc + ah.t() @ bl + al.t() @ bh
    about = 127 if mut == "byte127" else 128
    nat = (A.hi.double() + (torch.zeros_like(al) if mut == "drop_lo" else A.lo_value(about))) * pow2(-A.row_exp())[:, None]
    if mut == "last_row":
        nat = nat[:-1]
    return dict(dW=(acc * 2.0 ** -(ea + eb)).float(), db=nat.sum(0).float())
