"""One host-side description of a field pass, decided ONCE.  plan_pass: what the pass stores and in which form --
rendering._FieldPass allocates its forward and backward buffers from the plan and reads its weight gradients' operands from it;
geometry's density-only pass takes its tiling from it.  param_blocks / t_blocks: the blocks of the packed buffer P and of its
transposed copies, layout_offsets: where each sits (packing.NerfPacker derives all it does from these).  wgrad_schedule: the
launches that write the gradient of P, against which operands and into which block -- _FieldPass.backward executes that list and
holds no offset or exponent slot of its own.  Host arithmetic only -- neither the library nor a device is touched, all of it can
be built (and tested) anywhere."""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache
from itertools import accumulate

# constants of include/upnerf_hip.h that size a pass (_lib re-exports them beside the structs)
X0, AUXK, CK = 64, 80, 16
WG_F32, WG_F16_TILE, WG_F16_FRAG, WG_F24, WG_PLANES = range(5)  # UPNERF_WG_*: how a weight-gradient operand is stored
TILE_PART_STRIDE = 1288  # UPNERF_TILE_PART_STRIDE
RR_PART_STRIDE = 512  # UPNERF_RR_PART_STRIDE
RR_TILE = 256
MODES = ("f16x3", "f32", "f16")

# What is the same for every pass.  Buffer names in allocation order, by the launch they are allocated in front of:
STAGES = {"aux": ("aux",),
          "field": ("sigma_s", "sigma_c", "rgb", "x0", "h16", "hexp", "h_lo8", "h", "e", "e16", "eexp", "hmask", "mx32", "g1", "g1_16",
                    "g1exp", "g2", "g2_16", "g2exp", "r1", "r1_16", "r1exp"),
          "composite": ("w_all", "w_sj", "w_cj", "w_s", "E_s", "G_c", "sum_sfeat", "t_weight", "c_depth", "s_depth", "rgb_map",
                        "rgb_joint_map"),
          "cbwd": ("d_sigma_s", "d_sigma_c", "d_rgb"),
          "fbwd": ("gz_e", "gz_h", "gz16", "gzexp", "gz_lo8", "gz_rg", "gz_rg16", "gzrgexp", "gz_g1", "gz_g2", "gz_g2_16", "gzg2exp",
                   "gz_r1", "dpre_s", "dpre_c", "dpre_rgb"),
          "part": ("tile_part", "ray_part"), "sums": ("rs_c", "rs_r")}
F16 = frozenset(("h16", "e16", "g1_16", "g2_16", "r1_16", "gz16", "gz_rg16", "gz_g2_16"))
I32 = frozenset(("hexp", "eexp", "g1exp", "g2exp", "r1exp", "gzexp", "gzrgexp", "gzg2exp"))
DTYPES = {**dict.fromkeys(F16, "float16"), **dict.fromkeys(I32, "int32"), "h_lo8": "uint8", "gz_lo8": "uint8", "hmask": "int64"}
# fp32 rows the field kernels write in whole tiles: allocated with the plan's Mp rows behind the M visible ones of their shape
PADDED = frozenset(("x0", "e", "g1", "g2", "r1", "gz_rg", "gz_g1", "gz_g2", "gz_r1"))
ZEROED = frozenset(("mx32",))  # must start at zero
# How the weight gradients read one logical tensor: UPNERF_WG_* kind, leading dimension, the buffers that hold the data, the
# per-tile exponents and the residual bytes, and the layer of those buffers it is (None: per call, or the buffer has none)
Operand = namedtuple("Operand", "kind ld data exp lo at", defaults=(None, None, None))
# The decisions of plan_pass (explained where they are taken; tile_rows and rows_capacity as the argument structs state them),
# `buffers`: name -> shape as the kernels' callers see it (None: a form the pass does not use), `operands`: name -> Operand.
PassPlan = namedtuple("PassPlan", "M Mp use16 rr tile_rows rows_capacity planes store16 store24 ntile e_frag joined rg16 g2f "
                                  "partials ride buffers operands")


def plan_pass(W, W2, D, R, S, mode, use_cand, use_rgb, rgb_joint, train, *, FIELD_MODE, WGRAD_STORE, FIELD_RR, TILE_PARTIALS,
              WGRAD_CHAIN, JOIN_HEADS, VEC_RIDE) -> PassPlan:
    if FIELD_MODE not in MODES:
        raise ValueError(f"unknown FIELD_MODE {FIELD_MODE!r} (one of {MODES})")
    use16 = FIELD_MODE != "f32" and W == 256 and S >= 32  # the f16 matrix-core kernels (csrc/field16*.hip); otherwise fp32 MFMA
    if FIELD_MODE == "f16" and not use16:
        raise ValueError("FIELD_MODE 'f16' needs W = 256 and at least 32 samples per ray")
    if WGRAD_STORE == "f24" and not WGRAD_CHAIN:
        raise RuntimeError("UPNERF_WGRAD_STORE=f24 needs UPNERF_WGRAD_CHAIN=1 "
                           "(the hi + lo8 operands are read by the chained run only)")
    # register-resident fp16 kernels: 256-sample tiles, per-sample tensors padded to whole tiles, stored as operand fragments
    rr = bool(use16 and FIELD_MODE == "f16" and FIELD_RR)
    M = R * S
    Mp = (M + RR_TILE - 1) // RR_TILE * RR_TILE if rr else M
    joint, want_feat, cand, col = mode <= 1, mode != 2, train and use_cand, train and use_rgb
    # the trunk STORED as fp16 tiles + exponents: always in the f16 mode, on request in the f16x3 mode (rendering.WGRAD_STORE)
    store16 = bool(train and use16 and (FIELD_MODE == "f16" or WGRAD_STORE in ("f16", "f24")))
    store24 = store16 and FIELD_MODE != "f16" and WGRAD_STORE == "f24"
    ntile = Mp // 32 if rr else (M + 63) // 64  # one exponent per 64 rows whatever the kernel's tile (rr: per 32)
    # both heads on, chained f16 weight gradients, per-tile partial sums (upnerf_ray_sum, their fallback, wants dense tensors)
    joined = bool(cand and col and use16 and JOIN_HEADS and WGRAD_CHAIN and TILE_PARTIALS)
    # rr: e leaves as fragments only (compositing and the joined heads' weight gradient read those) unless a single head is on in
    # training, whose separate weight gradient wants fp32 rows
    e_frag = bool(rr and (joined if train else want_feat))
    rg16 = joined and rr  # [gz_r1 | gz_g1] as fp16 fragments only, against e's fragments
    g2f = bool(cand and e_frag)  # gz_g2 as fragments against g1's (candidate_encoding.2)
    # per-tile sums from the backward kernel: the 128-wide vector heads and the per-ray sums (rr: the per-ray sums only)
    partials = ("ray" if rr else "tile") if (use16 and TILE_PARTIALS and (cand or col)) else "none"
    ride = bool(train and VEC_RIDE and WGRAD_CHAIN and (rr or (FIELD_MODE != "f16" and W == 256)))
    ops = {}

    def forms(name, n16, nexp, on, frag, w):
        """Shapes of one logical [M][w] tensor (fp32 rows, or rr: fp16 operand fragments, their exponents per 32 rows) and the
        operand that reads it; one form at most."""
        if not on:
            return None, None, None
        ops[name] = Operand(WG_F16_FRAG, w, n16, nexp) if frag else Operand(WG_F32, w, name)
        return (None, (Mp, w), (Mp // 32,)) if frag else ((M, w), None, None)

    e, e16, eexp = forms("e", "e16", "eexp", train or want_feat, e_frag, W)
    g1, g1_16, g1exp = forms("g1", "g1_16", "g1exp", cand, e_frag, W2)
    g2, g2_16, g2exp = forms("g2", "g2_16", "g2exp", use_cand and (train or joint), e_frag, W2)
    r1, r1_16, r1exp = forms("r1", "r1_16", "r1exp", col, e_frag, W2)
    gz_rg, gz_rg16, gzrgexp = forms("gz_rg", "gz_rg16", "gzrgexp", joined, rg16, W)
    gz_g2, gz_g2_16, gzg2exp = forms("gz_g2", "gz_g2_16", "gzg2exp", cand, g2f, W2)
    per_ray, per_sample, trunk16 = (R, S), (M,), (D, Mp, W) if store16 else None
    # Without `train` nothing only the backward pass reads is planned: the kernels skip those stores, 8 of the 11 KB per sample
    buffers = {
        "aux": (R, AUXK) if use_rgb else None, "sigma_s": per_sample, "sigma_c": per_sample if use_cand else None,
        "rgb": (M, 3) if use_rgb else None, "x0": (M, X0), "h16": trunk16, "hexp": (D, ntile) if store16 else None,
        "h_lo8": (D, M, W) if store24 else None,
        # fp32 h: every layer, or beside h16 the last one only (for the density head and the final layer; rr: fragments do)
        "h": ((1 if store16 else D, M, W) if not (store16 and rr) else None) if train else None,
        "e": e, "e16": e16, "eexp": eexp,
        # ReLU decisions, 64 bits per lane and tile (rr: 128 per lane)
        "hmask": (((D + 3) * Mp * 4 if rr else (D + 1) * ((M + 127) // 128) * 512,)) if train else None,
        # running max|.| of the stored tensors (scales of the weight gradients): [0, 16) this pass, [16, 32) the backward kernel
        "mx32": (32,) if train else None,
        "g1": g1, "g1_16": g1_16, "g1exp": g1exp, "g2": g2, "g2_16": g2_16, "g2exp": g2exp, "r1": r1, "r1_16": r1_16, "r1exp": r1exp,
        "w_all": per_ray if joint else None, "w_sj": per_ray if joint else None, "w_cj": per_ray if joint else None, "w_s": per_ray,
        "E_s": (R, W) if want_feat else None, "G_c": (R, W2) if joint else None, "sum_sfeat": (R,) if want_feat else None,
        "t_weight": (R,) if joint else None, "c_depth": (R,) if joint else None, "s_depth": (R,),
        "rgb_map": (R, 3) if use_rgb else None, "rgb_joint_map": (R, 3) if rgb_joint else None,
        "d_sigma_s": per_sample if train else None, "d_sigma_c": per_sample if (train and joint) else None,
        "d_rgb": (M, 3) if col else None, "gz_e": (M, W) if (train and not rr) else None,  # (rr: layer D of gz16)
        "gz_h": (D, M, W) if (train and not store16) else None, "gz16": (D + int(rr), Mp, W) if store16 else None,
        "gzexp": (D + int(rr), ntile) if store16 else None, "gz_lo8": (D, M, W) if store24 else None,
        "gz_rg": gz_rg, "gz_rg16": gz_rg16, "gzrgexp": gzrgexp,
        "gz_g1": (M, W2) if (cand and not joined) else None,  # (joined: a column block of gz_rg)
        "gz_g2": gz_g2, "gz_g2_16": gz_g2_16, "gzg2exp": gzg2exp, "gz_r1": (M, W2) if (col and not joined) else None,
        "dpre_s": per_sample if train else None, "dpre_c": per_sample if cand else None, "dpre_rgb": (M, 4) if col else None,
        "tile_part": ((M + 63) // 64, TILE_PART_STRIDE) if partials == "tile" else None,
        "ray_part": (Mp // 32, RR_PART_STRIDE) if partials == "ray" else None,
        "rs_c": (R, W2) if cand else None, "rs_r": (R, W2) if col else None}
    if train:  # the trunk: fp32 rows, or fp16 tiles (rr: fragments; store24: + residual bytes); `at` None: the caller names the layer
        kind16 = WG_F24 if store24 else WG_F16_FRAG if rr else WG_F16_TILE
        ops["x0"] = Operand(WG_F32, X0, "x0")
        ops["h"] = h = Operand(kind16, W, "h16", "hexp", "h_lo8" if store24 else None) if store16 else Operand(WG_F32, W, "h")
        ops["gz"] = gz = Operand(kind16, W, "gz16", "gzexp", "gz_lo8" if store24 else None) if store16 else Operand(WG_F32, W, "gz_h")
        ops["h_last"] = h._replace(at=D - 1) if rr or not store16 else Operand(WG_F32, W, "h", at=0)
        ops["gz_e"] = gz._replace(at=D) if rr else Operand(WG_F32, W, "gz_e")
        if not joined:
            ops.update({k: Operand(WG_F32, W2, k) for k, on in (("gz_g1", cand), ("gz_r1", col)) if on})
    return PassPlan(M, Mp, use16, rr, RR_TILE if rr else 64, Mp if rr else 0, 1 if FIELD_MODE == "f16" else 2, store16, store24, ntile,
                    e_frag, joined, rg16, g2f, partials, ride, buffers, ops)


# ---- the parameter blocks: include/upnerf_hip.h:upnerf_layout stated ONCE -- offsets, packing, fragment copies, transposed copies
# and the destinations of the weight gradients are all read off these two tables
IN_XYZ, IN_DIR, A_DIM = 63, 27, 48  # used columns of the encodings and of the appearance embedding
EXP_FINAL, EXP_C1, EXP_C2, EXP_R1, EXP_HEAD_T = 8, 9, 10, 11, 12  # upnerf_frag16's exponent ids of the matrices; trunk layer l: id l
Part = namedtuple("Part", "name col0 cols")  # used columns [col0, col0 + cols) of a block and what they multiply


class Block(namedtuple("Block", "field layer rows cols ld matrix parts exp used_rows")):
    """One block of P, [rows][ld] floats rounded up to 4: the layout field it fills (layer: of `w` / `b`), `cols` used columns in
    `parts` (every other column, and the rows from used_rows on, are zero padding), matrix: stored as MFMA fragments on the
    kernel side under exponent id `exp`; a vector stays as it is."""
    __slots__ = ()

    def part(self, name) -> Part:
        return next(p for p in self.parts if p.name == name)


# A block of the transposed set PT, [rows][ld]: feed f puts f.src[:, f.col0 : f.col0 + f.cols]^T at columns [f.dst_col0, + f.src.rows)
TBlock = namedtuple("TBlock", "field layer rows ld feeds")
Feed = namedtuple("Feed", "src col0 cols dst_col0 exp")


def block_size(b) -> int:
    return (b.rows * b.ld + 3) // 4 * 4


def block_offset(L, b) -> int:
    """Where block b (of either table) starts in the layout L (LayoutOffsets or the kernels' struct)."""
    return getattr(L, b.field) if b.layer is None else getattr(L, b.field)[b.layer]


@lru_cache(maxsize=None)
def param_blocks(W, D, skip=-1):
    """The blocks of P in the order of the struct.  skip: the layer that also reads the encoding, -1 = none."""
    W2 = W // 2

    def mat(field, layer, rows, exp, *parts):  # parts: (name, used columns, columns taken)
        ps, c0 = [], 0
        for name, cols, width in parts:
            ps.append(Part(name, c0, cols))
            c0 += width
        return Block(field, layer, rows, sum(p.cols for p in ps), c0, True, tuple(ps), exp, rows)

    def vec(field, layer, cols, rows=1, used=1):
        return Block(field, layer, rows, cols, cols, False, (Part(field, 0, cols),), None, used)

    x, h = ("x", IN_XYZ, X0), ("h", W, W)
    trunk = [mat("w", l, W, l, *((x,) if l == 0 else (x, h) if l == skip else (h,))) for l in range(D)]
    return tuple(trunk + [vec("b", l, W) for l in range(D)] + [
        mat("we", None, W, EXP_FINAL, h), vec("be", None, W), vec("wsig", None, W), vec("bsig", None, 1),
        mat("wc1", None, W2, EXP_C1, ("e", W, W), ("c", CK, CK)), vec("bc1", None, W2),
        mat("wc2", None, W2, EXP_C2, ("g1", W2, W2)), vec("bc2", None, W2), vec("wcsig", None, W2), vec("bcsig", None, 1),
        mat("wr1", None, W2, EXP_R1, ("e", W, W), ("dir", IN_DIR, IN_DIR), ("a", A_DIM, AUXK - IN_DIR)), vec("br1", None, W2),
        vec("wr2", None, W2, rows=4, used=3), vec("br2", None, 3)])


@lru_cache(maxsize=None)
def blocks_by_field(W, D, skip=-1) -> dict:
    """param_blocks by layout field: one Block, or for `w` / `b` one per layer."""
    blocks = param_blocks(W, D, skip)
    return {**{b.field: b for b in blocks}, "w": blocks[:D], "b": blocks[D:2 * D]}


@lru_cache(maxsize=None)
def t_blocks(W, D, skip=-1):
    """The blocks of PT in the order of the struct's t_* fields.  t_skipx is always there and fed only under a skip."""
    W2, B = W // 2, blocks_by_field(W, D, skip)
    own = [(b, b.parts[-1].col0) for b in B["w"]]  # a layer's transposed copy: the columns of its last part, padding included
    xs = B["w"][skip] if 0 < skip < D else None
    return tuple([TBlock("t_w", b.layer, b.ld - c0, W, (Feed(b, c0, b.ld - c0, 0, b.exp),)) for b, c0 in own] + [
        TBlock("t_skipx", None, X0, W, (Feed(xs, 0, xs.part("h").col0, 0, xs.exp),) if xs else ()),
        TBlock("t_we", None, W, W, (Feed(B["we"], 0, W, 0, EXP_FINAL),)),
        TBlock("t_head", None, W, W, (Feed(B["wr1"], 0, W, 0, EXP_HEAD_T), Feed(B["wc1"], 0, W, W2, EXP_HEAD_T))),
        TBlock("t_wc2", None, W2, W2, (Feed(B["wc2"], 0, W2, 0, EXP_C2),))])


LayoutOffsets = namedtuple("LayoutOffsets", "W D skip w b we be wsig bsig wc1 bc1 wc2 bc2 wcsig bcsig wr1 br1 wr2 br2 total "
                                            "t_w t_skipx t_we t_head t_wc2 t_total")


@lru_cache(maxsize=None)
def layout_offsets(W, D, skip=-1) -> LayoutOffsets:
    """Offsets (floats) of the blocks of P and of the transposed copies PT: laid end to end in the order of the two tables, each
    starting on a multiple of 4 (w, b, t_w: one offset per layer)."""
    def end_to_end(blocks):
        ends = list(accumulate(block_size(b) for b in blocks))
        return [0] + ends[:-1], ends[-1]

    o, total = end_to_end(param_blocks(W, D, skip))
    t, t_total = end_to_end(t_blocks(W, D, skip))
    return LayoutOffsets(W, D, skip, tuple(o[:D]), tuple(o[D:2 * D]), *o[2 * D:], total, tuple(t[:D]), *t[D:], t_total)


# ---- the weight-gradient launches of a pass
# Slots of the two [16] tables of running maxima (upnerf_field_fwd_args.amax: the B operands, upnerf_field_bwd_args.gmax: the A
# operands) and of the exponents upnerf_scale_exponents makes of them.  Trunk layer l: slot l in both (h_l, gz_l); behind them:
ExpSlots = namedtuple("ExpSlots", "final g1 g2 r1 joined x0")  # e / gz_e, g1 / gz_g1, gz_g2, r1 / gz_r1, [gz_r1 | gz_g1], x0


def exp_slots(D) -> ExpSlots:
    return ExpSlots(D, D + 1, D + 2, D + 3, D + 4, D + 4)  # (joined is a slot of gmax, x0 one of amax)


# What a Launch is: MAT upnerf_wgrad16 (dW [N][ldo] = A^T B, db = column sums of A), VEC / VEC_FRAG upnerf_vec_wgrad / its twin
# for operand fragments (a 1- or 3-wide head `v` against the rows of B), PART the same result out of the backward kernel's per-tile
# sums (upnerf_tile_part_finish writes it, no launch of its own), RAY upnerf_wgrad over rays (fp32; per-ray sums A against the
# per-ray inputs B).
MAT, VEC, VEC_FRAG, PART, RAY = "mat", "vec", "vec_frag", "part", "ray"
# A, B: (name in PassPlan.operands, layer or None) -- RAY: (buffer of the backward pass, None), (saved input, None); v: the head's
# buffer [M] or [M][4], N of them used; ea / eb: exponent slots of A / B (MAT only); dW, db, dW2, db2: offsets into dP (floats);
# n2 > 0: rows [n2, N) go to dW2 / ldo2 / db2; ride: the VEC record of a 1-wide head that rides on this MAT launch, or None
Launch = namedtuple("Launch", "kind A B v N K ea eb dW ldo db n2 dW2 ldo2 db2 ride", defaults=(0, None, 0, None, None))
# trunk: the layers, the final layer and the shared density head; part: None, or the (candidate, colour) PART records (None: that
# head is off); cand, rgb: the heads' own launches (the joined first layers are the candidate segment's), () where a head is off
Schedule = namedtuple("Schedule", "trunk part cand rgb")


def wgrad_schedule(plan: PassPlan, L, skip, use_cand, use_rgb) -> Schedule:
    """Every launch of a training pass that writes into dP, in launch order; each parameter block of the heads that are on is
    written by exactly one of them.  L: the layout's offsets (LayoutOffsets, or anything hashable with its fields)."""
    frag = frozenset(k for k, o in plan.operands.items() if o.kind == WG_F16_FRAG)
    return _schedule(plan.joined, plan.ride, plan.partials == "tile", frag, L, skip, bool(use_cand), bool(use_rgb))


@lru_cache(maxsize=None)
def _schedule(joined, ride, tile_part, frag, L, skip, cand, rgb) -> Schedule:
    W, W2, D, E = L.W, L.W // 2, L.D, exp_slots(L.D)

    def mat(A, N, B, K, ea, eb, dW, ldo, db, **kw):
        return Launch(MAT, A, B, None, N, K, ea, eb, dW, ldo, db, **kw)

    def vec(v, nvec, X, K, dW, db, part=False):
        return Launch(PART if part else VEC_FRAG if X in frag else VEC, None, (X, None), v, nvec, K, None, None, dW, K, db)

    B = blocks_by_field(W, D, skip)
    trunk = []
    for l, b in enumerate(B["w"]):  # one launch per column part: the encoding's columns, the previous layer's
        for p in b.parts:
            X, K, eb = (("x0", None), X0, E.x0) if p.name == "x" else (("h", l - 1), W, l - 1)
            trunk.append(mat(("gz", l), W, X, K, l, eb, L.w[l] + p.col0, b.ld, L.b[l] if p is b.parts[0] else None))
    # the shared density head reads the final layer's B operand: where the plan says so its gradient rides on that launch
    sig = vec("dpre_s", 1, "h_last", W, L.wsig, L.bsig)
    trunk.append(mat(("gz_e", None), W, ("h_last", None), W, E.final, D - 1, L.we, B["we"].ld, L.be, ride=sig if ride else None))
    if not ride:
        trunk.append(sig)
    csig = vec("dpre_c", 1, "g2", W2, L.wcsig, L.bcsig, tile_part)
    rgb2 = vec("dpre_rgb", 3, "r1", W2, L.wr2, L.br2, tile_part)
    e, wc1, wc2, wr1 = ("e", None), B["wc1"], B["wc2"], B["wr1"]
    c, r = [], []
    if cand:
        if joined:  # rows [0, W2) -> wr1 / br1 (colour head), rows [W2, W) -> wc1 / bc1 (candidate head)
            c.append(mat(("gz_rg", None), W, e, W, E.joined, E.final, L.wr1, wr1.ld, L.br1, n2=W2, dW2=L.wc1, ldo2=wc1.ld,
                         db2=L.bc1))
        else:
            c.append(mat(("gz_g1", None), W2, e, W, E.g1, E.final, L.wc1, wc1.ld, L.bc1))
        c.append(Launch(RAY, ("rs_c", None), ("c_rows", None), None, W2, CK, None, None, L.wc1 + wc1.part("c").col0, wc1.ld, None))
        c.append(mat(("gz_g2", None), W2, ("g1", None), W2, E.g2, E.g1, L.wc2, wc2.ld, L.bc2))
        c += [] if tile_part else [csig]
    if rgb:
        if not joined:
            r.append(mat(("gz_r1", None), W2, e, W, E.r1, E.final, L.wr1, wr1.ld, L.br1))
        r.append(Launch(RAY, ("rs_r", None), ("aux", None), None, W2, AUXK, None, None, L.wr1 + wr1.part("dir").col0, wr1.ld, None))
        r += [] if tile_part else [rgb2]
    part = (csig if cand else None, rgb2 if rgb else None) if tile_part else None
    return Schedule(tuple(trunk), part, tuple(c), tuple(r))
