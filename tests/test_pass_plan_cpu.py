"""The plan of a field pass (upnerf_amd/pass_plan.py) over the full product of switches, pass kinds and shapes: every logical
tensor in exactly one storage form, nothing planned that the pass does not need, whole tiles behind the register-resident
kernels, operand kinds that follow the storage.  Its weight-gradient schedule over the same product and every skip position:
each parameter block of the layout written exactly once and at the pitch the table of blocks (param_blocks) states, by launches
whose operands the plan holds in a form the kernel takes.
Host arithmetic only: no library, no device."""
import itertools

import numpy as np
import pytest

from upnerf_amd import pass_plan as pp

# (mode, use_cand, use_rgb, rgb_joint): what render_rays produces (both heads / candidate only / colour only / neither), and the
# joint colour of encode_feat = False
PASSES = [(1, True, True, False), (0, True, False, False), (2, False, True, False), (3, False, False, False), (1, True, True, True)]
SHAPES = [(5, 31), (5, 32), (5, 33), (7, 40), (3, 256), (3, 257)]  # the 32-sample threshold, a ragged 64-tile, a 256-tile +- 1
FIELDS = [(256, 8), (64, 4)]
BOOLS = ("FIELD_RR", "TILE_PARTIALS", "WGRAD_CHAIN", "JOIN_HEADS", "VEC_RIDE")
SHAPE_MSG = "FIELD_MODE 'f16' needs W = 256 and at least 32 samples per ray"
F24_MSG = "UPNERF_WGRAD_STORE=f24 needs UPNERF_WGRAD_CHAIN=1 (the hi + lo8 operands are read by the chained run only)"
# one logical tensor -> the buffers that can hold it (fp32 rows first)
FORMS = {"e": ("e", "e16"), "g1": ("g1", "g1_16"), "g2": ("g2", "g2_16"), "r1": ("r1", "r1_16"), "gz": ("gz_h", "gz16"),
         "gz_g1": ("gz_g1", "gz_rg", "gz_rg16"), "gz_r1": ("gz_r1", "gz_rg", "gz_rg16"), "gz_g2": ("gz_g2", "gz_g2_16")}
EXPS = {"e16": "eexp", "g1_16": "g1exp", "g2_16": "g2exp", "r1_16": "r1exp", "gz_rg16": "gzrgexp", "gz_g2_16": "gzg2exp",
        "h16": "hexp", "gz16": "gzexp"}
# written by the field kernels in whole tiles (include/upnerf_hip.h, rows_capacity)
TILED = ("x0", "h16", "e", "e16", "g1", "g1_16", "g2", "g2_16", "r1", "r1_16", "gz16", "gz_rg", "gz_rg16", "gz_g1", "gz_g2",
         "gz_g2_16", "gz_r1")
BACKWARD_ONLY = ("h", "h16", "hexp", "h_lo8", "hmask", "mx32", "g1", "g1_16", "g1exp", "r1", "r1_16", "r1exp")
BACKWARD_STAGES = ("cbwd", "fbwd", "part", "sums")
ALL_NAMES = {k for names in pp.STAGES.values() for k in names}


def forms_check(p, sw, train, kind, W, D, use16):
    """Everything that does not depend on the number of samples beyond `use16`: which form each logical tensor has, the
    decisions, the operands."""
    mode, use_cand, use_rgb, rgb_joint = kind
    fm = sw["FIELD_MODE"]
    joint, want_feat = mode <= 1, mode != 2
    have = {k for k, shape in p.buffers.items() if shape is not None}
    assert set(p.buffers) == ALL_NAMES
    rr = bool(use16 and fm == "f16" and sw["FIELD_RR"])
    assert (p.use16, p.rr, p.planes, p.tile_rows) == (use16, rr, 1 if fm == "f16" else 2, 256 if rr else 64)
    assert p.store16 == bool(train and use16 and (fm == "f16" or sw["WGRAD_STORE"] != "f32"))
    assert p.store24 == (p.store16 and fm == "f16x3" and sw["WGRAD_STORE"] == "f24")
    # ---- one storage form per logical tensor, none where the pass has no use for it
    need = {"e": train or want_feat, "g1": use_cand and train, "g2": use_cand and (train or joint), "r1": use_rgb and train,
            "gz": train, "gz_g1": use_cand and train, "gz_r1": use_rgb and train, "gz_g2": use_cand and train}
    for name, forms in FORMS.items():
        assert len(have.intersection(forms)) == int(need[name]), (name, sorted(have.intersection(forms)))
    # h: every layer as fp32 or as fp16 tiles; beside the tiles a fp32 copy of the last layer unless its readers take fragments
    h = p.buffers["h"]
    assert ("h16" in have) == p.store16 and (h is not None) == (train and not (p.store16 and rr))
    assert h is None or h[0] == (1 if p.store16 else D)
    # gz_e: fp32 rows, or (rr) one more layer of gz16
    assert ("gz_e" in have) == (train and not rr)
    assert "gz16" not in have or p.buffers["gz16"][0] == D + int(rr)
    for k16, kexp in EXPS.items():
        assert (k16 in have) == (kexp in have)
    assert ("h_lo8" in have) == ("gz_lo8" in have) == p.store24
    if not train:
        assert not have.intersection(BACKWARD_ONLY) and not any(have.intersection(pp.STAGES[s]) for s in BACKWARD_STAGES)
        assert not (p.joined or p.rg16 or p.g2f or p.ride or p.store16) and p.partials == "none"
    # ---- decisions are off wherever something they depend on is
    joined = bool(train and use16 and use_cand and use_rgb and sw["JOIN_HEADS"] and sw["WGRAD_CHAIN"] and sw["TILE_PARTIALS"])
    assert p.joined == joined and p.rg16 == (joined and rr)
    assert p.e_frag == (rr and (joined if train else want_feat)) == ("e16" in have)
    assert p.g2f == bool(use_cand and train and p.e_frag) == ("gz_g2_16" in have)
    assert p.ride == bool(train and sw["VEC_RIDE"] and sw["WGRAD_CHAIN"] and (rr or (fm != "f16" and W == 256)))
    part = bool(train and use16 and sw["TILE_PARTIALS"] and (use_cand or use_rgb))
    assert p.partials == (("ray" if rr else "tile") if part else "none")
    assert ("tile_part" in have, "ray_part" in have) == (p.partials == "tile", p.partials == "ray")
    assert not joined or p.partials != "none"  # (upnerf_ray_sum, the fallback, reads separate dense gz_g1 / gz_r1)
    # ---- operand forms follow the storage
    kind16 = pp.WG_F24 if p.store24 else pp.WG_F16_FRAG if rr else pp.WG_F16_TILE
    for name, o in p.operands.items():
        assert o.data in have and (o.kind == pp.WG_F32 or o.kind == kind16), (name, o)
        assert (o.exp is not None) == (o.kind != pp.WG_F32) and (o.lo is not None) == (o.kind == pp.WG_F24)
        assert (o.exp is None or o.exp in have) and (o.lo is None or o.lo in have)
        assert (o.kind == pp.WG_F32) == (o.data not in pp.DTYPES) and o.ld == p.buffers[o.data][-1]
    if train:
        want = {"x0", "h", "gz", "h_last", "gz_e"} | {k for k in ("e", "g1", "g2", "r1", "gz_g2") if need[k]}
        want |= {"gz_rg"} if joined else {k for k in ("gz_g1", "gz_r1") if need[k]}
        assert set(p.operands) == want
    return have.intersection(TILED), have.intersection(EXPS.values())


def sizes_check(p, R, S, tiled, exps):
    """What depends on the shape: whole tiles behind the register-resident kernels, the length of every exponent table."""
    M = R * S
    if p.rr:
        assert p.M == M and p.Mp % 256 == 0 and 0 <= p.Mp - M < 256 and p.rows_capacity == p.Mp
        # (allocated rows: the plan's Mp for the names in PADDED, the sample axis of the shape otherwise)
        assert all(k in pp.PADDED or p.buffers[k][-2] == p.Mp for k in tiled)
    else:
        assert p.M == p.Mp == M and p.rows_capacity == 0
    for k in tiled:
        assert p.buffers[k][-2] == (M if k in pp.PADDED else p.Mp)
    ntile = p.Mp // 32 if p.rr else -(-M // 64)
    assert p.ntile == ntile and all(p.buffers[k][-1] == ntile for k in exps)


def test_every_plan_is_one_description():
    n = raised = 0
    for fm, ws, bits, train, kind, (W, D) in itertools.product(pp.MODES, ("f32", "f16", "f24"), itertools.product((0, 1), repeat=5),
                                                              (False, True), PASSES, FIELDS):
        sw = dict(zip(BOOLS, bits), FIELD_MODE=fm, WGRAD_STORE=ws)
        bad_f24 = ws == "f24" and not sw["WGRAD_CHAIN"]
        seen = {}  # use16 -> (the plan's forms as a tuple, what forms_check returned): the forms are checked once per class ...
        for R, S in SHAPES:
            use16 = fm != "f32" and W == 256 and S >= 32
            bad_shape = fm == "f16" and not use16
            if bad_shape or bad_f24:
                exc, msg = (ValueError, SHAPE_MSG) if bad_shape else (RuntimeError, F24_MSG)
                try:
                    pp.plan_pass(W, W // 2, D, R, S, *kind, train, **sw)
                except exc as e:
                    assert str(e) == msg
                    raised += 1
                    continue
                pytest.fail(f"no {exc.__name__} for {sw} W {W} S {S}")
            p = pp.plan_pass(W, W // 2, D, R, S, *kind, train, **sw)
            forms = (p[2:5], p[6:9], p[10:16], tuple(map(bool, p.buffers.values())), p.operands)
            if use16 not in seen:
                seen[use16] = (forms, forms_check(p, sw, train, kind, W, D, use16))
            assert forms == seen[use16][0]  # ... and are the same plan for every other shape of the class
            sizes_check(p, R, S, *seen[use16][1])
            n += 1
    assert n == 23200 and raised == 11360


def test_unknown_field_mode_raises():
    sw = dict(zip(BOOLS, (1,) * 5), FIELD_MODE="bf16", WGRAD_STORE="f32")
    with pytest.raises(ValueError, match=r"unknown FIELD_MODE 'bf16' \(one of \('f16x3', 'f32', 'f16'\)\)"):
        pp.plan_pass(256, 128, 8, 5, 33, 1, True, True, False, True, **sw)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layout's offsets and the weight-gradient schedule
LAYOUTS = [(256, 8, 4), (256, 8, -1), (256, 8, 1), (64, 4, -1), (256, 1, -1), (64, 1, -1)]  # (W, D, skip; -1: none)
SCHED_SHAPES = [(5, 31), (5, 33)]  # the schedule sees R and S through the plan only: one shape on each side of the 32-sample threshold
VEC_K = (32, 64, 128, 256)  # include/upnerf_hip.h: upnerf_vec_wgrad


def blocks(W, D, skip):
    """(trunk, candidate head, colour head): [(field of the layout, layer or None, rows, columns)] as include/upnerf_hip.h states
    the blocks -- what a pass must write, padding left out (bsig / bcsig: 1 of 4, wr2 / br2: 3 of 4 rows)."""
    W2 = W // 2
    kin = [pp.X0 if l == 0 else pp.X0 + W if l == skip else W for l in range(D)]
    trunk = [("w", l, W, kin[l]) for l in range(D)] + [("b", l, 1, W) for l in range(D)]
    trunk += [("we", None, W, W), ("be", None, 1, W), ("wsig", None, 1, W), ("bsig", None, 1, 1)]
    cand = [("wc1", None, W2, W + pp.CK), ("bc1", None, 1, W2), ("wc2", None, W2, W2), ("bc2", None, 1, W2), ("wcsig", None, 1, W2),
            ("bcsig", None, 1, 1)]
    rgb = [("wr1", None, W2, W + pp.AUXK), ("br1", None, 1, W2), ("wr2", None, 3, W2), ("br2", None, 1, 3)]
    return trunk, cand, rgb


def offset(L, name, l):
    return getattr(L, name) if l is None else getattr(L, name)[l]


@pytest.mark.parametrize("W,D,skip", LAYOUTS)
def test_layout_offsets_closed_form(W, D, skip):
    """Every block starts on a multiple of 4, the blocks are disjoint and ascend in the order of the struct, `total` is the end of
    the last one; the same for the transposed copies."""
    L = pp.layout_offsets(W, D, skip)
    assert (L.W, L.D, L.skip) == (W, D, skip) and len(L.w) == len(L.b) == len(L.t_w) == D
    end = 0
    for name, l, rows, cols in sum(blocks(W, D, skip), []):
        o = offset(L, name, l)
        assert o % 4 == 0 and end <= o < end + 4, (name, l)  # (at most the alignment's padding between two blocks)
        end = o + (4 if name == "wr2" else rows) * cols  # (the colour matrix has a fourth row of padding)
    assert L.total == (end + 3) // 4 * 4 == L.br2 + 4
    W2, end = W // 2, 0
    t = [(L.t_w[l], (pp.X0 if l == 0 else W) * W) for l in range(D)]
    for o, n in t + [(L.t_skipx, pp.X0 * W), (L.t_we, W * W), (L.t_head, W * W), (L.t_wc2, W2 * W2)]:
        assert o % 4 == 0 and o == end
        end = o + n
    assert L.t_total == end


def records(sched):
    """Every record of a schedule, the riding head and the tile-part targets included."""
    out = list(sched.trunk + sched.cand + sched.rgb) + [r for r in sched.part or () if r is not None]
    return out + [r.ride for r in out if r.ride is not None]


def coverage_check(sched, L, use_cand, use_rgb):
    """Each element of the blocks the pass's heads own is written exactly once, nothing else at all."""
    count, expect = np.zeros(L.total, np.int32), np.zeros(L.total, np.int32)

    def mark(a, off, rows, cols, ld):
        idx = off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        a[idx] += 1  # (an index past `total` raises)

    for r in records(sched):
        n1 = r.n2 or r.N
        mark(count, r.dW, n1, r.K, r.ldo)
        if r.db is not None:
            mark(count, r.db, 1, n1, 0)
        if r.n2:
            mark(count, r.dW2, r.N - r.n2, r.K, r.ldo2)
            mark(count, r.db2, 1, r.N - r.n2, 0)
        else:
            assert (r.dW2, r.ldo2, r.db2) == (None, 0, None)
        assert r.kind != pp.RAY or r.db is None
    trunk, cand, rgb = blocks(L.W, L.D, L.skip)
    for name, l, rows, cols in trunk + (cand if use_cand else []) + (rgb if use_rgb else []):
        mark(expect, offset(L, name, l), rows, cols, cols)
    assert int(expect.max()) == 1
    bad = np.flatnonzero(count != expect)
    assert bad.size == 0, (bad[:8], count[bad[:8]], expect[bad[:8]])


def pitches_check(sched, L):
    """Every matrix-shaped destination (MAT, RAY; the second row block of a split launch too) lies inside one block of the table
    of parameter blocks and is written at that block's pitch."""
    tab = [(pp.block_offset(L, b), b) for b in pp.param_blocks(L.W, L.D, L.skip)]
    for r in records(sched):
        if r.kind in (pp.MAT, pp.RAY):
            for dW, ldo, rows in ((r.dW, r.ldo, r.n2 or r.N),) + (((r.dW2, r.ldo2, r.N - r.n2),) if r.n2 else ()):
                o, b = max((x for x in tab if x[0] <= dW), key=lambda x: x[0])
                assert ldo == b.ld and b.matrix and rows == b.used_rows and (dW - o) + r.K <= b.ld, (r, b.field)


def operands_check(p, sched, W):
    """Every operand is planned in a form the launch takes (include/upnerf_hip.h: UPNERF_WG_*, upnerf_wgrad_desc.v, upnerf_vec_wgrad
    and its twin)."""
    planned = lambda k: p.buffers[k] is not None

    def operand(ref, width):
        name, l = ref
        o = p.operands[name]
        assert planned(o.data) and o.ld >= width and p.buffers[o.data][-1] >= width, (ref, o)
        assert o.kind == pp.WG_F32 or planned(o.exp), (ref, o)
        assert (l is None) or (o.at is None and 0 <= l < p.buffers[o.data][0]), (ref, o)  # a layer only where the caller names it
        return o.kind

    for r in records(sched):
        if r.kind == pp.MAT:
            ka, kb = operand(r.A, r.N), operand(r.B, r.K)
            assert ka == kb or (kb == pp.WG_F32 and r.B[0] == "x0"), r
            assert r.N % 4 == 0 and r.K % 4 == 0 and r.ldo % 4 == 0 and r.ldo >= r.K and r.v is None
            if ka in (pp.WG_F16_TILE, pp.WG_F24):
                assert (r.N, r.K) in ((256, 256), (256, 64)), r
            elif ka == pp.WG_F16_FRAG:
                assert (r.N, r.K) in ((256, 256), (128, 128)) if kb == ka else (r.N, r.K) == (256, 64), r
            if r.ride is not None:  # N = K = 256 on fp32 rows with the 3-term split, or on fragments on both sides
                assert (r.N, r.K) == (256, 256) and ka == kb and (ka == pp.WG_F16_FRAG or (ka == pp.WG_F32 and p.planes == 2)), r
                assert r.ride.B == r.B and r.ride.N == 1 and r.ride.kind in (pp.VEC, pp.VEC_FRAG)
        elif r.kind == pp.RAY:
            assert planned(r.A[0]) and p.buffers[r.A[0]][-1] == r.N and r.A[1] is None and r.B[1] is None
            assert (r.B[0], r.K) == ("c_rows", pp.CK) or (r.B[0] == "aux" and p.buffers["aux"][-1] == r.K == pp.AUXK), r
        else:
            kind = operand(r.B, r.K)
            v = p.buffers[r.v]
            assert v is not None and (r.N == 1 if len(v) == 1 else r.N <= v[-1]) and r.A is None and r.ldo == r.K, r
            if r.kind == pp.PART:
                assert planned("tile_part") and W == 256
            else:  # the twin exactly where the tensor is stored as fragments; no vector kernel reads fp16 tiles
                assert kind == (pp.WG_F16_FRAG if r.kind == pp.VEC_FRAG else pp.WG_F32), r
                assert r.K in ((128, 256) if r.kind == pp.VEC_FRAG else VEC_K), r


def decisions_check(p, sched, L, use_cand, use_rgb):
    W2, top = L.W // 2, sched.trunk + sched.cand + sched.rgb
    to = lambda off, kinds: [r for r in top if r.dW == off and r.kind in kinds]
    vecs = (pp.VEC, pp.VEC_FRAG)
    # the density head rides on the final layer's launch, or has a launch of its own
    final = sched.trunk[-1 if p.ride else -2]
    assert final.dW == L.we and (final.ride is not None) == p.ride and len(to(L.wsig, vecs)) == int(not p.ride)
    assert all(r.ride is None for r in top if r is not final)
    # the 128-wide vector heads leave with the per-tile sums, or have launches of their own
    tile = p.partials == "tile"
    assert (sched.part is not None) == tile
    assert len(to(L.wcsig, vecs)) == int(use_cand and not tile) and len(to(L.wr2, vecs)) == int(use_rgb and not tile)
    if tile:
        assert [r is not None for r in sched.part] == [use_cand, use_rgb]
        assert all(r is None or r.kind == pp.PART for r in sched.part) and not any(r.kind == pp.PART for r in top)
    # the heads' first layers: one launch split by rows, or one each
    two = [r for r in top if r.n2]
    assert len(two) == int(p.joined)
    if p.joined:
        assert (two[0].n2, two[0].N, two[0].dW, two[0].dW2) == (W2, 2 * W2, L.wr1, L.wc1) and to(L.wc1, (pp.MAT,)) == []
        assert to(L.wr1, (pp.MAT,)) == two
    else:
        assert len(to(L.wc1, (pp.MAT,))) == int(use_cand) and len(to(L.wr1, (pp.MAT,))) == int(use_rgb)
    assert (bool(sched.cand), bool(sched.rgb)) == (use_cand, use_rgb)
    # exponent slots: one per tensor and one tensor per slot, in each of the two tables
    for side in ("A", "B"):
        slots = {(getattr(r, side), r.ea if side == "A" else r.eb) for r in top if r.kind == pp.MAT}
        assert len({t for t, _ in slots}) == len({e for _, e in slots}) == len(slots) and all(0 <= e < 16 for _, e in slots)
    assert all(r.ea is None and r.eb is None for r in records(sched) if r.kind != pp.MAT)


def test_every_schedule_writes_each_block_once():
    n, covered = 0, set()
    for fm, ws, bits, kind, (W, D, skip) in itertools.product(pp.MODES, ("f32", "f16", "f24"), itertools.product((0, 1), repeat=5),
                                                              PASSES, LAYOUTS):
        sw = dict(zip(BOOLS, bits), FIELD_MODE=fm, WGRAD_STORE=ws)
        if ws == "f24" and not sw["WGRAD_CHAIN"]:
            continue  # (raises: test_every_plan_is_one_description)
        L = pp.layout_offsets(W, D, skip)
        _, use_cand, use_rgb, _ = kind
        for R, S in SCHED_SHAPES:
            if fm == "f16" and not (W == 256 and S >= 32):
                continue
            p = pp.plan_pass(W, W // 2, D, R, S, *kind, True, **sw)  # (a pass without gradient has no backward to schedule)
            sched = pp.wgrad_schedule(p, L, skip, use_cand, use_rgb)
            assert sched is pp.wgrad_schedule(p, L, skip, use_cand, use_rgb)  # built once
            if (sched, L, use_cand, use_rgb) not in covered:  # (a property of the schedule alone)
                coverage_check(sched, L, use_cand, use_rgb)
                pitches_check(sched, L)
                covered.add((sched, L, use_cand, use_rgb))
            operands_check(p, sched, W)
            decisions_check(p, sched, L, use_cand, use_rgb)
            n += 1
    assert n == 11200
