"""The plan of a field pass (upnerf_amd/pass_plan.py) over the full product of switches, pass kinds and shapes: every logical
tensor in exactly one storage form, nothing planned that the pass does not need, whole tiles behind the register-resident
kernels, operand kinds that follow the storage.  Host arithmetic only: no library, no device."""
import itertools

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
