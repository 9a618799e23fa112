"""A precondition of tests/test_hip_field_edges.py that needs no GPU: on every case that test adds, the fp32 restatement of the
field pass agrees with the fp64 one within HALF of each gate the stage comparison applies to the kernels -- activations, gradients
and the share of differing ReLU decisions.  The inputs are then conditioned well enough (no pre-activation sits on zero, no sum is
left over from cancelling terms) that a kernel which misses a gate against fp64 has itself to answer for it.  A draw that fails
here gets another seed or scale, never another gate."""
import pytest
import torch

import field_cases as fc
from golden_util import rel_err

CASES = fc.SYNTH_256 + [fc.SYNTH_SMALLEST] + fc.SYNTH_64 + fc.NOFEAT


@pytest.mark.parametrize("key", CASES, ids=fc.label)
def test_fp32_restatement_is_within_half_of_every_gate_of_the_fp64_one(key):
    s = fc.load(key)
    M = s["z"].numel()
    a32, g32, m32 = fc.ref_stages(fc.reference(s, torch.float32), s)
    a64, g64, m64 = fc.ref_stages(fc.reference(s, torch.float64), s)
    assert list(a32) == list(a64) and list(g32) == list(g64) and list(m32) == list(m64)
    bad = {}
    worst = {"x0": 0.0, "act": 0.0, "grad": 0.0}
    for k, (t, kind) in a64.items():
        e = rel_err(a32[k][0].detach(), t.detach())
        worst[kind] = max(worst[kind], e)
        if not e <= 0.5 * (fc.TOL_X0 if kind == "x0" else fc.TOL_ACT):
            bad[k] = e
    for k, t in g64.items():
        assert float(t.abs().max()) > 0 or s.get("dead") is not None, k  # (a gradient that is all zero would gate nothing)
        e = rel_err(g32[k], t)
        worst["grad"] = max(worst["grad"], e)
        if not e <= 0.5 * fc.TOL_GRAD:
            bad[k] = e
    share = row = 0.0
    for k, (t, by_zero) in m64.items():
        sh, rw = fc.mask_diff(m32[k][0], t, M, by_zero)
        share, row = max(share, sh), max(row, rw)
        if not (sh <= 0.5 * fc.MASK_FLIP and rw <= 0.5 * fc.MASK_FLIP_ROW):
            bad["mask_" + k] = (sh, rw)
    print(f"[fp32 vs fp64] {fc.label(key)}: x0 {worst['x0']:.1e} (gate {fc.TOL_X0:g}), activations {worst['act']:.1e} "
          f"({fc.TOL_ACT:g}), gradients {worst['grad']:.1e} ({fc.TOL_GRAD:g}), mask share {share:.1e} ({fc.MASK_FLIP:g}), "
          f"worst row {row:.1e} ({fc.MASK_FLIP_ROW:.1e})")
    assert not bad, bad


def test_the_dead_ray_is_dead_and_the_others_are_not():
    """The case with a dead ray: every trunk activation of that ray is zero in every layer (so whole 64-row tiles inside it are
    zero tiles), every other ray has live units in every layer."""
    key = next(k for k in fc.SYNTH_256 if k.dead is not None)
    s = fc.load(key)
    f = fc.reference(s, torch.float64).f
    ray = torch.arange(key.R * key.S) // key.S
    rows = ray == key.dead
    assert (int(rows.nonzero()[0]) + 63) // 64 * 64 + 128 <= int(rows.nonzero()[-1]) + 1  # two whole tiles inside the ray
    for l in range(key.D):
        h = f["h"][l].detach()
        assert float(h[rows].abs().max()) == 0.0, l
        assert float(f["pre_h"][l].grad[rows].abs().max()) == 0.0, l
        for r in range(key.R):
            if r != key.dead:
                live = float((h[ray == r] > 0).float().mean())
                assert live > 0.05, (l, r, live)


def test_the_cases_cover_what_they_claim():
    syn = fc.SYNTH_256 + fc.SYNTH_64
    ragged = [c for c in syn if (c.R * c.S) % 64]
    for v in ((0, True, False), (1, True, True), (2, False, True), (3, False, False), (3, False, True)):
        assert any((c.mode, c.use_cand, c.use_rgb) == v for c in ragged), v
    assert {(c.R, c.S) for c in fc.SYNTH_256} == {(1, 64), (7, 40), (5, 33), (3, 200), (2, 257), (9, 32)}
    assert {(c.R, c.S) for c in fc.SYNTH_64} == {(5, 33), (7, 40)}
    s = fc.load(next(c for c in syn if c.frac))
    assert 0 < s["wk_xyz"][4] < 1 and not any(s["wk_xyz"][5:]) and 0 < s["wk_dir"][1] < 1 and not any(s["wk_dir"][2:])
    s = fc.load(fc.SYNTH_256[1])  # per-ray side inputs over five decades
    assert float(s["c_rows"].abs().amax(1).max() / s["c_rows"].abs().amax(1).min()) > 1e4


@pytest.mark.parametrize("key", fc.SYNTH_256 + fc.NOFEAT[1:], ids=fc.label)
def test_fp16_operands_alone_leave_the_draw_inside_the_f16_gates(key):
    """The "f16" mode is held to its stated relaxed gates, and those are wide because a ReLU may decide the other way under 11-bit
    operands; on a few hundred samples one such flip in a sample that carries much of the gradient can fill the gate by itself.
    The fp64 restatement with both operands of every matrix product rounded to fp16 (a floating exponent per element: never
    coarser than the kernels' shared exponent per tile) must therefore meet the f16 gates against the plain fp64 one -- a draw
    on which arithmetic as good as the mode can be already misses them says nothing about the kernels, and gets another seed."""
    s = fc.load(key)
    a64, g64, _ = fc.ref_stages(fc.reference(s, torch.float64), s)
    aq, gq, _ = fc.ref_stages(fc.restate(s, torch.float64, quant=fc.round16), s)
    bad, worst = {}, [0.0, 0.0, 0.0]
    for k, (t, kind) in a64.items():
        e = rel_err(aq[k][0].detach(), t.detach())
        worst[0] = max(worst[0], e)
        if not e < fc.TOL_ACT_F16:
            bad[k] = e
    for k, t in g64.items():
        d, r = (gq[k] - t).reshape(-1), t.reshape(-1)
        l2, mx = float(d.norm() / r.norm().clamp_min(1e-30)), rel_err(gq[k], t)
        worst[1:] = max(worst[1], l2), max(worst[2], mx)
        if not (l2 < fc.TOL_GRAD_F16 and mx < fc.TOL_GRAD_F16_MAX):
            bad[k] = (l2, mx)
    print(f"[fp16 operands vs fp64] {fc.label(key)}: activations {worst[0]:.1e} (gate {fc.TOL_ACT_F16:g}), gradients L2 {worst[1]:.1e} "
          f"({fc.TOL_GRAD_F16:g}), single entry {worst[2]:.2f} ({fc.TOL_GRAD_F16_MAX:g})")
    assert not bad, bad


# ------------------------------------------------------------------------------------------ preconditions of tests/test_hip_field_plans.py
def _requested(key, variant, dtype, **kw):
    s = fc.load(key)
    ups = fc.variant_ups(variant, s)
    ref = fc.restate(s, dtype, ups=ups, **kw) if kw else fc.reference(s, dtype, ups)
    return s, ups, ref, fc.ref_grads(ref, s, fc.variant_leaves(variant, s))


@pytest.mark.parametrize("key,variant", fc.BACKWARD_PAIRS, ids=lambda v: v if isinstance(v, str) else fc.label(v))
def test_fp32_restatement_of_every_partial_backward_is_within_half_of_the_gates_of_the_fp64_one(key, variant):
    """Every (case, variant) pair of the GPU file: the gradients the variant requests, fp32 restatement against fp64, within half
    of TOL_GRAD (and, where P is requested, the trunk's gradient masks within half of the mask limits).  Every requested gradient
    the variant's upstreams reach is non-zero (the dead-ray case keeps its exemption); one they do not reach is exactly zero in
    both, which holds the kernels to an exact zero."""
    s, ups, r64, g64 = _requested(key, variant, torch.float64)
    _, _, r32, g32 = _requested(key, variant, torch.float32)
    assert list(g32) == list(g64) and g64
    M = s["z"].numel()
    none, bad, worst = fc.unreached(s, ups), {}, 0.0
    for k, t in g64.items():
        if k in none:
            assert float(t.abs().max()) == 0.0 and float(g32[k].abs().max()) == 0.0, k
            continue
        assert float(t.abs().max()) > 0 or s.get("dead") is not None, k
        e = rel_err(g32[k], t)
        worst = max(worst, e)
        if not e <= 0.5 * fc.TOL_GRAD:
            bad[k] = e
    share = row = 0.0
    if "P" in fc.variant_leaves(variant, s):
        for l in range(s["model"].packer.D):
            sh, rw = fc.mask_diff(r32.f["pre_h"][l].grad, r64.f["pre_h"][l].grad, M, True)
            share, row = max(share, sh), max(row, rw)
            if not (sh <= 0.5 * fc.MASK_FLIP and rw <= 0.5 * fc.MASK_FLIP_ROW):
                bad[f"mask_gz_h{l}"] = (sh, rw)
    print(f"[fp32 vs fp64] {fc.label(key)} {variant}: gradients {worst:.1e} (gate {fc.TOL_GRAD:g}), mask share {share:.1e} "
          f"({fc.MASK_FLIP:g}), worst row {row:.1e} ({fc.MASK_FLIP_ROW:.1e}); unreached: {sorted(none & set(g64))}")
    assert not bad, bad


F16_PAIRS = [(k, v) for k, v in fc.BACKWARD_PAIRS if "f16" in fc.modes_of(k)]


@pytest.mark.parametrize("key,variant", F16_PAIRS, ids=lambda v: v if isinstance(v, str) else fc.label(v))
def test_fp16_operands_alone_leave_every_partial_backward_inside_the_f16_gates(key, variant):
    """test_fp16_operands_alone_leave_the_draw_inside_the_f16_gates for the pairs the GPU file runs in the "f16" mode: a subset of
    upstreams or leaves changes which samples carry the gradient, so each pair is its own draw."""
    s, ups, _, g64 = _requested(key, variant, torch.float64)
    _, _, _, gq = _requested(key, variant, torch.float64, quant=fc.round16)
    bad, worst = {}, [0.0, 0.0]
    for k, t in g64.items():
        d, r = (gq[k] - t).reshape(-1), t.reshape(-1)
        l2, mx = float(d.norm() / r.norm().clamp_min(1e-30)), rel_err(gq[k], t)
        worst = [max(worst[0], l2), max(worst[1], mx)]
        if not (l2 < fc.TOL_GRAD_F16 and mx < fc.TOL_GRAD_F16_MAX):
            bad[k] = (l2, mx)
    print(f"[fp16 operands vs fp64] {fc.label(key)} {variant}: gradients L2 {worst[0]:.1e} ({fc.TOL_GRAD_F16:g}), "
          f"single entry {worst[1]:.2f} ({fc.TOL_GRAD_F16_MAX:g})")
    assert not bad, bad


@pytest.mark.parametrize("key", fc.DENSITY_ONLY, ids=fc.label)
def test_density_only_restatement_in_fp32_is_within_half_of_every_gate_of_the_fp64_one(key):
    """The density-only passes: what the forward-only comparison reads off the restatement (x0, sigma_s, s_depth, w_s)."""
    s = fc.load(key)
    assert s["c_rows"] is None and s["a_rows"] is None and (s["mode"], s["use_cand"], s["use_rgb"]) == (2, False, False)
    a32, a64 = fc.ref_stages(fc.reference(s, torch.float32), s)[0], fc.ref_stages(fc.reference(s, torch.float64), s)[0]
    assert {k for k in a64 if k.startswith("out_")} == {"out_s_depth", "out_w_s"}
    for k in ("x0", "sigma_s", "out_s_depth", "out_w_s"):
        e = rel_err(a32[k][0].detach(), a64[k][0].detach())
        print(f"[fp32 vs fp64] {fc.label(key)} {k}: {e:.1e}")
        assert float(a64[k][0].abs().max()) > 0 and e <= 0.5 * (fc.TOL_X0 if k == "x0" else fc.TOL_ACT), (k, e)
    with_rows = fc.load(key._replace(use_rgb=True, bare=False))  # (the rows do not reach the density)
    assert torch.equal(fc.reference(with_rows, torch.float64).out["w_s"], a64["out_w_s"][0])


def test_the_plan_cases_cover_what_they_claim():
    ragged = lambda k: isinstance(k, fc.Synth) and (k.R * k.S) % 64 != 0
    for v in fc.VARIANTS:
        assert any(ragged(k) for k, w in fc.BACKWARD_PAIRS if w == v), v
    dead = next(k for k in fc.SYNTH_256 if k.dead is not None)
    assert {v for k, v in fc.BACKWARD_PAIRS if k == dead} & {"frozen_appearance", "frozen_pose", "frozen_candidate"}
    assert {(k.W, k.R, k.S) for k in fc.DENSITY_ONLY} == {(256, 7, 40), (256, 3, 200), (256, 2, 257), (64, 5, 33)}
    assert any(k.S % 32 for k in fc.DENSITY_ONLY) and any(k.dead is not None for k in fc.DENSITY_ONLY)
    for k in fc.PLAN_CASES:  # the table's columns, per case: leaves and upstreams exist where a variant applies
        s = fc.load(k)
        assert fc.traits(k) == (s["mode"], s["use_cand"], s["use_rgb"]), k
        outs = set(fc.reference(s, torch.float32).out)
        for v in fc.variants_of(k):
            ups = fc.variant_ups(v, s)
            assert fc.variant_leaves(v, s) and (ups is None or set(ups) <= outs), (k, v)
    # no pair is run in a mode that would refuse it, no 256-wide pair misses a mode
    assert all(m == ["f16x3"] for m in map(fc.modes_of, fc.SYNTH_64 + fc.NOFEAT[:1] + fc.DENSITY_ONLY[3:]))
    assert all(fc.modes_of(k) == fc.MODES for k in fc.SYNTH_256 + fc.NOFEAT[1:] + fc.DENSITY_ONLY[:3])
    assert fc.modes_of(fc.SYNTH_SMALLEST) == ["f16x3", "f32"]


def test_the_forward_only_plans_differ_from_the_training_plans():
    """Host arithmetic only (pass_plan.plan_pass under the default switches): without `train` nothing the backward pass reads is
    planned in any mode, and in the "f16" mode's register-resident kernels e (and g2) change form on at least one case used --
    the GPU test then runs another store set and another compositing input than check_field_pass does."""
    from upnerf_amd.pass_plan import plan_pass
    sw = dict(WGRAD_STORE="f32", FIELD_RR=1, TILE_PARTIALS=1, WGRAD_CHAIN=1, JOIN_HEADS=1, VEC_RIDE=1)
    differ = []
    for key, fm in fc.FORWARD_RUNS + fc.DENSITY_RUNS:
        s = fc.load(key)
        pk, (R, S) = s["model"].packer, s["z"].shape
        plans = [plan_pass(pk.W, pk.W2, pk.D, R, S, s["mode"], s["use_cand"], s["use_rgb"], bool(s.get("rgb_joint")), train,
                           FIELD_MODE=fm, **sw) for train in (False, True)]
        ev, tr = (p.buffers for p in plans)
        gone = [k for k in ev if ev[k] is None and tr[k] is not None]
        for k in ("hmask", "mx32", "d_sigma_s", "dpre_s"):
            assert k in gone, (key, fm, k)
        assert "h" in gone or "h16" in gone, (key, fm)
        assert any(k in gone for k in ("gz_h", "gz16")), (key, fm)
        for k in ("h", "h16", "hmask", "mx32", "gz_e", "gz_h", "gz16", "gz_rg", "gz_rg16", "gz_g1", "gz_g2", "gz_g2_16", "gz_r1",
                  "d_sigma_s", "d_sigma_c", "d_rgb", "dpre_s", "dpre_c", "dpre_rgb", "tile_part", "ray_part", "g1", "g1_16", "r1", "r1_16"):
            assert ev[k] is None, (key, fm, k)
        if fm == "f16" and plans[0].e_frag != plans[1].e_frag:
            differ.append(fc.label(key))
        if fm != "f16":
            assert not plans[0].e_frag and not plans[1].e_frag
    print("[plans] e changes form between the training and the forward-only plan of the f16 mode on:", differ)
    assert differ
