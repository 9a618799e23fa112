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
