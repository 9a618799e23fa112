"""The small per-ray kernels -- fused loss + depth prior (upnerf_loss_fwd / _bwd), pose refinement + ray generation
(upnerf_pose_rays_fwd / _bwd) and inverse-CDF resampling + sort (upnerf_sample_pdf, upnerf_resample_sort, upnerf_sort_rows) --
against fp64 references at the shapes, clamp points and limits that tests/test_hip_kernels.py never reaches.

Gate of the element-wise outputs and gradients (parts 1 and 2), computed here on the CPU and never from a kernel's output:

    |kernel - fp64|  <=  4 * e32 + 2^-22 * scale,      e32 = |oracle in fp32 - oracle in fp64| on the same inputs,

taken per element for the loss gradients and per row (max over the row's entries) for the pose kernels; `scale` is the magnitude
of that element's / row's own fp64 value, not the tensor's maximum.  The factor 4 covers an equally valid operation order (Horner
in q = |w|^2 instead of a series in theta, analytic backward instead of autograd), the floor the rows where the fp32 oracle
happens to be exact.  Where the limit is 0 (fp64 value 0, fp32 oracle exact: clamped rays, sign 0, t_weight == 1) the kernel's
value has to be exactly 0.  No element is left out of any comparison: the inputs keep a margin of 1e-3 from every branch point
(asserted on the CPU at the top of each test), the planted rays sit ON the branch points with exactly representable values
(near = 0.125, far = 4, scale row 0), so fp32 and fp64 take the same branch everywhere.

Loss terms: 2e-6 relative to the term itself (l_beta: to the same sum over |log beta|), without a floor.

Resampling: the existing well-conditioned gate max |dz| < 5e-6 against orc.sample_pdf in fp32 (depths in [0.5, 4.5]: a range of
O(1)), bit equality for the fused kernel against the per-piece sequence and for the sort against torch.sort.

Two floors carry a derivation instead of the plain |fp64 value| (both computed from the inputs in fp64, beside loss_ref and in
prior_chain_scales): a gradient that is a SUM of contributions of opposite sign (d t_beta = d l_rgb_f + d l_beta,
d depth_scale_rows = d l_depth_c + d l_depth_f) is rounded at the size of its summands, so its scale is their summed magnitudes;
and the depth prior is a chain of a dozen fp32 operations (expf, p = a + shift with cancellation, 1 / p^2, ...) whose first-order
rounding bound, written out there, replaces the four roundings that 2^-22 stands for.  Every other output is held to the plain
gate, and a depth target that is clamped has to equal near resp. far exactly.

Worst measured ratio kernel error / (4 * e32 + floor) on an MI355X (gate: <= 1):
    part 1, loss gradients and depth targets   0.71  (d s_rgb_fine at R = 4097; d t_beta 0.66, d feat 0.50, depth targets 0.42,
                                                      d depth_scale_rows 0.26; loss terms: 0.14 of their 2e-6)
    part 2, rays_o / rays_d / d se3            0.72  (d se3 at R = 129)
    part 3, sample_pdf max |dz| / 5e-6         0.33  (S = 1024; S = 3 and S = 4 are bit-exact)
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from golden_util import orc

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22
EINVAL = -1  # UPNERF_EINVAL (include/upnerf_hip.h)
NEAR, FAR = 0.125, 4.0
DEPTH_MULT, ALPHA_REG = 1e-3, 0.75
TERMS = ("l_depth_c", "l_feat_c", "l_rgb_c", "l_depth_f", "l_feat_f", "l_rgb_f", "l_beta", "l_alpha")
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib, camera, losses
    return dict(lib=_lib, camera=camera, losses=losses)


def cpu(t):
    return t.detach().cpu()


def _u(g, shape, lo=0.0, hi=1.0):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def gate_ratio(got, ref64, ref32, rows=False, scale=None):
    """max over elements (rows=True: over rows, error / e32 / scale each the maximum over the row's entries) of
    |got - ref64| / (4 |ref32 - ref64| + 2^-22 scale), scale = |ref64| unless given; a limit of 0 asks for an error of exactly 0
    (ratio inf otherwise).  A NaN anywhere makes the ratio NaN, which fails `<= 1`."""
    got, ref64, ref32 = cpu(got).double(), ref64.detach().double(), ref32.detach().double()
    assert got.shape == ref64.shape == ref32.shape
    err, e32, scale = (got - ref64).abs(), (ref32 - ref64).abs(), ref64.abs() if scale is None else scale.detach().double()
    assert scale.shape == ref64.shape and bool((scale >= ref64.abs() * (1 - 1e-12)).all())
    if rows:
        n = ref64.shape[0]
        err, e32, scale = (x.reshape(n, -1).max(1)[0] for x in (err, e32, scale))
    lim = 4 * e32 + FLOOR * scale
    ratio = torch.where(lim > 0, err / lim.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    if torch.isnan(err).any():
        return NAN
    return float(ratio.max()) if ratio.numel() else 0.0


# ====================================================================================== 1. loss and depth prior
# planted rays, in this order behind the random ones (a set of R rays holds the first min(R, 9) of them as its last rays);
# unnamed fields: inv = 1, row = (0, 0) -> depth target 1, s_depth_coarse = 1.5, s_depth_fine = 0.5, the rest random
PLANTED = (
    ("p_at_far", dict(inv=0.25, s_c=1.0, s_f=3.0)),                  # p == 1/far: not clamped, gradient flows
    ("p_below_far", dict(inv=0.25, shift=-0.125, s_c=1.0, s_f=3.0)),  # clamped at 1/far: no gradient to the row
    ("d_at_near", dict(inv=8.0, s_c=1.0, s_f=3.0)),                  # d == near: not clamped
    ("d_below_near", dict(inv=16.0, s_c=1.0, s_f=3.0)),              # clamped at near: no gradient
    ("sign0", dict(inv=0.5, s_c=2.0, s_f=2.0)),                      # s_depth == depth target: sign 0 on both sides
    ("tw1", dict(tw=1.0)),
    ("tw0", dict(tw=0.0)),
    ("beta_min", dict(beta=0.03, rgb_f=(0.9921875, 0.0078125, 1.0), rgb=(0.0078125, 0.9921875, 0.0))),
    ("alpha0", dict(alpha=0.0)),
)


class LossInputs:
    pass


def loss_inputs(R, F, seed, fine=True, has_tw=True, encode_feat=True):
    """CPU fp32 inputs of UPNeRFLoss for R rays: random rays pushed 2e-3 away from every branch point, then the planted rays."""
    g = torch.Generator().manual_seed(seed)
    typs = ("coarse", "fine") if fine else ("coarse",)
    if not encode_feat:
        assert F == 3
    res = {}
    for typ in typs:
        res[f"s_depth_{typ}"] = _u(g, (R,), 0.2, 4.0)
        res[("feat_" if encode_feat else "c_rgb_") + typ] = _u(g, (R, F), -1.0, 1.0)
        if has_tw:
            res[f"t_weight_{typ}"] = _u(g, (R,))
        res[f"s_rgb_{typ}"] = _u(g, (R, 3))
    if fine:
        res["t_beta"], res["t_alpha"] = _u(g, (R, 1), 0.03, 1.0), _u(g, (R, 1))
    rgb = _u(g, (R, 3))
    feat = _u(g, (R, F), -1.0, 1.0) if encode_feat else rgb
    # prior depths log-uniform in [0.06, 8]: about one ray in seven clamps at near, one in seven at far
    inv = torch.exp(-_u(g, (R,), math.log(0.06), math.log(8.0)))
    rows = _u(g, (R, 2), -0.3, 0.3)

    def prior64():
        p = inv.double() * torch.exp(rows[:, 0].double()) + rows[:, 1].double()
        return p, torch.clamp(1.0 / torch.clamp(p, min=1.0 / FAR), min=NEAR)

    p, _ = prior64()
    rows[:, 1] += torch.where((p - 1.0 / FAR).abs() < 2e-3, 0.01, 0.0).float()
    p, _ = prior64()
    rows[:, 1] -= torch.where((1.0 / torch.clamp(p, min=1.0 / FAR) - NEAR).abs() < 2e-3, 0.5, 0.0).float()
    _, d = prior64()
    for typ in typs:
        s = res[f"s_depth_{typ}"]
        s.copy_(torch.where((s.double() - d).abs() < 2e-3, d + 0.01, s.double()).float())
    planted = {}
    K = min(R, len(PLANTED))
    for j, (name, v) in enumerate(PLANTED[:K]):
        r = R - K + j
        planted[name] = r
        inv[r] = v.get("inv", 1.0)
        rows[r, 0], rows[r, 1] = 0.0, v.get("shift", 0.0)
        res["s_depth_coarse"][r] = v.get("s_c", 1.5)
        if fine:
            res["s_depth_fine"][r] = v.get("s_f", 0.5)
        if "tw" in v and has_tw:
            for typ in typs:
                res[f"t_weight_{typ}"][r] = v["tw"]
        if "rgb" in v:
            rgb[r] = torch.tensor(v["rgb"])
            if fine:
                res["s_rgb_fine"][r] = torch.tensor(v["rgb_f"])
        if fine and "beta" in v:
            res["t_beta"][r] = v["beta"]
        if fine and "alpha" in v:
            res["t_alpha"][r] = v["alpha"]
    o = LossInputs()
    o.R, o.F, o.fine, o.has_tw, o.encode_feat, o.typs = R, F, fine, has_tw, encode_feat, typs
    o.res, o.rgb, o.feat, o.inv, o.rows, o.planted = res, rgb, feat, inv, rows, planted
    o.depth = orc.depth_prior(rows, inv, NEAR, FAR)  # the fp32 depth targets handed to UPNeRFLoss.forward
    return o


def check_loss_margins(o):
    """Every ray is 1e-3 away from each branch point of the depth prior and of |s_depth - depth|, except the planted rays that
    sit exactly on one; there fp32 and fp64 compute the same exact values."""
    p = o.inv.double() * torch.exp(o.rows[:, 0].double()) + o.rows[:, 1].double()
    d_raw = 1.0 / torch.clamp(p, min=1.0 / FAR)
    d = torch.clamp(d_raw, min=NEAR)
    on = lambda *names: [o.planted[n] for n in names if n in o.planted]
    free = torch.ones(o.R, dtype=torch.bool)
    free[on("p_at_far")] = False
    assert bool(((p - 1.0 / FAR).abs() >= 1e-3)[free].all()) and bool((p[on("p_at_far")] == 1.0 / FAR).all())
    free[:] = True
    free[on("d_at_near")] = False
    assert bool(((d_raw - NEAR).abs() >= 1e-3)[free].all()) and bool((d_raw[on("d_at_near")] == NEAR).all())
    free[:] = True
    free[on("sign0")] = False
    for typ in o.typs:
        s = o.res[f"s_depth_{typ}"].double()
        assert bool(((s - d).abs() >= 1e-3)[free].all()) and bool((s[on("sign0")] == d[on("sign0")]).all())
        assert bool(((s - o.depth.double()).abs() >= 1e-3)[free].all())
    for r in o.planted.values():  # exactly representable: the fp32 oracle's depth target IS the fp64 one
        assert float(o.depth[r]) == float(d[r]) and float(o.rows[r, 0]) == 0.0
    assert float((o.depth.double() - d).abs().max()) < 1e-5
    if o.fine:
        assert float(o.res["t_beta"].min()) >= float(np.float32(0.03))  # (both precisions read the same fp32 beta)


def loss_ref(o, m, dtype, direct, wts, use_total):
    """The oracle in `dtype` with autograd: terms, {input: gradient}, d depth_scale_rows, depth targets."""
    r = {k: v.to(dtype).clone().requires_grad_(not k.startswith("t_weight")) for k, v in o.res.items()}
    rw = o.rows.to(dtype).clone().requires_grad_(True)
    depth = o.depth.to(dtype) if direct else orc.depth_prior(rw, o.inv.to(dtype), NEAR, FAR)
    out = orc.upnerf_loss(r, o.rgb.to(dtype), o.feat.to(dtype), depth, m, DEPTH_MULT, ALPHA_REG, o.fine, o.encode_feat)
    # The two gradients that are sums of contributions of opposite sign (fp64 only; see the gate in the tests): their magnitudes
    # added up, per element.  d depth_scale_rows = d l_depth_c + d l_depth_f (the signs of s_depth - depth differ on about half
    # the rays), d t_beta = d l_rgb_f (negative) + d l_beta (positive).
    cond = {}
    if dtype == torch.float64:
        for name, x, parts in (("rows", rw, ("l_depth_c", "l_depth_f")), ("t_beta", r.get("t_beta"), ("l_rgb_f", "l_beta"))):
            gs = [torch.autograd.grad(out[k] * (1.0 if use_total else wts[k]), x, retain_graph=True, allow_unused=True)[0]
                  for k in parts if k in out and x is not None]
            gs = [g.abs() for g in gs if g is not None]
            if gs:
                cond[name] = sum(gs)
    (sum(out.values()) if use_total else sum(out[k] * wts[k] for k in out)).backward()
    return {k: v.detach() for k, v in out.items()}, {k: v.grad for k, v in r.items()}, rw.grad, depth.detach(), cond


def prior_chain_scales(o, d64, cond_rows):
    """Scales (to be multiplied by the 2^-22 floor) of the two outputs behind the depth prior's chain of fp32 operations, where
    the plain floor of 2^-22 = four roundings is below what ANY fp32 evaluation of the chain can promise.  With u = 2^-24 and
    first-order error propagation (expf is good to 1 ulp = 2u):
        a = inv * expf(scale)           relative error <= 3u
        p = a + shift                   relative error eps_p <= (3 |a| + |p|) u / |p|   (>= 4u; more where a and shift cancel)
        depth = 1 / p                   relative error <= eps_p + u
        dd = -1 / (p * p)               relative error <= 2 eps_p + 2u
        dd * inv * expf(scale)          relative error <= 2 eps_p + 6u
        gd = -(+-w_c +- w_f)            absolute error <= 8u (|w_c| + |w_f|): w = (1 - t_weight) * (depth_mult * (1 - m) / R) * g_term
        gd * (dd * inv * expf(scale))   absolute error <= (2 eps_p + 15u) * (|w_c| + |w_f|) |dd inv expf(scale)|
    and (|w_c| + |w_f|) |dd inv expf(scale)| is `cond_rows`, the summed magnitudes of the two terms' gradients (loss_ref).  Clamped
    rays: cond_rows = 0, so the limit of d depth_scale_rows there is 0; their depth target is the clamp value itself, which the
    tests hold to exact equality beside this gate (clamped_rays)."""
    u = 2.0 ** -24
    a = o.inv.double() * torch.exp(o.rows[:, 0].double())
    p = a + o.rows[:, 1].double()
    eps_p = (3 * a.abs() + p.abs()) * u / p.abs().clamp_min(1.0 / FAR)
    s_depth = d64.abs() * torch.clamp((eps_p + u) / FLOOR, min=1.0)
    s_rows = None if cond_rows is None else cond_rows * ((2 * eps_p + 15 * u) / FLOOR)[:, None]
    return s_depth, s_rows


def clamped_rays(o):
    """The rays whose depth target is a clamp value (in fp64; check_loss_margins keeps every other ray 1e-3 from the clamps)."""
    p = o.inv.double() * torch.exp(o.rows[:, 0].double()) + o.rows[:, 1].double()
    return (p < 1.0 / FAR) | (1.0 / torch.clamp(p, min=1.0 / FAR) < NEAR)


def term_scales(o, out64, m):
    """What each term's 2e-6 is relative to: the term itself (a sum of non-negative numbers); l_beta: the same mean over |log beta|."""
    sc = {k: abs(float(v)) for k, v in out64.items()}
    if "l_beta" in sc:
        sc["l_beta"] = float(torch.log(o.res["t_beta"].double()).abs().mean() * m)
    return sc


def term_weights(names, seed=80):
    g = torch.Generator().manual_seed(seed)
    w = _u(g, (8,), 0.5, 1.5)
    return {k: float(w[TERMS.index(k.replace("l_c_rgb", "l_feat"))]) for k in names}


def expected_names(m, fine, encode_feat=True):
    fc, ff = ("l_feat_c", "l_feat_f") if encode_feat else ("l_c_rgb_c", "l_c_rgb_f")
    on = {"l_depth_c": m < 1, fc: m < 1, "l_rgb_c": m > 0, "l_depth_f": fine and m < 1, ff: fine and m < 1,
          "l_rgb_f": fine and m > 0, "l_beta": fine and m > 0, "l_alpha": fine and m > 0}
    return [k for k in ("l_depth_c", fc, "l_rgb_c", "l_depth_f", ff, "l_rgb_f", "l_beta", "l_alpha") if on[k]]


def check_loss_planted(o, m, g64, rw64, direct):
    """The reference itself does on the planted rays what the table of the issue says (an input error otherwise)."""
    P = o.planted
    if m < 1 and not direct:
        if "p_at_far" in P:
            assert float(rw64[P["p_at_far"]].abs().min()) > 0  # live: the gradient flows to scale and shift
        for n in ("p_below_far", "d_below_near", "sign0"):
            if n in P:
                assert float(rw64[P[n]].abs().max()) == 0.0
        if "d_at_near" in P:
            assert float(rw64[P["d_at_near"]].abs().min()) > 0
    if m < 1:
        for typ in o.typs:
            g = g64[f"s_depth_{typ}"]
            if "sign0" in P:
                assert float(g[P["sign0"]]) == 0.0
            if "tw1" in P and o.has_tw:
                assert float(g[P["tw1"]]) == 0.0
            if "tw0" in P:
                assert float(g[P["tw0"]]) != 0.0


LOSS_CASES = [
    # R, F, m, fine, has_tw, encode_feat: every R in every phase, every F in the two phases that read the features
    (1, 8, 0, True, True, True), (63, 384, 0, True, False, True), (64, 6, 0, False, True, True), (65, 64, 0, True, True, True),
    (257, 8, 0, False, False, True), (4097, 384, 0, True, True, True), (4097, 6, 0, True, True, True),
    (1, 6, 0.37, True, True, True), (63, 64, 0.37, False, True, True), (64, 384, 0.37, True, False, True),
    (65, 8, 0.37, True, True, True), (257, 6, 0.37, True, False, True), (4097, 384, 0.37, True, True, True),
    (1, 384, 0.37, True, True, True), (65, 3, 0.37, True, True, False),
    (1, 8, 1, True, True, True), (63, 8, 1, False, True, True), (64, 8, 1, True, True, True), (65, 8, 1, True, False, True),
    (257, 8, 1, True, True, True), (4097, 8, 1, False, False, True),
]


@pytest.mark.parametrize("R,F,m,fine,has_tw,encode_feat", LOSS_CASES)
def test_loss_terms_and_gradients_match_fp64_per_element(hip, R, F, m, fine, has_tw, encode_feat):
    """UPNeRFLoss.forward_with_prior and .forward, gradients through the term dict and (prior form) through total() alone."""
    o = loss_inputs(R, F, 1000 + R + F, fine, has_tw, encode_feat)
    check_loss_margins(o)
    names = expected_names(m, fine, encode_feat)
    wts = term_weights(names)
    for direct, use_total in ((False, False), (True, False), (False, True)):
        t64, g64, rw64, d64, cond = loss_ref(o, m, torch.float64, direct, wts, use_total)
        t32, g32, rw32, d32, _ = loss_ref(o, m, torch.float32, direct, wts, use_total)
        assert list(t64) == names
        check_loss_planted(o, m, g64, rw64, direct)
        r = {k: v.cuda().requires_grad_(not k.startswith("t_weight")) for k, v in o.res.items()}
        rw = o.rows.cuda().requires_grad_(True)
        lf = hip["losses"].UPNeRFLoss(depth_mult=DEPTH_MULT, alpha_reg=ALPHA_REG, encode_feat=encode_feat, fine=fine, near=NEAR, far=FAR)
        if direct:
            out = lf(r, o.rgb.cuda(), o.feat.cuda(), o.depth.cuda(), m)
        else:
            out, depth = lf.forward_with_prior(r, o.rgb.cuda(), o.feat.cuda(), o.inv.cuda(), rw, m)
            ratio = gate_ratio(depth, d64, d32, scale=prior_chain_scales(o, d64, None)[0])
            assert ratio <= 1, ("depth targets", ratio)
            cl = clamped_rays(o)  # near and far are powers of two: the clamp value is the same number in every precision
            assert torch.equal(cpu(depth)[cl].double(), d64[cl])
        assert list(out) == names
        sc = term_scales(o, t64, m)
        for k in names:
            e = abs(float(out[k].detach()) - float(t64[k]))
            assert e <= 2e-6 * sc[k], (k, float(out[k]), float(t64[k]))
        (lf.total() if use_total else sum(out[k] * wts[k] for k in names)).backward()
        for k in r:
            if g64[k] is None:
                assert r[k].grad is None or float(r[k].grad.abs().max()) == 0.0, k
                continue
            ratio = gate_ratio(r[k].grad, g64[k], g32[k], scale=cond.get(k))  # (t_beta: the summed magnitudes, loss_ref)
            assert ratio <= 1, (k, ratio)
        if direct or rw64 is None:  # (m == 1: no term reads the depth target)
            assert rw.grad is None or float(rw.grad.abs().max()) == 0.0
        else:
            ratio = gate_ratio(rw.grad, rw64, rw32, scale=prior_chain_scales(o, d64, cond["rows"])[1])
            assert ratio <= 1, ("depth_scale_rows", ratio)
            for n in ("p_below_far", "d_below_near", "sign0"):
                if n in o.planted:
                    assert float(rw.grad[o.planted[n]].abs().max()) == 0.0, n


def test_loss_terms_of_the_two_stage_reduction_at_the_workload_length(hip):
    R, F, m = 8192, 384, 0.37
    o = loss_inputs(R, F, 8192)
    check_loss_margins(o)
    names = expected_names(m, True)
    t64 = loss_ref(o, m, torch.float64, False, term_weights(names), True)[0]
    lf = hip["losses"].UPNeRFLoss(depth_mult=DEPTH_MULT, alpha_reg=ALPHA_REG, fine=True, near=NEAR, far=FAR)
    with torch.no_grad():
        out, _ = lf.forward_with_prior({k: v.cuda() for k, v in o.res.items()}, o.rgb.cuda(), o.feat.cuda(), o.inv.cuda(),
                                       o.rows.cuda(), m)
    sc = term_scales(o, t64, m)
    for k in names:
        e = abs(float(out[k].detach()) - float(t64[k]))
        assert e <= 2e-6 * sc[k], (k, float(out[k]), float(t64[k]))


class RawLoss:
    """upnerf_loss_fwd / _bwd through the C ABI on the inputs of `o`; every output sits in front of `guard` NaN-filled floats."""

    def __init__(self, hip, o, sched, *, direct=False, sched_dev=None, term_mask=0, guard=0):
        self.L, self.o, self.G = hip["lib"], o, guard
        L, R, F = self.L, o.R, o.F
        self.dev = {k: v.cuda().contiguous() for k, v in o.res.items()}
        self.dev.update(rgb=o.rgb.cuda(), feat=o.feat.cuda().contiguous(), inv=o.inv.cuda(), rows=o.rows.cuda(), depth=o.depth.cuda())
        d = lambda k: L.ptr(self.dev[k].reshape(-1)) if k in self.dev else None
        self.buf = {k: torch.full((n + guard,), NAN, device="cuda") for k, n in dict(
            depth_out=R, terms=8, total=1, scratch=64 * 8, d_rows=2 * R, d_depth=R, d_sdc=R, d_sdf=R, d_fc=R * F, d_ff=R * F,
            d_rc=3 * R, d_rf=3 * R, d_beta=R, d_alpha=R).items()}
        b = lambda k: L.ptr(self.buf[k])
        self.a = L.LossArgs(R=R, F=F, fine=int(o.fine), has_tw=int(o.has_tw), sched=float(sched), depth_mult=DEPTH_MULT,
                            alpha_reg=ALPHA_REG, near=NEAR, far=FAR, depth_direct=d("depth") if direct else None,
                            inv_depth=None if direct else d("inv"), depth_scale_rows=None if direct else d("rows"),
                            s_depth_c=d("s_depth_coarse"), s_depth_f=d("s_depth_fine"), t_weight_c=d("t_weight_coarse"),
                            t_weight_f=d("t_weight_fine"), feat_c=d("feat_coarse"), feat_f=d("feat_fine"), feat_gt=d("feat"),
                            rgb_c=d("s_rgb_coarse"), rgb_f=d("s_rgb_fine"), rgb_gt=d("rgb"), beta=d("t_beta"), alpha=d("t_alpha"),
                            sched_dev=L.ptr(sched_dev), term_mask=term_mask, total=b("total"))
        self.g = L.LossGrads(d_depth_scale_rows=None if direct else b("d_rows"), d_depth=b("d_depth") if direct else None,
                             d_s_depth_c=b("d_sdc"), d_s_depth_f=b("d_sdf") if o.fine else None, d_feat_c=b("d_fc"),
                             d_feat_f=b("d_ff") if o.fine else None, d_rgb_c=b("d_rc"), d_rgb_f=b("d_rf") if o.fine else None,
                             d_beta=b("d_beta") if o.fine else None, d_alpha=b("d_alpha") if o.fine else None)
        self.keep = sched_dev

    def fwd(self):
        L, b = self.L, self.buf
        return L.lib.upnerf_loss_fwd(C.byref(self.a), L.ptr(b["depth_out"]), L.ptr(b["terms"]), L.ptr(b["scratch"]), L.stream())

    def bwd(self, g_terms=None, g_total=None):
        L = self.L
        self.a.g_total = L.ptr(g_total)
        rc = L.lib.upnerf_loss_bwd(C.byref(self.a), L.ptr(g_terms), C.byref(self.g), L.stream())
        torch.cuda.synchronize()
        self.a.g_total = None
        return rc

    def out(self, k):
        n = self.buf[k].numel() - self.G
        return cpu(self.buf[k][:n])

    def grads(self):
        """{UPNeRFLoss input name: gradient} of what the phase writes."""
        o, R = self.o, self.o.R
        g = {"s_depth_coarse": self.out("d_sdc"), "feat_coarse": self.out("d_fc").view(R, o.F),
             "s_rgb_coarse": self.out("d_rc").view(R, 3)}
        if o.fine:
            g.update({"s_depth_fine": self.out("d_sdf"), "feat_fine": self.out("d_ff").view(R, o.F),
                      "s_rgb_fine": self.out("d_rf").view(R, 3), "t_beta": self.out("d_beta").view(R, 1),
                      "t_alpha": self.out("d_alpha").view(R, 1)})
        return g


@pytest.mark.parametrize("fine", [True, False])
def test_loss_total_is_the_fp32_sum_of_the_masked_terms_in_term_order(hip, fine):
    o = loss_inputs(65, 8, 31, fine=fine)
    check_loss_margins(o)
    for mask in [1 << k for k in range(8)] + [0xFF, 0, 0b10100101]:
        raw = RawLoss(hip, o, 0.37, term_mask=mask)
        assert raw.fwd() == 0
        torch.cuda.synchronize()
        terms, total = raw.out("terms").numpy(), raw.out("total").numpy()
        assert np.isfinite(terms).all()
        want = np.float32(0.0)
        for k in range(8):
            want = np.float32(want + (terms[k] if (mask >> k) & 1 else np.float32(0.0)))
        assert total.view(np.uint32)[0] == np.array([want]).view(np.uint32)[0], (mask, float(total[0]), float(want))
        if not fine:  # the terms of the absent fine pass are written as exact zeros
            assert not terms[[3, 4, 5, 6, 7]].any()


def test_loss_multiplier_from_device_memory_overrides_the_static_one_and_follows_a_rewrite(hip):
    """sched = 0.5 names the phase (both term groups on); the multiplier itself is read from sched_dev at every launch."""
    o = loss_inputs(257, 8, 77)
    check_loss_margins(o)
    wts = term_weights(TERMS)
    sd = torch.tensor([0.25], device="cuda")
    gt = torch.tensor([wts[k] for k in TERMS], device="cuda")
    raw = RawLoss(hip, o, 0.5, sched_dev=sd)
    for m in (0.25, 0.75):
        sd.fill_(m)  # (the argument struct is not rebuilt)
        assert raw.fwd() == 0 and raw.bwd(g_terms=gt) == 0
        t64, g64, rw64, d64, cond = loss_ref(o, m, torch.float64, False, wts, False)
        t32, g32, rw32, d32, _ = loss_ref(o, m, torch.float32, False, wts, False)
        sc = term_scales(o, t64, m)
        terms = raw.out("terms")
        for i, k in enumerate(TERMS):
            assert abs(float(terms[i]) - float(t64[k])) <= 2e-6 * sc[k], (k, m)
        for k, g in raw.grads().items():
            ratio = gate_ratio(g, g64[k], g32[k], scale=cond.get(k))
            assert ratio <= 1, (k, m, ratio)
        ratio = gate_ratio(raw.out("d_rows").view(-1, 2), rw64, rw32, scale=prior_chain_scales(o, d64, cond["rows"])[1])
        assert ratio <= 1, ("depth_scale_rows", m, ratio)


@pytest.mark.parametrize("R,F", [(1, 6), (1, 384), (65, 6), (65, 384)])
def test_loss_kernels_write_nothing_past_their_outputs(hip, R, F):
    G = 64
    o = loss_inputs(R, F, 5 + R + F)
    check_loss_margins(o)
    gt = torch.ones(8, device="cuda")
    raw = RawLoss(hip, o, 0.37, term_mask=0xFF, guard=G)
    assert raw.fwd() == 0 and raw.bwd(g_terms=gt) == 0
    for k, b in raw.buf.items():
        assert bool(torch.isnan(b[-G:]).all()), k
        if k != "d_depth":  # (the prior form has no d_depth)
            assert not bool(torch.isnan(b[:-G]).any()), k
    assert bool(torch.isnan(raw.buf["d_depth"]).all())


# ====================================================================================== 2. pose refinement and rays
PI_BELOW = float(np.nextafter(np.float32(np.pi), np.float32(0.0)))  # the largest fp32 below pi
W_NORMS = (0.0, 1e-20, 1e-8, 1e-4, 1e-2, 0.1, 1.0, math.pi - 1e-3, PI_BELOW)
POSE_RS = (1, 127, 128, 129, 257)


def pose_rows():
    """[54, 6] se(3) rows: every |w| along one axis and along a generic direction, with u = ~1, 0, ~10."""
    generic = torch.tensor([0.48, -0.6, 0.64], dtype=torch.float64)  # a unit vector
    rows = []
    for iu, us in enumerate((1.0, 0.0, 10.0)):
        for iw, wn in enumerate(W_NORMS):
            for along_axis in (True, False):
                w = torch.zeros(3, dtype=torch.float64)
                if along_axis:
                    w[(iw + iu) % 3] = wn if iw % 2 == 0 else -wn
                else:
                    w = generic * wn
                u = torch.tensor([0.6, -0.64, 0.48], dtype=torch.float64) * us * (1.0 + 0.03 * iw)
                rows.append(torch.cat([w, u]))
    return torch.stack(rows).float()


def pose_inputs(R, seed=0):
    """se3 [R, 6] = the row set repeated, c2w [R, 3, 4] = one proper rotation with a translation of length 1e2 per repetition,
    directions with x, y in [-2, 2] and z = -1, and the upstream gradients of rays_o and rays_d."""
    g = torch.Generator().manual_seed(4000 + R + seed)
    base = pose_rows()
    n = base.shape[0]
    reps = (R + n - 1) // n
    q, _ = torch.linalg.qr(_u(g, (reps, 3, 3), -1.0, 1.0).double())
    q[:, :, 0] *= torch.linalg.det(q)[:, None]  # proper rotations
    t = _u(g, (reps, 3), -1.0, 1.0).double()
    t = 1e2 * t / t.norm(dim=-1, keepdim=True)
    poses = torch.cat([q, t[:, :, None]], -1).float()
    idx = torch.arange(R)
    se3, c2w = base[idx % n].clone(), poses[idx // n].clone()
    dirs = torch.cat([_u(g, (R, 2), -2.0, 2.0), -torch.ones(R, 1)], -1)
    return se3, c2w, dirs, _u(g, (R, 3), -1.0, 1.0), _u(g, (R, 3), -1.0, 1.0)


def check_pose_margins(se3, c2w, dirs):
    """No branch in kernel or oracle; what the gate assumes: |w| <= pi (series truncation < 1e-11), rotations proper and
    orthonormal to fp32 rounding, translations of length 1e2, |R dir| >= 1 so the normalisation is benign."""
    assert float(se3[:, :3].double().norm(dim=-1).max()) <= math.pi + 1e-6
    Rm = c2w[..., :3].double().reshape(-1, 3, 3)
    assert float((Rm @ Rm.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    assert float(torch.linalg.det(Rm).min()) > 0.999
    assert float((c2w[..., 3].double().reshape(-1, 3).norm(dim=-1) - 1e2).abs().max()) < 1e-3
    assert bool((dirs[:, 2] == -1.0).all()) and float(dirs[:, :2].abs().max()) <= 2.0


def pose_ref(se3, c2w, dirs, go, gd, dtype):
    s = None if se3 is None else se3.to(dtype).clone().requires_grad_(True)
    pose = c2w.to(dtype)
    if s is not None:
        refine = orc.se3_exp(s)
        pose = orc.compose_pair(refine, pose if pose.dim() == 3 else pose.expand(s.shape[0], 3, 4))
    o, d = orc.get_rays(dirs.to(dtype), pose)
    if s is not None:
        ((o * go.to(dtype)).sum() + (d * gd.to(dtype)).sum()).backward()
    return o.detach(), d.detach(), None if s is None else s.grad


def check_rays(tag, o, d, ref64, ref32, grad=None):
    for name, got, k in (("rays_o", o, 0), ("rays_d", d, 1)) + ((("d se3", grad, 2),) if grad is not None else ()):
        ratio = gate_ratio(got, ref64[k], ref32[k], rows=True)
        assert ratio <= 1, (tag, name, ratio)
    assert float((cpu(d).double().norm(dim=-1) - 1.0).abs().max()) <= FLOOR


@pytest.mark.parametrize("R", POSE_RS)
def test_pose_refinement_rays_and_gradients_match_fp64_per_row(hip, R):
    se3, c2w, dirs, go, gd = pose_inputs(R)
    check_pose_margins(se3, c2w, dirs)
    ref64, ref32 = (pose_ref(se3, c2w, dirs, go, gd, t) for t in (torch.float64, torch.float32))
    assert bool(torch.isfinite(ref64[2]).all())
    s = se3.cuda().requires_grad_(True)
    o, d = hip["camera"].refine_and_get_rays(s, c2w.cuda(), dirs.cuda())
    ((o * go.cuda()).sum() + (d * gd.cuda()).sum()).backward()
    assert bool(torch.isfinite(s.grad).all())  # (w = 0 and q underflowing included)
    check_rays(f"R={R}", o, d, ref64, ref32, s.grad)


def test_rays_without_refinement_and_from_one_shared_pose_match_fp64_per_row(hip):
    R = 129
    se3, c2w, dirs, go, gd = pose_inputs(R, seed=1)
    check_pose_margins(se3, c2w, dirs)
    cam = hip["camera"]
    # se3 = NULL, per-ray poses and one [3, 4] pose (both branches of get_rays)
    for tag, pose in (("no refinement", c2w), ("no refinement, shared pose", c2w[0])):
        ref64, ref32 = (pose_ref(None, pose, dirs, go, gd, t) for t in (torch.float64, torch.float32))
        o, d = cam.get_rays(dirs.cuda(), pose.cuda())
        check_rays(tag, o, d, ref64, ref32)
    # refinement of one shared pose
    ref64, ref32 = (pose_ref(se3, c2w[0], dirs, go, gd, t) for t in (torch.float64, torch.float32))
    s = se3.cuda().requires_grad_(True)
    o, d = cam.refine_and_get_rays(s, c2w[0].cuda(), dirs.cuda())
    ((o * go.cuda()).sum() + (d * gd.cuda()).sum()).backward()
    check_rays("shared pose", o, d, ref64, ref32, s.grad)


# ====================================================================================== 3. resampling at its limits
PDF_MAXS = 1024
ONE_BELOW = 1.0 - 2.0 ** -24


def pdf_inputs(R, S, n, u_rows, seed=0):
    """Sorted depths in [0.5, 4.5], weights in [0.2, 1] (every bin far heavier than eps), uniforms with 0 and 1 - 2^-24 planted."""
    g = torch.Generator().manual_seed(7000 + 13 * S + n + seed)
    z = torch.sort(_u(g, (R, S), 0.5, 4.5), -1)[0]
    w = _u(g, (R, S), 0.2, 1.0)
    u = _u(g, (u_rows, n))
    u.view(-1)[-1] = ONE_BELOW
    if u.numel() > 1:
        u.view(-1)[0] = 0.0
    return z, w, u


def check_pdf_margins(z, w, u):
    """The one branch of the arithmetic (bin mass < eps -> 1) is not taken: every bin is at least 20 eps = 2e-4 heavy.  That is a
    property of these inputs, asserted here, and not of the range alone: weights in [0.2, 1] only promise 0.2 / 1022 = 1.96e-4 at
    S = 1024; the uniform weights drawn there have a mean of about 0.6, so the lightest bin holds about 0.2 / (1022 * 0.6) = 3.3e-4.
    The inverse cdf is continuous at its knots, so WHICH bin a uniform falls into is no branch of the value."""
    pdf = (w[:, 1:-1].double() + 1e-5) / (w[:, 1:-1].double() + 1e-5).sum(1, keepdim=True)
    assert float(w.min()) >= 0.2 and float(pdf.min()) >= 20e-5
    assert float(u.min()) == 0.0 or u.numel() == 1
    assert float(u.max()) == ONE_BELOW < 1.0
    assert bool((z[:, 1:] >= z[:, :-1]).all())


PDF_CASES = [(3, 1), (3, 64), (3, 65), (4, 1), (4, 64), (4, 65), (65, 128), (1024, 2)]


@pytest.mark.parametrize("shared_u", [False, True])
@pytest.mark.parametrize("S,n", PDF_CASES)
def test_sample_pdf_from_one_bin_to_the_full_lds_row(hip, S, n, shared_u):
    L = hip["lib"]
    R, stride = 5, n + 3
    z, w, u = pdf_inputs(R, S, n, 1 if shared_u else R)
    check_pdf_margins(z, w, u)
    ref = orc.sample_pdf(0.5 * (z[:, :-1] + z[:, 1:]), w[:, 1:-1], n, False, u.expand(R, n))
    out = torch.full((R, stride), NAN, device="cuda")
    zd, wd, ud = z.cuda(), w.cuda(), u.cuda()
    L.check(L.lib.upnerf_sample_pdf(R, S, L.ptr(zd), L.ptr(wd), L.ptr(ud), 1 if shared_u else R, n, L.ptr(out), stride,
                                    L.stream()), "sample_pdf")
    got = cpu(out)
    assert bool(torch.isnan(got[:, n:]).all())  # the gaps between the rows are not written
    dz = float((got[:, :n] - ref).abs().max())
    assert dz < 5e-6, dz


def _resample_reference(L, R, Nc, z, sets, S):
    """The launch-per-piece sequence: upnerf_sample_pdf per set into its columns, then upnerf_sort_rows.  Returns (unsorted, sorted)."""
    ref = torch.empty(R, S, device="cuda")
    ref[:, :Nc] = z
    for w, n, col, u, rows in sets:
        if n:
            L.check(L.lib.upnerf_sample_pdf(R, Nc, L.ptr(z), L.ptr(w), L.ptr(u), rows, n, ref.data_ptr() + 4 * col, S, L.stream()),
                    "sample_pdf")
    unsorted = ref.clone()
    L.check(L.lib.upnerf_sort_rows(R, S, L.ptr(ref), L.stream()), "sort_rows")
    return unsorted, ref


@pytest.mark.parametrize("Nc,na,nb,mode", [(512, 256, 256, "keyed"), (1021, 3, 0, "buf"), (768, 0, 256, "det"), (3, 1, 0, "keyed"),
                                           (3, 1, 0, "buf"), (3, 0, 1, "det")])
def test_fused_resample_and_sort_at_the_full_row_and_at_three_coarse_depths(hip, Nc, na, nb, mode):
    L = hip["lib"]
    lib, ptr, st = L.lib, L.ptr, L.stream
    R, S = 5, Nc + na + nb
    assert S == PDF_MAXS or Nc == 3
    g = torch.Generator().manual_seed(Nc * 1000 + na)
    z = torch.sort(_u(g, (R, Nc), 0.1, 4.1), -1)[0].cuda().contiguous()
    wa, wb = (_u(g, (R, Nc)) ** 4).cuda().contiguous(), (_u(g, (R, Nc)) ** 8).cuda().contiguous()
    wa[3] = 0.0  # an all-eps cdf row
    seed, step, row0, stride = 0x1234567887654321, 17, 5, 3
    col_a, col_b = Nc + nb, Nc  # set A behind set B, as render_rays places them
    sets, us = [], {}
    for d, (w, n, col) in enumerate(((wa, na, col_a), (wb, nb, col_b)), start=1):
        u, rows = None, R
        if n and mode == "det":
            u, rows = torch.linspace(0, 1, n, device="cuda"), 1
        elif n and mode == "buf":
            u = _u(g, (R, n)).cuda().contiguous()
        elif n:
            u = torch.empty(R, n, device="cuda")
            L.check(lib.upnerf_uniform_keyed(R, n, seed, step, None, row0, stride, d, ptr(u), st()), "uniform_keyed")
        us[d] = u
        sets.append((w, n, col, u, rows))
    unsorted, ref = _resample_reference(L, R, Nc, z, sets, S)
    got = torch.full((R, S), NAN, device="cuda")
    rng = L.Rng(seed=seed, step=step, row0=row0, row_stride=stride, step_dev=None)
    keyed = mode == "keyed"
    L.check(lib.upnerf_resample_sort(R, Nc, ptr(z), ptr(wa), na, col_a, None if keyed else ptr(us[1]), 1, ptr(wb), nb, col_b,
                                     None if keyed else ptr(us[2]), 2, 1 if mode == "det" else R, C.byref(rng) if keyed else None,
                                     ptr(got), st()), "resample_sort")
    torch.cuda.synchronize()
    got, ref, unsorted = cpu(got), cpu(ref), cpu(unsorted)
    assert np.array_equal(got.numpy(), ref.numpy())  # bit for bit (no NaN left: array_equal would be False)
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    assert np.array_equal(got.numpy(), torch.sort(unsorted, -1)[0].numpy())  # a permutation of coarse depths and samples


def sort_rows_input(R, S, seed=0):
    g = torch.Generator().manual_seed(9000 + S + R + seed)
    z = _u(g, (R, S), -1.0, 1.0)
    if S >= 4:
        z[0, : S // 2] = z[0, S // 2: 2 * (S // 2)]  # duplicates
    special = torch.tensor([math.inf, -0.0, -math.inf, 0.0, 0.0, math.inf, -math.inf, -0.0])
    r = 0 if R == 1 else 2
    k = min(S, special.numel())
    pos = torch.linspace(0, S - 1, k).round().long()  # first and last element included
    z[r, pos] = special[:k]
    if R > 1:
        z[1] = float(z[1, 0])  # all equal
    return z


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("S", [1, 2, 1023, 1024])
def test_sort_rows_from_one_element_to_the_full_lds_row(hip, S, R):
    L = hip["lib"]
    z = sort_rows_input(R, S)
    zd = z.cuda().contiguous()
    L.check(L.lib.upnerf_sort_rows(R, S, L.ptr(zd), L.stream()), "sort_rows")
    assert np.array_equal(cpu(zd).numpy(), torch.sort(z, -1)[0].numpy())


def test_resampling_entry_points_refuse_rows_outside_their_limits(hip):
    """Host-side checks, nothing is launched: UPNERF_EINVAL, and the NaN-filled output stays as it was.  Every pointer is a real
    device buffer large enough for the refused shape."""
    L = hip["lib"]
    lib, ptr, st = L.lib, L.ptr, L.stream
    R, big = 3, PDF_MAXS + 8
    z = torch.sort(torch.rand(R, big), -1)[0].cuda()
    w, u = torch.rand(R, big).cuda() + 0.2, torch.rand(R, big).cuda()
    out = torch.full((R, 2 * big), NAN, device="cuda")
    rng = L.Rng(seed=1, step=0, row0=0, row_stride=1, step_dev=None)
    assert lib.upnerf_sample_pdf(R, PDF_MAXS + 1, ptr(z), ptr(w), ptr(u), R, 4, ptr(out), 2 * big, st()) == EINVAL
    assert lib.upnerf_sample_pdf(R, 2, ptr(z), ptr(w), ptr(u), R, 4, ptr(out), 2 * big, st()) == EINVAL
    assert lib.upnerf_sort_rows(R, PDF_MAXS + 1, ptr(out), st()) == EINVAL

    def fused(Nc, na, col_a, nb, col_b):
        return lib.upnerf_resample_sort(R, Nc, ptr(z), ptr(w), na, col_a, ptr(u), 1, ptr(w), nb, col_b, ptr(u), 2, R, C.byref(rng),
                                        ptr(out), st())

    assert fused(2, 1, 2, 0, 2) == EINVAL                      # Nc = 2
    assert fused(512, 256, 769, 257, 512) == EINVAL            # 1025 in all
    assert fused(1021, 4, 1021, 0, 1021) == EINVAL             # 1025 in all, one set
    assert fused(64, 8, 63, 0, 64) == EINVAL                   # set A starts inside the coarse depths
    assert fused(64, 8, 65, 0, 64) == EINVAL                   # set A ends behind the row
    assert fused(64, 8, 64, 8, 80) == EINVAL                   # set B starts behind the row
    assert fused(64, 8, 64, 8, 68) == EINVAL                   # the sets overlap
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # ... and the same buffers are accepted one step inside the limits
    assert lib.upnerf_sample_pdf(R, PDF_MAXS, ptr(z[:, :PDF_MAXS].contiguous()), ptr(w[:, :PDF_MAXS].contiguous()), ptr(u), R, 4,
                                 ptr(out), 2 * big, st()) == 0
    assert fused(64, 8, 64, 8, 72) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:, :4]).any())
