"""Stage-local fp64 references, input families, derived per-element gates and an fp32 emulation of csrc/transient.hip
(upnerf_transient_fwd / upnerf_transient_bwd).  CPU only: tests/test_transient_ref_cpu.py proves the gates on the emulation and on
planted defects, tests/test_hip_transient.py holds the kernels to them.  No gate is computed from an output under test.

The kernels write to global memory the very values they keep in LDS for the next stage (h[0..3], e, t, spre, alpha, rgb,
dz_heads, gz_t, gz_e, gz_h[3..0]), so the reference of a stage takes the STORED output of the stage before it as its input and
every gate is a one-stage bound.  With u = 2^-24, L terms per sum and S the fp64 sum of the terms' magnitudes:

  dense stages (h[l], e, t, spre, gz_t, [gz_e | g_temb], gz_h[l], g_feat)
      |stored - fp64| <= L u S          (tests/dense_ref.py: fp32 products and sums in any order)
      S = |x| |W|^T + |b|, L = K + 1 forward; S = |g| |W| (+ |dz_alpha| |w_alpha| for gz_h[3], L + 1), L = N backward.
      A forward ReLU output is gated on its pre-activation (ReLU is 1-Lipschitz), has to be >= 0 and exactly 0 where the fp64
      pre-activation lies below minus the gate.  A backward mask is read from the stored activation and is therefore exact: where
      that is <= 0 the gate is 0, and a gate of 0 asks for exactly 0 (so does S = 0: a dead layer kills everything upstream).
  element-wise stages (alpha, rgb, beta, dz_heads)
      |stored - fp64| <= 4 e32 + 2^-22 scale      (tests/test_hip_perray.py)
      e32 = |the same formula in torch float32 on the CPU - fp64| on the same (stored, fp32) inputs, scale = the element's own
      fp64 magnitude; a gradient that sums terms of opposite sign (d alpha = d_alpha + d_beta softplus(s)) takes the summed
      magnitudes.  alpha and rgb are sigmoids of a dot product that is not stored: their formula is evaluated at the fp64
      pre-activation rounded to fp32, and the dot product's own L u S enters through sigmoid's slope, <= 1/4.
      Where stored alpha or rgb is exactly 1.0f, 1 - y is 0 in fp32 and in fp64 alike: the limit is 0 and the gradient has to be.
"""
import math

import torch

import dense_ref as dr

U = dr.U
FLOOR = 2.0 ** -22
NAMES = ("w0", "b0", "w1", "b1", "w2", "b2", "w3", "b3", "wf", "bf", "wt", "bt", "wa", "ba", "wb", "bb", "wr", "br")
_KEYS = ("feat_encoder.0", "feat_encoder.2", "feat_encoder.4", "feat_encoder.6", "final_encoder", "t_encoder.0", "alpha_layer.0",
         "beta_layer.0", "rgb_layer.0")
BETA_MIN = 0.1
RS = (1, 15, 16, 17, 33, 129)
RMAX = 129
FAMILIES = ("synth", "heads", "dead", "big", "tiny")


# ---------------------------------------------------------------------------------------------------------------- inputs
def synth_params(seed=4):
    """The reference TransientNet's parameters (upnerf_amd.synth.transient_state) under the C ABI's names, fp32 on the CPU."""
    from upnerf_amd import synth
    sd = synth.transient_state(11, seed=seed)
    P = {}
    for j, k in enumerate(_KEYS):
        P[NAMES[2 * j]], P[NAMES[2 * j + 1]] = sd[k + ".weight"].float().contiguous(), sd[k + ".bias"].float().contiguous()
    P["temb_table"] = sd["embedding_t.weight"].float().contiguous()
    return P


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def forward64(P, feat, temb):
    """The whole forward in fp64 from the inputs (used to BUILD input families and to assert where they put their rows)."""
    d = lambda k: P[k].double()
    x, hs = feat.double(), []
    for l in range(4):
        x = (x @ d(f"w{l}").t() + d(f"b{l}")).clamp_min(0)
        hs.append(x)
    e = x @ d("wf").t() + d("bf")
    t = (torch.cat([e, temb.double()], 1) @ d("wt").t() + d("bt")).clamp_min(0)
    return dict(za=x @ d("wa")[0] + d("ba"), spre=t @ d("wb")[0] + d("bb"), zr=t @ d("wr").t() + d("br"), h=hs, e=e, t=t)


def family(name, seed=7):
    """(P, feat [129][384], t_emb [129][128], upstreams (d_alpha [129], d_rgb [129][3], d_beta [129])) of one input family; a
    case of R rows takes rows off .. off + R (the network has no coupling between rows).
      synth  synth.transient_state weights, normal features
      heads  the three heads' weights and biases rescaled so that spre spans about [-30, 40] (no row within 1e-3 of softplus'
             threshold 20, rows on both sides) and the alpha and rgb pre-activations about [-25, 25]: alpha and rgb round to
             exactly 1.0f in some rows and lie below 1e-7 in others.  The rows are ordered so that the first eight hold the
             extremes: every R >= 15 has them all, R = 1 is run at each of the offsets 0 .. 7.
      dead   b2 = -100: h[2] is all zero, so gz_h[2], gz_h[1], gz_h[0] and g_feat have to be exactly 0
      big    features times 2^12            tiny   features times 2^-20"""
    P = synth_params()
    feat = _randn((RMAX, 384), seed)
    temb = P["temb_table"][(torch.arange(RMAX) * 7) % 11].contiguous()
    up = (_randn((RMAX,), seed + 1), _randn((RMAX, 3), seed + 2), _randn((RMAX,), seed + 3))
    if name == "synth":
        pass
    elif name == "big":
        feat = feat * 4096.0
    elif name == "tiny":
        feat = feat * 2.0 ** -20
    elif name == "dead":
        P["b2"] = torch.full_like(P["b2"], -100.0)
    elif name == "heads":
        f = forward64(P, feat, temb)

        def rescale(w, pre, bias, lo, hi):  # pre = x . w + bias per row -> spans [lo, hi]
            z = pre - bias.double()
            s = (hi - lo) / float(z.max() - z.min())
            return (w.double() * s).float(), (bias.double() * 0 + (lo - s * float(z.min()))).float()

        P["wa"], P["ba"] = rescale(P["wa"], f["za"], P["ba"], -25.0, 25.0)
        P["wb"], P["bb"] = rescale(P["wb"], f["spre"], P["bb"], -30.0, 40.0)
        zr = f["zr"] - P["br"].double()
        s = 50.0 / float(zr.max() - zr.min())
        P["wr"], P["br"] = (P["wr"].double() * s).float(), (P["br"].double() * 0 - 25.0 - s * float(zr.min())).float()
        f = forward64(P, feat, temb)
        first = []
        for z in (f["za"], f["spre"], f["zr"].max(1)[0], f["zr"].min(1)[0]):
            first += [i for i in (int(z.argmax()), int(z.argmin())) if i not in first]
        order = torch.tensor(first + [i for i in range(RMAX) if i not in first])
        feat, temb = feat[order].contiguous(), temb[order].contiguous()
    else:
        raise KeyError(name)
    return P, feat.float().contiguous(), temb, up


def heads_family_facts(P, feat, temb):
    """What the heads family promises, from the inputs in fp64 (asserted on the CPU by both test modules)."""
    f = forward64(P, feat, temb)
    sig = lambda z: torch.sigmoid(z).float()
    return dict(spre_margin=float((f["spre"] - 20.0).abs().min()), above=int((f["spre"] > 20).sum()), below=int((f["spre"] < 20).sum()),
                spre_lo=float(f["spre"].min()), spre_hi=float(f["spre"].max()),
                alpha_one=int((sig(f["za"]) == 1.0).sum()), alpha_small=int((sig(f["za"]) < 1e-7).sum()),
                rgb_one=int((sig(f["zr"]) == 1.0).sum()), rgb_small=int((sig(f["zr"]) < 1e-7).sum()),
                first8=dict(above=int((f["spre"][:8] > 20).sum()), below=int((f["spre"][:8] < 20).sum()),
                            alpha_one=int((sig(f["za"][:8]) == 1.0).sum()), alpha_small=int((sig(f["za"][:8]) < 1e-7).sum()),
                            rgb_one=int((sig(f["zr"][:8]) == 1.0).sum()), rgb_small=int((sig(f["zr"][:8]) < 1e-7).sum())))


def offsets(name, R):
    return tuple(range(8)) if (name == "heads" and R == 1) else (0,)


def rows(x, off, R):
    return None if x is None else x[off:off + R].contiguous()


# ---------------------------------------------------------------------------------------------------- element-wise formulas
def softplus(x):
    """torch.nn.functional.softplus (beta 1, threshold 20) as csrc/transient.hip writes it, in x's dtype."""
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def beta_formula(spre, alpha, beta_min, dtype):
    s, a = spre.to(dtype), alpha.to(dtype)
    sa = softplus(s) * a
    bm = torch.tensor(float(torch.tensor(beta_min, dtype=torch.float32)), dtype=dtype)  # the fp32 number the kernel receives
    return sa + bm, sa.abs() + bm.abs()


def dz_formula(alpha, spre, rgb, up, dtype, no_alpha_in_dz_beta=False):
    """[R][8] head pre-activation gradients (columns 5 .. 7 zero) and the summed magnitudes of each element's summands."""
    al, s, y = alpha.to(dtype), spre.to(dtype), rgb.to(dtype)
    R = al.shape[0]
    z = lambda *sh: torch.zeros(*sh, dtype=dtype)
    da, drgb, db = (z(R) if up[0] is None else up[0].to(dtype), z(R, 3) if up[1] is None else up[1].to(dtype),
                    z(R) if up[2] is None else up[2].to(dtype))
    one = torch.tensor(1.0, dtype=dtype)
    t = db * softplus(s)
    dz = z(R, 8)
    dz[:, 0] = (da + t) * al * (one - al)
    dz[:, 1] = db * sigmoid(s) if no_alpha_in_dz_beta else db * al * sigmoid(s)
    dz[:, 2:5] = drgb * y * (one - y)
    scale = dz.abs().clone()
    scale[:, 0] = (da.abs() + t.abs()) * al * (one - al)
    return dz, scale


# ----------------------------------------------------------------------------------------------------------------- gates
def ew_gate(ref64, ref32, scale=None, extra=0.0):
    scale = ref64.abs() if scale is None else scale.double()
    assert bool((scale >= ref64.abs() * (1 - 1e-12)).all())
    return 4 * (ref32.double() - ref64).abs() + FLOOR * scale + extra


def dense(x, W, bias=None, rank1=None):
    """fp64 x . W^T (+ bias) (+ rank1 = (column [R], row [N]) outer product) and its gate L u S."""
    xd, Wd = x.double(), W.double()
    pre, S, L = xd @ Wd.t(), xd.abs() @ Wd.abs().t(), x.shape[1]
    if bias is not None:
        pre, S, L = pre + bias.double()[None, :], S + bias.double().abs()[None, :], L + 1
    if rank1 is not None:
        c, r = rank1[0].double(), rank1[1].double()
        pre, S, L = pre + c[:, None] * r[None, :], S + c.abs()[:, None] * r.abs()[None, :], L + 1
    return pre, dr.gate_fp32(L, S)


def relu_ratio(got, pre, gate):
    """Forward ReLU stage: the pre-activation's gate on max(pre, 0); inf if an element is negative or is not exactly 0 where the
    fp64 pre-activation lies below minus the gate."""
    r = dr.ratio(got, pre.clamp_min(0.0), gate)
    g = got.detach().cpu().double()
    if bool((g < 0).any()) or bool((g[pre < -gate] != 0).any()):
        return math.inf
    return r


def masked_ratio(got, pre, gate, act):
    """Backward stage masked by the STORED activation: the mask is exact, so the gate is 0 (exact zero) where act <= 0."""
    on = act.detach().cpu() > 0
    z = torch.zeros_like(pre)
    return dr.ratio(got, torch.where(on, pre, z), torch.where(on, gate, z))


# ----------------------------------------------------------------------------------------------------------------- checks
def forward_checks(P, feat, temb, out, beta_min=BETA_MIN):
    """{stage: worst error / gate} of a forward's stored outputs (dict of CPU tensors h [4][R][256], e, t, spre [R], alpha [R],
    rgb [R][3], beta [R]); each stage's reference starts from the stored output of the stage before it."""
    res = {}
    x = feat
    for l in range(4):
        pre, gate = dense(x, P[f"w{l}"], P[f"b{l}"])
        res[f"h{l}"] = relu_ratio(out["h"][l], pre, gate)
        x = out["h"][l]
    pre, gate = dense(x, P["wf"], P["bf"])
    res["e"] = dr.ratio(out["e"], pre, gate)
    pre, gate = dense(torch.cat([out["e"], temb], 1), P["wt"], P["bt"])
    res["t"] = relu_ratio(out["t"], pre, gate)
    za, ga = dense(out["h"][3], P["wa"], P["ba"])
    res["alpha"] = dr.ratio(out["alpha"], sigmoid(za[:, 0]), ew_gate(sigmoid(za[:, 0]), sigmoid(za[:, 0].float()), extra=ga[:, 0] / 4))
    pre, gate = dense(out["t"], P["wb"], P["bb"])
    res["spre"] = dr.ratio(out["spre"], pre[:, 0], gate[:, 0])
    zr, gr = dense(out["t"], P["wr"], P["br"])
    res["rgb"] = dr.ratio(out["rgb"], sigmoid(zr), ew_gate(sigmoid(zr), sigmoid(zr.float()), extra=gr / 4))
    b64, sc = beta_formula(out["spre"], out["alpha"], beta_min, torch.float64)
    b32, _ = beta_formula(out["spre"], out["alpha"], beta_min, torch.float32)
    res["beta"] = dr.ratio(out["beta"], b64, ew_gate(b64, b32, scale=sc))
    return res


def backward_checks(P, fwd, up, out):
    """{stage: worst error / gate} of a backward's stored outputs (dz_heads [R][8], gz_t, gz_e, gz_h [4][R][256] and, where
    present, g_temb and g_feat) given the STORED forward `fwd` and the upstreams (None = zero)."""
    res = {}
    d64, sc = dz_formula(fwd["alpha"], fwd["spre"], fwd["rgb"], up, torch.float64)
    d32, _ = dz_formula(fwd["alpha"], fwd["spre"], fwd["rgb"], up, torch.float32)
    res["dz_heads"] = dr.ratio(out["dz_heads"], d64, ew_gate(d64, d32, scale=sc))
    dz = out["dz_heads"]
    pre, gate = dense(dz[:, 1:5], torch.cat([P["wb"], P["wr"]], 0).t())
    res["gz_t"] = masked_ratio(out["gz_t"], pre, gate, fwd["t"])
    pre, gate = dense(out["gz_t"], P["wt"].t())
    res["gz_e"] = dr.ratio(out["gz_e"], pre[:, :256], gate[:, :256])
    if out.get("g_temb") is not None:
        res["g_temb"] = dr.ratio(out["g_temb"], pre[:, 256:], gate[:, 256:])
    pre, gate = dense(out["gz_e"], P["wf"].t(), rank1=(dz[:, 0], P["wa"][0]))
    res["gz_h3"] = masked_ratio(out["gz_h"][3], pre, gate, fwd["h"][3])
    for l in (2, 1, 0):
        pre, gate = dense(out["gz_h"][l + 1], P[f"w{l + 1}"].t())
        res[f"gz_h{l}"] = masked_ratio(out["gz_h"][l], pre, gate, fwd["h"][l])
    if out.get("g_feat") is not None:
        pre, gate = dense(out["gz_h"][0], P["w0"].t())
        res["g_feat"] = dr.ratio(out["g_feat"], pre, gate)
    return res


# ------------------------------------------------------------------------------------- fp32 emulation, with planted defects
DEFECTS = ("drop_kgroup", "swap_kgroup", "mask_prev_row", "no_rank1", "dz_beta_no_alpha", "temb_shift64")
# the stage a defect has to push outside its gate, per variant (layer) the CPU test plants it in
FWD_LAYERS = ("h0", "h1", "h2", "h3", "e", "t")
BWD_LAYERS = ("gz_e", "gz_h3", "gz_h2", "gz_h1", "gz_h0", "g_feat")
MASKED = ("gz_t", "gz_h3", "gz_h2", "gz_h1", "gz_h0")


def _mm(x, W, defect, stage, g=5):
    """x . W^T in fp32; for defect = (kind, stage): k-group g (columns 16 g .. 16 g + 15) dropped, or fed from the weights of
    k-group g + 1."""
    x, W = x.float(), W.float()
    if defect is not None and defect[1] == stage and defect[0] in ("drop_kgroup", "swap_kgroup"):
        W = W.clone()
        W[:, 16 * g:16 * g + 16] = 0.0 if defect[0] == "drop_kgroup" else W[:, 16 * g + 16:16 * g + 32].clone()
    return x @ W.t()


def emulate_fwd(P, feat, temb, beta_min=BETA_MIN, defect=None):
    out, x, hs = {}, feat.float(), []
    for l in range(4):
        x = (_mm(x, P[f"w{l}"], defect, f"h{l}") + P[f"b{l}"]).clamp_min(0)
        hs.append(x)
    out["h"] = torch.stack(hs)
    out["e"] = _mm(x, P["wf"], defect, "e") + P["bf"]
    out["t"] = (_mm(torch.cat([out["e"], temb], 1), P["wt"], defect, "t") + P["bt"]).clamp_min(0)
    out["alpha"] = sigmoid(x @ P["wa"][0] + P["ba"])
    out["spre"] = out["t"] @ P["wb"][0] + P["bb"]
    out["rgb"] = sigmoid(out["t"] @ P["wr"].t() + P["br"])
    out["beta"] = beta_formula(out["spre"], out["alpha"], beta_min, torch.float32)[0]
    return out


def _mask(g, act, defect, stage):
    on = act > 0
    if defect is not None and defect == ("mask_prev_row", stage) and act.shape[0] >= 2:
        on = on.clone()
        on[-1] = act[-2] > 0
    return torch.where(on, g, torch.zeros_like(g))


def emulate_bwd(P, fwd, up, defect=None, want_temb=True, want_feat=True):
    kind = defect[0] if defect else None
    out = {}
    dz = out["dz_heads"] = dz_formula(fwd["alpha"], fwd["spre"], fwd["rgb"], up, torch.float32, kind == "dz_beta_no_alpha")[0]
    out["gz_t"] = _mask(dz[:, 1:5] @ torch.cat([P["wb"], P["wr"]], 0), fwd["t"], defect, "gz_t")
    full = _mm(out["gz_t"], P["wt"].t(), defect, "gz_e", g=3)
    out["gz_e"] = full[:, :256].contiguous()
    temb = full[:, 256:].contiguous()
    out["g_temb"] = (torch.roll(temb, 64, 1) if kind == "temb_shift64" else temb) if want_temb else None
    gz = [None] * 4
    r1 = 0.0 if kind == "no_rank1" else dz[:, 0:1] * P["wa"]
    gz[3] = _mask(_mm(out["gz_e"], P["wf"].t(), defect, "gz_h3") + r1, fwd["h"][3], defect, "gz_h3")
    for l in (2, 1, 0):
        gz[l] = _mask(_mm(gz[l + 1], P[f"w{l + 1}"].t(), defect, f"gz_h{l}"), fwd["h"][l], defect, f"gz_h{l}")
    out["gz_h"] = torch.stack(gz)
    out["g_feat"] = _mm(gz[0], P["w0"].t(), defect, "g_feat") if want_feat else None
    return out
