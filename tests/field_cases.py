"""The fused field pass against the torch restatement (tests/kernel_space.py), stage by stage: the inputs of a pass (golden cases
and synthetic edge cases), the restatement's reference in fp32 or fp64, and the one comparison body the GPU tests share.
Importable without a GPU; only check_field_pass touches a device.

An fp64 reference starts where the kernels start (kernel_space.field(arg32=True): sample positions and encoding arguments as fp32
arithmetic gives them) and runs everything behind x0 -- trunk, heads, softplus / sigmoid, compositing, autograd -- in fp64."""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

import kernel_space as ks
from golden_util import Case, orc, rel_err

# Tolerances (max-normalised error, golden_util.rel_err): fp32 MFMA vs fp32 CPU BLAS differ only in summation order:
# 1e-5 on activations and per-ray maps, 1e-4 on gradients (the bar BASELINE.json states is 1e-4).
TOL_ACT = 1e-5
TOL_GRAD = 1e-4
TOL_X0 = 2e-6  # the encoding and the per-ray colour-head input: exact sincos of an fp32 argument, no contraction
# "f16" (BASELINE.json configs[3]: fp16 weights and activations, one MFMA per product, fp32 accumulate) is compared with the
# same restatement at STATED relaxed gates: 11-bit operands through ten chained layers give ~1e-3 on activations
# (max-normalised gate 1e-2).  Gradients: a ReLU whose pre-activation lies within 1e-3 of zero may decide the other way in
# fp16, which changes single entries by their full size, so the gate is on the whole tensor -- relative L2 error 6e-2 --
# plus a loose cap on any single entry (max-normalised 0.5).
TOL_ACT_F16, TOL_GRAD_F16, TOL_GRAD_F16_MAX = 1e-2, 6e-2, 0.5
TOL_X0_F16 = 1e-3  # f16: x0 is stored from the fp16 plane the layers read
# ... and, because an L2 gate that wide could hide a wrong ReLU-mask ROW (one sample's 256 mask bits of one layer are 1 / M of the
# tensor), the masks are compared directly (r5 VERDICT item 6): the share of elements whose sign decision differs from the
# restatement's -- stored activation h_l > 0 in the forward pass, pre-activation gradient gz_l != 0 in the backward pass -- stays
# below 1e-3 per layer, and no single sample row differs in more than an eighth of its bits (measured in round 6: worst share
# 2.1e-4, worst row 2 of 256 bits; the fp32-accurate modes are held to 1e-4 and 4 of 256 bits -- measured 1.0e-5 and 1 bit, a
# pre-activation within rounding of zero).
MASK_FLIP_F16, MASK_FLIP_ROW_F16 = 1e-3, 1.0 / 8
MASK_FLIP, MASK_FLIP_ROW = 1e-4, 1.0 / 64

OUT_NAMES = ["E_s", "G_c", "sum_sfeat", "t_weight", "c_depth", "s_depth", "rgb_map", "w_all", "w_s", "rgb_joint_map"]  # _FieldPass's


def gen(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


# ------------------------------------------------------------------------------------------ the inputs of a pass
def setup_pass(c, typ):
    """Inputs of one field pass of golden case `c` (CPU tensors) + the packer."""
    from test_packing_cpu import build_model
    from upnerf_amd.rendering import band_weights
    st = c.state(requires_grad=False)
    b = c.batch()
    idx = b["img_idx"]
    pose = orc.compose_pair(orc.se3_exp(st["se3_refine"][idx]), b["c2w"]) if c.pose_opt else b["c2w"]
    o, d = orc.get_rays(b["directions"], pose)
    model = build_model(c, typ, st)
    keep = {}
    real = orc.schedule_mult
    orc.schedule_mult = lambda p, s: c.sched
    try:
        with torch.no_grad():
            orc.training_forward(st, c.cfgs(), b, c.hparams(), c.progress, u_list=c.u_list, keep=keep)
    finally:
        orc.schedule_mult = real
    z = keep["z_coarse" if typ == "coarse" else "z_fine"].contiguous()
    use_cand = bool(c.sched < 1 and model.encode_candidate)
    use_rgb = bool(c.sched > 0 or not c.encode_feat)  # without features the colour head always runs (rendering.render_rays)
    mode = (1 if use_rgb else 0) if use_cand else (3 if c.sched < 1 else 2)
    return dict(model=model, o=o.contiguous(), d=d.contiguous(), z=z, a_rows=st[f"embedding_{typ}_a"][idx],
                c_rows=st[f"embedding_{typ}_c"][idx], use_cand=use_cand, use_rgb=use_rgb, mode=mode,
                rgb_joint=bool(not c.encode_feat and mode <= 1 and use_rgb),  # the shared colour under the joint weights too
                wk_xyz=band_weights(10, c.progress, c.c2f), wk_dir=band_weights(4, c.progress, c.c2f))


# Synthetic edge cases.  frac: the encoding bands as coarse-to-fine progress 0.28 of (0.1, 0.5) gives them -- xyz (1, 1, 1, 1, 0.5,
# 0, ...), direction (1, 0.905, 0, 0): one fractional weight, every band above it zero (the kernels skip the sincos of a zero
# band).  dead: the index of a ray whose trunk is entirely masked, see synth_pass.  seed: of the field's weights.
Synth = namedtuple("Synth", "W D R S mode use_cand use_rgb seed frac dead", defaults=(3, False, None))
SYNTH_256 = [
    Synth(256, 8, 1, 64, 1, True, True),                 # exactly one tile
    # (seed 8.  Under seed 3 fp16 operands alone miss the f16 gates on this draw (tests/test_field_cases_cpu.py asserts they do
    # not); under seed 4 one pre-activation of layer 6 lies 2e-8 of the layer's maximum from zero, below an fp32 ulp, and the f16x3
    # kernels decide it the other way: one flipped ReLU, inside the mask limits, whose row of gradients then differs in full.)
    Synth(256, 8, 7, 40, 1, True, True, seed=8, frac=True),  # 24-row tail; tiles straddle two and three rays
    Synth(256, 8, 5, 33, 0, True, False),                # S is odd
    Synth(256, 8, 3, 200, 2, False, True, dead=1),       # S > 64 and no multiple of 32; tiles 4 and 5 lie inside the dead ray
    Synth(256, 8, 2, 257, 3, False, True),               # two-row tail; mode 3 with the colour head on
    Synth(256, 8, 9, 32, 3, False, False, frac=True),    # half-tile rays
]
# The smallest pass the Python entry accepts is one sample of one ray: plan_pass sends S < 32 to the fp32 kernels in the f32 and
# f16x3 modes and refuses it in the f16 mode (the GPU test asserts that refusal).
SYNTH_SMALLEST = Synth(256, 8, 1, 1, 1, True, True)
SYNTH_64 = [Synth(64, 4, 5, 33, 1, True, True), Synth(64, 4, 7, 40, 3, False, True, frac=True)]  # the fp32 kernels in either mode
NOFEAT = [("nofeat_phase1", "fine"), ("nofeat_w256_phase1", "fine")]  # encode_feat = False: rgb_joint_map beside rgb_map
DEAD_X, DEAD_GAIN, DEAD_BIAS = 50.0, 0.2, 0.05


def synth_id(c):
    return (f"w{c.W}-{c.R}x{c.S}-m{c.mode}" + ("c" if c.use_cand else "") + ("r" if c.use_rgb else "")
            + ("-frac" if c.frac else "") + ("-dead" if c.dead is not None else ""))


def synth_pass(c):
    """The inputs of synthetic case `c`, from upnerf_amd.synth.nerf_state.  Per-ray side inputs span five decades, so the per-tile
    exponents differ between the tiles of one launch.

    A dead ray (one whose every trunk activation is zero, so that whole tiles of a live launch take the zero-tile exponent path
    in the forward and the backward pass) cannot come from the band weights, which hold for the whole launch as in the
    `small_allmasked` golden.  It comes from the weights: the x column of the two layers that read the encoding is made
    -(DEAD_GAIN + |w|) and the biases of the layers behind the first -DEAD_BIAS |b| (small, or the live rays would thin out layer by
    layer), and the dead ray starts at x = DEAD_X.  Its first and
    its skip layer are then negative in every unit, the layers between see zero inputs under non-positive biases; the live
    rays (|x| < 4) keep pre-activations of either sign."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    from upnerf_amd.rendering import band_weights
    R, S = c.R, c.S
    kw = dict(D=c.D, W=c.W, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    sd = synth.nerf_state("coarse", seed=c.seed, **kw)
    o = gen((R, 3), 70) * 0.3
    if c.dead is not None:
        for l in range(c.D):
            if l == 0 or l in (4,):  # (nerf_state's skips)
                w = sd[f"xyz_encoding_{l + 1}.0.weight"]
                w[:, 0] = -(DEAD_GAIN + w[:, 0].abs())
            if l > 0:
                sd[f"xyz_encoding_{l + 1}.0.bias"] = -DEAD_BIAS * sd[f"xyz_encoding_{l + 1}.0.bias"].abs()
        o[c.dead] = torch.tensor([DEAD_X, 0.1, -0.2])
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(sd)
    d = torch.nn.functional.normalize(gen((R, 3), 71), dim=-1)
    z = torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values
    scale = torch.logspace(-3, 2, R).reshape(R, 1)  # per-ray magnitudes of the side inputs span 5 decades
    c_rows, a_rows = gen((R, 16), 73) * scale, gen((R, 48), 74) * scale.flip(0)
    c2f = (0.1, 0.5) if c.frac else None
    return dict(model=model, o=o.contiguous(), d=d.contiguous(), z=z.contiguous(), a_rows=a_rows, c_rows=c_rows,
                use_cand=c.use_cand, use_rgb=c.use_rgb, mode=c.mode, rgb_joint=False, dead=c.dead,
                wk_xyz=band_weights(10, 0.28, c2f), wk_dir=band_weights(4, 0.28, c2f))


@lru_cache(maxsize=2)
def load(key):
    """The `s` dict of a case: key = a Synth, or (golden name, "coarse" | "fine").  `s["key"]` names it for reference()."""
    s = synth_pass(key) if isinstance(key, Synth) else setup_pass(Case(key[0]), key[1])
    s["key"] = key
    return s


def label(key):
    return synth_id(key) if isinstance(key, Synth) else f"{key[0]} {key[1]}"


# ------------------------------------------------------------------------------------------ the restatement's side
def round16(t):
    """t with every element rounded to fp16, derivative 1."""
    return t + (t.detach().float().half().to(t.dtype) - t).detach()


def restate(s, dtype, quant=None):
    """Kernel-space forward of pass `s` in `dtype` on the CPU with every pre-activation kept, random upstream gradients (the
    same fp32 draws whatever the dtype), backward.  Returns the leaves, the stage dicts and the upstream gradients.
    quant: kernel_space.field's (round16: what the "f16" mode's arithmetic alone does to this draw)."""
    model, pk = s["model"], s["model"].packer
    arg32 = dtype != torch.float32
    leaf = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)
    P = leaf(model.packed())
    o, d, c_rows, a_rows = leaf(s["o"]), leaf(s["d"]), leaf(s["c_rows"]), leaf(s["a_rows"])
    z = s["z"].to(dtype)
    aux = ks.ray_aux(d.detach(), a_rows, s["wk_dir"], arg32=arg32)
    f = ks.field(P, pk, o, d, z, c_rows, aux, s["wk_xyz"], s["use_cand"], s["use_rgb"], keep_pre=True, arg32=arg32, quant=quant)
    out = ks.composite(f, z, s["mode"], s["use_rgb"], pk.W)
    names = OUT_NAMES[:9] + (OUT_NAMES[9:] if s.get("rgb_joint") else [])
    ups = {n: gen(tuple(out[n].shape), 50 + i) for i, n in enumerate(names) if n in out}
    sum((out[n] * ups[n].to(dtype)).sum() for n in ups).backward()
    return SimpleNamespace(P=P, o=o, d=d, c_rows=c_rows, a_rows=a_rows, aux=aux, f=f, out=out, ups=ups, names=names)


@lru_cache(maxsize=2)
def _reference(key, dtype):
    return restate(load(key), dtype)


def reference(s, dtype):
    """restate(s, dtype), computed once per case and shared by the tests (and field modes) that compare against it."""
    return _reference(s["key"], dtype) if "key" in s else restate(s, dtype)


def param_pieces(s):
    """name -> (offset, length) of every parameter block the pass's heads write a gradient for."""
    pk = s["model"].packer
    L, W, W2 = pk.L, pk.W, pk.W2
    pieces = {"w0": (L.w[0], W * 64), "b0": (L.b[0], W), "we": (L.we, W * W), "be": (L.be, W), "wsig": (L.wsig, W),
              "bsig": (L.bsig, 1)}
    for l in range(1, pk.D):
        pieces[f"w{l}"] = (L.w[l], W * (64 + W if l == pk.skip else W))
        pieces[f"b{l}"] = (L.b[l], W)
    if s["use_cand"]:
        pieces.update(wc1=(L.wc1, W2 * (W + 16)), bc1=(L.bc1, W2), wc2=(L.wc2, W2 * W2), bc2=(L.bc2, W2),
                      wcsig=(L.wcsig, W2), bcsig=(L.bcsig, 1))
    if s["use_rgb"]:
        pieces.update(wr1=(L.wr1, W2 * (W + 80)), br1=(L.br1, W2), wr2=(L.wr2, 3 * W2), br2=(L.br2, 3))
    return pieces


def ref_stages(ref, s):
    """What the stage comparison reads off a restatement, by the tags it reports: acts {tag: (tensor, kind)} with kind "x0" (gate
    TOL_X0), "act" (TOL_ACT); grads {tag: tensor} (TOL_GRAD); masks {tag: (tensor, by_zero)} (the ReLU decisions of a layer)."""
    f, D = ref.f, s["model"].packer.D
    acts = {"x0": (f["x0"], "x0")}
    masks = {}
    for l in range(D):
        acts[f"h{l}"] = (f["h"][l], "act")
        masks[f"h{l}"] = (f["h"][l], False)
    acts["sigma_s"], acts["e"] = (f["sigma_s"], "act"), (f["e"], "act")
    if s["use_cand"]:
        for k in ("g1", "g2", "sigma_c"):
            acts[k] = (f[k], "act")
    if s["use_rgb"]:
        acts["aux"] = (ref.aux, "x0")
        for k in ("r1", "rgb"):
            acts[k] = (f[k], "act")
    for n in ref.names:
        if n in ref.out:
            acts["out_" + n] = (ref.out[n], "act")
    grads = {"dpre_s": f["pre_sig_s"].grad}
    for l in range(D):
        grads[f"gz_h{l}"] = f["pre_h"][l].grad
        masks[f"gz_h{l}"] = (f["pre_h"][l].grad, True)
    grads["gz_e"] = f["e"].grad
    if s["use_cand"]:
        grads.update(dpre_c=f["pre_sig_c"].grad, gz_g2=f["pre_g2"].grad, gz_g1=f["pre_g1"].grad, d_c_rows=ref.c_rows.grad)
    if s["use_rgb"]:
        grads.update(dpre_rgb=f["pre_rgb"].grad, gz_r1=f["pre_r1"].grad, d_a_rows=ref.a_rows.grad)
    grads.update(d_o=ref.o.grad, d_d=ref.d.grad)
    for k, (off, n) in param_pieces(s).items():
        grads["dP_" + k] = ref.P.grad[off:off + n]
    return acts, grads, masks


def mask_diff(got, ref, M, by_zero):
    """(share of differing ReLU decisions, worst share within one sample row): `by_zero` compares zero patterns (gradients: a
    masked element is an exact zero on both sides), otherwise signs of the stored activations."""
    g, r = got.detach().cpu().reshape(M, -1), ref.detach().reshape(M, -1)
    diff = ((g != 0) != (r != 0)) if by_zero else ((g > 0) != (r > 0))
    return float(diff.float().mean()), float(diff.float().mean(1).max())


# ------------------------------------------------------------------------------------------ the comparison body
def check_field_pass(hip, s, field_mode, ref_dtype, tag=""):
    """One training pass of `s` (a dict of setup_pass / synth_pass) through rendering._FieldPass under rendering.FIELD_MODE =
    field_mode (the caller has set it) against the restatement in `ref_dtype`: every stored stage of the forward pass, the
    outputs, every pre-activation gradient the backward pass exposes, the gradients of the ray inputs and of every parameter
    block, and the ReLU decisions of every trunk layer in both passes.  Prints each measured figure beside its gate."""
    cpu = lambda t: t.detach().cpu()
    f16 = field_mode == "f16"
    tol_act, tol_grad, tol_x0 = (TOL_ACT_F16, TOL_GRAD_F16, TOL_X0_F16) if f16 else (TOL_ACT, TOL_GRAD, TOL_X0)
    rd = hip["rendering"]
    model, pk = s["model"], s["model"].packer
    R, S = s["z"].shape
    # ---- CPU: kernel-space forward with every pre-activation kept, random upstream gradients
    ref = reference(s, ref_dtype)
    acts, grads, ref_masks = ref_stages(ref, s)
    names, ups = ref.names, ref.ups

    # ---- GPU
    model_g = model.cuda()
    P_g = model_g.packed().detach().clone().requires_grad_(True)
    assert rel_err(cpu(P_g), ref.P.detach()) < 1e-6
    o_g, d_g = s["o"].cuda().requires_grad_(True), s["d"].cuda().requires_grad_(True)
    c_g, a_g = s["c_rows"].cuda().requires_grad_(True), s["a_rows"].cuda().requires_grad_(True)
    cfg = rd._PassCfg(pk, s["mode"], s["use_cand"], s["use_rgb"], s["wk_xyz"], s["wk_dir"], rgb_joint=s.get("rgb_joint", False))
    outs = rd._FieldPass.apply(o_g, d_g, s["z"].cuda(), c_g, a_g, P_g, cfg)
    node = next(t.grad_fn for t in outs if t.grad_fn is not None)
    sv = node.saved
    M = R * S
    errs, seen, masks = {}, {}, {}

    def cmp(tag, got, ref_t, tol):
        g, r = cpu(got).reshape(-1).double(), ref_t.detach().reshape(-1).double()
        e = rel_err(g, r)
        if f16 and tol == tol_grad:  # gradients in the fp16 mode: relative L2 + a cap on single entries
            l2 = float((g - r).norm() / r.norm().clamp_min(1e-30))
            ok_ = l2 < tol and e < TOL_GRAD_F16_MAX
            e = l2
        else:
            ok_ = e < tol
        seen[tag] = (float(f"{e:.3g}"), tol)
        if not ok_:
            errs[tag] = float(f"{e:.3g}")
        return ok_

    def act(tag, got):
        r, kind = acts[tag]
        return cmp(tag, got, r, tol_x0 if kind == "x0" and tag == "x0" else TOL_X0 if kind == "x0" else tol_act)

    def mask_cmp(tag, got):
        r, by_zero = ref_masks[tag]
        share, worst_row = mask_diff(got, r, M, by_zero)
        masks[tag] = (float(f"{share:.2e}"), float(f"{worst_row:.2e}"))
        lim, lim_row = (MASK_FLIP_F16, MASK_FLIP_ROW_F16) if f16 else (MASK_FLIP, MASK_FLIP_ROW)
        if not (share <= lim and worst_row <= lim_row):
            errs["mask_" + tag] = masks[tag]
            return False
        return True

    def report(what):
        worst = {}
        for k, (e, tol) in seen.items():
            worst[k] = f"{e:.2g}/{tol:g}"
        print(f"[stages {what}] {tag} {field_mode} vs {str(ref_dtype)[6:]}: " + " ".join(f"{k}={v}" for k, v in worst.items()))
        seen.clear()

    ok = True
    ok &= act("x0", sv["x0"])
    # f16 mode stores fp16 tiles + exponents (the register-resident kernels: operand fragments, one exponent per 32 rows)
    hs = sv["h"] if sv.get("h16") is None else rd.dequant16(sv["h16"], sv["hexp"], frag=getattr(node, "rr", False))[:, :M]
    for l in range(pk.D):
        ok &= act(f"h{l}", hs[l])
        ok &= mask_cmp(f"h{l}", hs[l])
    if sv.get("h16") is not None and sv.get("h") is not None:  # (the register-resident kernels keep no fp32 copy)
        ok &= cmp("h_last_fp32", sv["h"][0], acts[f"h{pk.D - 1}"][0], tol_act)
    ok &= act("sigma_s", sv["sigma_s"])
    e_got = sv["e"] if sv.get("e") is not None else rd.dequant16(sv["e16"][None], sv["eexp"][None], frag=True)[0, :M]  # (rr: fragments only)
    ok &= act("e", e_got)
    def stored(k):  # (rr: g2 / r1 may be held as fp16 fragments only)
        return sv[k] if sv.get(k) is not None else rd.dequant16(sv[k + "_16"][None], sv[k + "exp"][None], frag=True)[0, :M]
    if s["use_cand"]:
        for k in ("g1", "g2", "sigma_c"):
            ok &= act(k, stored(k))
    if s["use_rgb"]:
        ok &= act("aux", sv["aux"])
        for k in ("r1", "rgb"):
            ok &= act(k, stored(k))
    for i, n in enumerate(names):
        if n in ref.out:
            ok &= act("out_" + n, outs[i])
    report("fwd")
    assert ok, "FWD over tolerance: " + repr(errs)

    # ---- backward
    sink = {}
    rd._DEBUG_SINK = sink
    try:
        sum((outs[i] * ups[n].cuda()).sum() for i, n in enumerate(names) if n in ups).backward()
    finally:
        rd._DEBUG_SINK = None
    got = {"dpre_s": sink["dpre_s"], "gz_e": sink["gz_e"], "d_o": o_g.grad, "d_d": d_g.grad}
    for l in range(pk.D):
        got[f"gz_h{l}"] = sink["gz_h"][l]
    if s["use_cand"]:
        got.update(dpre_c=sink["dpre_c"], gz_g2=sink["gz_g2"], gz_g1=sink["gz_g1"], d_c_rows=c_g.grad)
    if s["use_rgb"]:
        got.update(dpre_rgb=sink["dpre_rgb"][:, :3], gz_r1=sink["gz_r1"], d_a_rows=a_g.grad)
    for k, (off, n) in param_pieces(s).items():
        got["dP_" + k] = P_g.grad[off:off + n]
    assert set(got) == set(grads)
    ok = True
    for k, r in grads.items():
        ok &= cmp(k, got[k], r, tol_grad)
        if k in ref_masks:
            ok &= mask_cmp(k, got[k])
    print(f"[masks] {tag} {field_mode}: worst share {max(v[0] for v in masks.values()):.1e}, worst row {max(v[1] for v in masks.values()):.1e}")
    report("bwd")
    assert ok, "BWD over tolerance: " + repr(errs)
