"""The fused field pass against the torch restatement (tests/kernel_space.py), stage by stage: the inputs of a pass (golden cases
and synthetic edge cases), the restatement's reference in fp32 or fp64, and the comparison bodies the GPU tests share: check_field_pass
(the full training pass), check_forward_only and check_partial_backward (the plans outside it).  Importable without a GPU; only
those three touch a device.

An fp64 reference starts where the kernels start (kernel_space.field(arg32=True): sample positions and encoding arguments as fp32
arithmetic gives them) and runs everything behind x0 -- trunk, heads, softplus / sigmoid, compositing, autograd -- in fp64."""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import pytest
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
# bare: the pass gets no per-ray rows at all (c_rows = a_rows = None), see density_only.  vivid: a colour head whose colour
# varies along a ray, see VIVID_GAIN.
Synth = namedtuple("Synth", "W D R S mode use_cand use_rgb seed frac dead bare vivid", defaults=(3, False, None, False, False))
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
# Where rgb_map is the only output with an upstream gradient, the density receives delta_i (T_{i+1} c_i - sum_{j>i} w_j c_j) . g:
# the last sample of a ray is opaque (delta = 1e2), the weights of a ray sum to one, and the bracket is what the colour VARIES by
# along the ray.  Under nerf_state's weights the colour is all but constant along a ray (the per-ray inputs dominate the head), the
# bracket is the rounding of its two terms, and the density head's gradient from fp32 arithmetic -- the restatement's as much as
# the kernels' -- lies 3e-4 to 3e-3 from the fp64 one.  Such a draw gates nothing; a vivid case scales the columns of the colour
# head's first layer that read the field's feature (fp32 against fp64 then: 1.2e-5 at the worst).  The second layer stays as it is:
# a gain there saturates the sigmoid, and samples whose gradient is 1e-18 of their tile's largest are an exact zero under a shared
# exponent per tile (gains 30 and 10 on 7 x 40: the zero patterns of gz_h then differ in 7% of the elements; here the smallest
# sample row of any tile keeps 1.5e-6 of the tile's largest).
VIVID_GAIN = 300.0


def density_only(c):
    """The pass render_rays(coarse_sigma_only=True) runs over the samples of `c`: mode 2, neither head, no per-ray rows; its
    outputs are s_depth and w_s.  Weights, rays and depths are those of `c` (a dead ray stays dead: the trunk alone decides that)."""
    return c._replace(mode=2, use_cand=False, use_rgb=False, bare=True)


# 7 x 40, 3 x 200 (the dead ray; S no multiple of 32), 2 x 257, and the 64-wide 5 x 33
DENSITY_ONLY = [density_only(c) for c in (SYNTH_256[1], SYNTH_256[3], SYNTH_256[4], SYNTH_64[0])]


def synth_id(c):
    return (f"w{c.W}-{c.R}x{c.S}-m{c.mode}" + ("c" if c.use_cand else "") + ("r" if c.use_rgb else "")
            + ("-frac" if c.frac else "") + ("-dead" if c.dead is not None else "") + ("-bare" if c.bare else "") + ("-vivid" if c.vivid else "") + (f"-seed{c.seed}" if c.vivid and c.seed not in (3, 8) else ""))


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
    if c.vivid:
        sd["rgb_share_layer.0.weight"][:, :kw["feat_dim"]] *= VIVID_GAIN
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
    if c.bare:
        c_rows = a_rows = None
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


def restate(s, dtype, quant=None, ups=None):
    """Kernel-space forward of pass `s` in `dtype` on the CPU with every pre-activation kept, random upstream gradients (the
    same fp32 draws whatever the dtype), backward.  Returns the leaves, the stage dicts and the upstream gradients.
    quant: kernel_space.field's (round16: what the "f16" mode's arithmetic alone does to this draw).
    ups: the names of the outputs that receive an upstream gradient (None: all of them); an output's draw depends on its index
    alone, so it is the same under every subset.  Every leaf requires a gradient whatever a caller goes on to read: what one leaf
    receives does not depend on which others ask, and a leaf (or pre-activation) the upstreams do not reach keeps .grad None."""
    model, pk = s["model"], s["model"].packer
    arg32 = dtype != torch.float32
    leaf = lambda t: None if t is None else t.detach().cpu().to(dtype).clone().requires_grad_(True)
    P = leaf(model.packed())
    o, d, c_rows, a_rows = leaf(s["o"]), leaf(s["d"]), leaf(s["c_rows"]), leaf(s["a_rows"])
    z = s["z"].to(dtype)
    aux = ks.ray_aux(d.detach(), a_rows, s["wk_dir"], arg32=arg32)
    f = ks.field(P, pk, o, d, z, c_rows, aux, s["wk_xyz"], s["use_cand"], s["use_rgb"], keep_pre=True, arg32=arg32, quant=quant)
    out = ks.composite(f, z, s["mode"], s["use_rgb"], pk.W)
    names = OUT_NAMES[:9] + (OUT_NAMES[9:] if s.get("rgb_joint") else [])
    assert ups is None or (len(ups) and all(n in names and n in out for n in ups)), (ups, sorted(out))
    ups = {n: gen(tuple(out[n].shape), 50 + i) for i, n in enumerate(names) if n in out and (ups is None or n in ups)}
    sum((out[n] * ups[n].to(dtype)).sum() for n in ups).backward()
    return SimpleNamespace(P=P, o=o, d=d, c_rows=c_rows, a_rows=a_rows, aux=aux, f=f, out=out, ups=ups, names=names)


@lru_cache(maxsize=4)  # (fp32 and fp64 of the pair in hand, and of the one before it)
def _reference(key, dtype, ups):
    return restate(load(key), dtype, ups=ups)


def reference(s, dtype, ups=None):
    """restate(s, dtype, ups=ups), computed once per case and subset of upstreams and shared by the tests (and field modes) that
    compare against it."""
    ups = None if ups is None else tuple(n for n in OUT_NAMES if n in ups)
    return _reference(s["key"], dtype, ups) if "key" in s else restate(s, dtype, ups=ups)


# ------------------------------------------------------------------------------------------ the plans outside the full training pass
# Backward variants: the leaves that require a gradient (of o, d, c_rows, a_rows, P; c_rows counts only where the candidate head
# runs, a_rows only where the colour head does -- elsewhere the pass does not read them) and the outputs that get an upstream
# gradient (None: all).  `on`: the cases a variant applies to, by (mode, use_cand, use_rgb).
LEAVES = ("o", "d", "c_rows", "a_rows", "P")
Variant = namedtuple("Variant", "leaves ups on")
VARIANTS = {
    "weights_only": Variant(("P",), lambda mode: None, lambda mode, cand, rgb: True),                     # need_dxyz = 0
    "frozen_appearance": Variant(("a_rows",), lambda mode: ("rgb_map",), lambda mode, cand, rgb: rgb),       # dP is None, need_dxyz = 0
    "frozen_pose": Variant(("o", "d", "a_rows"), lambda mode: ("rgb_map",), lambda mode, cand, rgb: rgb),    # dP is None
    "frozen_candidate": Variant(("c_rows",), lambda mode: ("G_c", "t_weight"), lambda mode, cand, rgb: cand),
    "colour_loss_only": Variant(LEAVES, lambda mode: ("rgb_map",), lambda mode, cand, rgb: rgb),             # g_E_s, g_G_c NULL
    "feature_loss_only": Variant(LEAVES, lambda mode: ("E_s", "sum_sfeat") + (("G_c", "t_weight") if mode <= 1 else ()),
                                 lambda mode, cand, rgb: mode != 2),                                         # g_rgb_map NULL
}
MODES = ["f16x3", "f32", "f16"]


def traits(key):
    """(mode, use_cand, use_rgb) of a case without loading it (a NOFEAT golden: mode 1 with both heads, as load() then shows)."""
    return (key.mode, key.use_cand, key.use_rgb) if isinstance(key, Synth) else (1, True, True)


def variants_of(key):
    return [v for v, d in VARIANTS.items() if d.on(*traits(key))]


def variant_leaves(variant, s):
    return tuple(n for n in VARIANTS[variant].leaves if not (n == "c_rows" and not s["use_cand"]) and not (n == "a_rows" and not s["use_rgb"]))


def variant_ups(variant, s):
    return VARIANTS[variant].ups(s["mode"])


# Which case runs in which field mode: 256-wide fields of at least 32 samples a ray in all three; the smallest pass in the two
# that accept it (the f16 mode refuses it); 64-wide fields run the fp32 kernels whatever the mode, so once.
PLAN_CASES = SYNTH_256 + [SYNTH_SMALLEST] + SYNTH_64 + NOFEAT


def modes_of(key):
    if key in SYNTH_64 or key == NOFEAT[0] or (isinstance(key, Synth) and key.W != 256):
        return MODES[:1]
    return MODES[:2] if (isinstance(key, Synth) and key.S < 32) else MODES


FORWARD_RUNS = [(k, m) for k in PLAN_CASES for m in modes_of(k)]
DENSITY_RUNS = [(k, m) for k in DENSITY_ONLY for m in modes_of(k)]
# colour_loss_only wants a colour that varies along the ray (VIVID_GAIN): the synthetic cases get one.  The two feature-less goldens
# cannot be drawn again (fp32 restatement against fp64 on their density head under that variant: 2.9e-4 and 1.7e-4 of TOL_GRAD =
# 1e-4, which no fp32 kernel could meet either) and run every other variant.
# (The one-tile case under its own seed 3 as well: fp16 operands alone then leave the first layer's weight gradient 5.9e-2 from the
# fp64 one, at the f16 gate of 6e-2, and the f16 kernels measured 5.9e-2 too.  Seed 9: 1.3e-2.)
def vivid(k):
    return k._replace(vivid=True, seed=9 if k == SYNTH_256[0] else k.seed)


BACKWARD_PAIRS = [(vivid(k) if v == "colour_loss_only" else k, v) for k in PLAN_CASES for v in variants_of(k)
                  if not (v == "colour_loss_only" and k in NOFEAT)]
BACKWARD_RUNS = [(k, v, m) for k, v in BACKWARD_PAIRS for m in modes_of(k)]
CAND_BLOCKS, RGB_BLOCKS = ("wc1", "bc1", "wc2", "bc2", "wcsig", "bcsig"), ("wr1", "br1", "wr2", "br2")


def unreached(s, ups):
    """The gradient tags of pass `s` that no output of `ups` depends on.  The candidate head feeds the joint density only, which
    every output but s_depth, w_s and rgb_map (composited under the shared density alone) reads; the colour head feeds rgb_map and
    rgb_joint_map only.  The restatement leaves such a leaf's .grad None and such a parameter block zero; the kernels have to
    return an exact zero (or nothing) for them, which the gates then ask by themselves: a zero reference passes nothing else."""
    if ups is None:
        return set()
    out = set()
    if s["use_cand"] and not set(ups) - {"s_depth", "w_s", "rgb_map"}:
        out |= {"d_c_rows"} | {"dP_" + k for k in CAND_BLOCKS}
    if s["use_rgb"] and not set(ups) & {"rgb_map", "rgb_joint_map"}:
        out |= {"d_a_rows"} | {"dP_" + k for k in RGB_BLOCKS}
    return out


def ref_grads(ref, s, leaves):
    """{tag: tensor} of the gradients the leaves `leaves` receive in the restatement `ref`: d_o, d_d, d_c_rows, d_a_rows and one
    dP_<block> per block of param_pieces; a leaf the upstreams do not reach reads as zeros."""
    g = {}
    for n in leaves:
        t = getattr(ref, n)
        grad = t.grad if t.grad is not None else torch.zeros_like(t)
        if n == "P":
            g.update({"dP_" + k: grad[off:off + ln] for k, (off, ln) in param_pieces(s).items()})
        else:
            g["d_" + n] = grad
    return g


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


# ------------------------------------------------------------------------------------------ the other plans' comparison bodies
class _Gates:
    """check_field_pass's comparisons for the bodies below: the same figures under the same gates, by kind -- "x0" (TOL_X0, f16:
    TOL_X0_F16), "aux" (TOL_X0 in every mode), "act" (TOL_ACT), "grad" (TOL_GRAD; f16: relative L2 under TOL_GRAD_F16 and the
    single-entry cap) -- and the limits on differing ReLU decisions."""

    def __init__(self, field_mode, M):
        self.f16, self.M = field_mode == "f16", M
        act, grad, x0 = (TOL_ACT_F16, TOL_GRAD_F16, TOL_X0_F16) if self.f16 else (TOL_ACT, TOL_GRAD, TOL_X0)
        self.tol = {"x0": x0, "aux": TOL_X0, "act": act, "grad": grad}
        self.errs, self.seen, self.masks, self.worst = {}, {}, {}, {}

    def cmp(self, tag, got, ref_t, kind):
        g, r = got.detach().cpu().reshape(-1).double(), ref_t.detach().reshape(-1).double()
        assert g.shape == r.shape, (tag, tuple(got.shape), tuple(ref_t.shape))
        e, tol = rel_err(g, r), self.tol[kind]
        gate = kind
        if self.f16 and kind == "grad":  # gradients in the fp16 mode: relative L2 + a cap on single entries
            self.worst["grad_max"] = max(self.worst.get("grad_max", 0.0), e)
            l2 = float((g - r).norm() / r.norm().clamp_min(1e-30))
            ok = l2 < tol and e < TOL_GRAD_F16_MAX
            e = l2
        else:
            ok = e < tol
        self.worst[gate] = max(self.worst.get(gate, 0.0), e)
        self.seen[tag] = (float(f"{e:.3g}"), tol)
        if not ok:
            self.errs[tag] = float(f"{e:.3g}")
        return ok

    def mask_cmp(self, tag, got, ref_t, by_zero):
        share, worst_row = mask_diff(got, ref_t, self.M, by_zero)
        self.masks[tag] = (float(f"{share:.2e}"), float(f"{worst_row:.2e}"))
        lim, lim_row = (MASK_FLIP_F16, MASK_FLIP_ROW_F16) if self.f16 else (MASK_FLIP, MASK_FLIP_ROW)
        if not (share <= lim and worst_row <= lim_row):
            self.errs["mask_" + tag] = self.masks[tag]
            return False
        return True

    def report(self, head):
        print(f"[{head}] " + " ".join(f"{k}={e:.2g}/{tol:g}" for k, (e, tol) in self.seen.items()))
        if "grad_max" in self.worst:
            print(f"[{head} single entry] {self.worst['grad_max']:.2g}/{TOL_GRAD_F16_MAX:g}")
        if self.masks:
            print(f"[{head} masks] worst share {max(v[0] for v in self.masks.values()):.1e}, "
                  f"worst row {max(v[1] for v in self.masks.values()):.1e}")
        self.seen.clear()


def _held(pp, plan, got, names):
    """Every buffer of `names` the plan lists is held in `got` with the planned shape and dtype on storage of at least the planned
    rows; every form the plan omits is None."""
    for k in names:
        shape, t = plan.buffers[k], got[k]
        if shape is None:
            assert t is None, (k, "allocated although the plan omits it")
            continue
        assert t is not None, k
        assert tuple(t.shape) == shape and t.dtype == getattr(torch, pp.DTYPES.get(k, "float32")), (k, tuple(t.shape), t.dtype)
        numel = 1
        for n in ((plan.Mp,) + shape[1:] if k in pp.PADDED else shape):
            numel *= n
        assert t.untyped_storage().nbytes() >= numel * t.element_size(), (k, shape, plan.Mp)


def _gpu_inputs(s, requires):
    """The leaves of pass `s` on the device, by name; those named in `requires` require a gradient.  A bare pass has no rows."""
    dev = lambda t: None if t is None else t.detach().cuda().clone()
    leaves = dict(o=dev(s["o"]), d=dev(s["d"]), c_rows=dev(s["c_rows"]), a_rows=dev(s["a_rows"]),
                  P=s["model"].cuda().packed().detach().clone())
    for n in requires:
        leaves[n].requires_grad_(True)
    return leaves


def _apply(rd, s, leaves):
    """_FieldPass on `leaves` under the grad mode in force (the pass's configuration records it)."""
    cfg = rd._PassCfg(s["model"].packer, s["mode"], s["use_cand"], s["use_rgb"], s["wk_xyz"], s["wk_dir"],
                      rgb_joint=s.get("rgb_joint", False))
    return rd._FieldPass.apply(leaves["o"], leaves["d"], s["z"].cuda(), leaves["c_rows"], leaves["a_rows"], leaves["P"], cfg)


def check_forward_only(hip, s, field_mode, ref_dtype, tag=""):
    """The forward-only plan (train=False: what every validation image, metric, camera-path frame, mesh colour and baked scene
    runs) of pass `s` under rendering.FIELD_MODE = field_mode (the caller has set it), reached by both routes -- no_grad around
    leaves that require a gradient, and grad mode with no such leaf -- against the restatement in `ref_dtype`, against its plan,
    and against the forward of the training pass on the same inputs.  The pass leaves no graph node behind, so rendering._plan and
    rendering._alloc are wrapped for the duration of the call to hand over the plan and the buffers."""
    rd, pp = hip["rendering"], hip["pass_plan"]
    pk = s["model"].packer
    R, S = s["z"].shape
    M = R * S
    names = OUT_NAMES
    all_leaves =[n for n in LEAVES if n == "P" or s[n] is not None]
    planned, allocs = [], []
    real_plan, real_alloc = rd._plan, rd._alloc

    def plan_rec(*a, **kw):
        p = real_plan(*a, **kw)
        planned.append((a, kw, p))
        return p

    def alloc_rec(plan, stage, dev):
        b = real_alloc(plan, stage, dev)
        allocs.append((plan, stage, b))
        return b

    def route(grad, requires):
        del planned[:], allocs[:]
        with torch.set_grad_enabled(grad):
            outs = _apply(rd, s, _gpu_inputs(s, requires))
        torch.cuda.synchronize()
        assert all(t.grad_fn is None and not t.requires_grad for t in outs)
        assert [st for _, st, _ in allocs] == ["aux", "field", "composite"], [st for _, st, _ in allocs]
        plan = allocs[0][0]
        assert all(p is plan for p, _, _ in allocs)
        made = [(a, kw) for a, kw, p in planned if p is plan]
        assert len(made) == 1
        a, kw = made[0]
        assert (a[7] if len(a) > 7 else kw.get("train", False)) is False, "the pass planned a training pass"
        buf = {}
        for _, _, b in allocs:
            buf.update(b)
        return plan, buf, outs

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rd, "_plan", plan_rec)
        mp.setattr(rd, "_alloc", alloc_rec)
        plan, buf, outs = route(False, all_leaves)
        plan_b, buf_b, outs_b = route(True, ())
    assert rd._plan is real_plan and rd._alloc is real_alloc
    want = real_plan(pk, R, S, s["mode"], s["use_cand"], s["use_rgb"], s.get("rgb_joint", False), False)
    assert plan == want and plan_b == want
    for k in ("h", "hmask", "mx32", "h16", "hexp", "g1", "g1_16", "r1", "r1_16"):  # (what only a backward pass reads)
        assert plan.buffers[k] is None, k
    stages = pp.STAGES["aux"] + pp.STAGES["field"] + pp.STAGES["composite"]
    for b, o_ in ((buf, outs), (buf_b, outs_b)):
        assert set(b) == set(stages)
        _held(pp, plan, b, stages)
        for k, t in zip(names, o_):  # (an output the pass does not have comes back as an empty tensor)
            assert (t.numel() == 0) if plan.buffers[k] is None else (t.data_ptr() == b[k].data_ptr() and t.shape == b[k].shape), k
    for k, a, b in zip(names, outs, outs_b):
        assert torch.equal(a, b), ("the two routes to the forward-only plan differ", k)

    # ---- against the restatement
    ref = reference(s, ref_dtype)
    acts = ref_stages(ref, s)[0]
    gt = _Gates(field_mode, M)
    deq = lambda k: rd.dequant16(buf[k + "16" if k == "e" else k + "_16"][None], buf[k + "exp"][None], frag=True)[0, :M]
    ok = gt.cmp("x0", buf["x0"], acts["x0"][0], "x0")
    if s["use_rgb"]:
        ok &= gt.cmp("aux", buf["aux"], acts["aux"][0], "aux")
        ok &= gt.cmp("rgb", buf["rgb"], acts["rgb"][0], "act")
    ok &= gt.cmp("sigma_s", buf["sigma_s"], acts["sigma_s"][0], "act")
    if s["use_cand"]:
        ok &= gt.cmp("sigma_c", buf["sigma_c"], acts["sigma_c"][0], "act")
    for k in ("e", "g2"):
        rows, frag = plan.buffers[k], plan.buffers[k + "16" if k == "e" else k + "_16"]
        if rows is not None or frag is not None:
            ok &= gt.cmp(k, buf[k] if rows is not None else deq(k), acts[k][0], "act")
    n_out = 0
    for i, n in enumerate(ref.names):
        if n in ref.out:
            ok &= gt.cmp("out_" + n, outs[i], ref.out[n], "act")
            n_out += 1
    assert n_out == sum(t.numel() > 0 for t in outs)  # every output the pass returns was compared
    gt.report(f"forward-only {tag} {field_mode} vs {str(ref_dtype)[6:]}")
    assert ok, "forward-only pass over tolerance: " + repr(gt.errs)

    # ---- against the forward of the training pass
    outs_t = _apply(rd, s, _gpu_inputs(s, all_leaves))
    plan_t = next(t.grad_fn for t in outs_t if t.grad_fn is not None).plan
    torch.cuda.synchronize()
    forms = lambda p: (p.e_frag, p.buffers["g2_16"] is not None)
    if not gt.f16 or forms(plan_t) == forms(plan):
        for k, a, b in zip(names, outs, outs_t):
            assert torch.equal(a, b.detach()), ("the forward-only pass and the training forward differ", k)
        same = True
    else:  # the forward-only plan hands compositing fp16 fragments of e / g2 where the training plan keeps fp32 rows
        for i, n in enumerate(ref.names):
            if n in ref.out:
                ok &= gt.cmp("train_out_" + n, outs_t[i], ref.out[n], "act")
        gt.report(f"forms differ (e_frag, g2 fragments: forward-only {forms(plan)}, training {forms(plan_t)}) {tag} {field_mode}: "
                  "training forward")
        assert ok, "training forward over tolerance: " + repr(gt.errs)
        same = False
    return dict(worst=gt.worst, same_forms=same)


WGRAD_ENTRIES = ("upnerf_wgrad16", "upnerf_wgrad", "upnerf_vec_wgrad", "upnerf_vec_wgrad_frag16", "upnerf_scale_exponents")


def check_partial_backward(hip, s, variant, field_mode, ref_dtype, tag=""):
    """A backward pass of `s` outside the full training pass (VARIANTS: some leaves frozen, some outputs unread by the loss) under
    rendering.FIELD_MODE = field_mode against the restatement in `ref_dtype`: every requested gradient (and, where P is one,
    every parameter block and the ReLU decisions of the trunk's gradients) under check_field_pass's gates; no gradient for a leaf
    that did not ask; no weight-gradient launch where P did not ask; the same bits on a second run."""
    rd, lib = hip["rendering"], hip["lib"].lib
    pk = s["model"].packer
    R, S = s["z"].shape
    M = R * S
    leaves_v, ups_v = variant_leaves(variant, s), variant_ups(variant, s)
    ref = reference(s, ref_dtype, ups_v)
    want = ref_grads(ref, s, leaves_v)
    assert set(ref.ups) == (set(ups_v) if ups_v is not None else {n for n in ref.names if n in ref.out})

    def run():
        leaves = _gpu_inputs(s, leaves_v)
        outs = _apply(rd, s, leaves)
        calls = dict.fromkeys(WGRAD_ENTRIES, 0)
        real = {k: getattr(lib, k) for k in WGRAD_ENTRIES}

        def counted(k):
            def f(*a):
                calls[k] += 1
                return real[k](*a)
            return f

        sink = {}
        rd._DEBUG_SINK = sink
        for k in WGRAD_ENTRIES:
            setattr(lib, k, counted(k))
        try:
            sum((outs[i] * ref.ups[n].cuda()).sum() for i, n in enumerate(ref.names) if n in ref.ups).backward()
        finally:
            for k in WGRAD_ENTRIES:
                setattr(lib, k, real[k])
            rd._DEBUG_SINK = None
        torch.cuda.synchronize()
        for n, t in leaves.items():
            if t is not None and n not in leaves_v:
                assert t.grad is None, (n, "got a gradient it did not ask for")
        got = {}
        for n in leaves_v:
            grad = leaves[n].grad
            if n == "P":
                assert grad is not None
                got.update({"dP_" + k: grad[off:off + ln] for k, (off, ln) in param_pieces(s).items()})
                got["P"] = grad
            else:
                assert grad is not None or "d_" + n in unreached(s, ups_v), n
                got["d_" + n] = grad if grad is not None else torch.zeros_like(leaves[n])
        return got, sink, calls

    got, sink, calls = run()
    if "P" in leaves_v:
        assert calls["upnerf_wgrad16"] + calls["upnerf_wgrad"] > 0, calls
    else:
        assert not any(calls.values()), ("a frozen field launched weight gradients", calls)
    gt = _Gates(field_mode, M)
    ok = True
    for k, r in want.items():
        ok &= gt.cmp(k, got[k], r, "grad")
    if "P" in leaves_v:
        for l in range(pk.D):
            ok &= gt.mask_cmp(f"gz_h{l}", sink["gz_h"][l], ref.f["pre_h"][l].grad, True)
    gt.report(f"{variant} {tag} {field_mode} vs {str(ref_dtype)[6:]}")
    assert ok, f"{variant}: over tolerance: " + repr(gt.errs)
    again, _, calls2 = run()
    assert calls2 == calls
    for k in got:
        assert torch.equal(got[k], again[k]), ("a second run gave other bits", k)
    return dict(worst=gt.worst)
