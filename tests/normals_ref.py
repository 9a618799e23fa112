"""fp64 restatement of what upnerf_density_grad computes, and numpy restatements of the rules of upnerf_normal_composite and
upnerf_viz_normals.  Shared by tests/test_normals_cpu.py and tests/test_hip_normals.py.

density: encoding -> trunk -> share_sigma -> softplus in fp64 from the fp32 points and parameters cast up; the gradient by
torch.autograd in fp64.  2^k * float32(pi) is exact in fp64, and so is its product with an fp32 x up to the final rounding:
the argument of sin / cos is NOT rounded to fp32 here (the kernels round it: part of their error).  Per point the reference
also reports the MARGIN of its ReLU decisions: the smallest |pre-activation| over all units and layers relative to that
unit's sum_k |w_k h_k| + |b|.  A point whose margin is below MARGIN_MIN may legitimately flip a decision in fp32, which is
another piecewise-linear branch of the function and not an error of the arithmetic."""
import numpy as np
import torch

PI32 = float(np.float32(np.pi))
MARGIN_MIN = 1e-5
XYZ_L = 10
C2F = (0.1, 0.5)

# (W, D, skip or None) of the issue, and the seed of each: chosen so that at most 2 % of the 257 points of every band schedule
# fall below MARGIN_MIN in the reference (test_normals_cpu.py checks it).
#
# What the 2 % costs.  A point with U data-dependent units is left out with a probability that grows with U: measured on the
# reference, dense random fields lose 0 - 2 % of their points at (64, 2), 1 - 2 % at (256, 1) and (64, 8) -- seeds decide -- and
# 11 - 14 % at the 2048 units of (256, 8, 4) (seeds 11 - 13: 29 - 35 of 257 points), where no seed gets under 2 %.  Two fields
# therefore stand for that shape:
#   * the fp64 case under the 2 % rule (LIVE): every layer keeps 24 data-dependent units, three in each of its eight 32-column
#     blocks (columns 32 b + 0, 1, 2: all four waves and both accumulator blocks of a wave hold some); the other 232 units get
#     a bias of -1000 and are off at every point, decisively (margin ~ 1);
#   * the DENSE field (make_field(..., dense=True)): plain random weights, every unit decides by the data, every entry of every
#     256 x 256 matrix multiplies non-zero data.  tests/test_hip_normals.py holds the fused kernel on it to the parent route
#     (same forward, bit for bit) and to fp64 on the points above the margin, whose share it states.
SHAPES = [(64, 2, None), (64, 8, 4), (256, 8, 4), (256, 1, None)]
SEEDS = {(64, 2, None): 11, (64, 8, 4): 11, (256, 8, 4): 11, (256, 1, None): 11}
LIVE = {(256, 8, 4): 24}
BANDS = ("ones", "zeros", "partial")
N_POINTS = 257
SIZES = (1, 63, 64, 65, 257)  # one point, tile - 1, one tile, tile + 1, tiles + 1 (the kernel's tile is 64 points)


def band_weights(kind):
    """The ten weights w_k: all one, all zero (only the identity block carries gradient), or BARF's schedule at progress 0.3."""
    if kind == "ones":
        return [1.0] * XYZ_L
    if kind == "zeros":
        return [0.0] * XYZ_L
    from upnerf_amd.rendering import band_weights as bw
    return bw(XYZ_L, float(np.float32(0.3)), C2F)


def live_columns(W, live):
    """The `live` data-dependent units of a layer: the first live / (W / 32) columns of every 32-column block."""
    per = live // (W // 32)
    return torch.tensor([j for j in range(W) if j % 32 < per])


def make_field(W, D, skip, seed, head_bias=0.0, dense=False):
    """state_dict (fp32, the reference's names) of a seeded field whose density is neither saturated nor dead over [-1, 1]^3.
    dense: plain random weights even for a shape that LIVE thins out."""
    from upnerf_amd import synth
    live = None if dense else LIVE.get((W, D, skip))
    # (fewer live units carry the signal: their weights are scaled up so that it does not die out layer by layer)
    gain = 2.5 if live is None else 2.5 * (W / live) ** 0.5
    sd = synth.nerf_state("fine", D=D, W=W, skips=(skip,) if skip is not None else (), seed=seed, sigma_bias=head_bias,
                          sigma_gain=4.0 if live is None else 4.0 * (W / live) ** 0.5, trunk_gain=gain)
    if live is not None:
        off = torch.ones(W, dtype=torch.bool)
        off[live_columns(W, live)] = False
        for l in range(D):
            sd[f"xyz_encoding_{l + 1}.0.bias"][off] = -1000.0
    return sd


HEAD_BIAS_CASE = ((64, 2, None), 30.0)  # a head bias that puts every pre-activation of the softplus above 20: its `x > 20` branch


def build_module(W, D, skip, sd):
    """upnerf_amd.nerf.NeRF holding the state `sd` (on the CPU)."""
    from upnerf_amd.nerf import NeRF
    m = NeRF("fine", D=D, W=W, skips=[skip] if skip is not None else [], xyz_L=XYZ_L, dir_L=4, c2f=C2F)
    m.load_state_dict(sd)
    return m


def make_points(seed, n=N_POINTS):
    """[n, 3] fp32 in [-1, 1)^3; point 0 has a coordinate that is exactly 0."""
    from upnerf_amd import synth
    p = synth.uniform("normals.points", (n, 3), seed).clone()
    p[0, 1] = 0.0
    return p


def encode(x, wk):
    """[M, 63] fp64: [x, w_k sin(2^k pi x_n), w_k cos(2^k pi x_n)], per coordinate n ten sines then ten cosines."""
    freq = torch.tensor([PI32 * 2.0 ** k for k in range(XYZ_L)], dtype=torch.float64)
    w = torch.tensor([float(np.float32(v)) for v in wk], dtype=torch.float64)
    arg = x[:, :, None] * freq                                   # [M, 3, L]
    enc = torch.stack([arg.sin() * w, arg.cos() * w], dim=2)     # [M, 3, 2, L]
    return torch.cat([x, enc.reshape(x.shape[0], -1)], 1)


def density(sd, points, wk, D, skip):
    """(sigma [M], grad [M, 3], margin [M]) in fp64 (numpy) at the fp32 `points`."""
    p = {k: v.detach().double() for k, v in sd.items()}
    x = points.detach().double().clone().requires_grad_(True)
    x0 = encode(x, wk)
    h = x0
    margin = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    for l in range(D):
        if skip is not None and l == skip:
            h = torch.cat([x0, h], 1)
        w, b = p[f"xyz_encoding_{l + 1}.0.weight"], p[f"xyz_encoding_{l + 1}.0.bias"]
        pre = h @ w.t() + b
        with torch.no_grad():
            scale = h.abs() @ w.abs().t() + b.abs()
            margin = torch.minimum(margin, (pre.abs() / scale).min(dim=1).values)
        h = torch.relu(pre)
    pre = h @ p["share_sigma.0.weight"].t() + p["share_sigma.0.bias"]
    sigma = torch.nn.functional.softplus(pre[:, 0], threshold=1e9)
    (grad,) = torch.autograd.grad(sigma.sum(), x)
    return sigma.detach().numpy(), grad.numpy(), margin.numpy(), pre[:, 0].detach().numpy()


def density_only(sd, points64, wk, D, skip):
    """(sigma [M] fp64, ReLU decisions [M, D * W] bool) at fp64 points (central differences of the restatement itself)."""
    p = {k: v.detach().double() for k, v in sd.items()}
    x0 = encode(points64, wk)
    h = x0
    on = []
    for l in range(D):
        if skip is not None and l == skip:
            h = torch.cat([x0, h], 1)
        h = torch.relu(h @ p[f"xyz_encoding_{l + 1}.0.weight"].t() + p[f"xyz_encoding_{l + 1}.0.bias"])
        on.append(h > 0)
    pre = h @ p["share_sigma.0.weight"].t() + p["share_sigma.0.bias"]
    return torch.nn.functional.softplus(pre[:, 0], threshold=1e9), torch.cat(on, 1)


def rel_err(got, ref):
    """max |got - ref| / max_i ||ref_i|| (rows of a [M, 3] gradient; |ref_i| for a vector)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max() if ref.ndim == 1 else np.sqrt((ref ** 2).sum(1)).max()
    return float(np.abs(got - ref).max() / scale)


# ---- upnerf_normal_composite ---------------------------------------------------------------------------------------------------

def composite_ref(grad, w):
    """(normal [R, 3] fp64, tol [R]): normalise(sum_i w_i (-g_i / |g_i|)), a term zero where the fp32 length of g_i is 0 or not
    finite or w_i is not finite, (0, 0, 0) where the sum's length is 0.  tol: the fp32 error bound of a ray -- every term carries
    about three roundings and the sum of S terms at most S / 64 + 6 more, each relative to sum |w_i| at worst:
    16 eps sum|w| / |sum| + 4 eps."""
    R, S = w.shape
    g32 = np.asarray(grad, np.float32).reshape(R, S, 3)
    with np.errstate(all="ignore"):
        len32 = np.sqrt((g32 * g32).sum(-1, dtype=np.float32))
    ok = np.isfinite(len32) & (len32 > 0) & np.isfinite(w)
    g = np.where(ok[..., None], g32, 1.0).astype(np.float64)
    ww = np.where(ok, w, 0.0).astype(np.float64)
    unit = -g / np.sqrt((g * g).sum(-1, keepdims=True))
    s = (ww[..., None] * unit).sum(1)
    length = np.sqrt((s * s).sum(-1))
    out = np.where(length[:, None] > 0, s / np.where(length > 0, length, 1.0)[:, None], 0.0)
    eps = float(np.finfo(np.float32).eps)
    tol = np.where(length > 0, 16 * eps * np.abs(ww).sum(1) / np.where(length > 0, length, 1.0) + 4 * eps, 0.0)
    return out, tol


# ---- upnerf_viz_normals --------------------------------------------------------------------------------------------------------

def quant_ref(v):
    """(uint8) clamp(255 * v, 0, 255) in fp32, truncating; NaN -> 0 (upnerf_viz_rgb's rule)."""
    v = np.float32(255.0) * np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(v < 0, np.float32(0), np.where(v > 255, np.float32(255), v))
    return np.where(np.isnan(v), 0, v).astype(np.uint8)


def viz_ref(n, rot=None):
    """uint8 [P, 3]: q((n' + 1) / 2), n' = rot . n with every product and sum rounded to fp32 on its own; a normal that is
    exactly zero is (128, 128, 128)."""
    n = np.asarray(n, np.float32).reshape(-1, 3)
    zero = (n == 0).all(1)
    c = n
    if rot is not None:
        r = np.asarray(rot, np.float32)
        with np.errstate(all="ignore"):
            c = np.stack([(r[k, 0] * n[:, 0] + r[k, 1] * n[:, 1]) + r[k, 2] * n[:, 2] for k in range(3)], 1).astype(np.float32)
    with np.errstate(all="ignore"):
        out = quant_ref((c + np.float32(1.0)) * np.float32(0.5))
    out[zero] = 128
    return out
