"""Alpha compositing (upnerf_composite_fwd / _bwd) and the per-ray reductions (upnerf_ray_geom_bwd, upnerf_ray_sum) on their own,
through the C ABI, against fp64 references with a per-ray gate (golden_util.ray_rel_err): a ray whose values are far below the
batch maximum is judged on its own scale.

Reference: kernel_space.composite on the kernels' fp32 inputs cast to fp64, torch.autograd for d_sigma_s, d_sigma_c and d_rgb.
The kernels form alpha = 1 - expf(-delta sigma) in fp32, and 1 - alpha from that alpha, like the reference implementation; an
fp64 alpha differs from it by up to 2^-25 absolute, i.e. 3e-4 relative at alpha = 1e-4, which alone fails the 1e-5 gate on a ray
of faint samples.  So the reference takes the fp32 exponentials as the device computes them (torch.exp on the GPU, the
kernels' operation order) with a straight-through rounding: the value of the kernels' fp32 alpha, the derivative of the exact
one (kernel_space.composite(e32=...)).  Everything downstream of alpha -- transmittance, weights, sums, every gradient -- is
fp64 in the reference.

Regimes (one batch holds all of them; each is asserted to be present, so an edit cannot quietly make it benign): a transparent
ray, opaque walls at samples 0 / 63 / 64 / last, gradual saturation into a later 64-sample chunk (the cancellation case of the
backward), density on the last sample only (delta = 1e2), zero-length intervals (z[63] == z[64]), and rays whose magnitudes
differ by 1e4.  Every output is allocated one ray longer and NaN-filled: that ray and every buffer the mode does not own must
stay NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_space as ks
from golden_util import ray_rel_err

pytestmark = pytest.mark.gpu

TOL_ACT = 1e-5   # per-sample weights and per-ray maps
TOL_GRAD = 1e-4  # d_sigma_s, d_sigma_c, d_rgb
SS = (1, 2, 63, 64, 65, 129, 192, 256, 1024)
UPSTREAM = ("E_s", "G_c", "sum_sfeat", "t_weight", "c_depth", "s_depth", "rgb_map", "rgb_joint_map", "w_all", "w_s")
PER_SAMPLE = ("w_all", "w_sj", "w_cj", "w_s")


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib, rendering
    return dict(lib=_lib, rendering=rendering)


def _u(g, n, lo=0.0, hi=1.0):
    return torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo


def regimes(S, seed):
    """One batch of rays, one regime per ray: z, sigma_s, sigma_c [R, S] (fp32), per-ray scale of the upstream gradients,
    rays whose per-sample inputs (rgb, e, g2) are constant along the ray, and {regime: ray}.  R is never a multiple of 4."""
    g = torch.Generator().manual_seed(seed)

    def zrow():  # depths in [2, 6], evenly spaced with a jitter below half a step (strictly increasing)
        if S == 1:
            return _u(g, 1, 2.0, 6.0)
        return torch.linspace(2.0, 6.0, S, dtype=torch.float64) + (_u(g, S) - 0.5) * 0.5 * 4.0 / (S - 1)

    rays, tags = [], {}

    def add(tag, z, ss, sc, scale=1.0, const=False):
        tags[tag] = len(rays)
        rays.append((z.float(), ss.float(), sc.float(), scale, const))

    zero = torch.zeros(S, dtype=torch.float64)
    add("random", zrow(), _u(g, S, 0, 3), _u(g, S, 0, 3))
    add("transparent", zrow(), zero, zero)
    for k in sorted({0, 63, 64, S - 1}):
        if k < S:
            ss = _u(g, S, 0, 0.5)
            ss[k] = 1e4 * (1 + _u(g, 1).item())
            add(f"wall{k}", zrow(), ss, _u(g, S, 0, 0.5))
    if S >= 65:
        # optical depth tau spread evenly over samples 0 .. S-2, sigma 1 on the last one: transmittance falls below 1e-6 in the
        # second chunk or later (S = 65: on the last sample)
        tau = 20.0 * (S - 1) / max(S - 1, 128)
        for const in (False, True):  # (constant rows: the backward bracket telescopes to ~T_end G, a full cancellation)
            z = zrow().float().double()
            ss = torch.cat([tau / (S - 1) / (z[1:] - z[:-1]), torch.ones(1, dtype=torch.float64)])
            add("gradual" + ("_const" if const else ""), z, ss, 0.1 * ss, const=const)
    ss, sc = zero.clone(), zero.clone()
    ss[-1], sc[-1] = 0.02, 0.005
    add("last_only", zrow(), ss, sc)
    if S >= 2:
        z = zrow()
        z[1] = z[0]
        if S >= 8:
            z[5] = z[6] = z[4]
        if S >= 65:
            z[64] = z[63]
        add("zero_length", z, _u(g, S, 0, 3), _u(g, S, 0, 3))
    add("faint", zrow(), _u(g, S, 0, 3), _u(g, S, 0, 3), scale=1e-4)
    add("dense", zrow(), _u(g, S, 30, 300), _u(g, S, 0, 30))
    add("weak", zrow(), _u(g, S, 0, 0.3), _u(g, S, 0, 0.3), scale=1e-2)
    if len(rays) % 4 == 0:
        add("random2", zrow(), _u(g, S, 0, 3), _u(g, S, 0, 3))
    z, ss, sc = (torch.stack([r[i] for r in rays]) for i in range(3))
    return z, ss, sc, torch.tensor([r[3] for r in rays]), torch.tensor([r[4] for r in rays]), tags


def make_batch(S, W, seed, R=None, frag=0):
    """Inputs of one launch (CPU fp32) and random upstream gradients for every output (scaled per ray)."""
    z, ss, sc, scale, const, tags = regimes(S, seed)
    if R is not None:
        z, ss, sc, scale, const = z[:R], ss[:R], sc[:R], scale[:R], const[:R]
        tags = {k: v for k, v in tags.items() if v < R}
    R = z.shape[0]
    M, W2 = R * S, W // 2
    g = torch.Generator().manual_seed(seed + 1000)
    rgb = _u(g, (R, S, 3)).float()
    e, g2 = _u(g, (R, S, W), -1, 1).float(), _u(g, (R, S, W2), -1, 1).float()
    for t in (rgb, e, g2):
        t[const] = t[const][:, :1].expand_as(t[const]).clone()
    b = dict(R=R, S=S, W=W, z=z, sigma_s=ss.reshape(M), sigma_c=sc.reshape(M), rgb=rgb.reshape(M, 3), e=e.reshape(M, W),
             g2=g2.reshape(M, W2), scale=scale, tags=tags)
    shapes = dict(E_s=(R, W), G_c=(R, W2), sum_sfeat=(R,), t_weight=(R,), c_depth=(R,), s_depth=(R,), rgb_map=(R, 3),
                  rgb_joint_map=(R, 3), w_all=(R, S), w_s=(R, S))
    up = {}
    for k in UPSTREAM:
        x = _u(g, shapes[k], -1, 1) * scale.view(-1, *[1] * (len(shapes[k]) - 1))
        up[k] = x.float().reshape(M) if k in PER_SAMPLE else x.float()
    b["up"] = up
    if frag:  # e (and g2 when frag == 2) as the field kernels' fp16 operand fragments; the fp32 rows become what they decode to
        rd = _lib_rendering()
        Mp = (M + 31) // 32 * 32
        pad = lambda t: torch.cat([t, torch.zeros(Mp - M, t.shape[1])]).cuda()
        eexp = torch.randint(-3, 4, (Mp // 32,), generator=g).to(torch.int32).cuda()
        b["e16"], b["eexp"] = rd.quant16_frag(pad(b["e"]), eexp), eexp
        b["e"] = rd.dequant16(b["e16"][None], eexp[None], frag=True)[0, :M].cpu().contiguous()
        if frag == 2:
            gexp = torch.randint(-2, 3, (Mp // 32,), generator=g).to(torch.int32).cuda()
            b["g2_16"], b["g2exp"] = rd.quant16_frag(pad(b["g2"]), gexp), gexp
            b["g2"] = rd.dequant16(b["g2_16"][None], gexp[None], frag=True)[0, :M].cpu().contiguous()
    return b


def _lib_rendering():
    from upnerf_amd import rendering
    return rendering


def owned(mode, has_rgb, rgbj):
    joint = mode <= 1
    o = {"w_s", "s_depth", "d_sigma_s"}
    if joint:
        o |= {"w_all", "w_sj", "w_cj", "c_depth", "t_weight", "G_c", "d_sigma_c"}
    if mode != 2:
        o |= {"E_s", "sum_sfeat"}
    if has_rgb:
        o |= {"rgb_map", "d_rgb"}
    if joint and has_rgb and rgbj:
        o.add("rgb_joint_map")
    return o


def launch(lib, b, mode, has_rgb, rgbj, frag, null):
    """Forward then backward on fresh NaN-filled outputs one ray longer than the batch.  `null`: upstream gradients passed as
    NULL; e (g2) is passed as NULL to the backward whenever g_E_s (g_G_c) is."""
    from upnerf_amd._lib import CompositeBwdArgs, CompositeFwdArgs
    R, S, W = b["R"], b["S"], b["W"]
    M, W2 = R * S, W // 2
    nan = lambda *shp: torch.full(shp, float("nan"), device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    dv = {k: b[k].cuda() for k in ("z", "sigma_s", "sigma_c", "rgb", "e", "g2")}
    o = dict(w_all=nan(M + S), w_sj=nan(M + S), w_cj=nan(M + S), w_s=nan(M + S), E_s=nan(R + 1, W), G_c=nan(R + 1, W2),
             sum_sfeat=nan(R + 1), t_weight=nan(R + 1), c_depth=nan(R + 1), s_depth=nan(R + 1), rgb_map=nan(R + 1, 3),
             rgb_joint_map=nan(R + 1, 3) if rgbj else None)
    f16 = dict(e16=p(b.get("e16")), eexp=p(b.get("eexp")), g2_16=p(b.get("g2_16")), g2exp=p(b.get("g2exp")))
    fa = CompositeFwdArgs(R=R, S=S, W=W, mode=mode, has_rgb=has_rgb, z=p(dv["z"]), sigma_s=p(dv["sigma_s"]), sigma_c=p(dv["sigma_c"]),
                          rgb=p(dv["rgb"]), e=None if frag else p(dv["e"]), g2=None if frag == 2 else p(dv["g2"]),
                          **f16, **{k: p(v) for k, v in o.items()})
    assert lib.upnerf_composite_fwd(C.byref(fa), None) == 0
    up = {k: (None if (k in null or (k == "rgb_joint_map" and not rgbj)) else v.cuda()) for k, v in b["up"].items()}
    d = dict(d_sigma_s=nan(M + S), d_sigma_c=nan(M + S), d_rgb=nan(M + S, 3))
    ba = CompositeBwdArgs(R=R, S=S, W=W, mode=mode, has_rgb=has_rgb, z=p(dv["z"]), sigma_s=p(dv["sigma_s"]), sigma_c=p(dv["sigma_c"]),
                          rgb=p(dv["rgb"]), e=None if (frag or up["E_s"] is None) else p(dv["e"]),
                          g2=None if (frag == 2 or up["G_c"] is None) else p(dv["g2"]),
                          w_all=p(o["w_all"]), w_sj=p(o["w_sj"]), w_cj=p(o["w_cj"]), w_s=p(o["w_s"]),
                          **{"g_" + k: p(v) for k, v in up.items()}, **f16, **{k: p(v) for k, v in d.items()})
    assert lib.upnerf_composite_bwd(C.byref(ba), None) == 0
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in {**o, **d}.items() if v is not None}, up


def reference(b, mode, has_rgb, up):
    """kernel_space.composite in fp64 on the kernels' fp32 alphas; gradients by autograd with a zero for every NULL upstream."""
    R, S = b["R"], b["S"]
    zd = b["z"].cuda()
    ssd, scd = b["sigma_s"].cuda().view(R, S), b["sigma_c"].cuda().view(R, S)
    delta = torch.cat([zd[:, 1:] - zd[:, :-1], torch.full_like(zd[:, :1], 1e2)], 1)
    e32 = {k: v.cpu() for k, v in dict(s=torch.exp(-delta * ssd), c=torch.exp(-delta * scd), all=torch.exp(-delta * (ssd + scd))).items()}
    leaves = [b[k].double().requires_grad_(True) for k in ("sigma_s", "sigma_c", "rgb")]
    f = dict(sigma_s=leaves[0], sigma_c=leaves[1], rgb=leaves[2], e=b["e"].double(), g2=b["g2"].double())
    ref = ks.composite(f, b["z"].double(), mode, bool(has_rgb), b["W"], e32=e32)
    terms = [(ref[k].reshape(up[k].shape) * up[k].cpu().double()).sum() for k in UPSTREAM if k in ref and up.get(k) is not None]
    if terms:
        grads = torch.autograd.grad(sum(terms), leaves, allow_unused=True)
    else:
        grads = (None,) * 3
    grads = [torch.zeros_like(x) if gr is None else gr for x, gr in zip(leaves, grads)]
    out = {k: v.detach() for k, v in ref.items()}
    out.update(d_sigma_s=grads[0], d_sigma_c=grads[1], d_rgb=grads[2])
    return out


def check(lib, b, mode, has_rgb=1, rgbj=True, frag=0, null=()):
    """Runs the pair twice, checks sentinels, bitwise determinism and the per-ray gates; returns (kernel outputs, reference)."""
    R, S = b["R"], b["S"]
    M = R * S
    got, up = launch(lib, b, mode, has_rgb, rgbj, frag, null)
    again, _ = launch(lib, b, mode, has_rgb, rgbj, frag, null)
    mine = owned(mode, has_rgb, rgbj)
    bad = []
    for k, v in got.items():
        per_sample = k in PER_SAMPLE or k.startswith("d_")
        head, tail = (v[:M], v[M:]) if per_sample else (v[:R], v[R:])
        if k not in mine:
            if not torch.isnan(v).all():
                bad.append(f"{k}: written though mode {mode} / has_rgb {has_rgb} / rgb_joint_map {rgbj} does not own it")
            continue
        if not torch.isnan(tail).all():
            bad.append(f"{k}: wrote past the last ray")
        if not torch.isfinite(head).all():
            bad.append(f"{k}: {int((~torch.isfinite(head)).sum())} entries not written or not finite")
        if not torch.equal(v.view(torch.int32), again[k].view(torch.int32)):
            bad.append(f"{k}: two launches differ")
    assert not bad, bad
    ref = reference(b, mode, has_rgb, up)
    errs = {}
    for k in sorted(mine):
        n = (R, -1)
        tol = TOL_GRAD if k.startswith("d_") else TOL_ACT
        gk = (got[k][:M] if (k in PER_SAMPLE or k.startswith("d_")) else got[k][:R]).reshape(n).double().numpy()
        rk = ref[k].reshape(n).numpy()
        e = ray_rel_err(gk, rk)
        if not e < tol:
            per_ray = [ray_rel_err(gk[r:r + 1], rk[r:r + 1]) * np.abs(rk[r]).max() / max(np.abs(rk[r]).max(), 1e-3 * np.abs(rk).max())
                       for r in range(R)]
            worst = int(np.nanargmax(per_ray))
            errs[k] = (float(f"{e:.3g}"), worst, [t for t, r in b["tags"].items() if r == worst])
    assert not errs, errs
    return got, ref


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("S", SS)
def test_composite_regimes_against_fp64(hip, S, mode):
    """Every regime in one batch, fp32 rows of e / g2 (W = 64); colour in modes 1 and 2 (modes 0 and 3 pass a NaN-filled
    rgb_map / rgb_joint_map / d_rgb that must stay so)."""
    has_rgb = int(mode in (1, 2))
    b = make_batch(S, 64, seed=S * 10 + mode)
    got, ref = check(hip["lib"].lib, b, mode, has_rgb=has_rgb)
    # the regimes are really there
    tags, z, ss, sc = b["tags"], b["z"], b["sigma_s"].view(b["R"], S), b["sigma_c"].view(b["R"], S)
    joint = mode <= 1
    ws = got["w_s"][:b["R"] * S].view(-1, S)
    r = tags["transparent"]
    assert float(ss[r].abs().max()) == 0 and float(sc[r].abs().max()) == 0
    assert float(ws[r].abs().max()) == 0 and (not joint or float(got["w_all"][r * S:(r + 1) * S].abs().max()) == 0)
    assert float(ref["d_sigma_s"].view(-1, S)[r].abs().max()) > 0
    walls = [k for k in (0, 63, 64, S - 1) if k < S]
    for k in walls:
        r = tags[f"wall{k}"]
        assert float(ss[r, k]) >= 1e4
        behind = ref["w_s"].view(-1, S)[r, k + 1:]
        assert behind.numel() == 0 or float(behind.max()) < 1e-6
    if S >= 65:
        for t in ("gradual", "gradual_const"):
            r = tags[t]
            delta = torch.cat([z[r, 1:] - z[r, :-1], torch.tensor([1e2])]).double()
            for sig in ((ss[r],) + ((ss[r] + sc[r],) if joint else ())):
                T_after = torch.exp(-torch.cumsum(delta * sig.double(), 0))  # transmittance past sample i
                first = int(torch.nonzero(T_after < 1e-6)[0])
                assert first >= 64, (t, first)
    r = tags["last_only"]
    assert bool((ss[r, :-1] == 0).all()) and float(ss[r, -1]) > 0
    if S >= 2:
        r = tags["zero_length"]
        assert bool((z[r, 1:] == z[r, :-1]).any()) and (S < 65 or float(z[r, 63]) == float(z[r, 64]))
    mag = ref["d_sigma_s"].view(-1, S).abs().amax(1)
    assert float(mag[tags["faint"]]) < 1e-3 * float(mag.max())


@pytest.mark.parametrize("rgbj", [True, False])
@pytest.mark.parametrize("has_rgb", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_composite_colour_outputs(hip, mode, has_rgb, rgbj):
    """rgb_map / rgb_joint_map (encode_feat = False) / d_rgb in every mode, with rgb_joint_map given or NULL; W = 256 fp32 rows."""
    check(hip["lib"].lib, make_batch(129, 256, seed=500 + 8 * mode + 2 * has_rgb + rgbj), mode, has_rgb=has_rgb, rgbj=rgbj)


@pytest.mark.parametrize("S,mode,frag", [(1024, 1, 2), (1024, 3, 1), (1024, 0, 1), (63, 0, 2), (65, 1, 1), (192, 1, 2),
                                         (256, 3, 1), (129, 2, 1), (1, 1, 2)])
def test_composite_fp16_fragments_against_fp64(hip, S, mode, frag):
    """e (frag 1) or e and g2 (frag 2) as the field kernels' fp16 operand fragments, up to S = 1024 (the E16_MAXS LDS arrays);
    the reference composites what the fragments decode to."""
    check(hip["lib"].lib, make_batch(S, 256, seed=700 + S + mode, frag=frag), mode, has_rgb=int(mode != 0), frag=frag)


@pytest.mark.parametrize("null,mode,frag", [((k,), 1, 0) for k in UPSTREAM] + [(("E_s",), 3, 0), (("E_s",), 1, 2), (("G_c",), 1, 2),
                                                                              (tuple(UPSTREAM), 1, 0), (tuple(UPSTREAM), 3, 2)])
def test_composite_null_upstream_gradients(hip, null, mode, frag):
    """Each optional upstream gradient NULL in turn, then all of them (the reference takes a zero).  The backward gets e = NULL
    with g_E_s and g2 = NULL with g_G_c: it must not read them."""
    b = make_batch(129, 256, seed=900 + len(null) + mode, frag=frag)
    got, _ = check(hip["lib"].lib, b, mode, has_rgb=int(mode != 0), frag=frag, null=null)
    if len(null) == len(UPSTREAM):
        assert float(got["d_sigma_s"][:b["R"] * 129].abs().max()) == 0


@pytest.mark.parametrize("S", [1, 65, 1024])
def test_composite_single_ray(hip, S):
    check(hip["lib"].lib, make_batch(S, 256, seed=1100 + S, R=1), 1)


# ---------------------------------------------------------------------------------------------- per-ray reductions
def _scaled(R, n, seed, lo=0.0, hi=1.0):
    """[R, n] uniform values with a per-ray scale spread over 1e-4 .. 1 (the per-ray gate judges each ray on its own).  Not
    negative: a sum that cancels to near zero would make a relative gate measure the luck of the draw."""
    g = torch.Generator().manual_seed(seed)
    return (_u(g, (R, n), lo, hi) * 10 ** _u(g, (R, 1), -4, 0)).float()


@pytest.mark.parametrize("R", [1, 3, 4097])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 192, 1000])
def test_ray_geom_bwd_against_fp64(hip, S, R):
    """(d_o, d_d) = (sum_i dxyz_i, sum_i z_i dxyz_i) per ray; outputs one ray longer, NaN-filled."""
    lib = hip["lib"].lib
    dxyz = _scaled(R, S * 3, seed=S * 7 + R).cuda()
    z = _u(torch.Generator().manual_seed(S + R), (R, S), 2.0, 6.0).float().cuda()
    d_o, d_d = torch.full((R + 1, 3), float("nan"), device="cuda"), torch.full((R + 1, 3), float("nan"), device="cuda")
    assert lib.upnerf_ray_geom_bwd(R, S, dxyz.data_ptr(), z.data_ptr(), d_o.data_ptr(), d_d.data_ptr(), None) == 0
    torch.cuda.synchronize()
    g = dxyz.double().view(R, S, 3)
    ref_o, ref_d = g.sum(1), (z.double()[..., None] * g).sum(1)
    assert torch.isnan(d_o[R]).all() and torch.isnan(d_d[R]).all()
    assert ray_rel_err(d_o[:R].cpu().numpy(), ref_o.cpu().numpy()) < TOL_ACT
    assert ray_rel_err(d_d[:R].cpu().numpy(), ref_d.cpu().numpy()) < TOL_ACT


@pytest.mark.parametrize("S", [1, 33, 200])
@pytest.mark.parametrize("Cw", [1, 3, 64, 65, 128, 256])
def test_ray_sum_against_fp64(hip, Cw, S):
    """out[r][c] = sum_i X[r S + i][c] (two interleaved partial sums: odd and even S), one block per ray, C up to 256."""
    lib = hip["lib"].lib
    R = 37
    X = _scaled(R, S * Cw, seed=Cw * 3 + S).cuda()
    out = torch.full((R + 1, Cw), float("nan"), device="cuda")
    assert lib.upnerf_ray_sum(R, S, X.data_ptr(), Cw, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[R]).all()
    assert ray_rel_err(out[:R].cpu().numpy(), X.double().view(R, S, Cw).sum(1).cpu().numpy()) < TOL_ACT
