"""LPIPS (AlexNet) on the device (csrc/lpips.hip, upnerf_amd/lpips.py) against the fp64 restatement of its definition
(tests/lpips_ref.py) on seeded random weights: each convolution alone against the worst-case fp32 summation bound, the max
pool bit for bit, the whole metric at the project's parity criterion, its contracts (exact zero against itself; batch-, run-
and capture-invariant bits; NaN confinement; no write past a buffer), the refusals, and the TTO validation that reports it."""
import ctypes
import functools
import os
import pickle

import pytest
import torch
import torch.nn.functional as F

import lpips_ref

pytestmark = pytest.mark.gpu

REL_GATE = 1e-4  # README: "<=1e-4 rel, fp32"
SIZES = [(31, 31), (32, 32), (31, 64), (37, 61), (67, 95), (350, 500)]


@functools.lru_cache(maxsize=None)
def _weights():
    return lpips_ref.random_weights(1234)


@functools.lru_cache(maxsize=None)
def _model():
    from upnerf_amd.metrics import LpipsAlex
    w = _weights()
    return LpipsAlex(w["convs"], w["lins"]).to("cuda")


def _as_rays(x):
    """(N, C, H, W) -> contiguous [N, H*W, C]."""
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N, H * W, C).contiguous()


def _ray_strides(t, W):
    return (t.stride(0), t.stride(2), W * t.stride(1), t.stride(1))


def _conv_call(x, strides, N, H, W, layer, Wt, b, relu=1, scale_in=0, y=None):
    """One upnerf_conv2d call on device tensors; returns (rc, y [N, C_out, Ho, Wo])."""
    from upnerf_amd import _lib
    co, ci, k, s, p = lpips_ref.LAYERS[layer]
    Ho, Wo = lpips_ref.out_size(H, k, s, p), lpips_ref.out_size(W, k, s, p)
    if y is None:
        y = torch.full((N, co, Ho, Wo), float("nan"), device="cuda")
    a = _lib.Conv2dArgs(N=N, C_in=ci, H=H, W=W, C_out=co, k=k, stride=s, pad=p, relu=relu, scale_in=scale_in,
                        x=x.data_ptr(), w=Wt.data_ptr(), bias=b.data_ptr(), y=y.data_ptr())
    a.x_stride[:] = list(strides)
    return _lib.lib.upnerf_conv2d(ctypes.byref(a), _lib.stream()), y


# ---- 1. each convolution on its own -------------------------------------------------------------------------------

@pytest.mark.parametrize("image", [(31, 31), (37, 61), (67, 95)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("layer", range(5))
def test_each_convolution_is_inside_the_fp32_summation_bound(layer, image):
    """|got - ref64| <= 2 (K + 2) 2^-24 (conv(|x|, |W|) + |b|) elementwise, K = C_in k^2: the worst case of a K-term fp32 sum in
    any order, doubled.  Derived, not measured: an indexing, tail or padding mistake misses it by orders of magnitude."""
    co, ci, k, s, p = lpips_ref.LAYERS[layer]
    H, W = lpips_ref.layer_input_sizes(*image)[layer]
    N, K = 3, ci * k * k
    Wt, b = _weights()["convs"][layer]
    g = torch.Generator().manual_seed(100 * layer + H + W)
    x = torch.rand(N, ci, H, W, generator=g) if layer == 0 else torch.randn(N, ci, H, W, generator=g)
    xin = lpips_ref.scale_input(x) if layer == 0 else x.double()  # conv0 runs with the scaling layer on
    pre = lpips_ref.conv(xin, Wt, b, layer, relu=False)
    bound = 2 * (K + 2) * 2.0 ** -24 * lpips_ref.abs_bound(xin, Wt, b, layer)
    xd, Wd, bd = x.cuda(), Wt.cuda(), b.cuda()
    for relu in (1, 0):
        rc, y = _conv_call(xd, xd.stride(), N, H, W, layer, Wd, bd, relu=relu, scale_in=int(layer == 0))
        torch.cuda.synchronize()
        assert rc == 0
        want = F.relu(pre) if relu else pre
        err = (y.double().cpu() - want).abs()
        assert not torch.isnan(err).any()
        border = torch.zeros_like(err, dtype=torch.bool)
        border[..., 0, :] = border[..., -1, :] = border[..., :, 0] = border[..., :, -1] = True
        worst = lambda m: float((err / bound)[m].max()) if m.any() else 0.0
        inner = worst(~border)
        print(f"conv{layer} {H}x{W} relu={relu}: err/bound interior {inner:.3g} border {worst(border):.3g}")
        assert inner <= 1.0, f"conv{layer} interior pixels: {inner:.3g} x the bound"
        assert worst(border) <= 1.0, (f"conv{layer} border rows/columns: {worst(border):.3g} x the bound with the interior at "
                                      f"{inner:.3g} (padding must be zero in the SCALED image, not (0 - shift) / scale)")
    if layer == 0:  # the ray layout [N, H*W, 3], read in place, gives the bits of the NCHW view
        xr = _as_rays(xd)
        rc, y2 = _conv_call(xr, _ray_strides(xr, W), N, H, W, layer, Wd, bd, relu=0, scale_in=1)
        assert rc == 0 and torch.equal(y2, y)
        rc, y3 = _conv_call(xd[1:2], xd.stride(), 1, H, W, layer, Wd, bd, relu=0, scale_in=1)
        assert rc == 0 and torch.equal(y3, y[1:2])  # an image alone: the bits it has in the batch


# ---- 2. max pool ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(7, 7), (8, 14), (16, 23)])
def test_maxpool_is_bit_exact(H, W):
    from upnerf_amd import _lib
    N, C = 2, 5
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randn(N, C, H, W, generator=g)
    x[1, 2, 3, 4] = float("nan")
    want = F.max_pool2d(x, 3, 2)
    xd = x.cuda()
    y = torch.full((want.numel() + 1,), -7.0, device="cuda")
    a = _lib.Maxpool2dArgs(N=N, C=C, H=H, W=W, x=xd.data_ptr(), y=y.data_ptr())
    assert _lib.lib.upnerf_maxpool2d(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    got = y[:-1].reshape(want.shape).cpu()
    assert float(y[-1]) == -7.0
    assert torch.isnan(want).any() and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


# ---- 3. end to end -------------------------------------------------------------------------------------------------

def _pairs(H, W, seed, kinds=("random", "noise", "outside", "half")):
    """One (pred, gt) pair per kind, stacked as a batch: random; a render plus 1e-3 noise; values outside [0, 1]; an image with a
    constant half whose scaled value is exactly 0 (there conv0 is its bias: with negative biases every ReLU is dead and the
    normalisation takes its zero-norm branch, test_zero_norm_pixels_give_zero)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(3, H, W, generator=g)
    a = r()
    half = r()
    half[..., W // 2:] = lpips_ref.SHIFT.float()[:, None, None]
    half_gt = r()
    half_gt[..., W // 2:] = lpips_ref.SHIFT.float()[:, None, None]
    every = {"random": (r(), r()), "noise": (a, a + 1e-3 * torch.randn(3, H, W, generator=g)),
             "outside": (r() * 3 - 1, r() * 3 - 1), "half": (half, half_gt)}
    return torch.stack([every[k][0] for k in kinds]), torch.stack([every[k][1] for k in kinds])


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """(pred, gt, fp64 reference, fp32 CPU evaluation) of a size, computed once."""
    p, q = _pairs(H, W, seed=H * 7 + W, kinds=("random", "noise") if H * W > 100_000 else ("random", "noise", "outside", "half"))
    return p, q, lpips_ref.lpips(p, q, _weights()), lpips_ref.lpips(p, q, _weights(), dtype=torch.float32)


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_lpips_matches_the_fp64_reference(H, W):
    """|got - ref64| <= 1e-4 ref64 per pair; the device's error and that of the fp32 CPU evaluation are printed first (the
    near-identical "noise" pair is the hard one: DESIGN.md 2.26)."""
    from upnerf_amd.metrics import lpips_rays
    p, q, want, cpu32 = _case(H, W)
    m = _model()
    got = m(p.cuda(), q.cuda())
    rel = ((got.double().cpu() - want).abs() / want)
    rel32 = ((cpu32 - want).abs() / want)
    print(f"lpips {H}x{W}: values {want.tolist()} device rel err {rel.tolist()} fp32-CPU rel err {rel32.tolist()}")
    assert (want > 0).all() and float(rel.max()) <= REL_GATE, rel.tolist()
    by_rays = lpips_rays(m, _as_rays(p.cuda()), _as_rays(q.cuda()), (W, H))
    assert torch.equal(by_rays, got)  # the ray layout, read in place: the same bits
    assert torch.equal(m(q.cuda(), p.cuda()), got)  # symmetric


def test_zero_norm_pixels_give_zero():
    """All-zero feature pixels (every ReLU dead) contribute 0, not NaN: the epsilon is outside the root.  With negative biases
    an image whose scaled value is exactly 0 has conv0 = its bias, so every feature is dead: a half-constant render has such
    pixels at the first taps (the receptive fields of the later ones reach the live half), a wholly constant target at all five."""
    from upnerf_amd.metrics import LpipsAlex
    w = _weights()
    neg = {"convs": [(W, -b.abs()) for W, b in w["convs"]], "lins": w["lins"]}
    p, q = _pairs(67, 95, seed=5, kinds=("half", "half"))
    q[1] = lpips_ref.SHIFT.float()[:, None, None].expand(3, 67, 95)
    dead_p = [int((f.abs().sum(1) == 0).sum()) for f in lpips_ref.features(p, neg)]
    dead_q = [int((f[1].abs().sum(0) == 0).sum()) for f in lpips_ref.features(q, neg)]
    assert dead_p[0] > 0 and 0 < dead_p[0] < p.shape[0] * 16 * 23 and all(n > 0 for n in dead_q), (dead_p, dead_q)
    want = lpips_ref.lpips(p, q, neg)
    got = LpipsAlex(neg["convs"], neg["lins"]).to("cuda")(p.cuda(), q.cuda())
    rel = (got.double().cpu() - want).abs() / want
    print(f"zero-norm pixels per tap: render {dead_p}, constant target {dead_q}; device rel err {rel.tolist()}")
    assert not torch.isnan(got).any() and (want > 0).all() and float(rel.max()) <= REL_GATE


# ---- 4. contracts --------------------------------------------------------------------------------------------------

def test_self_distance_is_exactly_zero():
    p, q, _, _ = _case(37, 61)
    x = torch.cat([p, q]).cuda()
    out = _model()(x, x.clone())
    assert out.shape == (8,) and torch.equal(out, torch.zeros_like(out))


def test_batch_and_repeat_bits():
    p, q, _, _ = _case(37, 61)
    p, q = p.cuda(), q.cuda()
    m = _model()
    batch = m(p, q)
    assert batch.shape == (4,)
    for i in range(4):
        assert torch.equal(m(p[i:i + 1], q[i:i + 1]), batch[i:i + 1]), i
    for _ in range(3):
        assert torch.equal(m(p, q), batch)


def test_captured_graph_replays_the_eager_bits():
    p, q, _, _ = _case(67, 95)
    p, q = p.cuda(), q.cuda()
    m = _model()
    eager = m(p, q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(p, q)  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(p, q)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_nan_stays_in_its_pair():
    p, q, _, _ = _case(37, 61)
    p, q = p.cuda().clone(), q.cuda()
    m = _model()
    clean = m(p, q)
    p[2, 1, 7, 9] = float("nan")
    dirty = m(p, q)
    assert torch.isnan(dirty[2]) and not torch.isnan(clean).any()
    keep = [0, 1, 3]
    assert torch.equal(dirty[keep], clean[keep])


def test_buffers_are_not_written_past_their_end():
    from upnerf_amd.metrics import LpipsAlex
    w = _weights()
    m = LpipsAlex(w["convs"], w["lins"]).to("cuda")  # (its own scratch cache)
    N, H, W = 3, 33, 70
    g = torch.Generator().manual_seed(14)
    p, q = torch.rand(N, 3, H, W, generator=g).cuda(), torch.rand(N, 3, H, W, generator=g).cuda()
    want = _model()(p, q)
    sizes = [(t.numel(), t.dtype) for t in m.scratch(N, H, W, p.device)]
    guarded = [torch.full((n + 1,), float("nan"), dtype=dt, device="cuda") for n, dt in sizes]
    (key,) = m._scratch
    m._scratch[key] = tuple(t[:n] for t, (n, _) in zip(guarded, sizes))
    out = torch.full((N + 1,), float("nan"), device="cuda")
    m(p, q, out=out[:N])
    torch.cuda.synchronize()
    assert torch.isnan(out[N]) and all(torch.isnan(t[-1]) for t in guarded)
    assert torch.equal(out[:N], want)
    # the largest map of each buffer fills it: tap 0 ends on the last element of buffer 0, the partials are all written
    assert not torch.isnan(guarded[2][:-1]).any()


# ---- 5. refusals with real buffers ---------------------------------------------------------------------------------

def test_invalid_arguments_are_refused_with_real_buffers():
    from upnerf_amd import _lib
    m = _model()
    w = _weights()
    W0, b0 = (t.cuda() for t in w["convs"][0])
    x = torch.rand(2, 3, 31, 31, device="cuda")
    y = torch.full((2 * 64 * 7 * 7,), float("nan"), device="cuda")
    st = x.stride()

    def conv(x=x, Wt=W0, b=b0, y=y, **kw):
        a = _lib.Conv2dArgs(**{**dict(N=2, C_in=3, H=31, W=31, C_out=64, k=11, stride=4, pad=2, relu=1, scale_in=1), **kw},
                            x=None if x is None else x.data_ptr(), w=None if Wt is None else Wt.data_ptr(),
                            bias=None if b is None else b.data_ptr(), y=None if y is None else y.data_ptr())
        a.x_stride[:] = list(st)
        return _lib.lib.upnerf_conv2d(ctypes.byref(a), _lib.stream())

    assert conv(C_in=4) == -2 and conv(C_out=40) == -2
    assert conv(x=None) == -1 and conv(Wt=None) == -1 and conv(b=None) == -1 and conv(y=None) == -1
    assert conv(H=6) == -1 and conv(W=6) == -1 and conv(N=0) == -1
    for H, W in ((30, 31), (31, 30)):
        assert _lib.lib.upnerf_lpips_scratch(ctypes.byref(_lib.LpipsScratchArgs(N=1, H=H, W=W))) == -1
        with pytest.raises(ValueError):
            m(torch.rand(1, 3, H, W, device="cuda"), torch.rand(1, 3, H, W, device="cuda"))
    with pytest.raises(ValueError):
        m(torch.rand(1, 4, 32, 32, device="cuda"), torch.rand(1, 4, 32, 32, device="cuda"))
    with pytest.raises(TypeError):
        m(x.double(), x.double())
    with pytest.raises(RuntimeError):
        m(x.cpu(), x.cpu())
    pool = lambda xx, yy, H=7: _lib.lib.upnerf_maxpool2d(ctypes.byref(_lib.Maxpool2dArgs(
        N=2, C=3, H=H, W=7, x=None if xx is None else xx.data_ptr(), y=None if yy is None else yy.data_ptr())), _lib.stream())
    assert pool(None, y) == -1 and pool(x, None) == -1 and pool(x, y, H=2) == -1
    lin, out = w["lins"][0].cuda(), torch.full((3,), float("nan"), device="cuda")
    part = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    dist = lambda f, l, o, s, C=64: _lib.lib.upnerf_lpips_dist(ctypes.byref(_lib.LpipsDistArgs(
        N=1, C=C, H=7, W=7, feat=ptr(f), w=ptr(l), out=ptr(o))), ptr(s), _lib.stream())
    assert dist(None, lin, out, part) == -1 and dist(y, None, out, part) == -1 and dist(y, lin, None, part) == -1
    assert dist(y, lin, out, None) == -1 and dist(y, lin, out, part, C=0) == -1
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(out).all() and torch.isnan(part).all()  # nothing was launched


# ---- 6. TTO wiring (the synthetic 32 x 32 setup of tests/test_hip_metrics.py) --------------------------------------

def _ref_of_rays(rgb, gt):
    import ssim_ref
    return lpips_ref.lpips(ssim_ref.rays_to_nchw(rgb.cpu(), 32, 32), ssim_ref.rays_to_nchw(gt.cpu(), 32, 32), _weights())


def test_validation_step_reports_lpips_of_the_render():
    from test_hip_metrics import _tto
    from upnerf_amd.metrics import lpips_rays
    t, b = _tto()
    wh = dict(b, img_wh=torch.tensor([32, 32]))
    assert t.lpips_model is None and "lpips_model" not in dict(t.named_modules()) and not any("lpips" in k for k in t.state_dict())
    assert set(t.validation_step(wh)) == {"val_psnr", "val_ssim", "s_rgb_fine", "s_depth_fine"}
    keys = set(t.state_dict())
    t.lpips_model = _model()
    assert set(t.state_dict()) == keys
    assert set(t.validation_step(b)) == {"val_psnr", "s_rgb_fine", "s_depth_fine"}  # no image size: no image metric
    out = t.validation_step(wh)
    assert set(out) == {"val_psnr", "val_ssim", "val_lpips", "s_rgb_fine", "s_depth_fine"}
    assert out["val_lpips"].dim() == 0 and out["val_lpips"].is_cuda
    assert torch.equal(out["val_lpips"], lpips_rays(_model(), out["s_rgb_fine"], b["rgbs"], (32, 32))[0])
    want = float(_ref_of_rays(out["s_rgb_fine"], b["rgbs"])[0])
    print(f"val_lpips {float(out['val_lpips'])} fp64 {want}")
    assert want > 0 and abs(float(out["val_lpips"]) - want) <= REL_GATE * want


@pytest.mark.parametrize("attached", [True, False], ids=["model", "no-model"])
def test_run_stage_history_best_and_result_files(attached, tmp_path):
    from test_hip_metrics import _tto
    from upnerf_amd.nerf_system_optimize import read_nvs_results, run_stage, write_nvs_results
    t, b = _tto(True)
    if attached:
        t.lpips_model = _model()
    R = b["rgbs"].shape[0]

    def batches(epoch):
        perm = torch.randperm(R, device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + epoch))
        for lo in range(0, R, 256):
            yield {k: v[perm[lo:lo + 256]] for k, v in b.items()}

    tr = run_stage(t, batches, 4, max_epochs=3, val_batches=[dict(b, img_wh=torch.tensor([32, 32]))])
    top = max(tr.history, key=lambda h: h["val/psnr"])
    best = t.best
    assert len(tr.history) == 3 and all(("val/lpips" in h) == attached for h in tr.history)
    assert float(best["psnr"]) == top["val/psnr"] and float(best["ssim"]) == top["val/ssim"]
    rows = {"embedding_fine_a", "se3_refine", "psnr", "ssim", "step"}
    write_nvs_results(str(tmp_path), 7, best)
    r = read_nvs_results(str(tmp_path))
    if attached:
        assert set(best) == rows | {"lpips"}
        assert float(best["lpips"]) == top["val/lpips"] and best["lpips"].is_cuda  # the PSNR-best epoch's, not the lowest
        with open(tmp_path / "lpips.pkl", "rb") as f:
            table = pickle.load(f)
        assert list(table) == [7] and table[7].dim() == 0 and table[7].device.type == "cpu"
        assert float(table[7]) == float(best["lpips"])
        assert r == {"psnr": float(best["psnr"]), "ssim": float(best["ssim"]), "lpips": float(best["lpips"])}
    else:
        assert set(best) == rows
        assert r == {"psnr": float(best["psnr"]), "ssim": float(best["ssim"]), "lpips": None}
        assert not os.path.exists(tmp_path / "lpips.pkl")
