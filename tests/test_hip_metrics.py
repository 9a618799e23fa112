"""upnerf_ssim (csrc/metrics.hip) on the device against the fp64 restatement of the reference's SSIM (tests/ssim_ref.py),
its contracts (batch-, layout-, run- and capture-invariant bits, NaN confinement, no write past an output), and the
TTO validation that reports it (NeRFSystemOptimize.validation_step / validation_epoch_end / best, the result files)."""
import ctypes
import os
import pickle

import pytest
import torch

import ssim_ref

pytestmark = pytest.mark.gpu

MAP_TOL, IMG_TOL = 2e-6, 1e-6
SIZES = [(2, 2), (2, 65), (3, 3), (37, 61), ("half", 37, 61), (350, 500), (1200, 1600)]


def _pairs(N, H, W, seed):
    """(pred, gt) in NCHW: random; 1e-4 noise on an image with a flat half (fp32 cancellation of filter(x^2) - mu^2);
    a render against itself; values outside [0, 1]; one bright pixel per border class."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.rand(N, 3, H, W, generator=g)
    a = r()
    a[..., W // 2:] = 0.6
    bright = torch.full((N, 3, H, W), 0.2)
    bright[..., 0, W // 2] = bright[..., 1, 0] = bright[..., H - 1, W - 1] = 1.0
    return {"random": (r(), r()),
            "noise": (a, a + 1e-4 * torch.randn(N, 3, H, W, generator=g)),
            "self": (a, a.clone()),
            "outside": (r() * 2 - 0.5, r() * 2 - 0.5),
            "bright": (bright, torch.full_like(bright, 0.25))}


def _as_rays(x):
    """(N, C, H, W) -> contiguous [N, H*W, C]."""
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N, H * W, C).contiguous()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_matches_the_fp64_reference(size):
    from upnerf_amd import metrics
    half = size[0] == "half"
    H, W = size[-2:]
    N = 1 if H * W > 100_000 else 2
    for kind, (p, q) in _pairs(N, H, W, seed=H * 7 + W).items():
        pd, qd = p.cuda(), q.cuda()
        if half:  # the right half of an odd-width image, read in place as a strided view
            p, q, pd, qd = p[..., W // 2:], q[..., W // 2:], pd[..., W // 2:], qd[..., W // 2:]
            assert not pd.is_contiguous()
        want_map = ssim_ref.ssim_map(p, q)
        want = ssim_ref.ssim_per_image(p, q)
        got_map = metrics._ssim_launch(pd, qd, *pd.shape, pd.stride(), qd.stride(), want_map=True)[1]
        err_map = float((got_map.double().cpu() - want_map).abs().max())
        assert err_map < MAP_TOL, (kind, err_map)
        Hh, Wh = p.shape[-2:]
        by_rays = metrics.ssim_rays(_as_rays(pd), _as_rays(qd), (Wh, Hh))
        err = float((by_rays.double().cpu() - want).abs().max())
        assert err < IMG_TOL, (kind, err)
        # the reference's function: "mean" over the batch, "none" the clamped map
        m = metrics.ssim(pd, qd)
        assert m.dim() == 0 and abs(float(m) - float(want.mean())) < IMG_TOL
        none = metrics.ssim(pd, qd, reduction="none")
        want_none = 1 - 2 * torch.clamp((1 - want_map) / 2, 0, 1)
        assert none.shape == p.shape and float((none.double().cpu() - want_none).abs().max()) < MAP_TOL


def test_batch_layout_repeat_bits():
    """N = 5 in one call gives the bits of five single calls; the NCHW and ray layouts give the same bits; a repeat too."""
    from upnerf_amd import metrics
    H, W = 37, 61
    g = torch.Generator().manual_seed(11)
    p = torch.rand(5, 3, H, W, generator=g).cuda()
    q = (p + 0.05 * torch.randn(5, 3, H, W, generator=g).cuda()).contiguous()
    batch = metrics.ssim_rays(_as_rays(p), _as_rays(q), (W, H))
    assert batch.shape == (5,)
    for i in range(5):
        one = metrics.ssim_rays(_as_rays(p[i:i + 1])[0], _as_rays(q[i:i + 1])[0], (W, H))
        assert torch.equal(one, batch[i:i + 1]), i
    nchw, smap = metrics._ssim_launch(p, q, 5, 3, H, W, p.stride(), q.stride(), want_map=True)
    assert torch.equal(nchw, batch)
    pr, qr = _as_rays(p), _as_rays(q)
    st = lambda t: (t.stride(0), t.stride(2), W * t.stride(1), t.stride(1))
    nchw2, smap2 = metrics._ssim_launch(pr, qr, 5, 3, H, W, st(pr), st(qr), want_map=True)
    assert torch.equal(nchw2, batch) and torch.equal(smap2, smap)
    for _ in range(3):
        assert torch.equal(metrics.ssim_rays(pr, qr, (W, H)), batch)


def test_captured_graph_replays_the_eager_bits():
    from upnerf_amd import metrics
    H, W = 350, 500
    g = torch.Generator().manual_seed(12)
    p = torch.rand(2, H * W, 3, generator=g).cuda()
    q = torch.rand(2, H * W, 3, generator=g).cuda()
    eager = metrics.ssim_rays(p, q, (W, H))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.ssim_rays(p, q, (W, H))  # warm-up off the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = metrics.ssim_rays(p, q, (W, H))
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_nan_stays_in_its_image():
    from upnerf_amd import metrics
    H, W = 16, 24
    g = torch.Generator().manual_seed(13)
    p = torch.rand(5, 3, H, W, generator=g).cuda()
    q = torch.rand(5, 3, H, W, generator=g).cuda()
    clean = metrics.ssim_rays(_as_rays(p), _as_rays(q), (W, H))
    p[2, 1, 7, 9] = float("nan")
    dirty = metrics.ssim_rays(_as_rays(p), _as_rays(q), (W, H))
    assert torch.isnan(dirty[2]) and not torch.isnan(clean).any()
    keep = [0, 1, 3, 4]
    assert torch.equal(dirty[keep], clean[keep])
    smap = metrics.ssim(p, q, reduction="none")
    nan = torch.isnan(smap).cpu()
    assert nan[2, 1, 6:9, 8:11].all() and int(nan.sum()) == 9  # the 3 x 3 neighbourhood of the pixel, one channel


def _raw_call(N, C, H, W, p, q, ssim, smap, scratch):
    from upnerf_amd import _lib
    a = _lib.SsimArgs(N=N, C=C, H=H, W=W, pred=p.data_ptr() if p is not None else None,
                      gt=q.data_ptr() if q is not None else None, ssim=ssim.data_ptr() if ssim is not None else None,
                      map=smap.data_ptr() if smap is not None else None)
    a.pred_stride[:] = [C * H * W, H * W, W, 1]
    a.gt_stride[:] = [C * H * W, H * W, W, 1]
    return _lib.lib.upnerf_ssim(ctypes.byref(a), scratch.data_ptr() if scratch is not None else None, _lib.stream()), a


def test_outputs_are_not_written_past_their_end():
    from upnerf_amd import _lib
    N, C, H, W = 3, 3, 33, 70
    g = torch.Generator().manual_seed(14)
    p = torch.rand(N, C, H, W, generator=g).cuda()
    q = torch.rand(N, C, H, W, generator=g).cuda()
    ssim = torch.full((N + 1,), float("nan"), device="cuda")
    smap = torch.full((N * C * H * W + 1,), float("nan"), device="cuda")
    probe = _lib.SsimArgs(N=N, C=C, H=H, W=W)
    n = _lib.lib.upnerf_ssim_scratch(ctypes.byref(probe))
    assert n > 0
    scratch = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    rc, _ = _raw_call(N, C, H, W, p, q, ssim, smap, scratch)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.isnan(ssim[N]) and torch.isnan(smap[-1]) and torch.isnan(scratch[n])
    assert not torch.isnan(ssim[:N]).any() and not torch.isnan(smap[:-1]).any() and not torch.isnan(scratch[:n]).any()


def test_invalid_arguments_are_refused_with_real_buffers():
    p = torch.rand(1, 3, 8, 8, device="cuda")
    out = torch.empty(1, device="cuda")
    scratch = torch.empty(64, dtype=torch.float64, device="cuda")
    for N, C, H, W in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 1, 8), (1, 3, 8, 1)):
        assert _raw_call(N, C, H, W, p, p, out, None, scratch)[0] == -1
    assert _raw_call(1, 3, 8, 8, None, p, out, None, scratch)[0] == -1
    assert _raw_call(1, 3, 8, 8, p, None, out, None, scratch)[0] == -1
    assert _raw_call(1, 3, 8, 8, p, p, None, None, scratch)[0] == -1
    assert _raw_call(1, 3, 8, 8, p, p, out, None, None)[0] == -1


# ---- TTO: the synthetic setup of tests/test_trainer.py -------------------------------------------------------------

def _tto(pose_optimize=True):
    from test_trainer import _system
    from upnerf_amd import synth
    from upnerf_amd.nerf_system import SyntheticDataset
    from upnerf_amd.nerf_system_optimize import NeRFSystemOptimize
    I, R = 4, 1024
    trained = _system(I)
    hp = dict(trained.hparams)
    hp["nerf.perturb"] = 0.0
    torch.manual_seed(5)
    t = NeRFSystemOptimize(hp, SyntheticDataset(I), pose_optimize=pose_optimize)
    t.model_setup(trained_state=trained.state_dict(), n_test_images=1)
    t = t.cuda()
    b = {k: v.cuda() for k, v in synth.batch(R, I, seed=21).items()}
    b["img_idx"] = torch.zeros_like(b["img_idx"])
    return t, b


def test_validation_step_reports_ssim_of_the_render():
    from upnerf_amd import metrics
    t, b = _tto()
    old = t.validation_step(b)
    assert set(old) == {"val_psnr", "s_rgb_fine", "s_depth_fine"}
    for wh in ((32, 32), torch.tensor([32, 32]), torch.tensor([[32, 32]]), [torch.tensor([32]), torch.tensor([32])]):
        out = t.validation_step(dict(b, img_wh=wh))
        assert set(out) == {"val_psnr", "val_ssim", "s_rgb_fine", "s_depth_fine"}
        assert out["val_ssim"].dim() == 0 and out["val_ssim"].is_cuda
        assert torch.equal(out["val_psnr"], old["val_psnr"])
        s = out["s_rgb_fine"]
        assert torch.equal(out["val_ssim"], metrics.ssim_rays(s, b["rgbs"], (32, 32))[0])
        want = float(ssim_ref.ssim_per_image(ssim_ref.rays_to_nchw(s.cpu(), 32, 32),
                                             ssim_ref.rays_to_nchw(b["rgbs"].cpu(), 32, 32))[0])
        assert abs(float(out["val_ssim"]) - want) < IMG_TOL
    self_ssim = metrics.ssim_rays(s, s, (32, 32))
    x = ssim_ref.rays_to_nchw(s.cpu(), 32, 32)
    assert abs(float(self_ssim[0]) - float(ssim_ref.ssim_per_image(x, x)[0])) < IMG_TOL
    with pytest.raises(ValueError):
        t.validation_step(dict(b, img_wh=(32, 31)))


@pytest.mark.parametrize("pose_optimize", [True, False], ids=["pose", "appearance"])
def test_run_stage_history_best_and_result_files(pose_optimize, tmp_path):
    from upnerf_amd.nerf_system_optimize import read_nvs_results, run_stage, write_nvs_results
    t, b = _tto(pose_optimize)
    R = b["rgbs"].shape[0]

    def batches(epoch):
        perm = torch.randperm(R, device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + epoch))
        for lo in range(0, R, 256):
            yield {k: v[perm[lo:lo + 256]] for k, v in b.items()}

    assert t.best["psnr"] == 0 and t.best["ssim"] is None
    epochs = 4 if pose_optimize else 2
    tr = run_stage(t, batches, 4, max_epochs=epochs, val_batches=[dict(b, img_wh=torch.tensor([32, 32]))])
    assert len(tr.history) == epochs and all("val/ssim" in h for h in tr.history)
    top = max(tr.history, key=lambda h: h["val/psnr"])
    best = t.best
    assert float(best["psnr"]) == top["val/psnr"] and float(best["ssim"]) == top["val/ssim"]
    assert best["step"] == top["step"]
    rows = {"embedding_fine_a", "se3_refine"} if pose_optimize else {"embedding_fine_a"}
    assert rows | {"psnr", "ssim", "step"} == set(best)
    for k in rows:
        assert best[k].is_cuda and best[k].data_ptr() != getattr(t, k).weight.data_ptr()
    if top is tr.history[-1]:  # the rows of the best epoch are the final ones only when it is the last
        for k in rows:
            assert torch.equal(best[k], getattr(t, k).weight)

    write_nvs_results(str(tmp_path), 7, best)
    for name in ("psnr", "ssim"):
        with open(tmp_path / f"{name}.pkl", "rb") as f:
            table = pickle.load(f)
        assert list(table) == [7] and table[7].dim() == 0 and table[7].device.type == "cpu"
        assert float(table[7]) == float(best[name])
    r = read_nvs_results(str(tmp_path))
    assert r == {"psnr": float(best["psnr"]), "ssim": float(best["ssim"]), "lpips": None}
    assert not os.path.exists(tmp_path / "lpips.pkl")
