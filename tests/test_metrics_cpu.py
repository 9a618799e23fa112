"""SSIM without a GPU: the fp64 test reference (tests/ssim_ref.py) against an independent restatement and closed forms,
the border rule it pins, the host-side refusals of upnerf_ssim and metrics.py, and the
psnr.pkl / ssim.pkl bookkeeping of the TTO results."""
import ctypes
import math
import os
import pickle

import numpy as np
import pytest
import torch

import ssim_ref



def _scipy_ssim_map(x, y):
    """Second restatement: scipy's correlate with mode="mirror" (= torch reflect: row -1 reads row 1), numpy fp64."""
    nd = pytest.importorskip("scipy.ndimage")
    w = ssim_ref.window().numpy()
    f = lambda a: nd.correlate(a, w, mode="mirror")
    mu1, mu2 = f(x), f(y)
    s11, s22, s12 = f(x * x) - mu1 ** 2, f(y * y) - mu2 ** 2, f(x * y) - mu1 * mu2
    num = (2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)
    return num / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s11 + s22 + 9e-4) + 1e-12)


@pytest.mark.parametrize("H,W", [(2, 2), (3, 3), (2, 65), (37, 61)])
def test_reference_agrees_with_scipy_mirror(H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    a = torch.rand(2, 3, H, W, generator=g, dtype=torch.float64)
    b = (a + 0.2 * torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)).clamp(-0.5, 1.5)
    m = ssim_ref.ssim_map(a, b)
    for n in range(2):
        for c in range(3):
            want = _scipy_ssim_map(a[n, c].numpy(), b[n, c].numpy())
            assert np.abs(m[n, c].numpy() - want).max() < 1e-12


def test_reference_closed_forms():
    # ssim(x, x): s = AB / (AB + 1e-12) per pixel, A = 2 mu^2 + C1, B = 2 sigma^2 + C2; on black, AB = C1 * C2
    black = torch.zeros(1, 3, 8, 9, dtype=torch.float64)
    s_black = 9e-8 / (9e-8 + 1e-12)
    assert torch.allclose(ssim_ref.ssim_map(black, black), torch.full_like(black, s_black), rtol=0, atol=1e-15)
    assert 1.1e-5 < 1 - s_black < 1.2e-5
    x = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    m = ssim_ref.ssim_map(x, x)
    assert float(m.max()) < 1 and float((1 - m).max()) < 1.2e-5
    assert abs(float(ssim_ref.ssim_per_image(black, black)[0]) - s_black) < 1e-15
    # two constant images: the variances vanish
    for p, q in ((0.3, 0.7), (0.0, 1.0), (-0.25, 1.5), (0.5, 0.5)):
        a = torch.full((1, 3, 5, 7), p, dtype=torch.float64)
        b = torch.full((1, 3, 5, 7), q, dtype=torch.float64)
        want = (2 * p * q + 1e-4) * 9e-4 / ((p * p + q * q + 1e-4) * 9e-4 + 1e-12)
        assert torch.allclose(ssim_ref.ssim_map(a, b), torch.full_like(a, want), rtol=0, atol=1e-12)


@pytest.mark.parametrize("where", ["row0", "row1", "corner"])
def test_reflect_padding_is_the_border_rule(where):
    """A single bright pixel next to the border: reflect (mirror without repeating the edge) gives other values than
    replicate or zero padding, and the same as scipy's mirror."""
    y, x = {"row0": (0, 4), "row1": (1, 4), "corner": (0, 0)}[where]
    a = torch.full((1, 1, 6, 9), 0.2, dtype=torch.float64)
    a[0, 0, y, x] = 1.0
    b = torch.full_like(a, 0.25)
    refl = ssim_ref.ssim_map(a, b)
    for other in ("replicate", "zeros"):
        assert float((refl - ssim_ref.ssim_map(a, b, pad_mode=other)).abs().max()) > 1e-3, other
    assert np.abs(refl[0, 0].numpy() - _scipy_ssim_map(a[0, 0].numpy(), b[0, 0].numpy())).max() < 1e-12


def _args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)  # non-null, never dereferenced: every case below is refused on the host
    a = _lib.SsimArgs(N=2, C=3, H=4, W=5, pred=one, gt=one, ssim=one, map=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("case", [dict(N=0), dict(C=0), dict(H=1), dict(W=1), dict(H=-3), dict(pred=None), dict(gt=None),
                                  dict(ssim=None), "scratch", "args"])
def test_ssim_argument_errors_are_refused_before_launch(case):
    from upnerf_amd import _lib
    scratch = ctypes.c_void_p(16)
    if case == "scratch":
        a, scratch = _args(), None
    elif case == "args":
        assert _lib.lib.upnerf_ssim(None, scratch, None) == -1 and _lib.lib.upnerf_ssim_scratch(None) == -1
        return
    else:
        a = _args(**case)
        if "N" in case or "C" in case or "H" in case or "W" in case:
            assert _lib.lib.upnerf_ssim_scratch(ctypes.byref(a)) == -1
    assert _lib.lib.upnerf_ssim(ctypes.byref(a), scratch, None) == -1


def test_ssim_scratch_counts_tiles_per_image():
    from upnerf_amd import _lib
    a = _args(N=3, H=350, W=500)
    n = _lib.lib.upnerf_ssim_scratch(ctypes.byref(a))
    assert n > 0 and n % 3 == 0
    a1 = _args(N=1, H=350, W=500)
    assert _lib.lib.upnerf_ssim_scratch(ctypes.byref(a1)) * 3 == n


def test_metrics_refuse_cpu_tensors_bad_sizes_and_mismatched_img_wh():
    from upnerf_amd import metrics
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        metrics.ssim(x, x)
    with pytest.raises(RuntimeError):
        metrics.ssim_rays(torch.rand(64, 3), torch.rand(64, 3), (8, 8))
    for shape in ((1, 3, 1, 8), (1, 3, 8, 1)):
        with pytest.raises(ValueError):
            metrics.ssim(torch.rand(shape), torch.rand(shape))
    with pytest.raises(ValueError):
        metrics.ssim(x, x, window_size=11)
    with pytest.raises(ValueError):
        metrics.ssim(x, x, reduction="sum")
    with pytest.raises(ValueError):
        metrics.ssim(x, torch.rand(1, 3, 8, 9))
    r = torch.rand(64, 3)
    with pytest.raises(ValueError):
        metrics.ssim_rays(r, r, (8, 9))
    with pytest.raises(ValueError):
        metrics.ssim_rays(r, r, (64, 1))  # H = 1
    with pytest.raises(ValueError):
        metrics.ssim_rays(r, torch.rand(2, 64, 3), (8, 8))


def test_img_wh_forms():
    from upnerf_amd.metrics import parse_img_wh
    for wh in ([torch.tensor([32]), torch.tensor([24])], torch.tensor([32, 24]), torch.tensor([[32, 24]]), (32, 24), [32, 24]):
        assert parse_img_wh(wh) == (32, 24)
    with pytest.raises(ValueError):
        parse_img_wh(torch.tensor([1, 2, 3]))


def test_psnr_is_the_reference_formula():
    from upnerf_amd import metrics
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(4, 3, generator=g), torch.rand(4, 3, generator=g)
    mse = float(((a.double() - b.double()) ** 2).mean())
    assert abs(float(metrics.psnr(a, b)) + 10 * math.log10(mse)) < 1e-4
    mask = torch.tensor([True, False, True, True])
    assert torch.equal(metrics.psnr(a, b, mask), -10 * torch.log10(((a - b) ** 2)[mask].mean()))
    assert metrics.psnr(a, b, reduction="none").shape == (4, 3)


def test_nvs_result_files_merge_and_read_back(tmp_path):
    from upnerf_amd.nerf_system_optimize import read_nvs_results, write_nvs_results
    assert read_nvs_results(str(tmp_path)) == {"psnr": None, "ssim": None, "lpips": None}
    write_nvs_results(str(tmp_path), 0, {"psnr": torch.tensor(20.0), "ssim": torch.tensor(0.5), "step": 4})
    write_nvs_results(str(tmp_path), 3, {"psnr": torch.tensor(30.0), "ssim": torch.tensor(0.75), "step": 8})
    write_nvs_results(str(tmp_path), 0, {"psnr": torch.tensor(22.0), "ssim": torch.tensor(0.25), "step": 9})  # replaces 0
    assert not os.path.exists(tmp_path / "lpips.pkl")
    with open(tmp_path / "psnr.pkl", "rb") as f:
        psnr = pickle.load(f)
    assert sorted(psnr) == [0, 3] and all(torch.is_tensor(v) and v.dim() == 0 and v.device.type == "cpu" for v in psnr.values())
    r = read_nvs_results(str(tmp_path))
    assert r["psnr"] == pytest.approx(26.0) and r["ssim"] == pytest.approx(0.5) and r["lpips"] is None
