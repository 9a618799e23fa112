"""LPIPS without a GPU: the state-dict mapping of LpipsAlex (upnerf_amd/lpips.py) under the upstream key names, the result
files and the host-side refusals of the new entry points (nothing is launched)."""
import ctypes
import pickle

import pytest
import torch

import lpips_ref

CONV_KEYS = ("features.0", "features.3", "features.6", "features.8", "features.10")


def _state_dicts(seed=0):
    """Dictionaries under the key names of torchvision's alexnet checkpoint and the lpips package's alex.pth."""
    w = lpips_ref.random_weights(seed)
    alex = {}
    for key, (W, b) in zip(CONV_KEYS, w["convs"]):
        alex[f"{key}.weight"], alex[f"{key}.bias"] = W, b
    alex["classifier.1.weight"], alex["classifier.1.bias"] = torch.zeros(8, 8), torch.zeros(8)
    lin = {f"lin{i}.model.1.weight": v.reshape(1, -1, 1, 1) for i, v in enumerate(w["lins"])}
    return w, alex, lin


def _same(model, w):
    return (all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(model.convs, w["convs"]))
            and all(torch.equal(a, b) and a.dim() == 1 for a, b in zip(model.lins, w["lins"])))


def test_from_state_dicts_reads_the_upstream_keys():
    from upnerf_amd.metrics import LpipsAlex
    w, alex, lin = _state_dicts()
    m = LpipsAlex.from_state_dicts(alex, lin)
    assert _same(m, w)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for pair in m.convs for t in pair)


@pytest.mark.parametrize("key", ["features.0.weight", "features.6.bias", "features.10.weight", "lin0.model.1.weight",
                                 "lin4.model.1.weight"])
def test_missing_key_and_wrong_shape_name_the_key(key):
    from upnerf_amd.metrics import LpipsAlex
    _, alex, lin = _state_dicts()
    which = alex if key in alex else lin
    good = which.pop(key)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        LpipsAlex.from_state_dicts(alex, lin)
    which[key] = torch.zeros(tuple(good.shape[:-1]) + (good.shape[-1] + 1,)) if good.dim() > 1 else torch.zeros(good.shape[0] + 1)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        LpipsAlex.from_state_dicts(alex, lin)


def test_load_round_trips_through_torch_save(tmp_path):
    from upnerf_amd.metrics import LpipsAlex
    w, alex, lin = _state_dicts(seed=3)
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    assert _same(LpipsAlex.load(str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")), w)


def test_cpu_and_dtype_and_shape_errors():
    from upnerf_amd.metrics import LpipsAlex, lpips_rays
    w = lpips_ref.random_weights(0)
    m = LpipsAlex(w["convs"], w["lins"])
    x = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError):
        m(x, x)
    with pytest.raises(RuntimeError):
        lpips_rays(m, torch.rand(32 * 32, 3), torch.rand(32 * 32, 3), (32, 32))
    with pytest.raises(ValueError):
        m(x, torch.rand(1, 3, 32, 33))
    with pytest.raises(ValueError):
        lpips_rays(m, torch.rand(32 * 32, 3), torch.rand(32 * 32, 3), (32, 31))
    with pytest.raises(ValueError):
        LpipsAlex(w["convs"][:4], w["lins"])


def test_read_nvs_results_picks_up_a_hand_written_lpips_file(tmp_path):
    from upnerf_amd.nerf_system_optimize import read_nvs_results, write_nvs_results
    assert read_nvs_results(str(tmp_path)) == {"psnr": None, "ssim": None, "lpips": None}
    with open(tmp_path / "lpips.pkl", "wb") as f:  # as the reference writes it: {image number: 0-d CPU tensor}
        pickle.dump({3: torch.tensor(0.25), 8: torch.tensor(0.75)}, f)
    assert read_nvs_results(str(tmp_path)) == {"psnr": None, "ssim": None, "lpips": 0.5}
    # a best epoch without LPIPS leaves the file alone; one with it merges its image into the table
    write_nvs_results(str(tmp_path), 5, {"psnr": torch.tensor(20.0), "ssim": torch.tensor(0.5), "step": 1})
    with open(tmp_path / "lpips.pkl", "rb") as f:
        assert sorted(pickle.load(f)) == [3, 8]
    write_nvs_results(str(tmp_path), 5, {"psnr": torch.tensor(20.0), "ssim": None, "lpips": torch.tensor(0.5), "step": 1})
    with open(tmp_path / "lpips.pkl", "rb") as f:
        table = pickle.load(f)
    assert sorted(table) == [3, 5, 8] and table[5].dim() == 0 and float(table[5]) == 0.5
    assert read_nvs_results(str(tmp_path)) == {"psnr": 20.0, "ssim": 0.5, "lpips": 0.5}


def test_no_model_is_the_default():
    from upnerf_amd.nerf_system_optimize import NeRFSystemOptimize
    assert NeRFSystemOptimize.lpips_model is None


ONE = ctypes.c_void_p(16)  # (non-null, never dereferenced: every case below is refused on the host)
EINVAL, EUNSUP = -1, -2


def _conv(**kw):
    from upnerf_amd import _lib
    a = _lib.Conv2dArgs(N=2, C_in=3, H=31, W=31, C_out=64, k=11, stride=4, pad=2, relu=1, scale_in=1, x=ONE, w=ONE, bias=ONE, y=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("case,want", [
    (dict(N=0), EINVAL), (dict(H=0), EINVAL), (dict(W=0), EINVAL), (dict(H=6), EINVAL), (dict(W=6), EINVAL),
    (dict(x=None), EINVAL), (dict(w=None), EINVAL), (dict(bias=None), EINVAL), (dict(y=None), EINVAL),
    (dict(C_in=4), EUNSUP), (dict(C_out=40), EUNSUP), (dict(k=7), EUNSUP), (dict(stride=2), EUNSUP), (dict(pad=0), EUNSUP),
    (dict(C_in=64, k=5, stride=1, pad=2, scale_in=1), EINVAL),  # the scaling layer belongs to the RGB input
    (dict(C_in=128, k=3, stride=1, pad=1, scale_in=0), EUNSUP),
])
def test_conv2d_refuses_before_launch(case, want):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_conv2d(ctypes.byref(_conv(**case)), None) == want
    assert _lib.lib.upnerf_conv2d(None, None) == EINVAL


def test_maxpool_dist_and_scratch_refuse_before_launch():
    from upnerf_amd import _lib
    L = _lib.lib
    pool = lambda **kw: _lib.Maxpool2dArgs(**{**dict(N=1, C=4, H=7, W=7, x=ONE, y=ONE), **kw})
    for kw in (dict(N=0), dict(C=0), dict(H=2), dict(W=2), dict(x=None), dict(y=None)):
        assert L.upnerf_maxpool2d(ctypes.byref(pool(**kw)), None) == EINVAL, kw
    assert L.upnerf_maxpool2d(None, None) == EINVAL
    dist = lambda **kw: _lib.LpipsDistArgs(**{**dict(N=1, C=64, H=7, W=7, feat=ONE, w=ONE, out=ONE), **kw})
    for kw in (dict(N=0), dict(C=0), dict(H=0), dict(W=0), dict(feat=None), dict(w=None), dict(out=None)):
        assert L.upnerf_lpips_dist(ctypes.byref(dist(**kw)), ONE, None) == EINVAL, kw
    assert L.upnerf_lpips_dist(ctypes.byref(dist()), None, None) == EINVAL
    assert L.upnerf_lpips_dist(None, ONE, None) == EINVAL
    for kw in (dict(N=0, H=31, W=31), dict(N=1, H=30, W=31), dict(N=1, H=31, W=30)):
        assert L.upnerf_lpips_scratch(ctypes.byref(_lib.LpipsScratchArgs(**kw))) == EINVAL, kw
    assert L.upnerf_lpips_scratch(None) == EINVAL


@pytest.mark.parametrize("N,H,W", [(1, 31, 31), (3, 37, 61), (2, 350, 500)])
def test_scratch_is_the_closed_form_of_the_layer_plan(N, H, W):
    """Buffer 0 holds taps 0, 1, 2 and 4, buffer 1 the pooled maps and tap 3, each for 2N images; one partial per 256 pixels of
    tap 0 (the largest tap) per pair."""
    from upnerf_amd import _lib
    a = _lib.LpipsScratchArgs(N=N, H=H, W=W)
    assert _lib.lib.upnerf_lpips_scratch(ctypes.byref(a)) == 0
    ins = lpips_ref.layer_input_sizes(H, W)
    outs = [(lpips_ref.out_size(h, k, s, p), lpips_ref.out_size(w, k, s, p)) for (h, w), (_, _, k, s, p) in zip(ins, lpips_ref.LAYERS)]
    tap = [c[0] * h * w for c, (h, w) in zip(lpips_ref.LAYERS, outs)]
    pooled = [lpips_ref.LAYERS[i - 1][0] * ins[i][0] * ins[i][1] for i in (1, 2)]
    assert a.act0_elems == 2 * N * max(tap[0], tap[1], tap[2], tap[4])
    assert a.act1_elems == 2 * N * max(pooled + [tap[3]])
    assert a.part_elems == N * -(-(outs[0][0] * outs[0][1]) // 256)
    if (H, W) == (31, 31):
        assert outs[2:] == [(1, 1)] * 3
