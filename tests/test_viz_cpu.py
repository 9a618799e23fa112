"""Validation images without a GPU: which picture every `val.log_image_list` name gets, the JET table, the PNG sink, and the
host-side guards of the upnerf_viz_* entry points (CPU tensors raise, bad arguments are refused before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

# val.log_image_list of every scene YAML the reference ships
SHIPPED = ("rgb_fine", "c_depth_fine", "s_rgb_fine", "s_depth_fine", "t_weight_fine", "feat_fine", "t_beta", "t_alpha", "t_rgb")


def _shapes(n=12, F=8):
    """What a candidate-phase fine render returns (shapes only; `t_rgb` is not among the maps of this package's render)."""
    return {"rgb_fine": (n, 3), "s_rgb_fine": (n, 3), "c_depth_fine": (n,), "s_depth_fine": (n,), "t_weight_fine": (n,),
            "feat_fine": (n, F), "t_beta": (n,), "t_alpha": (n, 1), "s_weights_fine": (n, 64), "rgb_coarse": (n, 3)}


def test_shipped_log_image_list_gets_the_reference_dispatch():
    from upnerf_amd.visualization import plan_validation_images
    plan = plan_validation_images(SHIPPED, _shapes(), "fine", has_pca=True, has_inv_depths=True)
    assert plan == [("rgb_GT", "rgb", "rgbs"), ("feat_GT", "pca", "feats"), ("rescale_depth_GT", "pred_depth", "inv_depths"),
                    ("rgb_fine", "rgb", "rgb_fine"), ("c_depth_fine", "depth", "c_depth_fine"),
                    ("s_rgb_fine", "rgb", "s_rgb_fine"), ("s_depth_fine", "depth", "s_depth_fine"),
                    ("t_weight_fine", "grey", "t_weight_fine"), ("feat_fine", "pca", "feat_fine"),
                    ("t_beta", "grey", "t_beta"), ("t_alpha", "grey", "t_alpha")]  # t_rgb: not in results -> skipped


def test_dispatch_order_and_skips():
    from upnerf_amd.visualization import plan_validation_images
    res = dict(_shapes(), rgb_depth_feat=(12,), feat_rgb=(12, 8), s_weights_fine=(12, 64), odd_rgb=(12, 3))
    names = ("rgb_depth_feat", "feat_rgb", "s_weights_fine", "odd_rgb", "missing_depth")
    plan = plan_validation_images(names, res, "fine", has_pca=True, has_inv_depths=False)
    # "depth" is tested before "feat", "feat" before "rgb"; a multi-channel map with none of the three words is skipped,
    # and so is a name the render did not produce; without inv_depths there is no rescale_depth_GT
    assert plan == [("rgb_GT", "rgb", "rgbs"), ("feat_GT", "pca", "feats"), ("rgb_depth_feat", "depth", "rgb_depth_feat"),
                    ("feat_rgb", "pca", "feat_rgb"), ("odd_rgb", "rgb", "odd_rgb")]
    # without PCA data the reference's `"feat" in name and feats is not None` fails and the next test ("rgb") decides
    plan = plan_validation_images(("feat_rgb", "feat_fine"), res, "fine", has_pca=False, has_inv_depths=False)
    assert plan == [("rgb_GT", "rgb", "rgbs"), ("feat_rgb", "rgb", "feat_rgb")]
    coarse = {"rgb_coarse": (12, 3), "s_depth_coarse": (12,)}
    plan = plan_validation_images(SHIPPED, coarse, "coarse", has_pca=False, has_inv_depths=True)
    assert plan == [("rgb_GT", "rgb", "rgbs"), ("rescale_depth_GT", "pred_depth", "inv_depths")]
    assert plan_validation_images(None, coarse, "coarse", False, False) == [("rgb_GT", "rgb", "rgbs")]


def test_debug_returns_no_images():
    from upnerf_amd.visualization import validation_images

    class Sys:
        hparams = {"debug": True}

    assert validation_images(Sys(), {}, {}) == {}


def test_jet_table():
    from upnerf_amd.visualization import JET
    assert isinstance(JET, np.ndarray) and JET.shape == (256, 3) and JET.dtype == np.uint8
    assert not JET.flags.writeable
    b, g, r = (JET[:, k].astype(int) for k in range(3))  # cv2's BGR column order
    assert b[0] >= 120 and g[0] == 0 and r[0] == 0      # entry 0: dark blue only
    assert r[255] >= 120 and g[255] == 0 and b[255] == 0  # entry 255: dark red only
    for ch in (b, g, r):  # a trapezoid: up to the plateau, flat, down
        top = np.flatnonzero(ch == ch.max())
        assert ch.max() == 255 and np.all(np.diff(top) == 1)
        assert np.all(np.diff(ch[:top[0] + 1]) >= 0) and np.all(np.diff(ch[top[-1]:]) <= 0)
    assert np.argmax(b) < np.argmax(g) < np.argmax(r)  # blue peaks first, red last


def test_image_writer_round_trip(tmp_path):
    from PIL import Image
    from upnerf_amd.visualization import ImageWriter
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (7, 11, 3), generator=g, dtype=torch.uint8)
    other = torch.randint(0, 256, (7, 11, 3), generator=g, dtype=torch.uint8)
    w = ImageWriter(str(tmp_path / "viz"))
    paths = w("val_5", 1234, {"rgb_fine": img, "c_depth_fine": other})
    want = [str(tmp_path / "viz" / "val_5" / "step_00001234" / f"{n}.png") for n in ("rgb_fine", "c_depth_fine")]
    assert paths == want and w.written == want and all(os.path.isfile(p) for p in want)
    for p, t in zip(want, (img, other)):
        back = Image.open(p)
        assert back.mode == "RGB" and back.size == (11, 7)
        assert np.array_equal(np.asarray(back), t.numpy())
    with pytest.raises(ValueError):
        w("val_5", 1, {"bad": torch.zeros(7, 11, dtype=torch.uint8)})
    with pytest.raises(ValueError):
        w("val_5", 1, {"bad": torch.zeros(7, 11, 3)})


def test_cpu_tensors_raise():
    from upnerf_amd import visualization as viz
    d = torch.rand(6, 8)
    with pytest.raises(RuntimeError):
        viz.visualize_depth(d)
    with pytest.raises(RuntimeError):
        viz.depth_image(d, (8, 6))
    with pytest.raises(RuntimeError):
        viz.min_max_of(d)
    with pytest.raises(RuntimeError):
        viz.get_pca_img(torch.rand(6, 8, 16), torch.rand(16), torch.rand(3, 16))
    with pytest.raises(RuntimeError):
        viz.rgb_image(torch.rand(48, 3), (8, 6))
    with pytest.raises(ValueError):
        viz.visualize_depth(torch.rand(48))
    with pytest.raises(ValueError):
        viz.get_pca_img(torch.rand(48, 16), torch.rand(16), torch.rand(3, 16))


def _depth_args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)  # non-null, never dereferenced: every case below is refused on the host
    a = _lib.VizDepthArgs(H=4, W=5, pre=_lib.VIZ_PLAIN, range=_lib.VIZ_RANGE_OWN, x=one, x_stride=1, depth_scale=one,
                          range_dev=one, lut=one, rgb=one)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("case", [dict(H=0), dict(W=0), dict(H=-3), dict(lut=None), dict(x=None), dict(rgb=None), dict(pre=2),
                                  dict(range=3), dict(range=-1), dict(range=2, range_dev=None), dict(pre=1, depth_scale=None)])
def test_depth_argument_errors_are_refused_before_launch(case):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    assert _lib.lib.upnerf_viz_depth(ctypes.byref(_depth_args(**case)), one, None) == -1


def test_other_argument_errors_are_refused_before_launch():
    from upnerf_amd import _lib
    L, one = _lib.lib, ctypes.c_void_p(16)
    assert L.upnerf_viz_depth(None, one, None) == -1
    assert L.upnerf_viz_depth(ctypes.byref(_depth_args()), None, None) == -1  # its own range needs the scratch
    assert L.upnerf_viz_depth_scratch(ctypes.byref(_depth_args(H=0))) == -1
    assert L.upnerf_viz_depth_scratch(ctypes.byref(_depth_args(H=350, W=500))) > 2
    assert L.upnerf_viz_minmax_scratch(0) == -1 and L.upnerf_viz_minmax_scratch(1) == 2
    assert L.upnerf_viz_minmax(None, 4, 1, one, one, None) == -1
    assert L.upnerf_viz_minmax(one, 4, 1, None, one, None) == -1
    assert L.upnerf_viz_minmax(one, 4, 1, one, None, None) == -1
    assert L.upnerf_viz_minmax(one, 0, 1, one, one, None) == -1

    def pca(**kw):
        a = _lib.VizPcaArgs(H=4, W=5, F=384, feat=one, feat_ld=384, m=one, c=one, img=one, rgb=one)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for case in (dict(H=0), dict(W=0), dict(F=0), dict(F=513), dict(feat=None), dict(m=None), dict(c=None), dict(img=None),
                 dict(rgb=None), dict(feat_ld=383)):
        assert L.upnerf_viz_pca(ctypes.byref(pca(**case)), one, None) == -1, case
    assert L.upnerf_viz_pca(ctypes.byref(pca()), None, None) == -1
    assert L.upnerf_viz_pca_scratch(ctypes.byref(pca(F=513))) == -1
    assert L.upnerf_viz_pca_scratch(ctypes.byref(pca(F=512))) > 2

    def rgb(**kw):
        a = _lib.VizRgbArgs(H=4, W=5, C=3, x=one, stride=3, cstride=1, rgb=one)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for case in (dict(H=0), dict(W=0), dict(C=2), dict(C=0), dict(C=4), dict(x=None), dict(rgb=None)):
        assert L.upnerf_viz_rgb(ctypes.byref(rgb(**case)), None) == -1, case
    assert L.upnerf_viz_rgb(None, None) == -1
