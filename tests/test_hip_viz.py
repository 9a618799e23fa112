"""Validation images on the GPU (csrc/viz.hip, upnerf_amd/visualization.py) against numpy restatements of the reference's
formulas (utils/visualization.py, models/nerf_system.py:249-256, 276-307), written here from their definitions:

  depth   every step in the precision numpy gives it (fp32, `den` through fp64): index map and colours EQUAL element for element;
  PCA     fp64 restatement: float image within 5e-6, uint8 image off by at most 1 in at most 1e-3 of the elements.  Both gates
          come from the reference formula itself: fp32 torch on the CPU against fp64, unit-norm 384-wide features at 120 x 160,
          three seeds, gave a worst float error of 8.0e-7 and a worst share of differing uint8 elements of 8.7e-5 (never by more
          than 1).  The share cap is a condition, not a measurement, so every case also asserts that the fp32 torch-CPU
          restatement stays under both gates on the same inputs: the cap cannot hide a kernel worse than plain fp32;
  RGB     `(uint8) clamp(255 * v, 0, 255)`: EQUAL element for element.

Sizes are not multiples of any tile (37 x 53, 350 x 500); maps are also read in the strided ray layout."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PCA_FLOAT_GATE = 5e-6
PCA_SHARE_CAP = 1e-3
SIZES = [(37, 53), (350, 500)]


def _lut(seed=0):
    """A table with 256 distinct colours, so that equal colours mean equal indices."""
    g = np.random.default_rng(seed)
    t = np.stack([np.arange(256), g.permutation(256), g.permutation(256)], 1).astype(np.uint8)
    return t


def depth_ref(x, lut, min_max=None):
    """visualization.py:7-23 (index map, colours); `x` fp32 [H, W]."""
    x = np.nan_to_num(np.asarray(x, dtype=np.float32))
    mi, ma = (x.min(), x.max()) if min_max is None else min_max
    mi, ma = np.float32(mi), np.float32(ma)
    with np.errstate(all="ignore"):
        den = np.float32(np.float64(ma) - np.float64(mi) + 1e-8)
        t = (x - mi) / den
        assert t.dtype == np.float32
        t = np.clip(t, np.float32(0), np.float32(1))
        v = np.float32(255.0) * t
        q = np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)
    return q, lut[q]


def pred_depths_ref(inv, scale, shift, near, far):
    """nerf_system.py:249-256 in fp32, exp rounded once from fp64 (include/upnerf_hip.h)."""
    inv = np.asarray(inv, dtype=np.float32)
    es = np.float32(np.exp(np.float64(np.float32(scale))))
    v = inv * es
    v = v + np.float32(shift)
    lo = np.float32(1 / far)
    v = np.where(v < lo, lo, v)
    d = np.float32(1.0) / v
    d = np.where(d < np.float32(near), np.float32(near), d)
    assert d.dtype == np.float32
    return d


def quant_ref(v):
    with np.errstate(all="ignore"):
        v = np.float32(255.0) * np.asarray(v, dtype=np.float32)
        v = np.clip(v, np.float32(0), np.float32(255))
        return np.where(np.isnan(v), np.float32(0), v).astype(np.uint8)


def pca_ref64(feat, m, c):
    """get_pca_img in fp64 with the documented NaN rule: (float image, uint8 image)."""
    pc = (feat.astype(np.float64) - m.astype(np.float64)[None]) @ c.astype(np.float64).T
    mn, mx = np.nanmin(pc), np.nanmax(pc)
    img = (pc - mn) / (mx - mn)
    img = np.where(np.isnan(img), 0.0, img)
    return img, np.clip(255.0 * img, 0, 255).astype(np.uint8)


def _depth_map(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(H, W, generator=g) * 4.4 + 0.1


def _cuda_equal(t, want):
    got = t.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} elements differ"


# ---- depth ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SIZES)
def test_depth_own_range_given_range_device_range(H, W):
    from upnerf_amd import visualization as viz
    lut = _lut()
    d = _depth_map(H, W, 1)
    dc = d.cuda()
    for min_max in (None, (0.7, 3.1), (0.0, 10.0)):
        rgb, idx, _ = viz.depth_image(dc, (W, H), cmap=lut, min_max=min_max, want_index=True)
        q, col = depth_ref(d.numpy(), lut, min_max)
        _cuda_equal(idx, q)
        _cuda_equal(rgb, col)
    assert len(np.unique(depth_ref(d.numpy(), lut)[0])) > 200  # the whole table is in use
    # a range that lives on the device: the min / max of ANOTHER map, chained on the stream
    other = _depth_map(H, W, 2) * 0.5 + 0.4
    mm = viz.min_max_of(other.cuda())
    assert mm.is_cuda and mm.cpu().tolist() == [float(other.min()), float(other.max())]
    rgb, idx, _ = viz.depth_image(dc, (W, H), cmap=lut, min_max=mm, want_index=True)
    q, col = depth_ref(d.numpy(), lut, (other.min().numpy(), other.max().numpy()))
    _cuda_equal(idx, q)
    _cuda_equal(rgb, col)
    # the strided ray layout: the map is one column of an [H*W, 5] buffer
    buf = torch.rand(H * W, 5)
    buf[:, 2] = d.reshape(-1)
    col_view = buf.cuda()[:, 2]
    assert not col_view.is_contiguous()
    rgb2, idx2, _ = viz.depth_image(col_view, (W, H), cmap=lut, want_index=True)
    q, col = depth_ref(d.numpy(), lut)
    _cuda_equal(idx2, q)
    _cuda_equal(rgb2, col)
    # the reference's function: (3, H, W) floats, the ToTensor() of the picture; JET by default
    out = viz.visualize_depth(dc)
    assert out.shape == (3, H, W) and out.dtype == torch.float32 and out.is_cuda
    want = depth_ref(d.numpy(), viz.JET)[1].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(out.cpu().numpy(), want)
    out = viz.visualize_depth(dc, cmap=lut, min_max=(0.7, 3.1))
    assert np.array_equal(out.cpu().numpy(), depth_ref(d.numpy(), lut, (0.7, 3.1))[1].transpose(2, 0, 1).astype(np.float32) / np.float32(255))


def test_depth_nan_inf_and_constant_maps():
    from upnerf_amd import visualization as viz
    lut = _lut(3)
    H, W = 37, 53
    d = _depth_map(H, W, 4)
    d[3, 5] = float("nan")
    d[0, 0] = float("nan")
    d[36, 52] = float("inf")
    d[17, 20] = float("inf")
    # own range: NaN -> 0 joins the minimum, +inf -> FLT_MAX is the maximum
    rgb, idx, _ = viz.depth_image(d.cuda(), (W, H), cmap=lut, want_index=True)
    q, col = depth_ref(d.numpy(), lut)
    assert q[36, 52] == 255 and q[3, 5] == 0
    _cuda_equal(idx, q)
    _cuda_equal(rgb, col)
    # a given range, with -inf among the pixels
    d[20, 1] = float("-inf")
    for mm in ((0.5, 4.0), (-1.0, 1.0)):
        rgb, idx, _ = viz.depth_image(d.cuda(), (W, H), cmap=lut, min_max=mm, want_index=True)
        q, col = depth_ref(d.numpy(), lut, mm)
        assert q[20, 1] == 0 and q[36, 52] == 255
        _cuda_equal(idx, q)
        _cuda_equal(rgb, col)
    # constant maps: ma == mi, the 1e-8 decides (0 / 1e-8 = 0 everywhere; under a given degenerate range, above it -> 255)
    for value in (0.0, 2.5, -3.0):
        c = torch.full((H, W), value)
        rgb, idx, _ = viz.depth_image(c.cuda(), (W, H), cmap=lut, want_index=True)
        q, col = depth_ref(c.numpy(), lut)
        assert (q == 0).all()
        _cuda_equal(idx, q)
        _cuda_equal(rgb, col)
    d2 = _depth_map(H, W, 5)
    d2[4, 4] = 2.5
    rgb, idx, _ = viz.depth_image(d2.cuda(), (W, H), cmap=lut, min_max=(2.5, 2.5), want_index=True)
    q, col = depth_ref(d2.numpy(), lut, (2.5, 2.5))
    assert set(np.unique(q)) == {0, 255} and q[4, 4] == 0
    _cuda_equal(idx, q)
    _cuda_equal(rgb, col)
    # tiny ranges, where the double-precision `den` and the correctly rounded division matter
    e = torch.full((H, W), 1.0) + torch.rand(H, W, generator=torch.Generator().manual_seed(6)) * 1e-6
    rgb, idx, _ = viz.depth_image(e.cuda(), (W, H), cmap=lut, want_index=True)
    q, col = depth_ref(e.numpy(), lut)
    assert len(np.unique(q)) > 4
    _cuda_equal(idx, q)
    _cuda_equal(rgb, col)


@pytest.mark.parametrize("H,W", SIZES)
def test_pred_depths_pre_step(H, W):
    """rescale_depth_GT: inverse depths under the image's learnt (scale, shift), floors at 1 / far and near, coloured over the
    range of another map that stays on the device."""
    from upnerf_amd import visualization as viz
    lut = _lut(7)
    near, far = 0.1, 5.0
    g = torch.Generator().manual_seed(8)
    inv = torch.rand(H * W, generator=g) * 12.0 - 0.5  # some below 1 / far (also negative), some above 1 / near
    s_depth = _depth_map(H, W, 9).reshape(-1)
    for scale, shift in ((0.0, 0.0), (0.3127, -0.0571), (-1.25, 0.1)):
        row = torch.tensor([[scale, shift]])
        mm = viz.min_max_of(s_depth.cuda())
        rgb, idx, val = viz.depth_image(inv.cuda(), (W, H), cmap=lut, min_max=mm, depth_scale=row.cuda(), near=near, far=far,
                                        want_index=True, want_value=True)
        pd = pred_depths_ref(inv.numpy(), row[0, 0].numpy(), row[0, 1].numpy(), near, far)
        if scale == 0.0:  # both floors are in play
            assert (pd == np.float32(near)).any() and (pd == np.float32(1) / np.float32(1 / far)).any()
        _cuda_equal(val, pd)
        q, col = depth_ref(pd.reshape(H, W), lut, (s_depth.min().numpy(), s_depth.max().numpy()))
        _cuda_equal(idx, q)
        _cuda_equal(rgb, col)
        # and with its own range
        rgb, idx, _ = viz.depth_image(inv.cuda(), (W, H), cmap=lut, depth_scale=row.cuda(), near=near, far=far, want_index=True)
        q, col = depth_ref(pd.reshape(H, W), lut)
        _cuda_equal(idx, q)
        _cuda_equal(rgb, col)


# ---- PCA --------------------------------------------------------------------------------------------------------------

def _pca_inputs(n, F, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.nn.functional.normalize(torch.randn(n, F, generator=g), dim=-1)  # unit-norm descriptors
    m = torch.randn(F, generator=g) * (0.3 / F ** 0.5)
    c = torch.nn.functional.normalize(torch.randn(3, F, generator=g), dim=-1)
    return feat, m, c


def _check_pca(img, rgb, feat, m, c, torch_too=True):
    ref, ref8 = pca_ref64(feat.numpy(), m.numpy(), c.numpy())
    n = feat.shape[0]

    def gates(f32, u8, who):
        err = float(np.abs(f32.astype(np.float64).reshape(n, 3) - ref).max())
        d = np.abs(u8.reshape(n, 3).astype(np.int16) - ref8.astype(np.int16))
        share = float((d != 0).mean())
        print(f"PCA {who}: n={n} F={feat.shape[1]} float err {err:.3e} (gate {PCA_FLOAT_GATE:g}), uint8 share {share:.3e} "
              f"(cap {PCA_SHARE_CAP:g}), max step {int(d.max())}")
        assert err <= PCA_FLOAT_GATE, (who, err)
        assert int(d.max()) <= 1 and share <= PCA_SHARE_CAP, (who, int(d.max()), share)

    if torch_too:  # the reference's own fp32 formula on the CPU must pass the same gates on these inputs
        pc = (feat - m[None, :]) @ c.T
        t = (pc - pc.min()) / (pc.max() - pc.min())
        gates(t.numpy(), t.mul(255).clamp(0, 255).byte().numpy(), "torch fp32 CPU")
    gates(img.cpu().numpy(), rgb.cpu().numpy(), "kernel")


@pytest.mark.parametrize("H,W,F", [(37, 53, 384), (350, 500, 384), (37, 53, 64), (120, 160, 64), (37, 53, 50), (37, 53, 387),
                                   (37, 53, 512), (37, 53, 3)])
def test_pca_image_against_fp64(H, W, F):
    from upnerf_amd import visualization as viz
    feat, m, c = _pca_inputs(H * W, F, 100 + F)
    img, rgb = viz.pca_image(feat.cuda(), m.cuda(), c.cuda(), (W, H))
    assert img.shape == (H, W, 3) and img.dtype == torch.float32 and rgb.shape == (H, W, 3) and rgb.dtype == torch.uint8
    assert float(img.min()) == 0.0 and float(img.max()) == 1.0
    _check_pca(img, rgb, feat, m, c)
    # get_pca_img: the reference's name and shapes
    out = viz.get_pca_img(feat.cuda().view(H, W, F), m.cuda(), c.cuda())
    assert out.shape == (H, W, 3) and torch.equal(out, img)


@pytest.mark.parametrize("F,ld", [(384, 392), (64, 68), (64, 67), (50, 55)])
def test_pca_image_reads_strided_rows_in_place(F, ld):
    """Rows of a wider buffer (a slice of the ray layout): 16-byte loads when F and the row stride allow, the scalar path
    otherwise -- the same gates, and the same bits as the contiguous copy when both take one path."""
    from upnerf_amd import visualization as viz
    H, W = 37, 53
    feat, m, c = _pca_inputs(H * W, F, 200 + ld)
    wide = torch.rand(H * W, ld)
    wide[:, :F] = feat
    view = wide.cuda()[:, :F]
    assert not view.is_contiguous()
    img, rgb = viz.pca_image(view, m.cuda(), c.cuda(), (W, H))
    _check_pca(img, rgb, feat, m, c)
    if ld % 4 == 0 or F % 4 != 0:
        img2, rgb2 = viz.pca_image(feat.cuda(), m.cuda(), c.cuda(), (W, H))
        assert torch.equal(img, img2) and torch.equal(rgb, rgb2)


def test_pca_nan_features_are_left_out_and_written_as_zero():
    from upnerf_amd import visualization as viz
    H, W, F = 37, 53, 384
    feat, m, c = _pca_inputs(H * W, F, 31)
    clean_img, clean_rgb = viz.pca_image(feat.cuda(), m.cuda(), c.cuda(), (W, H))
    dirty = feat.clone()
    rows = torch.tensor([0, 7, 1000, H * W - 1])
    # rows that are neither the minimum nor the maximum of the clean picture, so that the range is unchanged
    ref, _ = pca_ref64(feat.numpy(), m.numpy(), c.numpy())
    assert all(0.0 < ref[r].min() and ref[r].max() < 1.0 for r in rows.tolist())
    dirty[rows, 5] = float("nan")
    img, rgb = viz.pca_image(dirty.cuda(), m.cuda(), c.cuda(), (W, H))
    assert not torch.isnan(img).any()
    flat, flat8 = img.view(-1, 3), rgb.view(-1, 3)
    assert (flat[rows.cuda()] == 0).all() and (flat8[rows.cuda()] == 0).all()
    keep = torch.ones(H * W, dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(flat[keep.cuda()], clean_img.view(-1, 3)[keep.cuda()])  # one NaN pixel does not touch the others
    assert torch.equal(flat8[keep.cuda()], clean_rgb.view(-1, 3)[keep.cuda()])
    _check_pca(img, rgb, dirty, m, c, torch_too=False)
    # every pixel NaN: all zeros, no NaN written
    img, rgb = viz.pca_image(torch.full((H * W, F), float("nan")).cuda(), m.cuda(), c.cuda(), (W, H))
    assert (img == 0).all() and (rgb == 0).all()


# ---- RGB / grey ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SIZES)
def test_rgb_and_grey_are_exact(H, W):
    from upnerf_amd import visualization as viz
    g = torch.Generator().manual_seed(41)
    x = torch.rand(H * W, 3, generator=g) * 1.2 - 0.1  # below 0 and above 1 too
    x[0] = torch.tensor([0.0, 1.0, 0.5])
    x[1] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    x[2] = torch.tensor([1.0 / 255, 254.999 / 255, 2.0 / 255])
    want = quant_ref(x.numpy()).reshape(H, W, 3)
    out = viz.rgb_image(x.cuda(), (W, H))
    assert out.shape == (H, W, 3) and out.dtype == torch.uint8
    _cuda_equal(out, want)
    wide = torch.rand(H * W, 6)
    wide[:, 1:4] = x
    view = wide.cuda()[:, 1:4]
    assert not view.is_contiguous()
    _cuda_equal(viz.rgb_image(view, (W, H)), want)
    _cuda_equal(viz.rgb_image(x.cuda().view(H, W, 3), (W, H)), want)
    grey = x[:, 0].contiguous()
    want1 = np.repeat(quant_ref(grey.numpy()).reshape(H, W, 1), 3, axis=2)
    _cuda_equal(viz.rgb_image(grey.cuda(), (W, H)), want1)
    _cuda_equal(viz.rgb_image(grey.cuda()[:, None], (W, H)), want1)
    _cuda_equal(viz.rgb_image(x.cuda()[:, 0], (W, H)), want1)  # a strided column


# ---- the same bytes alone, after other work, and from a captured graph -----------------------------------------------------

def test_same_bytes_alone_after_other_work_and_from_a_graph():
    from upnerf_amd import visualization as viz
    H, W, F = 37, 53, 384
    d = _depth_map(H, W, 51).cuda()
    x = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(52)).cuda()
    feat, m, c = (t.cuda() for t in _pca_inputs(H * W, F, 53))
    other = _depth_map(H, W, 54).cuda()

    def products():
        return [viz.depth_image(d, (W, H)), viz.depth_image(d, (W, H), min_max=viz.min_max_of(other)),
                *viz.pca_image(feat, m, c, (W, H)), viz.rgb_image(x, (W, H))]

    alone = [t.clone() for t in products()]
    torch.cuda.synchronize()
    busy = torch.rand(2048, 2048, device="cuda")
    for _ in range(3):
        busy = busy @ busy * 1e-3
        viz.pca_image(torch.rand(64 * 64, 128, device="cuda"), torch.rand(128, device="cuda"), torch.rand(3, 128, device="cuda"),
                      (64, 64))
    after = products()
    for a, b in zip(alone, after):
        assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        products()  # warm-up off the capture (uploads the JET table)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = products()
    for o in outs:
        o.zero_() if o.dtype == torch.uint8 else o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(alone, outs):
        assert torch.equal(a, b)


def test_outputs_are_not_written_past_their_end():
    """Raw calls with guard elements behind every output and scratch buffer, at a size that ends inside a thread's group of four."""
    import ctypes
    from upnerf_amd import _lib
    H, W, F = 37, 53, 50
    n = H * W
    lut = torch.from_numpy(_lut()).cuda()
    d = _depth_map(H, W, 61).reshape(-1).cuda()
    rgb = torch.full((3 * n + 8,), 77, dtype=torch.uint8, device="cuda")
    idx = torch.full((n + 8,), 77, dtype=torch.uint8, device="cuda")
    val = torch.full((n + 2,), float("nan"), device="cuda")
    a = _lib.VizDepthArgs(H=H, W=W, x=d.data_ptr(), x_stride=1, lut=lut.data_ptr(), rgb=rgb.data_ptr(), index=idx.data_ptr(),
                          value=val.data_ptr())
    ns = _lib.lib.upnerf_viz_depth_scratch(ctypes.byref(a))
    scratch = torch.full((ns + 2,), float("nan"), device="cuda")
    assert _lib.lib.upnerf_viz_depth(ctypes.byref(a), scratch.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert (rgb[3 * n:] == 77).all() and (idx[n:] == 77).all() and torch.isnan(val[n:]).all() and torch.isnan(scratch[ns:]).all()
    assert not torch.isnan(val[:n]).any()
    feat, m, c = (t.cuda() for t in _pca_inputs(n, F, 62))
    img = torch.full((3 * n + 4,), float("nan"), device="cuda")
    rgb.fill_(77)
    p = _lib.VizPcaArgs(H=H, W=W, F=F, feat=feat.data_ptr(), feat_ld=F, m=m.data_ptr(), c=c.data_ptr(), img=img.data_ptr(),
                        rgb=rgb.data_ptr())
    ns = _lib.lib.upnerf_viz_pca_scratch(ctypes.byref(p))
    scratch = torch.full((ns + 2,), float("nan"), device="cuda")
    assert _lib.lib.upnerf_viz_pca(ctypes.byref(p), scratch.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert (rgb[3 * n:] == 77).all() and torch.isnan(img[3 * n:]).all() and torch.isnan(scratch[ns:]).all()
    assert not torch.isnan(img[:3 * n]).any()
    x = torch.rand(n, 3, device="cuda")
    rgb.fill_(77)
    r = _lib.VizRgbArgs(H=H, W=W, C=3, x=x.data_ptr(), stride=3, cstride=1, rgb=rgb.data_ptr())
    assert _lib.lib.upnerf_viz_rgb(ctypes.byref(r), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert (rgb[3 * n:] == 77).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------

SHIPPED = ("rgb_fine", "c_depth_fine", "s_rgb_fine", "s_depth_fine", "t_weight_fine", "feat_fine", "t_beta", "t_alpha", "t_rgb")
VAL_W, VAL_H = 16, 10


def _val_setup(seed=11):
    """The synthetic scene of tests/test_trainer.py with two validation images of 16 x 10 rays that carry what the reference's
    validation items carry: img_wh, pca_m, pca_c."""
    from test_sampler import _sampler
    from test_trainer import _scene, _system
    bufs, I = _scene()
    smp = _sampler(bufs)
    g = torch.Generator().manual_seed(77)
    pca_m = torch.randn(384, generator=g) * 0.02
    pca_c = torch.nn.functional.normalize(torch.randn(3, 384, generator=g), dim=-1)
    val = []
    for i in range(2):
        b = {k: v[None] for k, v in smp.sample(torch.arange(i * 160, (i + 1) * 160)).items()}
        b["img_idx"] = torch.full_like(b["img_idx"], i + 1)  # one image per validation item, as in a real validation split
        b["img_wh"] = torch.tensor([[VAL_W, VAL_H]])
        b["pca_m"], b["pca_c"] = pca_m.cuda()[None], pca_c.cuda()[None]
        val.append(b)
    torch.manual_seed(seed)
    s = _system(I)
    s.hparams["val.log_image_list"] = SHIPPED
    return s, smp, val


def test_validation_images_of_a_validation_step():
    from upnerf_amd import visualization as viz
    s, smp, val = _val_setup()
    with torch.no_grad():
        s.depth_scale.weight.copy_(torch.tensor([[0.0, 0.0], [0.21, -0.03], [-0.4, 0.1], [0.0, 0.0]]))
    s.set_progress(0.3)  # inside the candidate schedule: the transient maps exist
    b = val[0]
    res = s.validation_step(b)["results"]
    wh = (VAL_W, VAL_H)
    images = viz.validation_images(s, b, res)
    shapes = {k: tuple(res[k].shape) for k in res if torch.is_tensor(res[k])}
    plan = viz.plan_validation_images(SHIPPED, shapes, "fine", True, True)
    assert list(images) == [name for name, _, _ in plan]
    assert {"rgb_GT", "feat_GT", "rescale_depth_GT", "rgb_fine", "s_rgb_fine", "s_depth_fine", "feat_fine", "t_beta",
            "t_alpha"} <= set(images) and "t_rgb" not in images
    for name, img in images.items():
        assert img.is_cuda and img.dtype == torch.uint8 and img.shape == (VAL_H, VAL_W, 3), name
    m, c = b["pca_m"][0], b["pca_c"][0]
    for name, kind, src in plan:
        if name == "rgb_GT":
            want = viz.rgb_image(b["rgbs"][0], wh)
        elif name == "feat_GT":
            want = viz.pca_image(b["feats"][0], m, c, wh)[1]
        elif kind == "depth":
            want = viz.depth_image(res[src], wh)
        elif kind == "pca":
            want = viz.pca_image(res[src], m, c, wh)[1]
        elif kind in ("rgb", "grey"):
            want = viz.rgb_image(res[src], wh)
        else:
            continue
        assert torch.equal(images[name], want), name
    # rescale_depth_GT from its definition: the prior's depths under image 1's row, over the range of the rendered depth
    pd = pred_depths_ref(b["inv_depths"][0].cpu().numpy(), np.float32(0.21), np.float32(-0.03), s.hparams["nerf.near"],
                         s.hparams["nerf.far"])
    sd = res["s_depth_fine"].cpu().numpy()
    want = depth_ref(pd.reshape(VAL_H, VAL_W), viz.JET, (sd.min(), sd.max()))[1]
    _cuda_equal(images["rescale_depth_GT"], want)
    # grey pictures replicate one channel; the pictures are not degenerate
    assert torch.equal(images["t_beta"][..., 0], images["t_beta"][..., 2])
    assert len(torch.unique(images["s_depth_fine"].view(-1, 3), dim=0)) > 8
    # a batch without PCA data or depth prior: those pictures are left out, feat_fine too
    bare = {k: v for k, v in b.items() if k not in ("pca_m", "pca_c")}
    few = viz.validation_images(s, bare, res)
    assert "feat_GT" not in few and "feat_fine" not in few and "rgb_GT" in few
    s.hparams["debug"] = True
    assert viz.validation_images(s, b, res) == {}
    s.hparams["debug"] = False
    # PCA data as a dataset item carries it (numpy arrays, no leading 1) gives the same pictures
    as_np = dict(b, pca_m=m.cpu().numpy(), pca_c=c.cpu().numpy())
    again = viz.validation_images(s, as_np, res)
    assert list(again) == list(images) and all(torch.equal(again[k], images[k]) for k in images)


def test_fit_with_an_image_writer_and_without(tmp_path):
    from PIL import Image
    from upnerf_amd import visualization as viz
    from upnerf_amd.trainer import Trainer
    MAX = 2 * 6  # six iterations: validations after the third and the sixth

    def run(sink):
        s, smp, val = _val_setup()
        batches = lambda epoch, start=0: smp.batches(128, seed=3, epoch=epoch, start=start)
        n_batches = (len(smp) + 127) // 128
        t = Trainer(MAX, val_check_interval=0.25, dirpath=None, seed=3, image_sink=sink).fit(s, batches, n_batches, val)
        return s, t

    before = _lib_calls()
    s0, t0 = run(None)
    plain_calls = _lib_calls() - before
    writer = viz.ImageWriter(str(tmp_path / "viz"))
    before = _lib_calls()
    s1, t1 = run(writer)
    assert _lib_calls() - before > plain_calls  # the pictures are extra library calls, and only with a sink
    assert len(writer.written) > 0
    # the same metrics and the same weights, bit for bit
    assert [h["step"] for h in t0.history] == [h["step"] for h in t1.history] == [6, 12]
    assert t0.history == t1.history
    sa, sb = s0.state_dict(), s1.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    # the files: <root>/val_<img_idx>/step_<step>/<name>.png, readable, of the image's size
    root = tmp_path / "viz"
    assert sorted(os.listdir(root)) == ["val_1", "val_2"]
    for tag in ("val_1", "val_2"):
        assert sorted(os.listdir(root / tag)) == ["step_00000006", "step_00000012"]
        for step in ("step_00000006", "step_00000012"):
            names = sorted(f[:-4] for f in os.listdir(root / tag / step))
            assert {"rgb_GT", "feat_GT", "rescale_depth_GT"} <= set(names), names
            if step == "step_00000012":  # progress 12 / 80 is past the start of the candidate schedule: the blended colour exists
                assert {"rgb_fine", "s_rgb_fine", "s_depth_fine", "feat_fine", "t_beta", "t_alpha"} <= set(names), names
            for n in names:
                im = Image.open(root / tag / step / f"{n}.png")
                im.load()
                assert im.mode == "RGB" and im.size == (VAL_W, VAL_H), (tag, step, n)
    assert sorted(writer.written) == sorted(str(p) for p in root.rglob("*.png"))


def _lib_calls():
    from upnerf_amd import _lib
    return _lib.CALLS[0]


def test_tto_system_yields_gt_and_rgb_fine(tmp_path):
    from PIL import Image
    from test_hip_metrics import _tto
    from upnerf_amd import visualization as viz
    from upnerf_amd.nerf_system_optimize import run_stage
    t, b = _tto()
    vb = dict(b, img_wh=torch.tensor([32, 32]))
    out = t.validation_step(vb)
    images = viz.validation_images(t, vb, out)
    assert list(images) == ["GT", "rgb_fine"]
    assert torch.equal(images["GT"], viz.rgb_image(b["rgbs"], (32, 32)))
    assert torch.equal(images["rgb_fine"], viz.rgb_image(out["s_rgb_fine"], (32, 32)))
    _cuda_equal(images["rgb_fine"], quant_ref(out["s_rgb_fine"].cpu().numpy()).reshape(32, 32, 3))
    with pytest.raises(ValueError):
        viz.validation_images(t, b, out)  # no img_wh: the size of the picture is unknown
    R = b["rgbs"].shape[0]

    def batches(epoch):
        perm = torch.randperm(R, device="cuda", generator=torch.Generator(device="cuda").manual_seed(100 + epoch))
        for lo in range(0, R, 256):
            yield {k: v[perm[lo:lo + 256]] for k, v in b.items()}

    writer = viz.ImageWriter(str(tmp_path / "tto"), pinned=True)
    tr = run_stage(t, batches, 4, max_epochs=2, val_batches=[vb], image_sink=writer)
    assert len(tr.history) == 2
    steps = sorted(os.listdir(tmp_path / "tto" / "val_0"))
    assert len(steps) == 2 and steps == [f"step_{h['step']:08d}" for h in tr.history]
    for st in steps:
        assert sorted(os.listdir(tmp_path / "tto" / "val_0" / st)) == ["GT.png", "rgb_fine.png"]
        gt = np.asarray(Image.open(tmp_path / "tto" / "val_0" / st / "GT.png"))
        assert np.array_equal(gt, images["GT"].cpu().numpy())
