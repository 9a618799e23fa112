"""DPT-Large inverse depth on the device (csrc/dpt.hip, upnerf_amd/dpt.py) against the fp64 restatement of its definition
(tests/dpt_ref.py) on seeded random weights: each new kernel alone at its tile edges, the whole network on two small
configurations with every returned stage at the project's parity criterion, the photograph-to-map route, and the tool's
files read back by the phototourism dataset.

Measured on an MI355X (worst error over the reference map's max-abs; the gate is 1e-4):
    upnerf_conv3x3 8.7e-7, upnerf_upsample2x 2.2e-7 (its own gate: 1e-6), upnerf_resize_cubic 1.3e-6, upnerf_depth_to_space and
    upnerf_vit_patches16 bit-for-bit; the network, worst stage: configuration a 1.8e-6, b 1.7e-6; inverse_depth 7.9e-7."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dpt_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_GATE = 1e-4  # README: "<=1e-4 rel, fp32", taken against the reference map's max-abs
C3_BM, C3_BN = 128, 64  # upnerf_conv3x3's workgroup tile: output pixels x output channels


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


# ---- 1. upnerf_conv3x3 ---------------------------------------------------------------------------------------------------

def _conv3x3(x, w, bias, res, H, W, ci, co, stride, pre_relu, relu, guard=2):
    """One launch on device tensors; x [H * W + guard][ci] (guard rows NaN), returns y [M + guard][co] (guard rows 7)."""
    from upnerf_amd import _lib
    M = ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    y = torch.full((M + guard, co), 7.0, device="cuda")
    a = _lib.Conv3x3Args(H=H, W=W, C_in=ci, C_out=co, stride=stride, pre_relu=pre_relu, relu=relu, x=x.data_ptr(), ldx=ci,
                         w=w.data_ptr(), bias=_lib.ptr(bias), res=_lib.ptr(res), ldr=co, y=y.data_ptr(), ldy=co)
    assert _lib.lib.upnerf_conv3x3(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    return y


def _check_conv3x3(H, W, ci, co, stride=1, bias=True, pre_relu=False, res=False, relu=False):
    from upnerf_amd.dpt import relay_conv3x3
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + ci + co + stride)
    x = torch.randn(H, W, ci, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
    b = torch.randn(co, generator=g) if bias else None
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    r = torch.randn(Ho, Wo, co, generator=g) if res else None
    want = R.conv3x3(x.double(), w.double(), b.double() if bias else None, r.double() if res else None, stride, pre_relu, relu)
    assert want.shape == (Ho, Wo, co)
    xd = torch.full((H * W + 2, ci), float("nan"))
    xd[:H * W] = x.reshape(H * W, ci)
    xd, wd = xd.cuda(), relay_conv3x3(w).cuda()
    bd, rd = b.cuda() if bias else None, r.reshape(Ho * Wo, co).contiguous().cuda() if res else None
    y = _conv3x3(xd, wd, bd, rd, H, W, ci, co, stride, int(pre_relu), int(relu))
    M = Ho * Wo
    assert torch.isfinite(y[:M]).all()
    err = _rel(y[:M].reshape(Ho, Wo, co), want)
    print(f"conv3x3 {H}x{W} {ci}->{co} s{stride} bias={bias} pre={pre_relu} res={res} relu={relu}: {err:.2e} of max-abs")
    assert err < REL_GATE
    assert torch.equal(y[M:].cpu(), torch.full((2, co), 7.0))  # rows past the map are not stored
    assert torch.equal(_conv3x3(xd, wd, bd, rd, H, W, ci, co, stride, int(pre_relu), int(relu)), y)  # the same bits every run


# one pixel short of, at and past the pixel tile: 127 = 1 x 127, 128 = 8 x 16, 129 = 3 x 43; 150 = 10 x 15: two workgroups
@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (2, 3), (7, 9), (1, C3_BM - 1), (8, C3_BM // 8), (3, (C3_BM + 1) // 3), (10, 15)])
@pytest.mark.parametrize("ci,co", [(32, 32), (64, 160), (96, 64)])
def test_conv3x3_against_fp64(H, W, ci, co):
    assert co % C3_BN in (0, 32)  # 160: two full channel tiles and a half one; 32: a half one alone
    _check_conv3x3(H, W, ci, co)


@pytest.mark.parametrize("H,W", [(7, 9), (8, 6), (1, 1), (2, 5), (17, 16)])  # odd and even sides; 17 x 16 -> 9 x 8
def test_conv3x3_stride2(H, W):
    _check_conv3x3(H, W, 64, 96, stride=2)


@pytest.mark.parametrize("bias,pre_relu,res,relu", [(False, False, False, False), (True, True, False, False), (True, True, True, False),
                                                    (True, False, False, True), (False, True, True, True)])
def test_conv3x3_flags(bias, pre_relu, res, relu):
    _check_conv3x3(7, 9, 64, 96, bias=bias, pre_relu=pre_relu, res=res, relu=relu)


def test_conv3x3_refusals():
    from upnerf_amd import _lib
    p = lambda n: ctypes.c_void_p(4096 * n)
    mk = lambda **kw: _lib.Conv3x3Args(**{**dict(H=2, W=2, C_in=32, C_out=32, stride=1, x=p(1), ldx=32, w=p(9), bias=p(10), res=None,
                                                 ldr=32, y=p(2), ldy=32), **kw})
    call = lambda a: _lib.lib.upnerf_conv3x3(ctypes.byref(a), None)
    for bad in (dict(C_in=48), dict(C_out=16), dict(C_in=1056, ldx=1056), dict(stride=3), dict(stride=0)):
        assert call(mk(**bad)) == -2, bad
    for bad in (dict(x=None), dict(w=None), dict(y=None), dict(H=0), dict(y=p(1)), dict(y=ctypes.c_void_p(4096 + 256)),
                dict(res=p(2)), dict(res=p(1)), dict(ldx=16), dict(ldy=34), dict(x=ctypes.c_void_p(4100)), dict(res=p(3), ldr=8)):
        assert call(mk(**bad)) == -1, bad
    assert _lib.lib.upnerf_conv3x3(None, None) == -1


# ---- 2. upnerf_upsample2x ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cn", [4, 33])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 4), (3, 2), (5, 7)])
def test_upsample2x(H, W, Cn):
    from upnerf_amd import _lib
    g = torch.Generator().manual_seed(H * 10 + W + Cn)
    x = torch.randn(H, W, Cn, generator=g)
    want = R.upsample2x(x.double())
    xd = torch.cat([x.reshape(H * W, Cn), torch.full((1, Cn), float("nan"))]).cuda()
    y = torch.full((4 * H * W + 1, Cn), 7.0, device="cuda")
    a = _lib.Upsample2xArgs(H=H, W=W, C=Cn, x=xd.data_ptr(), ldx=Cn, y=y.data_ptr(), ldy=Cn)
    assert _lib.lib.upnerf_upsample2x(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    err = _rel(y[:-1].reshape(2 * H, 2 * W, Cn), want)
    print(f"upsample2x {H}x{W} C={Cn}: {err:.2e} of max-abs")
    assert err < 1e-6  # four products and three sums of fp32 values: a few 2^-24 of the largest
    assert torch.equal(y[-1].cpu(), torch.full((Cn,), 7.0))
    a.y = xd.data_ptr()
    assert _lib.lib.upnerf_upsample2x(ctypes.byref(a), None) == -1 and _lib.lib.upnerf_upsample2x(None, None) == -1


# ---- 3. upnerf_resize_cubic ----------------------------------------------------------------------------------------------------

def _resize(x, h, w, H, W, Cn, u8=0, affine=False, mean=(0.5, 0.5, 0.5), std=(0.5, 0.25, 0.125)):
    from upnerf_amd import _lib
    y = torch.full((H * W * Cn + 1,), 7.0, device="cuda")
    a = _lib.ResizeCubicArgs(h=h, w=w, H=H, W=W, C=Cn, u8=u8, affine=int(affine), x=x.data_ptr(), y=y.data_ptr())
    a.mean[:], a.std[:] = mean, std
    assert _lib.lib.upnerf_resize_cubic(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert float(y[-1]) == 7.0
    return y[:-1].reshape(H, W, Cn)


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("h,w,H,W", [(5, 7, 11, 4), (11, 4, 5, 7), (5, 7, 5, 7)])
def test_resize_cubic(h, w, H, W, Cn, affine):
    g = torch.Generator().manual_seed(h + W + Cn)
    x = torch.rand(h, w, Cn, generator=g)
    want = R.cubic(x.double(), H, W)
    mean, std = torch.tensor([0.5, 0.5, 0.5])[:Cn].double(), torch.tensor([0.5, 0.25, 0.125])[:Cn].double()
    if affine:
        want = (want - mean) / std
    got = _resize(x.cuda(), h, w, H, W, Cn, affine=affine)
    err = _rel(got, want)
    print(f"resize_cubic {h}x{w} -> {H}x{W} C={Cn} affine={affine}: {err:.2e} of max-abs")
    assert err < REL_GATE
    if (h, w) == (H, W) and not affine:
        assert torch.equal(got.cpu(), x)  # the identity size: coefficients (0, 1, 0, 0)


def test_resize_cubic_uint8_and_refusals():
    from upnerf_amd import _lib
    img = R.make_photo(9, 6, 4)
    got = _resize(img.cuda(), 9, 6, 13, 8, 3, u8=1, affine=True)
    want = (R.cubic(img.double() / 255, 13, 8) - 0.5) / torch.tensor([0.5, 0.25, 0.125]).double()
    assert _rel(got, want) < REL_GATE
    one = ctypes.c_void_p(16)
    mk = lambda **kw: _lib.ResizeCubicArgs(**{**dict(h=4, w=4, H=8, W=8, C=3, x=one, y=one), **kw})
    assert _lib.lib.upnerf_resize_cubic(ctypes.byref(mk(C=2)), None) == -2
    for bad in (dict(h=0), dict(W=0), dict(x=None), dict(y=None), dict(affine=1)):  # (affine with std = 0)
        assert _lib.lib.upnerf_resize_cubic(ctypes.byref(mk(**bad)), None) == -1, bad


# ---- 4. upnerf_depth_to_space, upnerf_vit_patches16 ---------------------------------------------------------------------------

@pytest.mark.parametrize("s,Cn", [(2, 32), (4, 8), (2, 5)])
def test_depth_to_space_is_the_permuted_linear_output_plus_bias(s, Cn):
    from upnerf_amd import _lib
    g = torch.Generator().manual_seed(s + Cn)
    H, W = 3, 5
    wide, b = torch.randn(H * W, s * s * Cn, generator=g), torch.randn(Cn, generator=g)
    want = wide.reshape(H, W, s, s, Cn).permute(0, 2, 1, 3, 4).reshape(H * s * W * s, Cn) + b
    xd, bd = wide.cuda(), b.cuda()
    y = torch.full((H * W * s * s + 1, Cn), 7.0, device="cuda")
    a = _lib.DepthToSpaceArgs(H=H, W=W, C=Cn, s=s, x=xd.data_ptr(), ldx=s * s * Cn, bias=bd.data_ptr(), y=y.data_ptr(), ldy=Cn)
    assert _lib.lib.upnerf_depth_to_space(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:-1].cpu(), want) and torch.equal(y[-1].cpu(), torch.full((Cn,), 7.0))
    a.s = 3
    assert _lib.lib.upnerf_depth_to_space(ctypes.byref(a), None) == -2
    a.s, a.ldx = s, Cn
    assert _lib.lib.upnerf_depth_to_space(ctypes.byref(a), None) == -1


@pytest.mark.parametrize("H,W,P", [(32, 48, 16), (35, 20, 16), (8, 12, 4)])
def test_patches16_is_an_unfold(H, W, P):
    from upnerf_amd import _lib
    x = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(H))
    h0, w0 = H // P, W // P
    want = F.unfold(x.permute(2, 0, 1)[None, :, :h0 * P, :w0 * P], kernel_size=P, stride=P)[0].T  # [T][(c, ky, kx)]
    rows = torch.full((h0 * w0 + 1, 3 * P * P), 7.0, device="cuda")
    xd = x.cuda()
    a = _lib.VitPatches16Args(H=H, W=W, patch=P, image=xd.data_ptr(), rows=rows.data_ptr())
    assert _lib.lib.upnerf_vit_patches16(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows[:-1].cpu(), want.contiguous()) and float(rows[-1, 0]) == 7.0
    a.patch = 0
    assert _lib.lib.upnerf_vit_patches16(ctypes.byref(a), None) == -1


# ---- 5. the whole network ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    cfg = R.CONFIGS[name]
    sd = R.make_params(**cfg)
    x = R.make_input(cfg["H"], cfg["W"], cfg["seed"])
    out, stages = R.forward_net(sd, x, **cfg)
    return cfg, sd, x, out, stages


def _model(name, **kw):
    from upnerf_amd.dpt import DptDepth
    cfg, sd, *_ = _case(name)
    return DptDepth.from_state_dict(sd, **{**R.model_kwargs(cfg), **kw}).to("cuda")


@pytest.mark.parametrize("name", ["a", "b"])
def test_network_against_fp64_at_every_stage(name):
    cfg, sd, x, want, stages = _case(name)
    m = _model(name)
    got, gst = m.forward_net(x.float().cuda(), return_stages=True)
    assert got.shape == want.shape and got.dtype == torch.float32
    worst = 0.0
    for (stage, w), (_, g) in zip(R.stage_list(stages), R.stage_list(gst)):
        assert g.shape == w.shape, stage
        err = _rel(g, w)
        worst = max(worst, err)
        print(f"network {name}, {stage} {tuple(w.shape)}: {err:.2e} of max-abs {float(w.abs().max()):.2f}")
        assert err < REL_GATE, stage
    print(f"network {name}: worst {worst:.2e}")
    first = got.clone()
    assert torch.equal(m.forward_net(x.float().cuda()), first)  # the same bits every run


def test_inverse_depth_end_to_end():
    cfg, sd, *_ = _case("b")
    photo = R.make_photo(50, 70, 1)
    want = R.inverse_depth(sd, photo, 64, cfg)
    m = _model("b", net_size=64)
    assert m.net_size(50, 70) == (32, 64)
    got = m.inverse_depth(photo.cuda())
    assert got.shape == (50, 70) and got.dtype == torch.float32
    err = _rel(got, want)
    print(f"inverse_depth 50x70 via 32x64: {err:.2e} of max-abs {float(want.abs().max()):.2f}")
    assert err < REL_GATE
    f32 = m.inverse_depth((photo.float() / 255).cuda())  # fp32 pixels in [0, 1]: the same map to the rounding of v / 255
    assert _rel(f32, want) < REL_GATE


# ---- 6. the tool: a stub weight file -> <depth_dir>/<stem>.npy -> the dataset ------------------------------------------------

def test_extract_depth_into_the_dataset(tmp_path):
    import scene_synth
    from upnerf_amd.datasets import PhototourismDataset
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_depth as T
    cfg, sd, *_ = _case("b")
    info = scene_synth.write_phototourism_scene(str(tmp_path / "scene"), n_images=3)
    weights = str(tmp_path / "stub.pt")
    torch.save(sd, weights)
    depth_dir = str(tmp_path / "depth")
    names = T.main(["-i", os.path.join(info["root"], "dense", "images"), "-o", depth_dir, "-m", weights, "-t", "dpt_large",
                    "--tsv_path", os.path.join(info["root"], "synth.tsv"), "--optimize"],
                   model_kwargs={**R.model_kwargs(cfg), "net_size": 64})
    assert sorted(names) == sorted(info["names"])
    d = np.load(os.path.join(depth_dir, "img_000.npy"))
    assert d.shape == (30, 40) and d.dtype == np.float32 and np.isfinite(d).all() and d.max() > 0
    near, far = 0.1, 5.0
    tr = PhototourismDataset(info["root"], "synth", feat_dir=None, depth_dir=depth_dir, near=near, far=far, camera_noise=-1,
                             split="train", img_downscale=1)
    inv = tr.all_inv_depths
    assert inv is not None and inv.numel() == tr.N_images_train * 30 * 40
    assert torch.isfinite(inv).all() and float(inv.min()) >= 1 / far - 1e-6 and float(inv.max()) <= 1 / near + 1e-6
    with pytest.raises(NotImplementedError, match="dpt_large"):
        T.main(["-i", "x", "-o", "y", "-m", weights, "-t", "dpt_hybrid"])
    with pytest.raises(NotImplementedError, match="kitti_crop"):
        T.main(["-i", "x", "-o", "y", "-m", weights, "--kitti_crop"])
