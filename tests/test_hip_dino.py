"""DINO ViT descriptors and their PCA on the device (csrc/dino.hip, upnerf_amd/dino.py) against the fp64 restatement of their
definition (tests/dino_ref.py) on seeded random weights: each kernel alone at its tile edges, the whole extractor at the
project's parity criterion, the PCA against fp64 eigenvectors, and the round trip through the tool's writer into the
phototourism dataset and the PCA picture."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import dino_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_GATE = 1e-4  # README: "<=1e-4 rel, fp32", taken against the reference map's max-abs
AT_BQ, AT_BK = 128, 64  # the attention kernel's query and key tiles (32-key subtiles)


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


# ---- 1. upnerf_vit_attention ----------------------------------------------------------------------------------------

def _attention(qkv, N, heads, guard=3):
    """One launch on a [N + guard][3 D] buffer; returns the [N + guard][D] output buffer (guard rows pre-set to 7)."""
    from upnerf_amd import _lib
    D = heads * 64
    out = torch.full((N + guard, D), 7.0, device="cuda")
    a = _lib.VitAttentionArgs(N=N, heads=heads, head_dim=64, q=qkv.data_ptr(), k=qkv.data_ptr() + 4 * D, v=qkv.data_ptr() + 8 * D,
                              ldq=3 * D, ldk=3 * D, ldv=3 * D, scale=0.125, out=out.data_ptr(), ldo=D)
    assert _lib.lib.upnerf_vit_attention(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    return out


def _check_attention(qkv_host, N, heads, gate=REL_GATE):
    """qkv_host: [N][3 D] fp32.  Guard rows of NaN behind the inputs, of 7 behind the output."""
    D = heads * 64
    buf = torch.full((N + 3, 3 * D), float("nan"))
    buf[:N] = qkv_host
    x = qkv_host.double()
    want = R.attention(x[:, :D], x[:, D:2 * D], x[:, 2 * D:], heads)
    dev = buf.cuda()
    out = _attention(dev, N, heads)
    assert torch.isfinite(out[:N]).all()
    err = _rel(out[:N], want)
    print(f"attention N={N} heads={heads}: {err:.2e} of max-abs")
    assert err < gate
    assert torch.equal(out[N:].cpu(), torch.full((3, D), 7.0))  # rows past N are not stored
    assert torch.equal(_attention(dev, N, heads), out)  # the same bits every run
    return out[:N].cpu(), want


@pytest.mark.parametrize("heads", [1, 6])
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 257])
def test_attention_against_fp64(N, heads):
    g = torch.Generator().manual_seed(N * 10 + heads)
    _check_attention(torch.randn(N, 3 * heads * 64, generator=g) * 1.5, N, heads)


def test_attention_logits_reaching_80():
    """Scaled logits from -80 to +80, each row's maximum at its own index: for rows past the first key tile the running
    maximum rises by up to 160 mid-stream and the accumulator is rescaled by exp(-160)."""
    N = 200
    g = torch.Generator().manual_seed(5)
    k = torch.randint(0, 2, (N, 64), generator=g).float() * 2 - 1
    k[100:] = -k[:100]
    q = 10 * k
    v = torch.randn(N, 64, generator=g)
    logits = q.double() @ k.double().T / 8
    assert logits.max() >= 80 and logits.min() <= -80
    _check_attention(torch.cat([q, k, v], 1), N, 1)


def test_attention_one_key_dominates_every_row():
    N, j0 = 130, 97
    g = torch.Generator().manual_seed(6)
    q = torch.randn(N, 64, generator=g) + 3
    k = torch.randn(N, 64, generator=g) * 0.1
    k[j0] = 5
    v = torch.randn(N, 64, generator=g)
    got, want = _check_attention(torch.cat([q, k, v], 1), N, 1)
    assert float((want - v[j0].double()).abs().max()) < 1e-9  # (the case is what it says)
    assert float((got - v[j0]).abs().max()) < 1e-6


def test_attention_refusals():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    mk = lambda **kw: _lib.VitAttentionArgs(**{**dict(N=4, heads=2, head_dim=64, q=one, k=one, v=one, ldq=384, ldk=384, ldv=384,
                                                      scale=0.125, out=one, ldo=128), **kw})
    call = lambda a: _lib.lib.upnerf_vit_attention(ctypes.byref(a), None)
    assert call(mk(head_dim=32)) == -2
    for bad in (dict(N=0), dict(heads=0), dict(q=None), dict(out=None), dict(ldk=127), dict(ldo=130), dict(ldq=386),
                dict(v=ctypes.c_void_p(20))):
        assert call(mk(**bad)) == -1, bad


# ---- 2. upnerf_layernorm -------------------------------------------------------------------------------------------

def _layernorm(x, w, b, eps=1e-6):
    from upnerf_amd import _lib
    M, D = x.shape
    y = torch.full((M + 1, D), 7.0, device="cuda")
    rc = _lib.lib.upnerf_layernorm(M, D, x.data_ptr(), D, w.data_ptr(), b.data_ptr(), eps, y.data_ptr(), D, _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(y[M].cpu(), torch.full((D,), 7.0))
    return y[:M]


@pytest.mark.parametrize("D", [4, 128, 384, 1024])
def test_layernorm(D):
    g = torch.Generator().manual_seed(D)
    M = 6  # four rows per workgroup: two workgroups, the second half empty
    x = 1e4 + torch.randn(M, D, generator=g)  # the mean is 1e4 times the spread: E[x^2] - E[x]^2 in fp32 would be noise
    x[4] = torch.randn(D, generator=g) * 3
    x[5] = 2.5  # a constant row: variance 0, eps decides
    w, b = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    want = R.layernorm(x.double(), w.double(), b.double())
    got = _layernorm(x.cuda(), w.cuda(), b.cuda())
    err = _rel(got[:5], want[:5])
    print(f"layernorm D={D}: {err:.2e} of max-abs")
    assert err < 1e-5
    assert torch.equal(got[5].cpu(), b)  # exactly the bias
    assert torch.equal(_layernorm(x.cuda(), w.cuda(), b.cuda()), got)


def test_layernorm_refusals():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    f = lambda M, D, ldx=None, ldy=None: _lib.lib.upnerf_layernorm(M, D, one, ldx or D, one, one, 1e-6, one, ldy or D, None)
    assert f(4, 1028) == -2 and f(4, 6) == -2
    assert f(0, 8) == -1 and f(4, 8, ldx=4) == -1 and f(4, 8, ldy=10) == -1


# ---- 3. upnerf_vit_patches, upnerf_vit_gelu ---------------------------------------------------------------------------

@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "fp32"])
@pytest.mark.parametrize("H,W,stride,grid", [(40, 40, 4, (9, 9)), (36, 52, 4, (8, 12)), (32, 32, 8, (4, 4)), (43, 41, 4, (9, 9))])
def test_patches(H, W, stride, grid, u8):
    """Gate: 1e-6 absolute.  With u = 2^-24: v / 255, the fp32 mean and the subtraction err by at most (1 + 0.485 + 1) u together,
    divided by std >= 0.224 that is 11.2 u; the fp32 std and the division's rounding add 2 |out| u <= 5.4 u: 16.6 u = 9.9e-7."""
    from upnerf_amd import _lib
    img = R.make_image(H, W, H)
    if not u8:
        img = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(W))
    assert R.token_grid(H, W, 8, stride) == grid
    T = grid[0] * grid[1]
    rows = torch.full((T + 1, 192), 7.0, device="cuda")
    dev = img.cuda()
    a = _lib.VitPatchesArgs(H=H, W=W, stride=stride, u8=int(u8), image=dev.data_ptr(), rows=rows.data_ptr())
    a.mean[:], a.std[:] = R.MEAN, R.STD
    assert _lib.lib.upnerf_vit_patches(ctypes.byref(a), _lib.stream()) == 0
    torch.cuda.synchronize()
    want = R.patches(img, stride)
    assert want.shape == (T, 192)
    assert float((rows[:T].double().cpu() - want).abs().max()) < 1e-6
    assert torch.equal(rows[T].cpu(), torch.full((192,), 7.0))


def test_gelu():
    from upnerf_amd import _lib
    x = torch.cat([torch.tensor([0.0, -0.0, 1e-4, -1e-4, 6.0, -6.0, 20.0, -20.0]), torch.linspace(-8, 8, 300)])
    buf = torch.cat([x, torch.tensor([7.0])]).cuda()
    assert _lib.lib.upnerf_vit_gelu(buf.data_ptr(), x.numel(), _lib.stream()) == 0
    torch.cuda.synchronize()
    want = R.gelu(x.double())
    assert float((buf[:-1].double().cpu() - want).abs().max()) < 1e-6
    assert float(buf[-1]) == 7.0 and float(buf[0]) == 0.0 and float(buf[1]) == 0.0
    assert _lib.lib.upnerf_vit_gelu(None, 4, None) == -1 and _lib.lib.upnerf_vit_residual(buf.data_ptr(), None, 4, None) == -1


def test_embed_and_residual():
    from upnerf_amd import _lib
    g = torch.Generator().manual_seed(2)
    N, D = 19, 24
    tok, pos, cls = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g), torch.randn(D, generator=g)
    dev = tok.cuda()
    assert _lib.lib.upnerf_vit_embed(N, D, cls.cuda().data_ptr(), pos.cuda().data_ptr(), dev.data_ptr(), _lib.stream()) == 0
    want = tok + pos
    want[0] = cls + pos[0]
    assert torch.equal(dev.cpu(), want)
    y = torch.randn(N * D - 1, generator=g)
    assert _lib.lib.upnerf_vit_residual(dev.data_ptr(), y.cuda().data_ptr(), N * D - 1, _lib.stream()) == 0
    want.view(-1)[:-1] += y
    assert torch.equal(dev.cpu(), want)


# ---- 4. the extractor end to end -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _params(D, heads, depth):
    return R.make_params(D=D, heads=heads, depth=depth, P=5, seed=D + depth)


def _model(D, heads, depth, layer, stride, sd=None):
    from upnerf_amd.dino import DinoViT
    return DinoViT.from_state_dict(sd or _params(D, heads, depth), heads=heads, stride=stride, layer=layer).to("cuda")


@pytest.mark.parametrize("cfg", R.E2E, ids=lambda c: "-".join(map(str, c)))
def test_descriptors_against_fp64(cfg):
    D, heads, depth, layer, H, W, stride = cfg
    sd = _params(D, heads, depth)
    img = R.make_image(H, W, H + W)
    want = R.descriptors(sd, img, heads=heads, stride=stride, layer=layer)
    m = _model(D, heads, depth, layer, stride)
    got = m.descriptors(img.cuda())
    assert got.shape == want.shape and got.dtype == torch.float32
    err = _rel(got, want)
    print(f"descriptors {cfg}: {err:.2e} of max-abs {float(want.abs().max()):.2f}")
    assert err < REL_GATE
    assert torch.equal(m.descriptors(img.cuda()), got)
    f32 = m.descriptors((img.float() / 255).cuda())  # fp32 pixels in [0, 1]: the same map to the rounding of v / 255
    assert _rel(f32, want) < REL_GATE


def test_descriptor_channels_are_d_major_head_minor():
    D, heads, h1 = 128, 2, 1
    sd = dict(_params(D, heads, 3))
    img = R.make_image(32, 32, 3).cuda()
    base = _model(D, heads, 3, 0, 8, sd).descriptors(img)
    bias = sd["blocks.0.attn.qkv.bias"].clone()
    bias[D + h1 * 64:D + (h1 + 1) * 64] += 1000 + torch.arange(64.)  # key component d of head h1: + 1000 + d
    sd["blocks.0.attn.qkv.bias"] = bias
    diff = (_model(D, heads, 3, 0, 8, sd).descriptors(img) - base).cpu()
    want = torch.zeros(D)
    want[torch.arange(64) * heads + h1] = 1000 + torch.arange(64.)
    assert float((diff - want).abs().max()) < 1e-3


# ---- 5. fit_pca -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,D", [(81, 128), (625, 384), (2100, 128)])  # (the last: three chunks of fp64 partials)
def test_fit_pca(T, D):
    x = R.planted_descriptors(T, D, seed=T)
    mean, comps, val = R.pca(x)
    gaps = [float((val[i] - val[i + 1]) / val[0]) for i in range(3)]
    assert min(gaps) > 0.05, gaps  # well-separated leading eigenvalues: the eigenvectors are well conditioned
    m = _model(128, 2, 3, 0, 8)
    shape = (9, 9, D) if T == 81 else (T, D)
    gm, gc = m.fit_pca(x.cuda().reshape(shape))
    assert gm.shape == (D,) and gc.shape == (3, D) and gm.dtype == gc.dtype == torch.float32
    em, ec = float((gm.double().cpu() - mean).abs().max()), float((gc.double().cpu() - comps).abs().max())
    print(f"pca T={T} D={D}: mean {em:.2e}, components {ec:.2e}, gaps {gaps}")
    assert em < 1e-6 and ec < 1e-4
    for row in gc.cpu():
        assert row[row.abs().argmax()] > 0
    m2, g2 = m.pca_moments(x.cuda())
    m3, g3 = m.pca_moments(x.cuda())
    assert torch.equal(g2, g3) and torch.equal(m2, m3) and torch.equal(g2, g2.T)


# ---- 6. round trip: the tool's writer -> the dataset -> the PCA picture --------------------------------------------

def test_round_trip_into_the_dataset(tmp_path):
    import scene_synth
    from upnerf_amd.datasets import PhototourismDataset
    from upnerf_amd.dino import load_image
    from upnerf_amd.visualization import pca_image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_features as T
    info = scene_synth.write_phototourism_scene(str(tmp_path / "scene"), n_images=3)
    m = _model(128, 2, 3, 2, 4)

    def extract(path):
        desc = m.descriptors(load_image(path, 40).cuda())
        mean, comps = m.fit_pca(desc)
        return desc.cpu().numpy(), mean.cpu().numpy(), comps.cpu().numpy()

    feat_dir = str(tmp_path / "feats")
    names = T.run(os.path.join(info["root"], "dense", "images"), feat_dir, extract, os.path.join(info["root"], "synth.tsv"))
    assert sorted(names) == sorted(info["names"])
    assert np.load(os.path.join(feat_dir, "feature_maps", "img_000.npy")).shape == (9, 9, 128)
    ds = PhototourismDataset(info["root"], "synth", feat_dir=feat_dir, depth_dir=None, near=0.1, far=5.0, camera_noise=-1,
                             split="val", img_downscale=1, val_img_idx=[0])
    item = ds[0]
    W, H = item["img_wh"].tolist()
    assert item["feats"].shape == (W * H, 128) and item["pca_m"].shape == (128,) and item["pca_c"].shape == (3, 128)
    img, rgb = pca_image(item["feats"], torch.as_tensor(item["pca_m"]).cuda(), torch.as_tensor(item["pca_c"]).cuda(), (W, H))
    assert img.shape == (H, W, 3) and torch.isfinite(img).all() and float(img.max() - img.min()) > 0.5
    tr = PhototourismDataset(info["root"], "synth", feat_dir=feat_dir, depth_dir=None, near=0.1, far=5.0, camera_noise=-1,
                             split="train", img_downscale=1)
    assert tr.feat_maps.shape == (tr.N_images_train, 9, 9, 128)
