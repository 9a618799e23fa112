"""DINO ViT descriptors and their PCA from weights the user supplies: the `<feat_dir>/feature_maps/*.npy` and
`<feat_dir>/pca_infos/*_{mean,components}.npy` that datasets.py reads, which the reference makes with
preprocess/save_dino_feature.py (a dino-vit-features checkout, torch.hub, scikit-learn).

The arithmetic runs in HIP (csrc/dino.hip: `upnerf_vit_patches`, `upnerf_vit_embed`, `upnerf_layernorm`,
`upnerf_vit_attention`, `upnerf_vit_gelu`, `upnerf_vit_residual`, `upnerf_pca_fit`; the projections are `upnerf_linear`);
there is no CPU path and no pretrained file in this repository.  The user has the file: the `dino_vits8` checkpoint;
`DinoViT.load` reads it.

Everything this module knows about the network and the extractor is in the table below (MODEL, KEYS, the functions
`token_grid`, `resize_pos_embed` and `key_rows`, and PREPROCESS).  It is written from memory of DINO's vision_transformer.py
and of dino-vit-features' extractor.py and has NOT been compared with either: neither is installed where this was written,
and neither are the pretrained weights.  A user who finds a mismatch changes this one table."""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import _lib, vit
from .ops import TIMER

# ---- the network: dino_vits8 -----------------------------------------------------------------------------------------
#   patch 8, width D = 384, 12 blocks, 6 heads of 64, MLP ratio 4, qkv_bias=True; LayerNorm eps 1e-6; GELU in its exact erf
#   form; softmax scale head_dim ** -0.5; pre-norm residual blocks:
#       x += proj(attn(norm1 x));  x += fc2(gelu(fc1(norm2 x)))
MODEL = dict(patch=8, heads=6, head_dim=64, mlp_ratio=4, ln_eps=1e-6)
# state-dict keys and shapes (D: width, P: pretraining grid side, i: block); anything else (`norm.*`, heads) is ignored
KEYS = dict(cls="cls_token",                         # [1, 1, D]
            pos="pos_embed",                         # [1, 1 + P * P, D]
            pe_w="patch_embed.proj.weight",          # [D, 3, 8, 8]
            pe_b="patch_embed.proj.bias")            # [D]
BLOCK_KEYS = vit.BLOCK_KEYS  # per block: norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2 (weight and bias each)
# ---- the extractor: ViTExtractor(model_type="dino_vits8", stride=4).extract_descriptors(x, layer=9, facet="key", bin=False,
#      include_cls=False) ----------------------------------------------------------------------------------------------
#   the patch convolution runs at `stride` without padding; the descriptor is the KEY third of blocks[layer].attn.qkv's
#   output without the class token: blocks past `layer`, and block `layer` past its norm1 and the K rows of its qkv, never run
EXTRACTOR = dict(stride=4, layer=9)
# ---- preprocessing: PIL resize to (resize, resize), bilinear (torchvision's Resize on a PIL image), / 255, ImageNet statistics
PREPROCESS = dict(resize=448, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))


def token_grid(H, W, patch=MODEL["patch"], stride=EXTRACTOR["stride"]):
    """(h0, w0) of the patch convolution at `stride` without padding; pixels past the last full patch are not seen."""
    if H < patch or W < patch:
        raise ValueError(f"the image ({H} x {W}) is smaller than one {patch} x {patch} patch")
    return 1 + (H - patch) // stride, 1 + (W - patch) // stride


def resize_pos_embed(pos, h0, w0, H=None, W=None):
    """DINO's interpolate_pos_encoding as the extractor patches it: the P x P patch part of pos_embed [1, 1 + P * P, D]
    resized bicubically (align_corners=False) to (h0, w0) with scale factors ((h0 + 0.1) / P, (w0 + 0.1) / P) that are used as
    given (recompute_scale_factor=False); the class row is kept.  Unchanged when the grid is the pretraining one and the image
    square.  Returns [1 + h0 * w0, D]."""
    n = pos.shape[1] - 1
    P = int(round(math.sqrt(n)))
    if P * P != n:
        raise ValueError(f"pos_embed: {n} patch rows are not a square grid")
    if h0 * w0 == n and H == W:
        return pos[0]
    D = pos.shape[-1]
    grid = pos[0, 1:].reshape(1, P, P, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, scale_factor=((h0 + 0.1) / P, (w0 + 0.1) / P), mode="bicubic", align_corners=False,
                         recompute_scale_factor=False)
    if tuple(grid.shape[-2:]) != (h0, w0):
        raise RuntimeError(f"pos_embed resize gave {tuple(grid.shape[-2:])}, expected {(h0, w0)}")
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(h0 * w0, D)], 0)


def key_rows(D, heads):
    """Source rows of qkv.weight for the descriptor channels.  The extractor orders channels (d, head): channel
    c = d * heads + h holds key component d of head h (`x.permute(0, 2, 3, 1).flatten(-2)` of a [B, heads, tokens, d] tensor),
    so row c of the permuted matrix is source row D + h * 64 + d.  Training from features made here does not depend on this
    order (a fixed permutation of channels trains the same; L2 normalisation and PCA are equivariant to it): it matters only for
    mixing feature files made here with files made by the reference."""
    hd = D // heads
    c = torch.arange(D)
    return D + (c % heads) * hd + c // heads


# ----------------------------------------------------------------------------------------------------------------------

def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class DinoViT:
    """The weights as fp32 tensors plus buffers per image size.  A plain object, not an nn.Module."""

    def __init__(self, params, *, patch=MODEL["patch"], heads=MODEL["heads"], stride=EXTRACTOR["stride"],
                 layer=EXTRACTOR["layer"]):
        def get(key):
            if key not in params:
                raise ValueError(f"missing key {key!r}")
            return params[key]

        def want(key, shape):
            t = get(key)
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
            return _f32(t)

        if patch != MODEL["patch"]:
            raise ValueError(f"the patch kernels are built for {MODEL['patch']} x {MODEL['patch']} patches, got patch={patch}")
        if stride < 1:
            raise ValueError(f"stride must be positive, got {stride}")
        cls = get(KEYS["cls"])
        if cls.dim() != 3 or tuple(cls.shape[:2]) != (1, 1):
            raise ValueError(f"{KEYS['cls']}: expected shape (1, 1, D), got {tuple(cls.shape)}")
        D = int(cls.shape[-1])
        if heads < 1 or D % heads or D // heads != MODEL["head_dim"]:
            raise ValueError(f"width {D} with {heads} heads is a head dim of {D / max(heads, 1):g}; the attention kernel is "
                             f"built for {MODEL['head_dim']}")
        if D % 8:
            raise ValueError(f"width {D} is not a multiple of 8")
        depth = 0
        while f"blocks.{depth}.norm1.weight" in params:
            depth += 1
        if not 0 <= layer < depth:
            raise ValueError(f"layer={layer} with {depth} blocks in the weights")
        pos = get(KEYS["pos"])
        if pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[2] != D or pos.shape[1] < 2:
            raise ValueError(f"{KEYS['pos']}: expected shape (1, 1 + P * P, {D}), got {tuple(pos.shape)}")
        P = int(round(math.sqrt(pos.shape[1] - 1)))
        if P * P != pos.shape[1] - 1:
            raise ValueError(f"{KEYS['pos']}: expected shape (1, 1 + P * P, {D}), got {tuple(pos.shape)}")
        self.D, self.heads, self.patch, self.stride, self.layer, self.depth = D, heads, patch, stride, layer, depth
        self.hidden = MODEL["mlp_ratio"] * D
        self.cls = _f32(cls.reshape(D))
        self.pos = _f32(pos)  # resized per (h0, w0) on the host at setup, resize_pos_embed
        self.pe_w = want(KEYS["pe_w"], (D, 3, patch, patch)).reshape(D, 3 * patch * patch)
        self.pe_b = want(KEYS["pe_b"], (D,))
        dims = {"D": D, "3D": 3 * D, "4D": self.hidden}
        self.blocks = []
        for i in range(layer + 1):  # blocks past `layer` never run and are not kept
            blk = {}
            for name, shape in BLOCK_KEYS:
                if i == layer and not name.startswith(("norm1", "attn.qkv")):
                    continue
                blk[name] = want(f"blocks.{i}.{name}", [dims[s] for s in shape.split(",")])
            self.blocks.append(blk)
        rows = key_rows(D, heads)
        last = self.blocks[layer]
        self.key_w = last.pop("attn.qkv.weight")[rows].contiguous()
        self.key_b = last.pop("attn.qkv.bias")[rows].contiguous()
        self._pos_cache, self._bufs, self._pca_scratch = {}, {}, {}

    @classmethod
    def from_state_dict(cls, sd, **kw):
        return cls(sd, **kw)

    @classmethod
    def load(cls, path, **kw):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        for wrap in ("state_dict", "teacher", "model"):  # (a training checkpoint keeps the backbone one level down)
            if isinstance(sd, dict) and KEYS["cls"] not in sd and wrap in sd and isinstance(sd[wrap], dict):
                sd = sd[wrap]
        sd = {k[len("backbone."):] if k.startswith("backbone.") else k: v for k, v in sd.items()}
        return cls.from_state_dict(sd, **kw)

    def _tensors(self):
        yield from ("cls", "pe_w", "pe_b", "key_w", "key_b")

    def to(self, device):
        for n in self._tensors():
            setattr(self, n, getattr(self, n).to(device))
        self.blocks = [{k: v.to(device) for k, v in b.items()} for b in self.blocks]
        self._pos_cache, self._bufs, self._pca_scratch = {}, {}, {}
        return self

    def cuda(self):
        return self.to("cuda")

    @property
    def device(self):
        return self.cls.device

    def grid(self, H, W):
        return token_grid(H, W, self.patch, self.stride)

    def _pos_rows(self, H, W, device):
        h0, w0 = self.grid(H, W)
        key = (h0, w0, H == W, str(device))
        if key not in self._pos_cache:
            self._pos_cache[key] = resize_pos_embed(self.pos, h0, w0, H, W).contiguous().to(device)
        return self._pos_cache[key]

    def _buffers(self, T, device):
        key = (T, str(device))
        if key not in self._bufs:
            N, D = T + 1, self.D
            e = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)
            self._bufs[key] = dict(rows=e(T, 3 * self.patch * self.patch), tok=e(N, D), xn=e(N, D), qkv=e(N, 3 * D), att=e(N, D),
                                   hid=e(N, self.hidden))
        return self._bufs[key]

    def descriptors(self, image: torch.Tensor) -> torch.Tensor:
        """image: [H][W][3] on the device, uint8 (divided by 255 on the way in) or fp32 already in [0, 1]; it is normalised with
        the ImageNet statistics as its pixels are gathered.  Returns the key descriptors of block `layer`, [h0][w0][D] fp32."""
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError(f"expected an [H][W][3] image, got {tuple(image.shape)}")
        if not image.is_cuda:
            raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
        if image.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"the extractor takes uint8 or fp32 images (got {image.dtype})")
        if self.device != image.device:
            raise RuntimeError(f"DinoViT weights are on {self.device}, the image on {image.device}; call .to()")
        image = image.contiguous()
        H, W = int(image.shape[0]), int(image.shape[1])
        h0, w0 = self.grid(H, W)
        T, N, D = h0 * w0, h0 * w0 + 1, self.D
        pos = self._pos_rows(H, W, image.device)
        B = self._buffers(T, image.device)
        rows, tok, xn, qkv, att, hid = B["rows"], B["tok"], B["xn"], B["qkv"], B["att"], B["hid"]
        lib, st = _lib.lib, _lib.stream()
        Kp = rows.shape[1]

        pa = _lib.VitPatchesArgs(H=H, W=W, stride=self.stride, u8=int(image.dtype == torch.uint8), image=_lib.ptr(image),
                                 rows=_lib.ptr(rows))
        pa.mean[:], pa.std[:] = PREPROCESS["mean"], PREPROCESS["std"]
        _lib.check(TIMER.run("dino_patches", lambda: lib.upnerf_vit_patches(C.byref(pa), st)), "upnerf_vit_patches")
        vit.linear("dino_patch_proj", T, D, Kp, _lib.ptr(rows), Kp, self.pe_w, self.pe_b, tok.data_ptr() + 4 * D, D)
        _lib.check(TIMER.run("dino_embed", lambda: lib.upnerf_vit_embed(N, D, _lib.ptr(self.cls), _lib.ptr(pos), _lib.ptr(tok), st)),
                   "upnerf_vit_embed")
        vit.run_blocks(self.blocks[:self.layer], N, D, self.heads, self.hidden, tok, xn, qkv, att, hid, "dino")
        last = self.blocks[self.layer]
        vit.layernorm("dino_layernorm", N, D, tok, last["norm1.weight"], last["norm1.bias"], xn, MODEL["ln_eps"])
        out = torch.empty(h0, w0, D, dtype=torch.float32, device=image.device)
        # the key rows in (d, head) order, from token row 1 on: the descriptor map in its final layout
        vit.linear("dino_key", T, D, D, xn.data_ptr() + 4 * D, D, self.key_w, self.key_b, _lib.ptr(out), D)
        return out

    def pca_moments(self, desc: torch.Tensor):
        """(mean [D] fp32, centred Gram matrix [D][D] fp64) of the L2-normalised descriptor rows, on the device."""
        if not desc.is_cuda:
            raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
        if desc.dtype != torch.float32:
            raise TypeError(f"fit_pca takes fp32 descriptors (got {desc.dtype})")
        D = int(desc.shape[-1])
        x = desc.reshape(-1, D).contiguous()
        T = int(x.shape[0])
        if T < 2:
            raise ValueError("fit_pca needs at least two descriptors")
        key = (T, D, str(x.device))
        if key not in self._pca_scratch:
            n = _lib.lib.upnerf_pca_fit_scratch(T, D)
            if n < 0:
                _lib.check(int(n), "upnerf_pca_fit_scratch")
            self._pca_scratch[key] = torch.empty(n, dtype=torch.float64, device=x.device)
        mean = torch.empty(D, dtype=torch.float32, device=x.device)
        gram = torch.empty(D, D, dtype=torch.float64, device=x.device)
        a = _lib.PcaFitArgs(T=T, D=D, x=_lib.ptr(x), ldx=D, mean=_lib.ptr(mean), gram=_lib.ptr(gram))
        st = _lib.stream()
        _lib.check(TIMER.run("dino_pca_fit", lambda: _lib.lib.upnerf_pca_fit(C.byref(a), _lib.ptr(self._pca_scratch[key]), st)),
                   "upnerf_pca_fit")
        return mean, gram

    def fit_pca(self, desc: torch.Tensor, n_components: int = 3):
        """PCA of the L2-normalised descriptors (save_dino_feature.py: `desc / desc.norm(dim=-1, keepdim=True)`, no epsilon, then
        PCA(3)): (mean [D], components [3][D]) fp32 on the device.  The moments are upnerf_pca_fit; the D x D symmetric
        eigenproblem is torch.linalg.eigh in fp64 on the host copy (tiny, once per image).  Components are the leading
        eigenvectors as rows, each signed so that its entry of largest magnitude is positive.

        Two differences from the reference: it calls scikit-learn's PCA(3), which at this size picks a randomised solver with
        an unseeded state, so its files are not reproducible to the bit, and its sign rule depends on the scikit-learn
        version.  The exact eigenvectors computed here are what it approximates."""
        mean, gram = self.pca_moments(desc)
        comps = pca_components(gram.cpu(), n_components)
        return mean, comps.to(torch.float32).to(desc.device)


def pca_components(gram: torch.Tensor, n_components: int = 3) -> torch.Tensor:
    """The `n_components` leading eigenvectors of a symmetric fp64 matrix as rows, by falling eigenvalue, each signed so that
    its entry of largest magnitude is positive."""
    g = gram.to(torch.float64)
    _, vec = torch.linalg.eigh((g + g.T) / 2)
    comps = vec[:, -n_components:].T.flip(0).contiguous()
    idx = comps.abs().argmax(dim=1, keepdim=True)
    return comps * torch.sign(comps.gather(1, idx))


def load_image(path, resize=PREPROCESS["resize"]) -> torch.Tensor:
    """An image file as the uint8 [resize][resize][3] array the extractor takes: decode and bilinear resize in PIL on the host
    (as torchvision's Resize does on a PIL image), next to the decode as in datasets.py."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert("RGB")
    if resize:
        img = img.resize((resize, resize), Image.BILINEAR)
    return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())
