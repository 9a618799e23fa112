"""fp64 restatement of the DINO ViT key-descriptor extractor (the table at the top of upnerf_amd/dino.py) in plain torch, and a
seeded parameter generator.  CPU only; tests/test_dino_ref_cpu.py checks it against itself and in fp32, tests/test_hip_dino.py
holds the HIP kernels to it."""
import math

import torch
import torch.nn.functional as F

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EPS = 1e-6
HEAD_DIM = 64


# (D, heads, blocks, layer, H, W, stride) of the end-to-end cases: 82, 97 and 17 tokens
E2E = ((384, 6, 12, 9, 40, 40, 4), (384, 6, 12, 9, 36, 52, 4), (128, 2, 3, 2, 32, 32, 8), (128, 2, 3, 0, 32, 32, 8))


def make_params(D=384, heads=6, depth=12, P=5, patch=8, seed=0, dtype=torch.float32):
    """Weights at fan_in ** -0.5 scale, qkv at 1.5 times that, LayerNorm gains 1 + 0.2 n, biases and embeddings 0.1-0.5 n."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"cls_token": 0.5 * n(1, 1, D), "pos_embed": 0.5 * n(1, 1 + P * P, D),
          "patch_embed.proj.weight": n(D, 3, patch, patch) * (3 * patch * patch) ** -0.5, "patch_embed.proj.bias": 0.1 * n(D)}
    for i in range(depth):
        b = f"blocks.{i}."
        sd[b + "norm1.weight"], sd[b + "norm1.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)
        sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"] = 1.5 * n(3 * D, D) * D ** -0.5, 0.1 * n(3 * D)
        sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"] = n(D, D) * D ** -0.5, 0.1 * n(D)
        sd[b + "norm2.weight"], sd[b + "norm2.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)
        sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = n(4 * D, D) * D ** -0.5, 0.1 * n(4 * D)
        sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = n(D, 4 * D) * (4 * D) ** -0.5, 0.1 * n(D)
    sd["norm.weight"], sd["norm.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)  # (ignored by the extractor)
    return {k: v.to(dtype) for k, v in sd.items()}


def make_image(H, W, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)


def token_grid(H, W, patch=8, stride=4):
    return 1 + (H - patch) // stride, 1 + (W - patch) // stride


def patches(image, stride, patch=8, dtype=torch.float64):
    """[h0 * w0][3 * 8 * 8] rows in (c, ky, kx) order of the normalised image (uint8: / 255 first; float: already in [0, 1])."""
    x = image.to(dtype) / 255 if image.dtype == torch.uint8 else image.to(dtype)
    x = (x - torch.tensor(MEAN, dtype=dtype)) / torch.tensor(STD, dtype=dtype)
    h0, w0 = token_grid(x.shape[0], x.shape[1], patch, stride)
    rows = [x[ty * stride:ty * stride + patch, tx * stride:tx * stride + patch].permute(2, 0, 1).reshape(-1)
            for ty in range(h0) for tx in range(w0)]
    return torch.stack(rows, 0)


def pos_rows(pos, h0, w0, square):
    n = pos.shape[1] - 1
    P = int(round(math.sqrt(n)))
    if h0 * w0 == n and square:
        return pos[0]
    D = pos.shape[-1]
    grid = pos[0, 1:].reshape(1, P, P, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, scale_factor=((h0 + 0.1) / P, (w0 + 0.1) / P), mode="bicubic", align_corners=False,
                         recompute_scale_factor=False)
    assert tuple(grid.shape[-2:]) == (h0, w0)
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(h0 * w0, D)], 0)


def layernorm(x, w, b, eps=EPS):
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * w + b


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, heads):
    """q, k, v: [N][heads * 64] -> [N][heads * 64] with a materialised score matrix per head."""
    N = q.shape[0]
    sp = lambda t: t.reshape(N, heads, HEAD_DIM).permute(1, 0, 2)
    s = torch.softmax(sp(q) @ sp(k).transpose(1, 2) * HEAD_DIM ** -0.5, dim=-1)
    return (s @ sp(v)).permute(1, 0, 2).reshape(N, heads * HEAD_DIM)


def tokens_before(sd, image, heads, stride, layer, dtype=torch.float64, patch=8):
    """The token matrix [1 + T][D] that enters block `layer` (after `layer` full blocks)."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    D = p["cls_token"].shape[-1]
    H, W = image.shape[:2]
    h0, w0 = token_grid(H, W, patch, stride)
    x = patches(image, stride, patch, dtype) @ p["patch_embed.proj.weight"].reshape(D, -1).T + p["patch_embed.proj.bias"]
    x = torch.cat([p["cls_token"].reshape(1, D), x], 0) + pos_rows(p["pos_embed"], h0, w0, H == W)
    for i in range(layer):
        b = f"blocks.{i}."
        y = layernorm(x, p[b + "norm1.weight"], p[b + "norm1.bias"])
        qkv = y @ p[b + "attn.qkv.weight"].T + p[b + "attn.qkv.bias"]
        a = attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], heads)
        x = x + a @ p[b + "attn.proj.weight"].T + p[b + "attn.proj.bias"]
        y = layernorm(x, p[b + "norm2.weight"], p[b + "norm2.bias"])
        h = gelu(y @ p[b + "mlp.fc1.weight"].T + p[b + "mlp.fc1.bias"])
        x = x + h @ p[b + "mlp.fc2.weight"].T + p[b + "mlp.fc2.bias"]
    return x


def descriptors(sd, image, heads=6, stride=4, layer=9, dtype=torch.float64, permute_rows=False):
    """[h0][w0][D]: the key third of blocks[layer].attn.qkv without the class token, channels in (d, head) order.
    permute_rows: take the permuted weight rows (what the HIP path does) instead of permuting the output."""
    x = tokens_before(sd, image, heads, stride, layer, dtype)
    D = x.shape[-1]
    b = f"blocks.{layer}."
    y = layernorm(x, sd[b + "norm1.weight"].to(dtype), sd[b + "norm1.bias"].to(dtype))[1:]
    w, bias = sd[b + "attn.qkv.weight"].to(dtype), sd[b + "attn.qkv.bias"].to(dtype)
    h0, w0 = token_grid(image.shape[0], image.shape[1], 8, stride)
    if permute_rows:
        c = torch.arange(D)
        rows = D + (c % heads) * HEAD_DIM + c // heads
        return (y @ w[rows].T + bias[rows]).reshape(h0, w0, D)
    k = (y @ w.T + bias)[:, D:2 * D]                      # [T][heads * 64], head-major as the module computes it
    k = k.reshape(1, -1, heads, HEAD_DIM).permute(0, 2, 1, 3)  # [B, heads, T, d]
    return k.permute(0, 2, 3, 1).flatten(-2).reshape(h0, w0, D)  # the extractor's (d, head) flattening


def pca(desc, n=3):
    """fp64 PCA of the L2-normalised rows: (mean [D], components [n][D] signed at the largest entry, eigenvalues falling)."""
    x = desc.reshape(-1, desc.shape[-1]).to(torch.float64)
    x = x / x.norm(dim=-1, keepdim=True)
    m = x.mean(0)
    c = x - m
    val, vec = torch.linalg.eigh(c.T @ c)
    comps = vec[:, -n:].T.flip(0)
    idx = comps.abs().argmax(dim=1, keepdim=True)
    return m, comps * torch.sign(comps.gather(1, idx)), val.flip(0)


def planted_descriptors(T, D, seed=0):
    """Rows with three planted dominant directions of well-separated strength (3 : 2 : 1.2) over isotropic noise."""
    g = torch.Generator().manual_seed(77 + seed)
    q, _ = torch.linalg.qr(torch.randn(D, 3, generator=g, dtype=torch.float64))
    coef = torch.randn(T, 3, generator=g, dtype=torch.float64) * torch.tensor([3.0, 2.0, 1.2], dtype=torch.float64)
    base = torch.randn(D, generator=g, dtype=torch.float64) * 4 / math.sqrt(D)
    x = base + coef @ q.T + 0.05 * torch.randn(T, D, generator=g, dtype=torch.float64)
    return x.to(torch.float32)
