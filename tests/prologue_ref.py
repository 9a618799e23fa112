"""References and case lists of the training step's prologue kernels (upnerf_amd/csrc/rays.hip: upnerf_sample_coarse[_keyed],
upnerf_uniform_keyed, upnerf_ray_aux, upnerf_gather_rays), computed on the CPU and never from a kernel's output.  Each
floating-point reference restates the kernel's arithmetic in its stated operation order and runs in torch.float32 (the fp32
restatement, bit for bit what the oracle / tests/kernel_space.py give) and in torch.float64 on the same fp32 inputs widened;
e32 = |fp32 - fp64| per element is the error any fp32 evaluation makes and feeds the gate of tests/test_hip_prologue.py.
tests/test_prologue_ref_cpu.py pins these restatements and asserts what the GPU test relies on; both generate their cases here."""
import functools
import math

import numpy as np
import torch

from golden_util import orc

AUXK = 80
U_MAX = 1.0 - 2.0 ** -24  # the largest value (x >> 8) * 2^-24 takes, and torch.rand's largest fp32


# ================================================================================================ Philox4x32-10
def philox4x32_10(c, k):
    """numpy restatement of Philox4x32-10 (Salmon et al., SC'11): c [N,4] uint32 counters, k (k0, k1)."""
    c = c.astype(np.uint64).copy()
    k0, k1 = np.uint64(k[0]), np.uint64(k[1])
    M0, M1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[:, 0], M1 * c[:, 2]
        n0 = ((p1 >> np.uint64(32)) ^ c[:, 1] ^ k0) & MASK
        n2 = ((p0 >> np.uint64(32)) ^ c[:, 3] ^ k1) & MASK
        c = np.stack([n0, p1 & MASK, n2, p0 & MASK], 1)
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK
    return c.astype(np.uint32)


def philox_uniform(seed, step, rows, n, draw):
    """The keyed uniforms of the global rows `rows`, [len(rows), n] float32: word (column & 3) of Philox4x32-10 with counter
    (global row, column // 4, step, draw) and key (seed & 0xffffffff, seed >> 32), as (x >> 8) * 2^-24."""
    rows = np.asarray(rows, dtype=np.int64)
    q4 = (n + 3) // 4
    rr, qq = np.meshgrid(rows, np.arange(q4), indexing="ij")
    m = rows.size * q4
    ctr = np.stack([rr.ravel() & 0xFFFFFFFF, qq.ravel(), np.full(m, step), np.full(m, draw)], 1).astype(np.uint32)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(rows.size, q4 * 4)[:, :n]
    return (x >> 8).astype(np.float32) * np.float32(2.0 ** -24)


# ================================================================================================ coarse depths
def coarse_depths(near_far, steps, u, perturb, use_disp, dtype, edges=False):
    """sample_coarse_kernel in `dtype`: near_far [R,2], steps [S], u [R,S] (read when perturb > 0), all fp32 and widened here.
    base_z = near (1 - s) + far s, or 1 / (1 / near (1 - s) + 1 / far s); bin edges = mid-points, the first lower and the last
    upper edge the end depths themselves; z = lower + (upper - lower) (perturb u).  edges: also return (lower, upper)."""
    nf = near_far.to(dtype)
    near, far = nf[:, :1], nf[:, 1:]
    s = steps.to(dtype)
    if not use_disp:
        z = near * (1 - s) + far * s
    else:
        z = 1 / (1 / near * (1 - s) + 1 / far * s)
    lower = upper = z
    if perturb > 0:
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        upper = torch.cat([mid, z[:, -1:]], -1)
        lower = torch.cat([z[:, :1], mid], -1)
        z = lower + (upper - lower) * (perturb * u.to(dtype))
    return (z, lower, upper) if edges else z


# R x S: R S = 255, 256, 257 around the 256-thread block at S = 1; S = 2, 3 where the i > 0 / i < S - 1 arms meet; a block edge
# inside a row (86 x 3 = 258); one row per 64 and the multi-block odd shape
COARSE_SHAPES = ((255, 1), (256, 1), (257, 1), (7, 2), (86, 3), (6, 64), (37, 65))
PERTURBS = (0.0, 0.5, 1.0)
# rows planted behind the random ones (near, far), then the two u rows at the front
COARSE_PLANTED = ((2.0, 2.0), (0.125, 4.0), (2.0 ** -10, 2.0 ** 10))
KEYED = dict(seed=(0xC0FFEE11 << 32) | 0x12345678, step=2 ** 24 - 1, row0=5, row_stride=3)


@functools.lru_cache(maxsize=None)
def coarse_case(R, S):
    """(near_far [R,2], steps [S], u [R,S]) in fp32: near in [0.05, 0.3], far in [3, 6], both fixed points of x -> 1 / (1 / x) in
    fp32 (column 0 and the last column of disparity mode then ARE near and far); u row 0 all 0, row 1 all 1 - 2^-24; the last
    three rows COARSE_PLANTED."""
    g = torch.Generator().manual_seed(1000 * S + R)
    nf = torch.stack([torch.rand(R, generator=g) * 0.25 + 0.05, torch.rand(R, generator=g) * 3.0 + 3.0], 1)
    for _ in range(4):
        nf = 1 / (1 / nf)
    u = torch.rand(R, S, generator=g)
    u[0], u[1] = 0.0, U_MAX
    nf[R - len(COARSE_PLANTED):] = torch.tensor(COARSE_PLANTED)
    return nf, torch.linspace(0, 1, S), u


def keyed_u(R, S):
    k = KEYED
    return torch.from_numpy(philox_uniform(k["seed"], k["step"], k["row0"] + k["row_stride"] * np.arange(R), S, 0))


@functools.lru_cache(maxsize=None)
def coarse_refs(R, S, use_disp, perturb, keyed=False):
    """(z in fp32, z in fp64, lower edges in fp32) of coarse_case(R, S); keyed: u = the Philox draws of KEYED."""
    nf, steps, u = coarse_case(R, S)
    if keyed:
        u = keyed_u(R, S)
    z32, lo32, _ = coarse_depths(nf, steps, u, perturb, use_disp, torch.float32, edges=True)
    return z32, coarse_depths(nf, steps, u, perturb, use_disp, torch.float64), lo32


# ================================================================================================ keyed uniforms
UNIFORM_N = (1, 2, 3, 4, 5, 7, 8, 129)
UNIFORM_R = (1, 64, 257)
UNIFORM_DRAWS = (0, 1, 7)
UNIFORM_KEY = dict(seed=(0x89ABCDEF << 32) | 0x01234567, step=4711, row0=70000, row_stride=8)  # rows up to 72048 > 2^16


# ================================================================================================ direction encoding
def ray_aux(d, a_rows, wk, dtype):
    """ray_aux_kernel in `dtype`: [d | per axis n: sin(d_n fl32(pi) 2^k) wk_k (k = 0..3), cos(...) wk_k (k = 0..3) | a | 0], the
    fp32 inputs (d [R,3], a_rows [R,48] or None, wk 4 floats) widened; the argument is ONE product d_n * (fl32(pi) 2^k)."""
    R = d.shape[0]
    x = d.to(dtype)
    pi32 = torch.tensor(math.pi, dtype=torch.float32).to(dtype)
    w = torch.tensor(wk, dtype=torch.float32).to(dtype)
    out = torch.zeros(R, AUXK, dtype=dtype)
    out[:, :3] = x
    for n in range(3):
        for k in range(4):
            arg = x[:, n] * (pi32 * 2.0 ** k)
            out[:, 3 + 8 * n + k] = torch.sin(arg) * w[k]
            out[:, 3 + 8 * n + 4 + k] = torch.cos(arg) * w[k]
    if a_rows is not None:
        out[:, 27:75] = a_rows.to(dtype)
    return out


AUX_R = (1, 127, 128, 129)
# (1, 0.75, 0.25, 0) is the old test's; (0, 0, 0, 1) tells a reversed band order from the right one
AUX_WK = ((1.0, 1.0, 1.0, 1.0), (1.0, 0.75, 0.25, 0.0), (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
AUX_PLANTED = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0),
               (0.0, 0.0, -1.0), (1.0, -1.0, 0.0))


@functools.lru_cache(maxsize=None)
def aux_case(R):
    """(d [R,3], a_rows [R,48]) in fp32: unit directions on the even rows, un-normalised ones of norm in (1, 4] on the odd rows (the
    validation path passes such), the first min(R, 8) of AUX_PLANTED as the last rows."""
    g = torch.Generator().manual_seed(77 + R)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=1)
    d[1::2] *= torch.rand(d[1::2].shape[0], 1, generator=g) * 2.9 + 1.05
    K = min(R, len(AUX_PLANTED))
    d[R - K:] = torch.tensor(AUX_PLANTED[:K])
    return d, torch.rand(R, 48, generator=g) * 2 - 1


# ================================================================================================ ray gather
GATHER_KEYS = ("ray_infos", "directions", "img_idx", "c2w", "rgbs", "feats", "inv_depths")
GATHER_C = (1, 63, 64, 65, 384)
GATHER_H = (1, 2, 9)
GATHER_R = (1, 4, 5, 261)
GATHER_N, GATHER_I = 300, 3


def gather(bufs, idx):
    return orc.sample_train_rays(bufs, idx)


def planted_coords(h):
    """0, 1, k / (h - 1) (exact in fp32 for h - 1 = 1, 8) and the fp32 neighbours of each inside [0, 1]."""
    base = sorted({0.0, 1.0} | {k / (h - 1) for k in range(h)} if h > 1 else {0.0, 1.0})
    v = []
    for b in np.asarray(base, dtype=np.float32):
        v += [b] + ([np.nextafter(b, np.float32(-1))] if b > 0 else []) + ([np.nextafter(b, np.float32(2))] if b < 1 else [])
    return torch.from_numpy(np.asarray(v, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def gather_case(C, h):
    """The flat buffers of a split of GATHER_N rays in GATHER_I images with [h][h][C] feature maps, and the number of planted rays
    at its front: every planted coordinate paired with another planted one, with a random row and with a random column.  The
    random coordinates are (cell + frac) / (h - 1) with frac in [0.01, 0.99]: 1e-2 / (h - 1) away from the floor's steps."""
    g = torch.Generator().manual_seed(31 * C + h)
    N, I = GATHER_N, GATHER_I
    cells = max(h - 1, 1)
    pxl = (torch.randint(0, cells, (N, 2), generator=g) + torch.rand(N, 2, generator=g) * 0.98 + 0.01) / cells
    P = planted_coords(h)
    n = P.numel()
    pxl[:n, 0], pxl[:n, 1] = P, P[(7 * torch.arange(n) + 3) % n]
    pxl[n:2 * n, 0] = P
    pxl[2 * n:3 * n, 1] = P
    img = torch.randint(0, I, (N, 1), generator=g).float()
    img[0], img[N - 1] = I - 1, 0
    bufs = {"all_ray_infos": torch.cat([torch.rand(N, 2, generator=g), img], 1),
            "all_directions": torch.randn(N, 3, generator=g), "all_rgbs": torch.rand(N, 3, generator=g),
            "all_pxl_coords": pxl, "all_inv_depths": torch.rand(N, generator=g),
            "feat_maps": torch.randn(I, h, h, C, generator=g), "poses": torch.randn(I, 3, 4, generator=g)}
    return bufs, 3 * n


def gather_idx(R):
    """The last and the first ray of the split, a repeat, then the rays in order (R = 261 reaches every planted one)."""
    return torch.tensor(([GATHER_N - 1, 0, 7, 7] + list(range(GATHER_N)))[:R], dtype=torch.int64)


def bilinear(bufs, idx, dtype):
    """feats [R,C] in `dtype`: the reference's bilinear sample, vectorised and written independently of the oracle's loop --
    (y, x) = coords (h - 1), corners (floor, min(h - 1, floor + 1)), weights (y2 - y)(x2 - x) ..., summed 11, 12, 21, 22."""
    fm = bufs["feat_maps"].to(dtype)
    h = fm.shape[1]
    img = bufs["all_ray_infos"][idx, 2].long()
    pm = bufs["all_pxl_coords"][idx].to(dtype) * (h - 1)
    y, x = pm[:, 0], pm[:, 1]
    y1, x1 = torch.floor(y).long(), torch.floor(x).long()
    y2, x2 = torch.clamp(y1 + 1, max=h - 1), torch.clamp(x1 + 1, max=h - 1)
    wy2, wy1, wx2, wx1 = y2.to(dtype) - y, y - y1.to(dtype), x2.to(dtype) - x, x - x1.to(dtype)
    v = (wy2 * wx2)[:, None] * fm[img, y1, x1]
    v = v + (wy2 * wx1)[:, None] * fm[img, y1, x2]
    v = v + (wy1 * wx2)[:, None] * fm[img, y2, x1]
    return v + (wy1 * wx1)[:, None] * fm[img, y2, x2]


@functools.lru_cache(maxsize=None)
def gather_refs(C, h, R):
    """(oracle batch, feats in fp32, feats in fp64) of gather_case(C, h) at gather_idx(R)."""
    bufs, _ = gather_case(C, h)
    idx = gather_idx(R)
    return gather(bufs, idx), bilinear(bufs, idx, torch.float32), bilinear(bufs, idx, torch.float64)
