"""Coarse-to-fine baked scenes: the total variation of a scene's point arrays with its gradient (`upnerf_baked_tv`) and the doubling
of a scene's resolution (`upnerf_baked_upsample`, `upnerf_brick_upsample_mark` / `_fill`), for dense grids and for brick pools
(csrc/baked_reg.hip; include/upnerf_hip.h states the definitions).

    value, grad = tv(rgbs, rgbs[..., 3], scene.occupancy, (0, 0, 0, 1), 1e-8)            # dense: TV of sigma alone
    value, grad = tv(pool_coef, pool_sigma, scene.occupancy, w, 1e-8, layout=scene)      # a pool, the face sum included
    finer = scene.upsample()                                                             # 2 C cells per axis, the same layout
    tuner = scene.tune(lr=1e-2, tv_sigma=1e-3, tv_colour=1e-4); tuner = tuner.upsampled()

The TV runs over the cells whose occupancy bit is set; a point whose sigma is exactly zero receives no gradient (the rule of the
marcher's backward pass).  The value comes back as a 0-dim device tensor: no host read.  No atomics anywhere: two runs give the same
bits.  The refined scene is the same continuous field as its parent -- a trilinear interpolant reproduces a trilinear function -- up
to the rounding of the children and the pruning at `level`.  There is no CPU path."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .baked import POINT_BYTES, BakedScene, Layout, _aligned, _aligned_copy, _level, a_scene, brick_table, face_sum as _sum_faces, pool_layout
from .ops import TIMER
from .static_scene import require_cuda

__all__ = ["tv", "tv_backward", "upsample", "MAX_FLOATS"]

MAX_FLOATS = 28  # floats per point of one upnerf_baked_tv launch (the width of its weight array)


def _sigma_stride(sigma: torch.Tensor, shape) -> int:
    """The element stride of `sigma`, a fp32 tensor of the points' shape that is contiguous or a regular view of a wider array
    (rgbs[..., 3]): every stride the same multiple of the contiguous one."""
    if sigma.dtype != torch.float32 or tuple(sigma.shape) != tuple(shape):
        raise ValueError(f"sigma is a fp32 tensor {tuple(shape)}: one per point")
    if sigma.is_contiguous():
        return 1
    k = sigma.stride(-1)
    if k < 1 or tuple(sigma.stride()) != tuple(s * k for s in torch.empty(shape, device="meta").stride()):
        raise ValueError("sigma is contiguous, or a view with one element stride (rgbs[..., 3])")
    return int(k)


def tv_backward(data: torch.Tensor, sigma: torch.Tensor, occupancy, weights: Sequence[float], eps: float, layout=None,
                out: Optional[torch.Tensor] = None, face_sum: bool = True) -> tuple:
    """upnerf_baked_tv.  data: contiguous fp32 [Nz, Ny, Nx, ...] (F floats per point, any trailing shape, none: F = 1) of a dense
    grid, or with `layout` (a pool's baked.Layout, a sparse BakedScene or a PoolParams) [n_bricks, 9, 9, 9, ...] of its pool; sigma: the points' sigmas
    (liveness), `data`'s leading shape, possibly a view such as rgbs[..., 3]; weights: F finite floats; eps > 0.  The gradient is
    ADDED into `out` (data's shape; zeroed here when None).  On a pool the face sum runs over `out` afterwards unless
    face_sum = False, which leaves each copy with what the cells of its own brick give it.  Returns (value, out): the value a 0-dim
    device tensor."""
    require_cuda("baked_reg.tv", data, sigma)
    Cx, Cy, Cz = occupancy.dims
    if layout is not None:
        layout = pool_layout(layout)
        if layout.occupancy.dims != (Cx, Cy, Cz):
            raise ValueError("the layout and the occupancy are of different grids")
        slots, bricks, n_bricks, shape = layout.slots, layout.bricks, layout.shape[0], layout.shape
    else:
        slots = bricks = None
        n_bricks, shape = 0, (Cz + 1, Cy + 1, Cx + 1)
    if data.dtype != torch.float32 or data.dim() < len(shape) or tuple(data.shape[:len(shape)]) != shape or not data.is_contiguous():
        raise ValueError(f"data is a contiguous fp32 tensor {shape + ('...',)}")
    F = data.numel() // int(np.prod(shape))
    w = [float(x) for x in weights]
    if len(w) != F or not 1 <= F <= MAX_FLOATS:
        raise ValueError(f"weights are one float per float of a point ({F} here, {MAX_FLOATS} at the most), got {len(w)}")
    stride = _sigma_stride(sigma, shape)
    if out is None:
        out = torch.zeros_like(data)
    if out.dtype != torch.float32 or tuple(out.shape) != tuple(data.shape) or not out.is_contiguous() or out.device != data.device:
        raise ValueError("out is a contiguous fp32 tensor of data's shape on its device")
    blocks = int(lib.upnerf_baked_tv_blocks(Cx, Cy, Cz, n_bricks))
    if blocks < 0:
        check(blocks, "upnerf_baked_tv_blocks")
    partial = torch.empty(blocks, device=data.device, dtype=torch.float32)
    a = _lib.BakedTvArgs(Cx=Cx, Cy=Cy, Cz=Cz, n_bricks=n_bricks, F=F, sigma_stride=stride, eps=float(eps),
                         w=(C.c_float * 28)(*(w + [0.0] * (28 - F))), words=ptr(occupancy.words), slots=ptr(slots), bricks=ptr(bricks),
                         data=ptr(data), sigma=sigma.data_ptr(), grad=ptr(out), partial=ptr(partial))
    check(TIMER.run("baked_tv", lambda: lib.upnerf_baked_tv(C.byref(a), stream()), units=int(np.prod(shape)) * F), "upnerf_baked_tv")
    if layout is not None and face_sum:
        _sum_faces(out, layout)
    return partial.sum(), out


def tv(data: torch.Tensor, sigma: torch.Tensor, occupancy, weights: Sequence[float], eps: float, layout=None, face_sum: bool = True):
    """(value, grad) of the total variation of `data` (tv_backward into a zeroed gradient)."""
    return tv_backward(data, sigma, occupancy, weights, eps, layout=layout, face_sum=face_sum)


def tuner_tv(tuner) -> torch.Tensor:
    """The TV gradient of a tuner's masters added into its gradient, weights per occupied cell (the host folds 1 / tuner.tv_cells, the number of
    occupied cells counted when the tuner was made, into w); on a pool the per-copy gradient, the caller sums the faces.  Returns the value."""
    ls, lc = tuner.tv_sigma / tuner.tv_cells, tuner.tv_colour / tuner.tv_cells
    layout = tuner.layout if tuner.layout.sparse else None
    if tuner.degree == 0:
        rgbs = tuner.masters[0]
        value, _ = tv_backward(rgbs, rgbs[..., 3], tuner.occupancy, (lc, lc, lc, ls), tuner.tv_eps, layout=layout, out=tuner.grads[0],
                               face_sum=False)
        return value
    coef, sigma = tuner.masters
    value = torch.zeros((), device=sigma.device)
    if lc != 0:
        value = value + tv_backward(coef, sigma, tuner.occupancy, (lc,) * (coef.shape[-1] * 3), tuner.tv_eps, layout=layout,
                                    out=tuner.grads[0], face_sum=False)[0]
    if ls != 0:
        value = value + tv_backward(sigma, sigma, tuner.occupancy, (ls,), tuner.tv_eps, layout=layout, out=tuner.grads[1], face_sum=False)[0]
    return value


# ---- doubling the resolution --------------------------------------------------------------------------------------------------------

def _store(n_points: int, degree: int, dev) -> torch.Tensor:
    E = POINT_BYTES[degree]
    return _aligned(n_points * E, E, dev)[:n_points * E]


@torch.no_grad()
def upsample(scene: BakedScene, level: Optional[float] = None) -> BakedScene:
    """The scene of twice the cells per axis (2 N - 1 points), the same bounds, degree and layout, its children pruned at `level`
    (default: the scene's).  Dense: upnerf_baked_upsample, the bits rebuilt from the child's sigmas.  Sparse, pool to pool with
    nothing the size of either grid but the bits: upnerf_brick_upsample_mark, upnerf_brick_table (the one host read: the child's
    brick count), upnerf_brick_upsample_fill, upnerf_brick_occ."""
    return _upsample(a_scene(scene, "upsample"), level).with_environment(scene.env)  # (the environment is no function of the grid: carried along)


def _upsample(scene: BakedScene, level: Optional[float]) -> BakedScene:
    level = scene.level if level is None else _level(level)
    degree, dev = scene.sh_degree, scene.device
    Nx, Ny, Nz = scene.resolution
    Cx, Cy, Cz = Nx - 1, Ny - 1, Nz - 1
    Mx, My, Mz = 2 * Nx - 1, 2 * Ny - 1, 2 * Nz - 1
    E = POINT_BYTES[degree]
    if lib.upnerf_occ_words(2 * Cx, 2 * Cy, 2 * Cz) < 0:
        raise ValueError(f"{2 * Cx} x {2 * Cy} x {2 * Cz} cells are more than an occupancy grid holds")
    if not scene.sparse:
        points = _aligned_copy(scene.grid.contiguous().view(torch.uint8), E)
        out = _store(Mz * My * Mx, degree, dev).view(Mz, My, Mx, E)
        a = _lib.BakedUpsampleArgs(Cx=Cx, Cy=Cy, Cz=Cz, degree=degree, level=level, points=ptr(points), out=ptr(out))
        check(TIMER.run("baked_upsample", lambda: lib.upnerf_baked_upsample(C.byref(a), stream()), units=Mz * My * Mx), "upnerf_baked_upsample")
        return BakedScene.from_points(out, scene.bounds, level, degree)
    res = (Mx, My, Mz)
    P = _lib.BRICK_POINTS
    B = tuple((2 * c + 7) // 8 for c in (Cx, Cy, Cz))
    if scene.n_bricks == 0:
        slots = torch.full((B[2], B[1], B[0]), -1, device=dev, dtype=torch.int32)
        return BakedScene._sparse(Layout.empty_pool(degree, dev), slots, torch.empty(0, device=dev, dtype=torch.int32), res, scene.bounds, level, degree)
    words = torch.empty(int(lib.upnerf_occ_words(2 * Cx, 2 * Cy, 2 * Cz)), device=dev, dtype=torch.int32)  # (its brick words are written)
    pool, slots = scene.layout.pointers(scene.points)
    common = dict(Cx=Cx, Cy=Cy, Cz=Cz, degree=degree, level=level, n_bricks=scene.n_bricks, slots=slots, pool=pool)
    a = _lib.BrickUpsampleArgs(words=ptr(words), **common)
    check(TIMER.run("brick_upsample_mark", lambda: lib.upnerf_brick_upsample_mark(C.byref(a), stream()), units=B[0] * B[1] * B[2]),
          "upnerf_brick_upsample_mark")
    slots, bricks, n = brick_table(words, (2 * Cx, 2 * Cy, 2 * Cz))
    del words
    if n == 0:
        return BakedScene._sparse(Layout.empty_pool(degree, dev), slots, bricks, res, scene.bounds, level, degree)
    out = _store(n * P ** 3, degree, dev).view(n, P, P, P, E)
    f = _lib.BrickUpsampleArgs(n_child=n, child_bricks=ptr(bricks), out=ptr(out), **common)
    check(TIMER.run("brick_upsample_fill", lambda: lib.upnerf_brick_upsample_fill(C.byref(f), stream()), units=n * P ** 3),
          "upnerf_brick_upsample_fill")
    return BakedScene._sparse(out if degree else out.view(torch.float32), slots, bricks, res, scene.bounds, level, degree)
