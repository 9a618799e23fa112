"""A baked scene: the static field sampled ONCE into a colour-density grid, and frames marched from that grid without touching
the field -- a preview renderer that costs a few memory reads per sample instead of an 8 x 256 network.

    bounds = bounds_from_cameras(system, margin=0.5)
    scene = BakedScene.build(system, bounds, (256, 256, 256), level=10.0, img_id=3)
    out = render_path(system, path, baked=scene, baked_step=0.01)      # or scene.render(rays, step=0.01)
    scene.save("scene.npz"); scene = BakedScene.load("scene.npz", "cuda")

The grid holds r, g, b, sigma at the Nx x Ny x Nz points of `density_grid`; a point whose sigma is below `level` (or not finite)
is stored as (0, 0, 0, 0), and the occupancy bits are those of the kept sigmas (`OccupancyGrid.from_density` at the smallest
positive fp32, no dilation): an unoccupied cell has eight exact zeros and contributes exactly nothing, so the bits only say where
the integrand is zero and never change the picture.  Colour is the static colour head at sched_mult = 1 with ONE appearance row
and, at sh_degree = 0 (the default), for ONE viewing direction: such a scene has NO view dependence.  The marcher is
`upnerf_baked_render` (csrc/baked.hip; include/upnerf_hip.h states its arithmetic).  There is no CPU path.

    scene = BakedScene.build(system, bounds, (256, 256, 256), level=10.0, img_id=3, sh_degree=2)    # dirs=sphere_directions(48)

With sh_degree = 1 or 2 a grid point holds instead the coefficients of a real spherical-harmonic expansion of its colour over
the viewing direction -- the least-squares fit to the colour head at K directions, stored as fp16 beside the fp32 sigma in a
record of 32 or 64 bytes -- and `upnerf_baked_sh_render` evaluates the expansion for each ray's own direction.
`scene.rgbs` is None then and `scene.records` holds the grid; everything else (bits, skipping, save / load, render_path) is the
same.  Still ONE appearance.  How close either kind comes to the field on a TRAINED scene is unchecked.

    sparse = scene.sparsify()                                           # or BakedScene.build(..., sparse=True)

A sparse scene of any degree stores only the occupied 8 x 8 x 8-cell bricks of the grid, 9 x 9 x 9 points each, in `scene.pool`,
found through `scene.slots` (include/upnerf_hip.h states the layout; csrc/brick.hip).  The marcher
(`upnerf_baked_sparse_render`, the same march with another layout) never visits a sample outside an occupied brick, so the
picture is bit for bit the dense scene's; `rgbs` and `records` are None then and `grid` is the pool.

    scene = BakedScene.build(system, bounds, (256, 256, 256), level=10.0, img_id=3, env_size=64)    # or scene.with_environment(env)

A scene of any kind may carry an environment (`scene.env`, a `baked_env.Environment`: a cube map of what the field shows from the
box outwards).  Its render then marches with background 0 and composites the map behind the march; sparsify,
densify, upsample, the tuners and save / load carry it along unchanged.  The map has no parallax."""
from __future__ import annotations

import copy
import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .occupancy import OccupancyGrid
from .ops import TIMER
from .static_scene import box, c_float3, field_of, refined_training_poses, require_cuda

__all__ = ["BakedScene", "Layout", "field_colour", "pool_colour", "sphere_directions", "sh_basis", "sh_weights", "save_bricks", "load_bricks", "TINY"]

TINY = float(np.float32(2.0 ** -149))  # the smallest positive fp32: the level at which the kept sigmas are packed into bits


def _field_rgb(model, o: torch.Tensor, d: torch.Tensor, z: torch.Tensor, view: torch.Tensor, a_rows: Optional[torch.Tensor]):
    """(sigma_s [R, S], rgb [R, S, 3]) of `model` at o + d z, the colour for the viewing directions `view` [R, 3] and the
    appearance rows `a_rows` [R, dim]: the sibling of geometry._field_sigma with the colour head on (use_rgb = 1, r1 = NULL:
    inference, nothing stored for a backward pass).  The side input of the colour head is built by upnerf_ray_aux as
    rendering._FieldPass builds it, from `view` -- the grid-column rays o, d still place the samples."""
    from . import rendering as rd
    pk, L = model.packer, model.packer.L
    R, S = z.shape
    dev, st = z.device, stream()
    P = model.packed().detach().contiguous()
    plan = rd._plan(pk, R, S, 2, False, True)  # mode 2, colour head, no gradient
    PF, P16, _, wexp, wnorm = rd._weights(pk, P, plan)
    progress = model.host_progress_value()
    buf = rd._alloc(plan, "aux", dev)
    wk = (C.c_float * 4)(*rd.band_weights(model.dir_L, progress, model.c2f))
    check(lib.upnerf_ray_aux(R, ptr(view), ptr(a_rows), wk, None, ptr(buf["aux"]), st), "upnerf_ray_aux")
    buf.update(rd._alloc(plan, "field", dev))
    fa = rd._args(_lib.FieldFwdArgs, buf, R=R, S=S, use_cand=0, use_rgb=1, rays_o=ptr(o), rays_d=ptr(d), z=ptr(z),
                  wk_xyz=(C.c_float * 10)(*rd.band_weights(model.xyz_L, progress, model.c2f)), P=ptr(PF), P16=ptr(P16),
                  wexp=ptr(wexp), planes=plan.planes, tile_rows=plan.tile_rows, wnorm=ptr(wnorm), rows_capacity=plan.rows_capacity)
    fn = lib.upnerf_field_fwd_f16x3 if plan.use16 else lib.upnerf_field_fwd
    check(TIMER.run("baked_colour", lambda: fn(C.byref(L), C.byref(fa), st), units=R * S), "upnerf_field_fwd")
    return buf["sigma_s"].view(R, S), buf["rgb"].view(R, S, 3)


def _appearance(system, model, field: str, img_id, rows, dev) -> Optional[torch.Tensor]:
    """The one appearance row [1, dim] of a bake, or None for a field without an appearance embedding."""
    if not model.encode_appearance:
        return None
    if (img_id is None) == (rows is None):
        raise ValueError("give either img_id (a training image's appearance) or rows (an appearance row of your own)")
    w = system.embeddings[f"{field}_a"].weight.detach()
    if rows is not None:
        row = torch.as_tensor(rows, dtype=torch.float32).to(dev).reshape(1, -1)
        if row.shape[1] != w.shape[1]:
            raise ValueError(f"rows is one appearance row of width {w.shape[1]}, got {row.shape[1]}")
        return row.contiguous()
    if not 0 <= int(img_id) < w.shape[0]:
        raise ValueError(f"img_id must be a training image index in [0, {w.shape[0]})")
    return w[int(img_id)].reshape(1, -1).to(torch.float32).contiguous()


def mean_optical_axis(system) -> torch.Tensor:
    """[3] the normalised mean optical axis of the refined training cameras (a camera looks down its -z axis)."""
    poses = refined_training_poses(system, otherwise="pass view_dir yourself")
    axis = -poses[:, :, 2].double().mean(0)
    n = float(axis.norm())
    if not n > 0 or not np.isfinite(n):
        raise ValueError("the training cameras' optical axes cancel: pass view_dir yourself")
    return (axis / n).to(torch.float32)


@torch.no_grad()
def field_colour(system, bounds, resolution: Sequence[int], view_dir, img_id=None, rows=None, field: str = "fine",
                 chunk: Optional[int] = None) -> torch.Tensor:
    """[Nz, Ny, Nx, 3] fp32 device tensor: the static colour head (sched_mult = 1) of the `field` network at the grid points of
    `density_grid`, for the viewing direction `view_dir` (normalised here) and one appearance row, `chunk` grid columns at a
    time.  The values do not depend on `chunk`."""
    from .geometry import MIN_SAMPLES, grid_columns
    model, dev = field_of(system, field, "field_colour")
    lo, hi = box(bounds)
    Nx, Ny, Nz = (int(n) for n in resolution)
    if min(Nx, Ny, Nz) < 1:
        raise ValueError(f"resolution is the number of grid points per axis, got {tuple(resolution)}")
    v, a_row = _view_and_row(system, model, field, view_dir, img_id, rows, dev)
    S = max(Nz, MIN_SAMPLES)
    cols = Nx * Ny
    chunk = int(chunk) if chunk is not None else max(1, (1 << 20) // S)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    chunk = min(chunk, cols)
    out = torch.empty(Nz, cols, 3, device=dev, dtype=torch.float32)
    view = v.expand(chunk, 3).contiguous()
    a_rows = a_row.expand(chunk, -1).contiguous() if a_row is not None else None
    for c0 in range(0, cols, chunk):
        n = min(chunk, cols - c0)
        o, d, z = grid_columns((lo, hi), (Nx, Ny, Nz), c0, n, S, device=dev)
        _, rgb = _field_rgb(model, o, d, z, view[:n], a_rows[:n] if a_rows is not None else None)
        out[:, c0:c0 + n].copy_(rgb[:, :Nz].transpose(0, 1))
    return out.view(Nz, Ny, Nx, 3)


def _view_and_row(system, model, field, view_dir, img_id, rows, dev):
    """(the normalised viewing direction [3] fp32 on the device, the one appearance row or None) of a colour pass."""
    v = torch.as_tensor(view_dir, dtype=torch.float64).reshape(3)
    n = float(v.norm())
    if not n > 0 or not np.isfinite(n):
        raise ValueError("view_dir is a direction: three finite numbers, not all zero")
    return (v / n).to(torch.float32).to(dev), _appearance(system, model, field, img_id, rows, dev)


@torch.no_grad()
def pool_colour(system, bounds, resolution: Sequence[int], bricks: torch.Tensor, view_dir, img_id=None, rows=None,
                field: str = "fine", chunk: Optional[int] = None) -> torch.Tensor:
    """[n_bricks, 9, 9, 9, 3] fp32: field_colour at the pool points of the bricks `bricks` alone (upnerf_brick_columns: one ray per
    line (slot, ly, lx) of a brick, its first nine samples the line's points), `chunk` lines at a time.  o + d z of a point
    inside the grid is field_colour's, in the same bits, and so is the colour but for the field kernels' last bit: the f16
    kernels scale every tile of samples by a power of two taken from the tile's own largest magnitude (csrc/common16.cuh), so
    which samples share a tile can move a sample's colour by one unit in the last place (DESIGN.md 2.33 has the count)."""
    from .geometry import MIN_SAMPLES
    model, dev = field_of(system, field, "pool_colour")
    lo, hi = box(bounds)
    Nx, Ny, Nz = (int(n) for n in resolution)
    v, a_row = _view_and_row(system, model, field, view_dir, img_id, rows, dev)
    nb, S, P = bricks.numel(), MIN_SAMPLES, _lib.BRICK_POINTS
    lines = nb * P * P
    chunk = int(chunk) if chunk is not None else max(1, (1 << 20) // S)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    chunk = min(chunk, lines)
    col = torch.empty(lines, P, 3, device=dev, dtype=torch.float32)  # [line][s = lz]
    view = v.expand(chunk, 3).contiguous()
    a_rows = a_row.expand(chunk, -1).contiguous() if a_row is not None else None
    o, d, z = (torch.empty(chunk, k, device=dev, dtype=torch.float32) for k in (3, 3, S))
    for l0 in range(0, lines, chunk):
        n = min(chunk, lines - l0)
        a = _lib.BrickColumnsArgs(Nx=Nx, Ny=Ny, Nz=Nz, S=S, lo=c_float3(lo), hi=c_float3(hi), line0=l0, count=n, n_bricks=nb,
                                  bricks=ptr(bricks), o=ptr(o), d=ptr(d), z=ptr(z))
        check(TIMER.run("brick_columns", lambda: lib.upnerf_brick_columns(C.byref(a), stream()), units=n), "upnerf_brick_columns")
        _, rgb = _field_rgb(model, o[:n], d[:n], z[:n], view[:n], a_rows[:n] if a_rows is not None else None)
        col[l0:l0 + n].copy_(rgb[:, :P])
    return col.view(nb, P * P, P, 3).permute(0, 2, 1, 3).contiguous().view(nb, P, P, P, 3)  # [slot][lz][ly][lx]


RECORD_BYTES = {1: 32, 2: 64}  # one grid point of an SH scene (include/upnerf_hip.h)
SIGMA_BYTE = {1: 24, 2: 56}
POINT_BYTES = {0: 16, **RECORD_BYTES}  # one point of a scene of each degree: what a brick pool stores 729 of per brick
SIGMA_AT = {0: 12, **SIGMA_BYTE}


def _aligned(nbytes: int, size: int, dev) -> torch.Tensor:
    """A uint8 device vector of `nbytes` (one at least) whose address is a multiple of `size`."""
    spare = torch.empty(max(nbytes, size) + size, dtype=torch.uint8, device=dev)
    off = -spare.data_ptr() % size
    return spare[off:off + max(nbytes, size)]


def _aligned_copy(t: torch.Tensor, size: int) -> torch.Tensor:
    """The contiguous tensor `t` itself where its address is a multiple of `size`, else a copy of it at such an address."""
    n = t.numel() * t.element_size()
    return t if t.data_ptr() % size == 0 else _aligned(n, size, t.device)[:n].view(t.dtype).view(t.shape).copy_(t)


class Layout:
    """What the marcher needs beside a point array, dense grid or brick pool, and everything that follows from it: the (frozen)
    `occupancy`, the `bounds`, the `degree`, and of a pool its table `slots` [Bz, By, Bx] and `bricks` [n_bricks] (both None for a
    dense grid).  Derived once: `resolution` (the grid's points per axis), `sparse`, `shape`, `point_bytes`, `sigma_at`, `nb` and
    `param_shapes`.  Immutable; no device work, so CPU tensors do for its arithmetic."""

    __slots__ = ("occupancy", "bounds", "degree", "slots", "bricks", "resolution", "sparse", "shape", "point_bytes", "sigma_at", "nb",
                 "param_shapes", "_spare")

    def __init__(self, occupancy, bounds, degree: int, slots: Optional[torch.Tensor] = None, bricks: Optional[torch.Tensor] = None):
        if (slots is None) != (bricks is None):
            raise ValueError("a pool's table is both slots and bricks; a dense grid has neither")
        sparse, P, nb = slots is not None, _lib.BRICK_POINTS, (int(degree) + 1) ** 2
        resolution = tuple(c + 1 for c in occupancy.dims)
        shape = (bricks.numel(), P, P, P) if sparse else resolution[::-1]  # the points' leading shape: bricks, or (Nz, Ny, Nx)
        E = POINT_BYTES.get(degree)
        # the fp32 parameters: (rgbs,) at degree 0, else (coef, sigma)
        param_shapes = (shape + (4,),) if degree == 0 else (shape + (3, nb), shape)
        # with no brick at all the marcher is still given an address: one spare aligned point (never read)
        spare = _aligned(E, E, slots.device) if sparse and E and shape[0] == 0 else None
        values = (occupancy, bounds, int(degree), slots, bricks, resolution, sparse, shape, E, SIGMA_AT.get(degree), nb, param_shapes, spare)
        for name, value in zip(self.__slots__, values):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a Layout is immutable")

    def zeros(self, device) -> tuple:
        """Zeroed gradients of the parameter shapes."""
        return tuple(torch.zeros(shape, device=device) for shape in self.param_shapes)

    @staticmethod
    def empty_pool(degree: int, device) -> torch.Tensor:
        """The pool of a degree with no brick: [0, 9, 9, 9, 4] fp32, or [0, 9, 9, 9, 32 | 64] uint8."""
        P = _lib.BRICK_POINTS
        if degree == 0:
            return torch.empty((0, P, P, P, 4), device=device, dtype=torch.float32)
        return torch.empty((0, P, P, P, POINT_BYTES[degree]), device=device, dtype=torch.uint8)

    def marched(self, points: torch.Tensor) -> torch.Tensor:
        """The tensor whose address the marcher is given for `points`: `points`, or the spare point of a pool with no brick."""
        return points if self._spare is None or points.numel() else self._spare

    def pointers(self, points: torch.Tensor) -> tuple:
        """(the points' address, the slots' or None): the pair the C structs take."""
        return ptr(self.marched(points)), ptr(self.slots)


DENSE_REFUSAL = ("a dense baked scene has no brick pool to tune: use baked_tune (scene.tune), or scene.sparsify() first")


def a_scene(scene, what: str) -> "BakedScene":
    if not isinstance(scene, BakedScene):
        raise ValueError(f"{what} takes a baked.BakedScene")
    return scene


def pool_layout(of) -> Layout:
    """The Layout of a brick pool: `of` itself, or that of a sparse BakedScene or of a baked_sparse_tune.PoolParams."""
    if isinstance(of, BakedScene) and not of.sparse:
        raise ValueError(DENSE_REFUSAL)
    layout = of if isinstance(of, Layout) else getattr(of, "layout", None)
    if not isinstance(layout, Layout) or not layout.sparse:
        raise ValueError("the layout is a brick pool's baked.Layout, a sparse baked.BakedScene or a PoolParams")
    return layout


def brick_table(words: torch.Tensor, dims: Sequence[int]):
    """(slots int32 [Bz, By, Bx], bricks int32 [n_bricks], n_bricks) of the brick bits of an occupancy grid's words
    (upnerf_brick_table).  One host read: the count."""
    Cx, Cy, Cz = (int(c) for c in dims)
    B = tuple((c + 7) // 8 for c in (Cx, Cy, Cz))
    dev = words.device
    slots = torch.empty(B[2], B[1], B[0], device=dev, dtype=torch.int32)
    bricks = torch.empty(slots.numel(), device=dev, dtype=torch.int32)
    count = torch.empty(1, device=dev, dtype=torch.int32)
    scratch = _aligned(int(lib.upnerf_brick_table_scratch(Cx, Cy, Cz)), 16, dev)
    a = _lib.BrickTableArgs(Cx=Cx, Cy=Cy, Cz=Cz, words=ptr(words), slots=ptr(slots), bricks=ptr(bricks), count=ptr(count),
                            scratch=ptr(scratch))
    check(TIMER.run("brick_table", lambda: lib.upnerf_brick_table(C.byref(a), stream()), units=slots.numel()), "upnerf_brick_table")
    n = int(count.cpu())  # the one host read of a build: it sizes the pool
    return slots, bricks[:n].clone(), n


def brick_gather(grid: torch.Tensor, bricks: torch.Tensor, out_dtype=None) -> torch.Tensor:
    """The pool [n_bricks, 9, 9, 9, k] of a dense grid [Nz, Ny, Nx, k] (fp32 or uint8, 4, 16, 32 or 64 bytes per point) for the
    bricks `bricks` (upnerf_brick_gather); points beyond the grid are zero.  With no brick nothing is launched."""
    Nz, Ny, Nx, k = grid.shape
    g = grid.contiguous().view(torch.uint8)
    E, n, P = g.shape[3], bricks.numel(), _lib.BRICK_POINTS
    g = _aligned_copy(g, min(E, 16))
    store = _aligned(n * P ** 3 * E, E, grid.device)
    if n:
        a = _lib.BrickGatherArgs(Cx=Nx - 1, Cy=Ny - 1, Cz=Nz - 1, n_bricks=n, E=E, bricks=ptr(bricks), grid=ptr(g), pool=ptr(store))
        check(TIMER.run("brick_gather", lambda: lib.upnerf_brick_gather(C.byref(a), stream()), units=n * P ** 3), "upnerf_brick_gather")
    pool = store[:n * P ** 3 * E].view(n, P, P, P, E)
    return pool.view(grid.dtype)


def brick_scatter(pool: torch.Tensor, bricks: torch.Tensor, resolution: Sequence[int]) -> torch.Tensor:
    """The dense grid [Nz, Ny, Nx, k] of a pool [n_bricks, 9, 9, 9, k] (upnerf_brick_scatter): zero outside the bricks."""
    Nx, Ny, Nz = (int(n) for n in resolution)
    p = pool.contiguous().view(torch.uint8)
    E, n = p.shape[4], bricks.numel()
    store = _aligned(Nz * Ny * Nx * E, max(E, 16), pool.device).zero_()
    if n:
        p = _aligned_copy(p, E)
        a = _lib.BrickScatterArgs(Cx=Nx - 1, Cy=Ny - 1, Cz=Nz - 1, n_bricks=n, E=E, bricks=ptr(bricks), pool=ptr(p), grid=ptr(store))
        check(TIMER.run("brick_scatter", lambda: lib.upnerf_brick_scatter(C.byref(a), stream()), units=n * 729), "upnerf_brick_scatter")
    grid = store[:Nz * Ny * Nx * E].view(Nz, Ny, Nx, E)
    return grid.view(pool.dtype)


def brick_words(pool_bytes: torch.Tensor, slots: torch.Tensor, n_bricks: int, resolution: Sequence[int], E: int, sigma_at: int) -> torch.Tensor:
    """The occupancy words (cell bits, then brick bits) of a pool and its table (upnerf_brick_occ): a cell is occupied iff one of
    its eight pool corners has a finite sigma >= the smallest positive fp32."""
    Nx, Ny, Nz = (int(n) for n in resolution)
    words = torch.empty(int(lib.upnerf_occ_words(Nx - 1, Ny - 1, Nz - 1)), device=slots.device, dtype=torch.int32)
    a = _lib.BrickOccArgs(Cx=Nx - 1, Cy=Ny - 1, Cz=Nz - 1, n_bricks=n_bricks, E=E, sigma_offset=sigma_at, slots=ptr(slots),
                          pool=ptr(pool_bytes) if n_bricks else None, words=ptr(words))
    check(TIMER.run("brick_occ", lambda: lib.upnerf_brick_occ(C.byref(a), stream()), units=words.numel()), "upnerf_brick_occ")
    return words


def brick_face(op: str, t: torch.Tensor, layout: Layout, what: str) -> torch.Tensor:
    """upnerf_brick_face_<op> (sum | max) in place on the pool-shaped fp32 tensor `t` [n_bricks, 9, 9, 9, ...] (any trailing shape:
    F floats per point): every copy of a grid point that bricks share becomes the sum (in ascending brick order) or the maximum
    over its copies.  With no brick nothing is shared and nothing is launched.  Returns `t`."""
    require_cuda(what, t)
    n, P = layout.shape[:2]
    if t.dtype != torch.float32 or t.dim() < 4 or tuple(t.shape[:4]) != layout.shape or not t.is_contiguous():
        raise ValueError(f"a pool-shaped tensor is contiguous fp32 [{n}, {P}, {P}, {P}, ...]")
    if n == 0:
        return t
    Cx, Cy, Cz = layout.occupancy.dims
    F = t.numel() // (n * P ** 3)
    a = _lib.BrickFaceSumArgs(Cx=Cx, Cy=Cy, Cz=Cz, n_bricks=n, F=F, slots=ptr(layout.slots), bricks=ptr(layout.bricks), data=ptr(t))
    fn = getattr(lib, "upnerf_brick_face_" + op)
    check(TIMER.run("brick_face_" + op, lambda: fn(C.byref(a), stream()), units=n * 386 * F), "upnerf_brick_face_" + op)
    return t


def face_sum(t: torch.Tensor, scene) -> torch.Tensor:
    """upnerf_brick_face_sum in place on the pool-shaped fp32 tensor `t` of `scene` (a pool's Layout, a sparse BakedScene or a
    PoolParams): every copy of a shared grid point becomes the sum over its copies, in ascending brick order.  Returns `t`."""
    return brick_face("sum", t, pool_layout(scene), "baked_sparse_tune.face_sum")


_Y = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)


def _level(level) -> float:
    level = float(level)
    if level != level:
        raise ValueError("level is not a number")
    return level


def _degree(sh_degree) -> int:
    if sh_degree not in (1, 2):
        raise ValueError(f"sh_degree is 1 or 2 (0: a scene without view dependence), got {sh_degree!r}")
    return int(sh_degree)


def sphere_directions(K: int = 48) -> np.ndarray:
    """[K, 3] fp64 unit vectors: a Fibonacci lattice on the WHOLE sphere (z evenly spaced, the longitude advancing by the golden
    angle).  A field trained from one side of a scene has seen nothing of the other, and what its colour head says there is
    extrapolation that the fit weighs like everything else; `dirs` restricted to the training cameras' hemisphere is the
    alternative.  Which of the two is better on a trained scene is unchecked."""
    K = int(K)
    if K < 1:
        raise ValueError(f"K is a number of directions, got {K}")
    i = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / K
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


def sh_basis(dirs, sh_degree: int) -> np.ndarray:
    """[K, nb] fp64: the real spherical-harmonic basis of include/upnerf_hip.h at the directions `dirs` [K, 3] (normalised
    here)."""
    nb = (_degree(sh_degree) + 1) ** 2
    d = np.asarray(dirs, np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError("dirs are [K, 3]")
    n = np.linalg.norm(d, axis=1)
    if not np.isfinite(d).all() or not (n > 0).all():
        raise ValueError("dirs are directions: three finite numbers each, not all zero")
    x, y, z = (d / n[:, None]).T
    B = [np.full_like(x, _Y[0]), -_Y[1] * y, _Y[1] * z, -_Y[1] * x, _Y[2] * x * y, -_Y[2] * y * z,
         _Y[3] * (2 * z * z - x * x - y * y), -_Y[2] * x * z, _Y[4] * (x * x - y * y)]
    return np.stack(B[:nb], 1)


def sh_weights(dirs, sh_degree: int) -> np.ndarray:
    """[nb, K] fp32: the pseudo-inverse of the fp64 basis matrix of `dirs`, rounded once -- the weights with which the colours at
    the K directions sum to the least-squares coefficients.  Refused: K < nb, and a basis matrix whose smallest singular value is
    below 1e-6 of its largest (a rank test in fp64: directions that do not determine the expansion, e.g. coplanar ones at
    degree 2)."""
    B = sh_basis(dirs, sh_degree)
    K, nb = B.shape
    if K < nb:
        raise ValueError(f"degree {sh_degree} has {nb} coefficients: {K} directions cannot determine them")
    sv = np.linalg.svd(B, compute_uv=False)
    if not sv[-1] >= 1e-6 * sv[0]:
        raise ValueError(f"the directions do not determine a degree-{sh_degree} expansion (singular values {sv[0]:.3g} .. {sv[-1]:.3g})")
    return np.ascontiguousarray(np.linalg.pinv(B).astype(np.float32))


def pack_records(coef: torch.Tensor, sigma: torch.Tensor, degree: int, level: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The records [shape of sigma, 32 | 64] of fp32 coefficients and sigmas (upnerf_baked_sh_pack at `level`)."""
    size, n = RECORD_BYTES[degree], sigma.numel()
    if out is None:
        out = _aligned(n * size, size, sigma.device)[:n * size].view(tuple(sigma.shape) + (size,))
    a = _lib.BakedShPackArgs(n=n, level=float(level), degree=degree, sigma=ptr(sigma), acc=ptr(coef), records=ptr(out), kept=None)
    check(TIMER.run("baked_sh_pack", lambda: lib.upnerf_baked_sh_pack(C.byref(a), stream()), units=n), "upnerf_baked_sh_pack")
    return out


def _render_args(rays, step, background, stop):
    step, background, stop = float(step), float(background), float(stop)
    if not (step > 0 and np.isfinite(step)):
        raise ValueError(f"step is a positive, finite length in units of t, got {step}")
    if not np.isfinite(background):
        raise ValueError(f"background is a finite grey level, got {background}")
    if not 0 <= stop < 1:
        raise ValueError(f"stop is a transmittance in [0, 1) (0: never), got {stop}")
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or rays.shape[0] < 1:
        raise ValueError("rays are a fp32 tensor [R, 8] (o | d | near | far) with R >= 1")
    return step, background, stop


def pack_rgbs(sigma: torch.Tensor, rgb: Optional[torch.Tensor], level: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The points [shape of sigma, 4] fp32 of contiguous fp32 sigmas and colours [shape of sigma, 3] (None: black), pruned at
    `level` (upnerf_baked_pack), written to `out` where given: a pool wants its own aligned store."""
    if out is None:
        out = torch.empty(tuple(sigma.shape) + (4,), device=sigma.device, dtype=torch.float32)
    a = _lib.BakedPackArgs(n=sigma.numel(), level=level, sigma=ptr(sigma), rgb=ptr(rgb), rgbs=ptr(out), kept=None)
    check(TIMER.run("baked_pack", lambda: lib.upnerf_baked_pack(C.byref(a), stream()), units=sigma.numel()), "upnerf_baked_pack")
    return out


def _upstream(R: int, g_rgb, g_depth, g_opacity) -> None:
    """The upstream gradients of R rays, as every backward wrapper takes them."""
    if g_rgb.dtype != torch.float32 or tuple(g_rgb.shape) != (R, 3):
        raise ValueError("g_rgb is a fp32 tensor [R, 3]")
    for g in (g_depth, g_opacity):
        if g is not None and (g.dtype != torch.float32 or tuple(g.shape) != (R,)):
            raise ValueError("g_depth and g_opacity are fp32 tensors [R] or None")


def _common(occupancy, bounds, rays, step, background, stop):
    Cx, Cy, Cz = occupancy.dims
    lo, hi = bounds
    return dict(Cx=Cx, Cy=Cy, Cz=Cz, R=rays.shape[0], lo=c_float3(lo), hi=c_float3(hi), step=step, background=background, stop=stop,
                words=ptr(occupancy.words), rays=ptr(rays))


def _rays16(rays: torch.Tensor) -> torch.Tensor:
    rays = rays.detach().contiguous()
    return rays.clone() if rays.data_ptr() % 16 else rays


def march(points: torch.Tensor, layout: Layout, rays, step, background, stop, rgb, depth, opacity) -> None:
    """One launch of the marcher on checked arguments (_render_args, _rays16) into rgb [>= R, 3], depth and opacity [>= R]: through
    the pool `points` of a sparse layout, else on the records `points` at degree 1 | 2 and on rgbs at degree 0."""
    common = dict(_common(layout.occupancy, layout.bounds, rays, step, background, stop), rgb=ptr(rgb), depth=ptr(depth), opacity=ptr(opacity))
    points, slots = layout.pointers(points)
    if layout.sparse:
        name, a = "baked_sparse_render", _lib.BakedSparseRenderArgs(degree=layout.degree, pool=points, slots=slots, **common)
    elif layout.degree:
        name, a = "baked_sh_render", _lib.BakedShRenderArgs(degree=layout.degree, records=points, **common)
    else:
        name, a = "baked_render", _lib.BakedRenderArgs(rgbs=points, **common)
    fn = getattr(lib, "upnerf_" + name)
    check(TIMER.run(name, lambda: fn(C.byref(a), stream()), units=rays.shape[0]), "upnerf_" + name)


class BakedScene:
    """`rgbs` [Nz, Ny, Nx, 4] fp32 on the device (r, g, b, sigma at the grid points, pruned at `level`), the box it spans and
    the OccupancyGrid of its kept sigmas.  An SH scene (from_records, from_direction_grids, build(sh_degree=1 | 2)) has
    `rgbs` None, `sh_degree` 1 or 2 and `records` [Nz, Ny, Nx, 32 | 64] uint8 instead."""

    sh_degree = 0
    records = None
    pool = slots = bricks = None  # a sparse scene's (sparsify, from_bricks, build(sparse=True)): see _sparse
    layout = None  # the scene's Layout: what the marcher, the tuners and the regularisers take beside a point array
    env = None  # a baked_env.Environment behind the march (with_environment, build(env_size=...)), or None: the flat `background`

    def with_environment(self, env) -> "BakedScene":
        """This scene (the same tensors, nothing copied) with the environment `env` behind it, a `baked_env.Environment` on the
        scene's device, or None to remove it."""
        from .baked_env import Environment
        if env is not None and (not isinstance(env, Environment) or env.device != self.device):
            raise ValueError("env is a baked_env.Environment on the scene's device, or None")
        other = copy.copy(self)
        other.env = env
        return other

    def _set(self, points: torch.Tensor, bounds, level: float, degree: int, slots=None, bricks=None, resolution=None) -> "BakedScene":
        """What every constructor ends in, on checked arguments: `points` are rgbs (degree 0) or records of a dense scene, or with
        the table `slots` and `bricks` the pool of a grid of `resolution` points.  The bits are the kept sigmas': of a dense scene
        from its sigmas (upnerf_occ_build), of a sparse one from the pool alone (upnerf_brick_occ)."""
        sparse = slots is not None
        self.sh_degree = int(degree)
        self.rgbs = points if not sparse and degree == 0 else None
        self.records = points if not sparse and degree else None
        self.pool, self.slots, self.bricks = (points, slots, bricks) if sparse else (None, None, None)
        self.bounds = box(bounds, strict=True)
        self.level = float(level)
        E, at = POINT_BYTES[self.sh_degree], SIGMA_AT[self.sh_degree]
        if sparse:
            Nx, Ny, Nz = (int(n) for n in resolution)
            words = brick_words(points, slots, bricks.numel(), (Nx, Ny, Nz), E, at)
            occupancy = OccupancyGrid(words, self.bounds, (Nx - 1, Ny - 1, Nz - 1))
        else:
            sigma = points[..., 3] if degree == 0 else points[..., at:at + 4].contiguous().view(torch.float32).squeeze(-1)
            occupancy = OccupancyGrid.from_density(sigma.contiguous(), self.bounds, level=TINY, dilate=0)
        self.occupancy = occupancy
        self.layout = Layout(occupancy, self.bounds, self.sh_degree, slots, bricks)
        return self

    @classmethod
    def _new(cls, *args, **kwargs) -> "BakedScene":
        return cls.__new__(cls)._set(*args, **kwargs)

    def __init__(self, rgbs: torch.Tensor, bounds, level: float):
        require_cuda("BakedScene", rgbs)
        if rgbs.dtype != torch.float32 or rgbs.dim() != 4 or rgbs.shape[3] != 4 or not rgbs.is_contiguous():
            raise ValueError("rgbs is a contiguous fp32 tensor [Nz, Ny, Nx, 4]")
        self._set(rgbs, bounds, level, 0)

    @classmethod
    def from_records(cls, records: torch.Tensor, bounds, level: float, sh_degree: int) -> "BakedScene":
        """An SH scene from its records, a contiguous uint8 device tensor [Nz, Ny, Nx, 32 (degree 1) | 64 (degree 2)] laid out as
        include/upnerf_hip.h says; the occupancy bits are those of the records' sigmas."""
        degree = _degree(sh_degree)
        require_cuda("BakedScene.from_records", records)
        size = RECORD_BYTES[degree]
        if records.dtype != torch.uint8 or records.dim() != 4 or records.shape[3] != size or min(records.shape[:3]) < 2:
            raise ValueError(f"records is a uint8 tensor [Nz, Ny, Nx, {size}] with two points per axis at least")
        return cls._new(_aligned_copy(records.contiguous(), size), bounds, level, degree)  # (a record is aligned to its own size)

    @classmethod
    def from_points(cls, points: torch.Tensor, bounds, level: float, degree: int) -> "BakedScene":
        """The dense scene of a point array [Nz, Ny, Nx, ...] of `degree`, given as bytes or as fp32: rgbs at degree 0 (the scene
        of BakedScene(rgbs, ...)), else records (from_records), at an address aligned to a point as from_records aligns."""
        if degree:
            return cls.from_records(points.view(torch.uint8), bounds, level, degree)
        return cls(_aligned_copy(points.view(torch.float32), POINT_BYTES[0]), bounds, level)

    # ---- sparse scenes: a pool of the occupied bricks (include/upnerf_hip.h states the layout) -------------------

    @classmethod
    def _sparse(cls, pool: torch.Tensor, slots: torch.Tensor, bricks: torch.Tensor, resolution, bounds, level: float,
                degree: int) -> "BakedScene":
        """The sparse scene of a pool [n_bricks, 9, 9, 9, 4] fp32 (degree 0) or [n_bricks, 9, 9, 9, 32 | 64] uint8 aligned to its
        point size, and its table.  Every sparse scene gets its bits here, from the pool alone (upnerf_brick_occ)."""
        return cls._new(pool, slots=slots, bricks=bricks, resolution=resolution, bounds=bounds, level=level, degree=degree)

    @torch.no_grad()
    def sparsify(self) -> "BakedScene":
        """The same scene with only its occupied bricks stored: upnerf_brick_table on the brick bits, upnerf_brick_gather, and the
        bits again from the pool.  The marcher visits no sample outside an occupied brick, so the picture is bit for bit this
        scene's."""
        if self.sparse:
            return self
        slots, bricks, n = brick_table(self.occupancy.words, self.occupancy.dims)
        sparse = self._sparse(brick_gather(self.grid, bricks), slots, bricks, self.resolution, self.bounds, self.level, self.sh_degree)
        return sparse.with_environment(self.env)

    @torch.no_grad()
    def densify(self) -> "BakedScene":
        """The dense scene of a sparse one (upnerf_brick_scatter into a zeroed grid)."""
        if not self.sparse:
            return self
        grid = brick_scatter(self.pool, self.bricks, self.resolution)
        return self.from_points(grid, self.bounds, self.level, self.sh_degree).with_environment(self.env)

    @classmethod
    def from_bricks(cls, pool: torch.Tensor, bricks: torch.Tensor, resolution: Sequence[int], bounds, level: float,
                    sh_degree: int = 0) -> "BakedScene":
        """A sparse scene from volumes of the caller's own: `pool` [n_bricks, 9, 9, 9, 4] fp32 (degree 0) or
        [n_bricks, 9, 9, 9, 32 | 64] uint8 (degree 1 | 2) on the device, contiguous and aligned to the bytes of one point;
        `bricks` int32 [n_bricks], the linear brick indices (bz * By + by) * Bx + bx in strictly ascending order; `resolution`
        the grid POINTS per axis.  Refused with ValueError: another dtype, shape or alignment, bricks unsorted, duplicated or out
        of range, a degree outside {0, 1, 2}.  One host read: the bricks, to check them."""
        if sh_degree not in (0, 1, 2):
            raise ValueError(f"sh_degree is 0, 1 or 2, got {sh_degree!r}")
        degree, P = int(sh_degree), _lib.BRICK_POINTS
        E = POINT_BYTES[degree]
        want = (torch.float32, 4) if degree == 0 else (torch.uint8, E)
        if not torch.is_tensor(pool) or pool.dtype != want[0] or pool.dim() != 5 or tuple(pool.shape[1:]) != (P, P, P, want[1]) or \
                not pool.is_contiguous():
            raise ValueError(f"the pool of degree {degree} is a contiguous {want[0]} tensor [n_bricks, {P}, {P}, {P}, {want[1]}]")
        if pool.numel() and pool.data_ptr() % E:
            raise ValueError(f"the pool is aligned to the {E} bytes of one point")
        res = tuple(int(n) for n in resolution)
        if len(res) != 3 or min(res) < 2:
            raise ValueError(f"resolution is the number of grid points per axis (two at least), got {tuple(resolution)}")
        B = tuple((n - 1 + 7) // 8 for n in res)
        if not torch.is_tensor(bricks) or bricks.dtype != torch.int32 or bricks.dim() != 1 or bricks.numel() != pool.shape[0]:
            raise ValueError("bricks is an int32 tensor [n_bricks], one linear brick index per brick of the pool")
        b = bricks.detach().cpu().numpy().astype(np.int64)
        if b.size and (b.min() < 0 or b.max() >= B[0] * B[1] * B[2] or not (np.diff(b) > 0).all()):
            raise ValueError(f"bricks are strictly ascending linear indices in [0, {B[0] * B[1] * B[2]})")
        require_cuda("BakedScene.from_bricks", pool, bricks)
        bricks = bricks.detach().contiguous()
        slots = torch.full((B[2], B[1], B[0]), -1, device=pool.device, dtype=torch.int32)
        slots.view(-1)[bricks.long()] = torch.arange(bricks.numel(), device=pool.device, dtype=torch.int32)
        return cls._sparse(pool.detach(), slots, bricks, res, bounds, level, degree)

    # ---- construction ------------------------------------------------------------------------------------------------------

    @classmethod
    @torch.no_grad()
    def from_grids(cls, sigma: torch.Tensor, rgb: Optional[torch.Tensor], bounds, level: float = 0.0, sparse: bool = False) -> "BakedScene":
        """From a density grid [Nz, Ny, Nx] and a colour grid [Nz, Ny, Nx, 3] (None: black) of the caller's own, fp32 on the
        device.  A point is kept iff its sigma is finite, positive and >= level; every other point becomes (0, 0, 0, 0)
        (upnerf_baked_pack).  sparse: the dense scene's sparsify() -- the caller's grids are dense already, so the dense records
        exist for the length of this call."""
        require_cuda("BakedScene.from_grids", sigma, *([rgb] if rgb is not None else []))
        if sigma.dtype != torch.float32 or sigma.dim() != 3 or min(sigma.shape) < 2:
            raise ValueError("sigma is a fp32 tensor [Nz, Ny, Nx] with two points per axis at least")
        if rgb is not None and (rgb.dtype != torch.float32 or tuple(rgb.shape) != tuple(sigma.shape) + (3,)):
            raise ValueError("rgb is a fp32 tensor [Nz, Ny, Nx, 3]")
        level = _level(level)
        sigma = sigma.detach().contiguous()
        rgb = rgb.detach().contiguous() if rgb is not None else None
        scene = cls(pack_rgbs(sigma, rgb, level), bounds, level)
        return scene.sparsify() if sparse else scene

    @classmethod
    @torch.no_grad()
    def _project(cls, sigma: torch.Tensor, colour_of, dirs, bounds, level: float, sh_degree: int) -> "BakedScene":
        """The SH scene of sigma [Nz, Ny, Nx] and colour_of(k) -> [Nz, Ny, Nx, 3], the colour grid for direction k of `dirs`."""
        return cls.from_records(cls._project_records(sigma, colour_of, dirs, level, sh_degree), bounds, level, _degree(sh_degree))

    @staticmethod
    @torch.no_grad()
    def _project_records(sigma: torch.Tensor, colour_of, dirs, level: float, sh_degree: int) -> torch.Tensor:
        """The records [shape of sigma, 32 | 64] uint8 of sigma (any shape: a grid [Nz, Ny, Nx] or a pool [n, 9, 9, 9]) and
        colour_of(k) -> [shape of sigma, 3]: upnerf_sh_accumulate for k = 0 .. K-1 in order (one direction's colours and the
        accumulator resident at a time), then upnerf_baked_sh_pack."""
        degree = _degree(sh_degree)
        W = sh_weights(dirs, degree)
        nb, K = W.shape
        level = _level(level)
        sigma = sigma.detach().contiguous()
        n, dev = sigma.numel(), sigma.device
        acc = torch.empty(tuple(sigma.shape) + (3, nb), device=dev, dtype=torch.float32)
        for k in range(K):
            rgb = colour_of(k)
            if rgb.dtype != torch.float32 or tuple(rgb.shape) != tuple(sigma.shape) + (3,) or rgb.device != dev:
                raise ValueError("the colours of a direction are a fp32 tensor [shape of sigma, 3] on sigma's device")
            rgb = rgb.detach().contiguous()
            a = _lib.ShAccumulateArgs(n=n, nb=nb, first=int(k == 0), w=(C.c_float * 9)(*W[:, k].tolist()), rgb=ptr(rgb), acc=ptr(acc))
            check(TIMER.run("sh_accumulate", lambda: lib.upnerf_sh_accumulate(C.byref(a), stream()), units=n), "upnerf_sh_accumulate")
        return pack_records(acc, sigma, degree, level)

    @classmethod
    @torch.no_grad()
    def from_direction_grids(cls, sigma: torch.Tensor, rgb_dirs: torch.Tensor, dirs, bounds, level: float = 0.0,
                             sh_degree: int = 1, sparse: bool = False) -> "BakedScene":
        """The SH sibling of from_grids: a density grid [Nz, Ny, Nx] and the colour grids rgb_dirs [K, Nz, Ny, Nx, 3] of the
        caller's own for the K directions `dirs` [K, 3], fp32 on the device.  Each coefficient is the least-squares fit
        sum_k W[j][k] rgb_k (sh_weights), summed in fp32 in the order of k.  A point is kept iff its sigma is finite, positive
        and >= level and its coefficients are finite; every other point becomes a zero record (upnerf_baked_sh_pack).  sparse:
        the dense scene's sparsify(), as in from_grids."""
        require_cuda("BakedScene.from_direction_grids", sigma, rgb_dirs)
        if sigma.dtype != torch.float32 or sigma.dim() != 3 or min(sigma.shape) < 2:
            raise ValueError("sigma is a fp32 tensor [Nz, Ny, Nx] with two points per axis at least")
        K = np.asarray(dirs).shape[0] if np.asarray(dirs).ndim == 2 else -1
        if rgb_dirs.dtype != torch.float32 or tuple(rgb_dirs.shape) != (K,) + tuple(sigma.shape) + (3,):
            raise ValueError("rgb_dirs is a fp32 tensor [K, Nz, Ny, Nx, 3], one colour grid per row of dirs [K, 3]")
        scene = cls._project(sigma, lambda k: rgb_dirs[k], dirs, bounds, level, sh_degree)
        return scene.sparsify() if sparse else scene

    @classmethod
    @torch.no_grad()
    def build(cls, system, bounds, resolution: Sequence[int], level: float, img_id=None, rows=None, view_dir=None,
              field: str = "fine", chunk: Optional[int] = None, sh_degree: int = 0, dirs=None, sparse: bool = False,
              env_size: Optional[int] = None, env_far: Optional[float] = None) -> "BakedScene":
        """Bake the static scene of `system`: sigma = geometry.density_grid, colour = field_colour with the appearance row of
        training image `img_id` (or `rows`, a row of the caller's own) for the viewing direction `view_dir` (default: the
        normalised mean optical axis of the refined training cameras).  `level` has no default: the useful threshold depends on
        the scene's scale (see extract_surface).  `resolution` counts grid POINTS per axis, two at least.

        sh_degree = 1 | 2: colour is instead the degree's spherical-harmonic fit to field_colour at the directions `dirs` [K, 3]
        (default sphere_directions(48): the whole sphere -- see there), K passes over the field; view_dir has no meaning then and
        is refused, as dirs is at degree 0.

        sparse = True: a sparse scene, with the bricks, the sigmas and the bits of build(...).sparsify() -- and its colours, to
        the last bit of the field kernels' output (pool_colour says why not always bit for bit) -- but the colour passes, the
        accumulator and the records only where the scene is occupied.  sigma is still evaluated on the whole grid (one pass, 4
        bytes a point: the field has to be asked everywhere to know where it is empty); its occupied bricks are found
        (upnerf_brick_table) and it is gathered to the pool; the colour is then evaluated on the pool's lines alone
        (pool_colour), once or once per direction, and packed as above.  The cost: a line is one ray of the field kernels'
        minimum of 32 samples for 9 stored points, and a brick stores 729 points for its 512 cells, so with f_b the share of
        occupied bricks the colour work is f_b * (729 / 512) * (32 / 9) ~ 5.06 f_b of the dense bake's: a sparse bake is the
        cheaper one only below f_b ~ 0.20 (`brick_fraction` reports f_b).  `chunk` counts lines in the colour passes then.

        env_size = E: the scene also carries baked_env.Environment.build(system, bounds, E, far=env_far, ...) with the scene's
        own appearance (img_id / rows) and field; env_far defaults to the largest far plane of the training images."""
        if env_size is None:
            if env_far is not None:
                raise ValueError("env_far belongs to env_size=")
            return cls._build(system, bounds, resolution, level, img_id, rows, view_dir, field, chunk, sh_degree, dirs, sparse)
        from .baked_env import Environment, _size
        _size(env_size)  # (refused before any pass over the field)
        scene = cls._build(system, bounds, resolution, level, img_id, rows, view_dir, field, chunk, sh_degree, dirs, sparse)
        return scene.with_environment(Environment.build(system, bounds, env_size, far=env_far, img_id=img_id, rows=rows, field=field))

    @classmethod
    @torch.no_grad()
    def _build(cls, system, bounds, resolution, level, img_id, rows, view_dir, field, chunk, sh_degree, dirs, sparse) -> "BakedScene":
        """build without the environment."""
        from .geometry import density_grid
        if min(int(n) for n in resolution) < 2:
            raise ValueError(f"resolution is the number of grid points per axis (two at least), got {tuple(resolution)}")
        if sh_degree != 0:
            _degree(sh_degree)
            if view_dir is not None:
                raise ValueError("view_dir is the ONE direction of a scene without view dependence: with sh_degree > 0 pass dirs")
            dirs = sphere_directions() if dirs is None else np.asarray(torch.as_tensor(dirs).detach().cpu().numpy(), np.float64)
            sh_weights(dirs, sh_degree)  # (refused before any pass over the field)
        elif dirs is not None:
            raise ValueError("dirs are the directions of a spherical-harmonic fit: pass sh_degree = 1 or 2 with them")
        elif view_dir is None:
            view_dir = mean_optical_axis(system)
        sigma = density_grid(system, bounds, resolution, field=field, chunk=chunk)
        if sparse:
            return cls._build_sparse(system, sigma, bounds, resolution, level, img_id, rows, view_dir, field, chunk, int(sh_degree), dirs)
        colour = lambda d: field_colour(system, bounds, resolution, d, img_id=img_id, rows=rows, field=field, chunk=chunk)
        if sh_degree != 0:
            return cls._project(sigma, lambda k: colour(dirs[k]), dirs, bounds, level, sh_degree)
        return cls.from_grids(sigma, colour(view_dir), bounds, level)

    @classmethod
    @torch.no_grad()
    def _build_sparse(cls, system, sigma, bounds, resolution, level, img_id, rows, view_dir, field, chunk, degree, dirs) -> "BakedScene":
        """build(sparse=True) from the dense sigma on: table, sigma to the pool, colour on the pool's lines, packing."""
        level = _level(level)
        res = tuple(int(n) for n in resolution)
        # the cells that touch a kept point: a corner finite and >= max(level, TINY) is a corner that is finite, > 0 and >= level
        occ = OccupancyGrid.from_density(sigma, bounds, level=max(level, TINY), dilate=0)
        slots, bricks, n = brick_table(occ.words, occ.dims)
        pool_sigma = brick_gather(sigma.unsqueeze(-1), bricks).squeeze(-1)  # [n, 9, 9, 9]; zero beyond the grid: dropped below
        del sigma, occ
        P, dev = _lib.BRICK_POINTS, pool_sigma.device
        E = POINT_BYTES[degree]
        if n == 0:
            pool = Layout.empty_pool(degree, dev)
        elif degree == 0:
            rgb = pool_colour(system, bounds, res, bricks, view_dir, img_id=img_id, rows=rows, field=field, chunk=chunk)
            pool = pack_rgbs(pool_sigma, rgb, level, out=_aligned(n * P ** 3 * E, E, dev)[:n * P ** 3 * E].view(n, P, P, P, E).view(torch.float32))
        else:
            colour = lambda k: pool_colour(system, bounds, res, bricks, dirs[k], img_id=img_id, rows=rows, field=field, chunk=chunk)
            pool = cls._project_records(pool_sigma, colour, dirs, level, degree)
        return cls._sparse(pool, slots, bricks, res, bounds, level, degree)

    # ---- rendering ---------------------------------------------------------------------------------------------------------

    def render(self, rays: torch.Tensor, step: float, background: float = 0.0, stop: float = 0.0, out: Optional[dict] = None) -> dict:
        """With an environment (`self.env` not None): the march below at background 0, then upnerf_env_composite in place on its
        rgb -- rgb + (1 - opacity) env(d); `background` is NOT LOOKED AT then (it is still checked to be finite); depth and opacity
        are the march's own (depth still gets (1 - opacity) far).  Without one, no launch is added and every bit is as it was:

        {"rgb" [R, 3], "depth" [R], "opacity" [R]} of [R, 8] device rays (upnerf_baked_render; upnerf_baked_sh_render for an
        SH scene; upnerf_baked_sparse_render for a sparse scene of any degree, the same march and the same bits; each sample's colour then being the expansion at the ray's own direction, clamped to [0, 1]): samples every
        `step` of t from near + step / 2, alpha-composited front to back; what the ray does not hit shows `background` at depth
        `far`.  stop > 0 ends a ray once its transmittance falls below it.  out: preallocated buffers of at least R rows."""
        require_cuda("BakedScene.render", rays)
        step, background, stop = _render_args(rays, step, background, stop)
        rays = _rays16(rays)
        R, dev = rays.shape[0], rays.device
        if out is None:
            out = {"rgb": torch.empty(R, 3, device=dev), "depth": torch.empty(R, device=dev), "opacity": torch.empty(R, device=dev)}
        for k, shape in (("rgb", (3,)), ("depth", ()), ("opacity", ())):
            t = out[k]
            if t.dtype != torch.float32 or t.shape[0] < R or tuple(t.shape[1:]) != shape or t.device != dev:
                raise ValueError("the outputs are fp32 [>= R, 3], [>= R] and [>= R] on the rays' device")
        march(self.grid, self.layout, rays, step, background if self.env is None else 0.0, stop, out["rgb"], out["depth"], out["opacity"])
        if self.env is not None:
            self.env.composite_(rays, out["rgb"], out["opacity"])
        return {k: out[k][:R] for k in ("rgb", "depth", "opacity")}

    def tune(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, tv_sigma: float = 0.0, tv_colour: float = 0.0, tv_eps: float = 1e-8):
        """A `baked_tune.BakedTuner` on this (dense) scene: Adam on its points against target pixels, with a total
        variation penalty where tv_sigma or tv_colour is not zero."""
        from .baked_tune import BakedTuner
        return BakedTuner(self, lr, betas=betas, eps=eps, tv_sigma=tv_sigma, tv_colour=tv_colour, tv_eps=tv_eps)

    def tune_pool(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, tv_sigma: float = 0.0, tv_colour: float = 0.0, tv_eps: float = 1e-8):
        """A `baked_sparse_tune.PoolTuner` on this (sparse) scene: Adam on the points of its pool, in place, with
        the same optional total variation penalty."""
        from .baked_sparse_tune import PoolTuner
        return PoolTuner(self, lr, betas=betas, eps=eps, tv_sigma=tv_sigma, tv_colour=tv_colour, tv_eps=tv_eps)

    def upsample(self, level: Optional[float] = None) -> "BakedScene":
        """The scene of twice the cells per axis (2 N - 1 points): the same bounds, degree and layout -- dense stays dense, sparse
        stays sparse, pool to pool -- every child point the trilinear value of this grid, pruned at `level` (default: this scene's).
        `baked_reg.upsample`; DESIGN.md 2.37."""
        from .baked_reg import upsample
        return upsample(self, level)

    def visibility(self, rays: torch.Tensor, step: float, stop: float = 0.0, chunk: int = 16384) -> torch.Tensor:
        """Per point, the largest compositing weight any of `rays` gives a sample in a cell touching it (at least 2^-126 where a
        ray reaches such a cell with light left, else 0): fp32 [Nz, Ny, Nx], or [n_bricks, 9, 9, 9] of a sparse scene, the copies
        of a shared point equal.  The same bits every run and for every `chunk`.  `baked_prune.visibility`; DESIGN.md 2.39."""
        from .baked_prune import visibility
        return visibility(self, rays, step, stop, chunk)

    def prune(self, rays: torch.Tensor, step: float, min_weight: Optional[float] = None, stop: float = 0.0, chunk: int = 16384) -> "BakedScene":
        """A new scene of the same bounds, degree, level, layout and environment without the points whose visibility from `rays`
        is below `min_weight` (default 2^-126: only what no ray sees goes, and `rays` render to the same bits at this `step` and
        `stop`); a sparse scene loses the bricks that are left empty.  This scene is not modified.  `baked_prune.prune`."""
        from .baked_prune import prune
        return prune(self, rays, step, min_weight, stop, chunk)

    # ---- files -------------------------------------------------------------------------------------------------------------

    def save(self, path: str) -> None:
        """An .npz holding the grid (`rgbs`, or `records` and `degree` of an SH scene), the bounds and the level; the bits are
        rebuilt on load.  A sparse scene: pool, bricks, resolution, degree, bounds, level (save_bricks)."""
        env = self.env.env.cpu().numpy() if self.env is not None else None  # (a scene without one writes the file it always wrote)
        if self.sparse:
            save_bricks(path, self.pool.detach().cpu().numpy(), self.bricks.cpu().numpy(), self.resolution, self.bounds, self.level,
                        sh_degree=self.sh_degree, env=env)
        elif self.sh_degree:
            save_arrays(path, self.records.detach().cpu().numpy(), self.bounds, self.level, sh_degree=self.sh_degree, env=env)
        else:
            save_arrays(path, self.rgbs.detach().cpu().numpy(), self.bounds, self.level, env=env)

    @classmethod
    def load(cls, path: str, device="cuda") -> "BakedScene":
        """The scene of a file `save` wrote; with the array `env` in it (ENV_KEY: a file of a scene with an environment) the
        environment too, else `env` None."""
        with np.load(path) as f:
            env = _env_array(path, f[ENV_KEY]) if ENV_KEY in f.files else None
        scene = cls._load(path, device)
        if env is None:
            return scene
        from .baked_env import Environment
        return scene.with_environment(Environment.from_array(env, device))

    @classmethod
    def _load(cls, path: str, device) -> "BakedScene":
        with np.load(path) as f:
            keys = set(f.files) - {ENV_KEY}
        if keys == BRICK_KEYS:
            pool, bricks, resolution, bounds, level, degree = load_bricks(path)
            E = POINT_BYTES[degree]
            store = _aligned(pool.nbytes, E, torch.device(device))[:pool.nbytes].view(pool.shape[:4] + (E,))
            store.copy_(torch.from_numpy(pool.view(np.uint8).reshape(pool.shape[:4] + (E,))))
            return cls.from_bricks(store if degree else store.view(torch.float32), torch.from_numpy(bricks).to(device), resolution,
                                   bounds, level, degree)
        grid, bounds, level, *degree = load_arrays(path)
        if degree:
            return cls.from_records(torch.from_numpy(grid).to(device).contiguous(), bounds, level, degree[0])
        return cls(torch.from_numpy(grid).to(device).contiguous(), bounds, level)

    # ---- accessors ---------------------------------------------------------------------------------------------------------

    @property
    def grid(self) -> torch.Tensor:
        """The tensor the marcher reads: `pool` of a sparse scene, `records` of an SH scene, else `rgbs`."""
        if self.sparse:
            return self.pool
        return self.records if self.sh_degree else self.rgbs

    @property
    def sparse(self) -> bool:
        """Whether only the occupied bricks are stored (`pool`, `slots`, `bricks`)."""
        return self.pool is not None

    @property
    def n_bricks(self) -> int:
        """Occupied bricks: the bricks of a sparse scene's pool; of a dense scene, the set brick bits (a device reduction)."""
        return int(self.bricks.numel()) if self.sparse else int(self.occupancy.bricks().sum())

    @property
    def brick_fraction(self) -> float:
        """f_b: the occupied share of the bricks."""
        Bx, By, Bz = self.occupancy.brick_dims
        return self.n_bricks / (Bx * By * Bz)

    @property
    def device(self):
        return self.occupancy.words.device

    @property
    def points(self) -> torch.Tensor:
        """The tensor whose address the marcher is given: `grid`, or of a sparse scene with no brick its layout's spare point."""
        return self.layout.marched(self.grid)

    @property
    def resolution(self):
        return self.layout.resolution

    @property
    def nbytes(self) -> int:
        """Device bytes of the grid and its bits; of a sparse scene, of the pool, its table (slots and bricks) and the bits."""
        if self.sparse:
            return self.pool.numel() * self.pool.element_size() + (self.slots.numel() + self.bricks.numel() + self.occupancy.words.numel()) * 4
        return self.grid.numel() * self.grid.element_size() + self.occupancy.words.numel() * 4

    @property
    def fraction(self) -> float:
        """Occupied share of the cells."""
        return self.occupancy.fraction


ENV_KEY = "env"  # the one optional array of a scene's file: the environment map [6, E+1, E+1, 4] fp32


def _env_array(what: str, env) -> np.ndarray:
    env = np.asarray(env)
    if env.dtype != np.float32 or env.ndim != 4 or env.shape[0] != 6 or env.shape[1] != env.shape[2] or env.shape[1] < 2 or env.shape[3] != 4:
        raise ValueError(f"{what}: the environment is a fp32 array [6, E+1, E+1, 4], got {env.dtype} {env.shape}")
    return np.ascontiguousarray(env)


def _env_entry(what: str, env) -> dict:
    return {} if env is None else {ENV_KEY: _env_array(what, env)}


def save_arrays(path: str, rgbs: np.ndarray, bounds, level: float, sh_degree: int = 0, env=None) -> None:
    """rgbs: the fp32 grid [Nz, Ny, Nx, 4]; with sh_degree = 1 | 2 the uint8 records [Nz, Ny, Nx, 32 | 64] instead, written as
    the arrays records, degree, bounds, level.  env: the environment map [6, E+1, E+1, 4] fp32 or None (no array `env` then)."""
    grid = np.asarray(rgbs)
    if sh_degree != 0:
        if grid.dtype != np.uint8 or grid.ndim != 4 or grid.shape[3] != RECORD_BYTES[_degree(sh_degree)]:
            raise ValueError(f"the records of degree {sh_degree} are a uint8 array [Nz, Ny, Nx, {RECORD_BYTES[sh_degree]}]")
        arrays = dict(records=grid, degree=np.int64(sh_degree))
    else:
        if grid.dtype != np.float32 or grid.ndim != 4 or grid.shape[3] != 4:
            raise ValueError("rgbs is a fp32 array [Nz, Ny, Nx, 4]")
        arrays = dict(rgbs=grid)
    lo, hi = box(bounds, strict=True)
    with open(path, "wb") as fh:  # (a file object: numpy appends no .npz of its own to the name)
        np.savez(fh, **arrays, **_env_entry("save_arrays", env), bounds=np.asarray([lo, hi], np.float64), level=np.float64(level))


BRICK_KEYS = {"pool", "bricks", "resolution", "degree", "bounds", "level"}


def _brick_arrays(what: str, pool, bricks, resolution, degree):
    """The arrays of a sparse scene, checked against each other; ValueError names `what`."""
    pool, bricks, resolution, degree = np.asarray(pool), np.asarray(bricks), np.asarray(resolution), np.asarray(degree)
    bad = ValueError(f"{what}: not a sparse baked scene (pool {pool.dtype} {pool.shape}, bricks {bricks.dtype} {bricks.shape}, "
                     f"resolution {resolution.tolist() if resolution.size < 8 else resolution.shape}, degree {degree.tolist() if degree.size < 8 else degree.shape})")
    if degree.shape != () or degree.dtype.kind not in "iu" or int(degree) not in POINT_BYTES:
        raise bad
    if resolution.shape != (3,) or resolution.dtype.kind not in "iu" or resolution.min() < 2:
        raise bad
    d, P = int(degree), _lib.BRICK_POINTS
    want = (np.float32, 4) if d == 0 else (np.uint8, POINT_BYTES[d])
    if pool.dtype != want[0] or pool.ndim != 5 or pool.shape[1:] != (P, P, P, want[1]):
        raise bad
    B = [(int(n) - 1 + 7) // 8 for n in resolution]
    if bricks.dtype != np.int32 or bricks.shape != (pool.shape[0],):
        raise bad
    if bricks.size and (bricks.min() < 0 or bricks.max() >= B[0] * B[1] * B[2] or not (np.diff(bricks.astype(np.int64)) > 0).all()):
        raise bad
    return np.ascontiguousarray(pool), np.ascontiguousarray(bricks), tuple(int(n) for n in resolution), d


def save_bricks(path: str, pool: np.ndarray, bricks: np.ndarray, resolution, bounds, level: float, sh_degree: int = 0, env=None) -> None:
    """A sparse scene's file: the arrays pool ([n_bricks, 9, 9, 9, 4] fp32, or [n_bricks, 9, 9, 9, 32 | 64] uint8 at sh_degree
    1 | 2), bricks (int32 [n_bricks], strictly ascending), resolution (Nx, Ny, Nz), degree, bounds, level, and with `env` given the
    environment map `env`.  Anything else raises ValueError."""
    pool, bricks, resolution, degree = _brick_arrays("save_bricks", pool, bricks, np.asarray(resolution, np.int64), np.int64(sh_degree) if sh_degree in (0, 1, 2) else np.float64(-1))
    lo, hi = box(bounds, strict=True)
    with open(path, "wb") as fh:
        np.savez(fh, pool=pool, bricks=bricks, resolution=np.asarray(resolution, np.int64), degree=np.int64(degree),
                 bounds=np.asarray([lo, hi], np.float64), level=np.float64(level), **_env_entry("save_bricks", env))


def load_bricks(path: str):
    """(pool, bricks, resolution, bounds, level, degree) of a file save_bricks wrote; any other key set, and arrays that do not
    fit each other, raise ValueError."""
    with np.load(path) as f:
        if set(f.files) - {ENV_KEY} != BRICK_KEYS:
            raise ValueError(f"{path}: not a sparse baked scene (arrays {sorted(f.files)})")
        pool, bricks, resolution, degree, bounds, level = (f[k] for k in ("pool", "bricks", "resolution", "degree", "bounds", "level"))
    if bounds.shape != (2, 3) or level.shape != ():
        raise ValueError(f"{path}: not a sparse baked scene (bounds {bounds.shape}, level {level.shape})")
    pool, bricks, resolution, degree = _brick_arrays(path, pool, bricks, resolution, degree)
    return pool, bricks, resolution, box(bounds.tolist(), strict=True), float(level), degree


def load_arrays(path: str):
    """(rgbs fp32 [Nz, Ny, Nx, 4], bounds, level) of a file BakedScene.save wrote, or (records uint8 [Nz, Ny, Nx, 32 | 64],
    bounds, level, degree) of an SH scene's; anything else raises ValueError."""
    with np.load(path) as f:
        files = set(f.files) - {ENV_KEY}  # (the environment, where there is one, is BakedScene.load's to read)
        if files == {"records", "degree", "bounds", "level"}:
            records, bounds, level, degree = f["records"], f["bounds"], float(f["level"]), f["degree"]
            if degree.shape != () or int(degree) not in RECORD_BYTES or records.dtype != np.uint8 or records.ndim != 4 or \
                    records.shape[3] != RECORD_BYTES[int(degree)] or bounds.shape != (2, 3) or min(records.shape[:3]) < 2:
                raise ValueError(f"{path}: not a baked scene (records {records.dtype} {records.shape}, degree {degree}, bounds {bounds.shape})")
            return np.ascontiguousarray(records), box(bounds.tolist(), strict=True), level, int(degree)
        if files != {"rgbs", "bounds", "level"}:
            raise ValueError(f"{path}: not a baked scene (arrays {sorted(f.files)})")
        rgbs, bounds, level = f["rgbs"], f["bounds"], float(f["level"])
    if rgbs.dtype != np.float32 or rgbs.ndim != 4 or rgbs.shape[3] != 4 or bounds.shape != (2, 3) or min(rgbs.shape[:3]) < 2:
        raise ValueError(f"{path}: not a baked scene (rgbs {rgbs.dtype} {rgbs.shape}, bounds {bounds.shape})")
    return np.ascontiguousarray(rgbs), box(bounds.tolist(), strict=True), level
