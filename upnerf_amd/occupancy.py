"""Empty-space skipping: a bit-packed occupancy grid of the trained density, and the rays of a frame walked through it.

    bounds = bounds_from_cameras(system, margin=0.5)
    occ = OccupancyGrid.build(system, bounds, (256, 256, 256), level=10.0, dilate=1)
    out = render_path(system, path, occupancy=occ)          # only the rays that touch something, over the part that does

The cells are the boxes between the points of a `density_grid` (the cells marching tetrahedra walks); a cell is occupied iff
one of its corners is finite and >= level -- the comparison of `extract_surface`, so the mesh at that level lies in occupied
cells.  Everything on the render path is HIP (csrc/occupancy.hip): `upnerf_occ_build` packs the grid,
`upnerf_occ_spans` walks the rays, `upnerf_occ_compact` / `upnerf_occ_scatter` take the hit rows out and put their results
back.  There is no CPU path.  A skipped pixel shows the BACKGROUND, not what the full render would have composited from faint
density below `level`: `level` and `dilate` trade speed for that."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .ops import TIMER
from .static_scene import box, c_float3, require_cuda

__all__ = ["OccupancyGrid", "ray_spans", "compact_hits", "compact_rays", "scatter_results", "BRICK"]

BRICK = 8  # cells per brick edge (OCC_BRICK)


def _bounds(bounds):  # hi > lo on every axis, or the cells have no size
    return box(bounds, strict=True)


def _unpack(words: torch.Tensor, n: int) -> torch.Tensor:
    """The first n bits of int32 words as a bool vector (an accessor for tests and statistics, not on the render path)."""
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    return ((words[:, None] >> shifts) & 1).bool().reshape(-1)[:n]


class OccupancyGrid:
    """Packed occupancy of Cx x Cy x Cz cells over `bounds`: `words` (int32 device tensor) holds the fine bits -- cell
    (x, y, z) is bit (z * Cy + y) * Cx + x, 32 per word -- and after them one bit per 8 x 8 x 8 brick."""

    def __init__(self, words: torch.Tensor, bounds, dims: Sequence[int]):
        self.words = words
        self.bounds = _bounds(bounds)
        self.dims = tuple(int(c) for c in dims)  # (Cx, Cy, Cz)
        Cx, Cy, Cz = self.dims
        n = lib.upnerf_occ_words(Cx, Cy, Cz)
        if n < 0 or words.numel() != n or words.dtype != torch.int32:
            raise ValueError(f"{Cx} x {Cy} x {Cz} cells are packed into {n} int32 words")
        self.n_cells = Cx * Cy * Cz
        self.brick_dims = tuple((c + BRICK - 1) // BRICK for c in self.dims)
        self.fine_words = (self.n_cells + 31) // 32

    # ---- construction ------------------------------------------------------------------------------------------------------

    @classmethod
    def _build(cls, bounds, dims, dev, dilate, grid=None, cells=None, level=0.0) -> "OccupancyGrid":
        Cx, Cy, Cz = dims
        dilate = int(dilate)
        if dilate < 0:
            raise ValueError(f"dilate is a number of rounds >= 0, got {dilate}")
        if min(dims) < 1:
            raise ValueError(f"an occupancy grid has at least one cell per axis (two grid points), got {dims} cells")
        n = lib.upnerf_occ_words(Cx, Cy, Cz)
        if n < 0:
            check(int(n), f"upnerf_occ_words({Cx}, {Cy}, {Cz})")
        words = torch.empty(n, device=dev, dtype=torch.int32)
        scratch = torch.empty(lib.upnerf_occ_build_scratch(Cx, Cy, Cz), device=dev, dtype=torch.uint8)
        a = _lib.OccBuildArgs(Cx=Cx, Cy=Cy, Cz=Cz, dilate=dilate, level=float(level), grid=ptr(grid), cells=ptr(cells),
                              words=ptr(words), scratch=ptr(scratch))
        check(TIMER.run("occ_build", lambda: lib.upnerf_occ_build(C.byref(a), stream()), units=Cx * Cy * Cz), "upnerf_occ_build")
        return cls(words, bounds, dims)

    @classmethod
    def from_density(cls, grid: torch.Tensor, bounds, level: float, dilate: int = 1) -> "OccupancyGrid":
        """From a [Nz, Ny, Nx] fp32 device grid of densities at grid points (density_grid): cell occupied iff a corner is finite
        and >= level, then `dilate` rounds of 26-neighbour dilation.  `level` has no default: the useful threshold depends on
        the scene's scale (see extract_surface)."""
        require_cuda("OccupancyGrid.from_density", grid)
        if grid.dtype != torch.float32 or grid.dim() != 3:
            raise ValueError("the grid is a fp32 tensor [Nz, Ny, Nx]")
        level = float(level)
        if level != level:
            raise ValueError("level is not a number")
        grid = grid.detach().contiguous()
        Nz, Ny, Nx = grid.shape
        return cls._build(_bounds(bounds), (Nx - 1, Ny - 1, Nz - 1), grid.device, dilate, grid=grid, level=level)

    @classmethod
    def from_cells(cls, cells: torch.Tensor, bounds, dilate: int = 0) -> "OccupancyGrid":
        """From a [Cz, Cy, Cx] bool or uint8 device tensor (non-zero = occupied)."""
        require_cuda("OccupancyGrid.from_cells", cells)
        if cells.dtype not in (torch.bool, torch.uint8) or cells.dim() != 3:
            raise ValueError("the cells are a bool or uint8 tensor [Cz, Cy, Cx]")
        cells = cells.detach().to(torch.uint8).contiguous()
        Cz, Cy, Cx = cells.shape
        return cls._build(_bounds(bounds), (Cx, Cy, Cz), cells.device, dilate, cells=cells)

    @classmethod
    def build(cls, system, bounds, resolution: Sequence[int], level: float, dilate: int = 1, field: str = "fine") -> "OccupancyGrid":
        """density_grid(system, bounds, resolution, field) and from_density: `resolution` counts grid POINTS per axis."""
        from .geometry import density_grid
        return cls.from_density(density_grid(system, bounds, resolution, field=field), bounds, level, dilate=dilate)

    # ---- accessors ---------------------------------------------------------------------------------------------------------

    def cells(self) -> torch.Tensor:
        """bool [Cz, Cy, Cx] device tensor of the fine bits."""
        Cx, Cy, Cz = self.dims
        return _unpack(self.words[:self.fine_words], self.n_cells).reshape(Cz, Cy, Cx)

    def bricks(self) -> torch.Tensor:
        """bool [Bz, By, Bx] device tensor of the brick bits."""
        Bx, By, Bz = self.brick_dims
        return _unpack(self.words[self.fine_words:], Bx * By * Bz).reshape(Bz, By, Bx)

    def n_occupied(self) -> int:
        """The number of occupied cells, counted from the packed words themselves: a population count per word in a few
        word-sized integer passes (8 bytes a word, a quarter of a byte a cell -- nothing per cell, unlike cells()), the last word
        masked to the grid's cells.  One host read."""
        w = self.words[:self.fine_words].to(torch.int64) & 0xFFFFFFFF
        tail = self.n_cells - 32 * (self.fine_words - 1)
        w[-1] &= (1 << tail) - 1
        w = w - ((w >> 1) & 0x55555555)
        w = (w & 0x33333333) + ((w >> 2) & 0x33333333)
        w = (w + (w >> 4)) & 0x0F0F0F0F
        return int(((w * 0x01010101 >> 24) & 0xFF).sum())

    @property
    def fraction(self) -> float:
        """Occupied share of the cells."""
        return float(self.cells().float().mean())


def _rays(what: str, rays: torch.Tensor) -> torch.Tensor:
    require_cuda(what, rays)
    if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or rays.shape[0] < 1:
        raise ValueError("rays are a fp32 tensor [R, 8] (o | d | near | far) with R >= 1")
    return rays.contiguous()


def ray_spans(occ: OccupancyGrid, rays: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """(t0 fp32 [R], t1 fp32 [R], hit uint8 [R]) of [R, 8] device rays (upnerf_occ_spans): entry into the first occupied cell
    (>= near), exit from the last (<= far), hit = 1 iff t1 > t0; a miss has t0 = t1 = far.  `out`: preallocated buffers with at
    least R entries."""
    rays = _rays("ray_spans", rays)
    R, dev = rays.shape[0], rays.device
    if out is None:
        out = (torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev, dtype=torch.uint8))
    t0, t1, hit = out
    if min(t0.numel(), t1.numel(), hit.numel()) < R or t0.dtype != torch.float32 or t1.dtype != torch.float32 or hit.dtype != torch.uint8:
        raise ValueError(f"t0, t1 are fp32 and hit is uint8, each with at least {R} entries")
    Cx, Cy, Cz = occ.dims
    lo, hi = occ.bounds
    a = _lib.OccSpansArgs(Cx=Cx, Cy=Cy, Cz=Cz, R=R, lo=c_float3(lo), hi=c_float3(hi), words=ptr(occ.words),
                          rays=ptr(rays), t0=ptr(t0), t1=ptr(t1), hit=ptr(hit))
    check(TIMER.run("occ_spans", lambda: lib.upnerf_occ_spans(C.byref(a), stream()), units=R), "upnerf_occ_spans")
    return t0[:R], t1[:R], hit[:R]


def compact_workspace(R: int, dims: Sequence[int], device) -> dict:
    """The buffers of spans, compaction and scatter for up to R rays and row tables of widths `dims`."""
    f32 = dict(device=device, dtype=torch.float32)
    return {"t0": torch.empty(R, **f32), "t1": torch.empty(R, **f32), "hit": torch.empty(R, device=device, dtype=torch.uint8),
            "index": torch.empty(R, device=device, dtype=torch.int32), "count": torch.empty(1, device=device, dtype=torch.int32),
            "rays_c": torch.empty(R, 8, **f32), "rows_c": [torch.empty(R, d, **f32) for d in dims],
            "scan": torch.empty(lib.upnerf_occ_compact_scratch(R), device=device, dtype=torch.uint8)}


def compact_hits(rays: torch.Tensor, t0: torch.Tensor, t1: torch.Tensor, hit: torch.Tensor, rows: Sequence[torch.Tensor] = (),
                 ws: Optional[dict] = None):
    """(rays_c [n_hit, 8], [rows_c [n_hit, dim]], index int32 [n_hit], n_hit) -- the rows with hit != 0 in ascending order
    (upnerf_occ_compact), near / far of the ray rows replaced by t0 / t1.  One host read: the hit count."""
    rays = _rays("compact_hits", rays)
    require_cuda("compact_hits", t0, t1, hit, *rows)
    R, dev = rays.shape[0], rays.device
    if t0.dtype != torch.float32 or t1.dtype != torch.float32 or hit.dtype not in (torch.uint8, torch.bool):
        raise ValueError("t0, t1 are fp32 [R] and hit is uint8 [R]")
    if not (t0.numel() == t1.numel() == hit.numel() == R):
        raise ValueError("t0, t1 and hit hold one entry per ray")
    if len(rows) > _lib.PATH_MAX_TABLES:
        raise ValueError(f"at most {_lib.PATH_MAX_TABLES} row tables per launch, got {len(rows)}")
    for t in rows:
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != R or not 1 <= t.shape[1] <= _lib.PATH_MAX_DIM:
            raise ValueError(f"a row table is fp32 [R, dim] with dim <= {_lib.PATH_MAX_DIM}")
    hit = (hit != 0).to(torch.uint8) if hit.dtype == torch.bool else hit.contiguous()
    t0, t1 = t0.contiguous(), t1.contiguous()
    if ws is None:
        ws = compact_workspace(R, [t.shape[1] for t in rows], dev)
    a = _lib.OccCompactArgs(R=R, n_tables=len(rows), hit=ptr(hit), t0=ptr(t0), t1=ptr(t1), rays=ptr(rays),
                            rays_c=ptr(ws["rays_c"]), index=ptr(ws["index"]), count=ptr(ws["count"]), scratch=ptr(ws["scan"]))
    if ws["rays_c"].shape[0] < R or ws["index"].numel() < R or len(ws["rows_c"]) != len(rows):
        raise ValueError("the workspace is smaller than the chunk")
    keep = []  # (contiguous copies stay alive until the launch is enqueued)
    for j, (t, o) in enumerate(zip(rows, ws["rows_c"])):
        t = t.contiguous()
        keep.append(t)
        if o.shape[0] < R or o.shape[1] != t.shape[1]:
            raise ValueError("the workspace is smaller than the chunk")
        a.tables[j] = _lib.PathTable(table=ptr(t), dim=t.shape[1], n_rows=R, out=ptr(o))
    check(TIMER.run("occ_compact", lambda: lib.upnerf_occ_compact(C.byref(a), stream()), units=R), "upnerf_occ_compact")
    n = int(ws["count"].cpu())  # the one host read: render_rays takes R from a tensor shape
    return ws["rays_c"][:n], [o[:n] for o in ws["rows_c"]], ws["index"][:n], n


def compact_rays(occ: OccupancyGrid, rays: torch.Tensor, rows: Sequence[torch.Tensor] = (), ws: Optional[dict] = None):
    """ray_spans and compact_hits: (rays_c, rows_c, index, n_hit) of the rays that touch an occupied cell."""
    rays = _rays("compact_rays", rays)
    require_cuda("compact_rays", *rows)
    if ws is None:
        ws = compact_workspace(rays.shape[0], [t.shape[1] for t in rows], rays.device)
    t0, t1, hit = ray_spans(occ, rays, out=(ws["t0"], ws["t1"], ws["hit"]))
    return compact_hits(rays, t0, t1, hit, rows, ws=ws)


def scatter_results(index: torch.Tensor, rays: torch.Tensor, rgb_c: Optional[torch.Tensor], depth_c: Optional[torch.Tensor] = None,
                    background: float = 0.0, want_depth: Optional[bool] = None, out_rgb: Optional[torch.Tensor] = None,
                    out_depth: Optional[torch.Tensor] = None):
    """(rgb [R, 3], depth [R] or None): the results of the compacted rows (`rgb_c` [n_hit, 3], `depth_c` [n_hit]) at the rows
    `index` names, the background colour and the ray's own far on every other row (upnerf_occ_scatter).  n_hit = len(index);
    with n_hit == 0 rgb_c / depth_c may be None.  want_depth defaults to `depth_c is not None`."""
    rays = _rays("scatter_results", rays)
    require_cuda("scatter_results", index, *[t for t in (rgb_c, depth_c) if t is not None])
    R, dev, n = rays.shape[0], rays.device, index.numel()
    if index.dtype != torch.int32 or n > R:
        raise ValueError("index is int32 [n_hit] with n_hit <= R")
    want_depth = (depth_c is not None) if want_depth is None else bool(want_depth)
    if n > 0 and (rgb_c is None or rgb_c.dtype != torch.float32 or tuple(rgb_c.shape) != (n, 3)):
        raise ValueError("rgb_c is fp32 [n_hit, 3]")
    if n > 0 and want_depth and (depth_c is None or depth_c.dtype != torch.float32 or depth_c.numel() != n):
        raise ValueError("depth_c is fp32 [n_hit]")
    rgb = torch.empty(R, 3, device=dev) if out_rgb is None else out_rgb
    depth = (torch.empty(R, device=dev) if out_depth is None else out_depth) if want_depth else None
    for t, shape in ((rgb, (3,)), (depth, ())):
        if t is not None and (t.dtype != torch.float32 or t.shape[0] < R or tuple(t.shape[1:]) != shape):
            raise ValueError("the outputs are fp32 [>= R, 3] and [>= R]")
    keep = [x.contiguous() if x is not None and n > 0 else None for x in (index, rgb_c, depth_c if want_depth else None)]
    a = _lib.OccScatterArgs(R=R, n_hit=n, background=float(background), index=ptr(keep[0]), rays=ptr(rays), rgb_c=ptr(keep[1]),
                            depth_c=ptr(keep[2]), rgb=ptr(rgb), depth=ptr(depth))
    check(TIMER.run("occ_scatter", lambda: lib.upnerf_occ_scatter(C.byref(a), stream()), units=R), "upnerf_occ_scatter")
    return rgb[:R], (depth[:R] if depth is not None else None)
