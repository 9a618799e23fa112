"""Geometry of a trained scene: the shared density on a grid, its iso-surface as a coloured triangle mesh, a PLY file.

    bounds = bounds_from_cameras(system, margin=0.5)
    grid = density_grid(system, bounds, (256, 256, 256))
    mesh = extract_surface(grid, bounds, level=10.0)
    mesh.colours = colour_vertices(system, mesh, img_id=3, slab=0.02)
    mesh.write_ply("scene.ply")

The density pass runs the field kernels the training step runs (`upnerf_field_fwd*`, density head only) on rays that ARE grid
columns (`upnerf_grid_columns`); the surface is marching tetrahedra on the Kuhn split of every cell, in HIP
(`upnerf_mtet_count` / `upnerf_mtet_emit`, csrc/mesh.hip).  There is no CPU path for either.  The case tables
live HERE and are handed to the kernels; PLY files and camera bounds are plain host code.

A surface without a density threshold: the depth maps the model renders from its refined training poses, fused into a
truncated signed distance volume whose zero level is meshed (csrc/tsdf.hip):

    vol = fuse_views(system, bounds, (256, 256, 256))
    mesh = vol.extract()           # vertices, normals towards the cameras, faces and the fused colours
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .ops import TIMER
from .novel_view import path_rays
from .static_scene import (appearance_rows, box, c_float3, field_of, intrinsics, near_far, per_image, plane, refined_training_poses,
                           render_static, require_cuda, static_keys)

__all__ = ["TETS", "EDGES", "TET_EDGES", "TRI_TABLE", "edge_owner", "Mesh", "read_ply", "density_grid", "grid_columns",
           "extract_surface", "colour_vertices", "bounds_from_cameras", "refine_normals", "TsdfVolume", "fuse_views"]

# ---- the tables of the split (the only copy: the kernels receive them as an argument) ---------------------------------------
# Corner c of a cell is its origin + (c & 1, (c >> 1) & 1, c >> 2).  The Kuhn split: one tetrahedron per order in which the
# three axes are walked from corner 0 to corner 7, in the order of itertools.permutations((0, 1, 2)); vertices 1 and 2 of the
# odd orders are swapped, so that det(v1 - v0, v2 - v0, v3 - v0) > 0 for all six and one triangle table serves them all.
TETS = ((0, 1, 3, 7), (0, 5, 1, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 6, 4, 7))
# The seven edges a grid point owns, slot s -> offset of the far end: +x, +y, +z, the face diagonals xy, xz, yz, the body diagonal.
EDGES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# The six edges of a tetrahedron as pairs of its vertices.
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# case = sum of (vertex i inside) << i  ->  triangles as triples of tet edges, wound so that the geometric normal points from the
# inside vertices to the outside ones (towards lower density) in a positively oriented tetrahedron.  One inside (or outside)
# vertex: its three edges in ascending order, two of them swapped where the winding asks for it; two inside vertices a < b and
# outside c < d: the quad (ac, ad, bd, bc) cut along ac-bd.
TRI_TABLE = (
    (),
    ((0, 1, 2),),
    ((0, 4, 3),),
    ((1, 2, 4), (1, 4, 3)),
    ((1, 3, 5),),
    ((0, 5, 2), (0, 3, 5)),
    ((0, 4, 5), (0, 5, 1)),
    ((2, 4, 5),),
    ((2, 5, 4),),
    ((0, 1, 5), (0, 5, 4)),
    ((0, 5, 3), (0, 2, 5)),
    ((1, 5, 3),),
    ((1, 3, 4), (1, 4, 2)),
    ((0, 3, 4),),
    ((0, 2, 1),),
    (),
)
MIN_SAMPLES = 32  # the field kernels' minimum of samples per ray (UPNERF_EUNSUP below it)


def edge_owner(c0: int, c1: int) -> Tuple[Tuple[int, int, int], int]:
    """The cell edge between corners c0 and c1 -> (offset of the grid point that owns it from the cell origin, its slot there).
    Only nested corners (one contains the other's axes) are joined by an edge of the split: anything else raises."""
    lo, hi = (c0, c1) if c0 & c1 == c0 else (c1, c0)
    if lo & hi != lo or lo == hi:
        raise ValueError(f"corners {c0} and {c1} are not joined by an edge of the Kuhn split")
    d = lo ^ hi
    return (lo & 1, (lo >> 1) & 1, lo >> 2), EDGES.index((d & 1, (d >> 1) & 1, d >> 2))


def _tables() -> "_lib.MtetTables":
    t = _lib.MtetTables()
    for i, tet in enumerate(TETS):
        for k, c in enumerate(tet):
            t.tets[i][k] = c
    for s, off in enumerate(EDGES):
        for k, v in enumerate(off):
            t.edges[s][k] = v
    for e, pair in enumerate(TET_EDGES):
        t.tet_edges[e][0], t.tet_edges[e][1] = pair
    for case, tris in enumerate(TRI_TABLE):
        t.tris[case][0] = len(tris)
        for j, tri in enumerate(tris):
            for k, e in enumerate(tri):
                t.tris[case][1 + 3 * j + k] = e
    return t


# ---- meshes and PLY files (host code) -------------------------------------------------------------------------------------------

_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {V}\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
               "property uchar blue\nelement face {F}\nproperty list uchar int vertex_indices\nend_header\n")
_PLY_VERTEX = np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)])
_PLY_FACE = np.dtype([("k", "u1"), ("v", "<i4", 3)])


@dataclass
class Mesh:
    """An indexed triangle mesh: device tensors out of extract_surface, host or device tensors anywhere else."""
    vertices: torch.Tensor                   # [V, 3] fp32
    normals: torch.Tensor                    # [V, 3] fp32, unit length or (0, 0, 0)
    faces: torch.Tensor                      # [F, 3] int32
    colours: Optional[torch.Tensor] = None   # [V, 3] fp32 in [0, 1] (colour_vertices) or uint8; None: written as grey

    def write_ply(self, path: str) -> None:
        """Binary little-endian PLY: x y z nx ny nz red green blue per vertex, a `uchar int` index list per face."""
        v = self.vertices.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
        n = self.normals.detach().cpu().numpy().astype("<f4").reshape(-1, 3)
        f = self.faces.detach().cpu().numpy().astype("<i4").reshape(-1, 3)
        if self.colours is None:
            c = np.full((v.shape[0], 3), 128, np.uint8)
        else:
            c = self.colours.detach().cpu()
            if c.dtype != torch.uint8:  # as visualization.rgb_image quantises: x 255, clamped, truncated; NaN -> 0
                c = torch.nan_to_num(c.float() * 255.0, nan=0.0).clamp(0, 255).to(torch.uint8)
            c = c.numpy().reshape(-1, 3)
        if n.shape != v.shape or c.shape != v.shape:
            raise ValueError("normals and colours hold one row per vertex")
        vert = np.zeros(v.shape[0], _PLY_VERTEX)
        vert["p"], vert["n"], vert["c"] = v, n, c
        face = np.zeros(f.shape[0], _PLY_FACE)
        face["k"], face["v"] = 3, f
        with open(path, "wb") as fh:
            fh.write(_PLY_HEADER.format(V=v.shape[0], F=f.shape[0]).encode("ascii"))
            fh.write(vert.tobytes())
            fh.write(face.tobytes())


def read_ply(path: str) -> Mesh:
    """A file Mesh.write_ply wrote, back as host tensors (colours uint8).  Not a general PLY reader: another header raises."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError(f"{path}: no PLY header")
    head = data[:end + 11].decode("ascii")
    try:
        lines = head.split("\n")
        V, F = int(lines[2].split()[2]), int(lines[12].split()[2])
    except (IndexError, ValueError):
        raise ValueError(f"{path}: not a header Mesh.write_ply writes") from None
    if head != _PLY_HEADER.format(V=V, F=F):
        raise ValueError(f"{path}: not a header Mesh.write_ply writes")
    body = data[end + 11:]
    if len(body) != V * _PLY_VERTEX.itemsize + F * _PLY_FACE.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes of data for {V} vertices and {F} faces")
    vert = np.frombuffer(body, _PLY_VERTEX, V)
    face = np.frombuffer(body, _PLY_FACE, F, offset=V * _PLY_VERTEX.itemsize)
    if F and not (face["k"] == 3).all():
        raise ValueError(f"{path}: a face that is not a triangle")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).reshape(-1, 3)
    return Mesh(t(vert["p"], np.float32), t(vert["n"], np.float32), t(face["v"], np.int32), t(vert["c"], np.uint8))


# ---- camera bounds (host code) --------------------------------------------------------------------------------------------------

def bounds_from_cameras(system, margin: float, poses=None):
    """((x0, y0, z0), (x1, y1, z1)): the box round the refined training camera centres and the points at `far` on their optical
    axes (a camera looks down its -z axis: centre - far * R[:, 2]), grown by `margin` on every side.

    `far` per image is the dataset's `fars` where it has them, hparams["nerf.far"] otherwise.  poses: [N, 3, 4] refined
    camera-to-world poses to use instead of refining the dataset's with the trained se(3) rows (which runs the HIP pose kernel)."""
    if poses is None:
        poses = refined_training_poses(system, otherwise="pass bounds yourself")
    c2w = np.asarray(torch.as_tensor(poses).detach().cpu(), dtype=np.float64).reshape(-1, 3, 4)
    fars = [plane(system, "far", i) for i in range(c2w.shape[0])]
    centre = c2w[:, :, 3]
    ahead = centre - np.asarray(fars)[:, None] * c2w[:, :, 2]
    pts = np.concatenate([centre, ahead])
    if not np.isfinite(pts).all():
        raise ValueError("a camera pose or far plane is not finite")
    m = float(margin)
    return tuple(float(v) - m for v in pts.min(0)), tuple(float(v) + m for v in pts.max(0))


# ---- density on a grid ---------------------------------------------------------------------------------------------------------

def grid_columns(bounds, resolution: Sequence[int], col0: int, count: int, S: Optional[int] = None, device="cuda"):
    """(o [count, 3], d [count, 3], z [count, S]) of grid columns [col0, col0 + count) (upnerf_grid_columns): column y * Nx + x
    is the ray o = (x, y, 0), d = (0, 0, 1) whose depths are the z coordinates, the last one repeated up to S >= Nz."""
    lo, hi = box(bounds)
    Nx, Ny, Nz = (int(n) for n in resolution)
    S = max(Nz, MIN_SAMPLES) if S is None else int(S)
    dev = torch.device(device)
    require_cuda("grid_columns", dev)
    o = torch.empty(count, 3, device=dev, dtype=torch.float32)
    d = torch.empty(count, 3, device=dev, dtype=torch.float32)
    z = torch.empty(count, S, device=dev, dtype=torch.float32)
    a = _lib.GridColumnsArgs(Nx=Nx, Ny=Ny, Nz=Nz, S=S, lo=c_float3(lo), hi=c_float3(hi), col0=int(col0),
                             count=int(count), o=ptr(o), d=ptr(d), z=ptr(z))
    check(lib.upnerf_grid_columns(C.byref(a), stream()), "upnerf_grid_columns")
    return o, d, z


def _field_sigma(model, o: torch.Tensor, d: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """sigma_s [R, S] of `model` at o + d z: the density-only forward pass of rendering._FieldPass (mode 2, nothing stored for
    a backward pass) in the kernel family of the global field mode, without the compositing that follows it there."""
    from . import rendering as rd
    pk, L = model.packer, model.packer.L
    R, S = z.shape
    M, dev, st = R * S, z.device, stream()
    P = model.packed().detach().contiguous()
    plan = rd._plan(pk, R, S)  # density only, no gradient: the tiling, and with it the rows x0 is allocated with
    PF, P16, _, wexp, wnorm = rd._weights(pk, P, plan)
    progress = model.host_progress_value()
    sigma = torch.empty(R, S, device=dev, dtype=torch.float32)
    x0 = torch.empty(plan.Mp, _lib.X0, device=dev, dtype=torch.float32)
    fa = _lib.FieldFwdArgs(R=R, S=S, use_cand=0, use_rgb=0, rays_o=ptr(o), rays_d=ptr(d), z=ptr(z),
                           wk_xyz=(C.c_float * 10)(*rd.band_weights(model.xyz_L, progress, model.c2f)), P=ptr(PF),
                           sigma_s=ptr(sigma), x0=ptr(x0), P16=ptr(P16), wexp=ptr(wexp), planes=plan.planes,
                           tile_rows=plan.tile_rows, wnorm=ptr(wnorm), rows_capacity=plan.rows_capacity)
    fn = lib.upnerf_field_fwd_f16x3 if plan.use16 else lib.upnerf_field_fwd
    check(TIMER.run("density_grid", lambda: fn(C.byref(L), C.byref(fa), st), units=M), "upnerf_field_fwd")
    return sigma


@torch.no_grad()
def density_grid(system, bounds, resolution: Sequence[int], field: str = "fine", chunk: Optional[int] = None) -> torch.Tensor:
    """[Nz, Ny, Nx] fp32 device tensor: the shared density (sigma_s, after the softplus) of the `field` ("fine" or "coarse")
    network at the Nx x Ny x Nz grid points of `bounds`, with the BARF band weights of the model's current progress.

    The grid is evaluated as rays, one per (x, y) column (grid_columns), `chunk` columns at a time (default: about a million
    samples), so device memory is the chunk's workspace and the result whatever the resolution.  The values do not depend on
    `chunk`.  Columns shorter than the field kernels' 32 samples are padded and the padding dropped."""
    model, dev = field_of(system, field, "density_grid")
    lo, hi = box(bounds)
    Nx, Ny, Nz = (int(n) for n in resolution)
    if min(Nx, Ny, Nz) < 1:
        raise ValueError(f"resolution is the number of grid points per axis, got {tuple(resolution)}")
    S = max(Nz, MIN_SAMPLES)
    cols = Nx * Ny
    chunk = int(chunk) if chunk is not None else max(1, (1 << 20) // S)
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    chunk = min(chunk, cols)
    out = torch.empty(Nz, cols, device=dev, dtype=torch.float32)
    for c0 in range(0, cols, chunk):
        n = min(chunk, cols - c0)
        o, d, z = grid_columns((lo, hi), (Nx, Ny, Nz), c0, n, S, device=dev)
        sigma = _field_sigma(model, o, d, z)
        out[:, c0:c0 + n].copy_(sigma[:, :Nz].t())  # (a strided copy: column-major samples into the [z][y][x] grid)
    return out.view(Nz, Ny, Nx)


# ---- iso-surface ---------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def extract_surface(grid: torch.Tensor, bounds, level: float, observed_only: bool = False) -> Mesh:
    """The surface `grid == level` of a [Nz, Ny, Nx] fp32 device tensor over `bounds` as a Mesh on the device: marching
    tetrahedra (csrc/mesh.hip), inside = finite and >= level, normals = -gradient (towards lower values), faces wound to match.
    Vertices come in (grid point, edge slot) order and faces in (cell, tetrahedron, triangle) order: the same grid gives the
    same mesh, bit for bit.  `level` has no default: the useful threshold depends on the scene's scale.

    observed_only: a non-finite sample means "nobody looked here", not "outside" (UPNERF_MTET_SKIP_NONFINITE): an edge is
    crossed only between two finite samples and a tetrahedron is triangulated only if its four corners are finite, so no wall
    is built where observed samples meet unobserved ones (TsdfVolume.extract).  A vertex may remain that no face uses."""
    require_cuda("extract_surface", grid)
    if grid.dtype != torch.float32 or grid.dim() != 3:
        raise ValueError("the grid is a fp32 tensor [Nz, Ny, Nx]")
    lo, hi = box(bounds)
    grid = grid.detach().contiguous()
    Nz, Ny, Nx = grid.shape
    dev, st = grid.device, stream()
    nbytes = lib.upnerf_mtet_scratch(Nx, Ny, Nz)
    if nbytes < 0:
        check(int(nbytes), f"upnerf_mtet_scratch({Nx}, {Ny}, {Nz})")
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    totals = torch.empty(2, device=dev, dtype=torch.int32)
    a = _lib.MtetArgs(Nx=Nx, Ny=Ny, Nz=Nz, level=float(level), lo=c_float3(lo), hi=c_float3(hi), grid=ptr(grid),
                      tab=_tables(), flags=_lib.MTET_SKIP_NONFINITE if observed_only else 0)
    check(TIMER.run("mtet_count", lambda: lib.upnerf_mtet_count(C.byref(a), ptr(scratch), ptr(totals), st), units=grid.numel()),
          "upnerf_mtet_count")
    V, F = (int(x) for x in totals.cpu())  # the one host read: the mesh is allocated exactly
    vertices = torch.empty(V, 3, device=dev, dtype=torch.float32)
    normals = torch.empty(V, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
    a.n_vertices = a.cap_vertices = V
    a.n_faces = a.cap_faces = F
    a.vertices, a.normals, a.faces = ptr(vertices), ptr(normals), ptr(faces)
    check(TIMER.run("mtet_emit", lambda: lib.upnerf_mtet_emit(C.byref(a), ptr(scratch), st), units=grid.numel()), "upnerf_mtet_emit")
    return Mesh(vertices, normals, faces)


@torch.no_grad()
def refine_normals(system, mesh: Mesh, field: str = "fine") -> Mesh:
    """`mesh` with its vertex normals replaced by the field's own: -grad sigma / |grad sigma| at the vertices
    (normals.density_gradient, upnerf_density_grad) instead of the central differences of the sampled grid, which are off by the
    grid spacing where the surface is thin.  Vertices, faces and colours are the same tensors; a vertex whose analytic gradient
    is zero or not finite keeps its grid normal."""
    from . import normals as nm
    _, g = nm.density_gradient(system, mesh.vertices, field=field)
    length = g.norm(dim=1, keepdim=True)
    ok = torch.isfinite(length) & (length > 0)
    n = torch.where(ok, -g / torch.where(ok, length, torch.ones_like(length)), mesh.normals.to(g.dtype))
    return Mesh(mesh.vertices, n.contiguous(), mesh.faces, mesh.colours)


# ---- vertex colours ------------------------------------------------------------------------------------------------------------

def vertex_rays(mesh: Mesh, slab: float) -> torch.Tensor:
    """[V, 8] ray rows (o | d | near | far) through the surface at every vertex: o = p + slab * n, d = -n, near = 0,
    far = 2 * slab; a vertex without a normal looks along d = (0, 0, 1)."""
    p, n = mesh.vertices, mesh.normals
    slab = float(slab)
    if not slab > 0:
        raise ValueError(f"slab must be positive, got {slab}")
    flat = (n == 0).all(dim=1, keepdim=True)
    d = torch.where(flat, torch.tensor([0.0, 0.0, 1.0], device=p.device), -n)
    o = p + slab * n
    nf = torch.tensor([0.0, 2.0 * slab], device=p.device).expand(p.shape[0], 2)
    return torch.cat([o, d, nf], 1).contiguous()


@torch.no_grad()
def colour_vertices(system, mesh: Mesh, img_id: int, slab: float, chunk: Optional[int] = None) -> torch.Tensor:
    """[V, 3] fp32 static colour (`s_rgb_fine`; `s_rgb_coarse` without a fine field) of every vertex, rendered by the public
    render_rays along vertex_rays(mesh, slab) at sched_mult = 1 with the appearance row of training image `img_id` (passed as
    `embed_rows`, as novel_view.render_path does), `chunk` rays at a time (default val.chunk_size)."""
    dev = next(system.parameters()).device
    require_cuda("colour_vertices", dev, mesh.vertices)
    typ = "fine" if system.fine else "coarse"
    rays = vertex_rays(mesh, slab)
    V = rays.shape[0]
    out = torch.empty(V, 3, device=dev, dtype=torch.float32)
    chunk = int(chunk or system.hparams["val.chunk_size"])
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    # No check of the system's own schedule, unlike render_path and fuse_views: the colour head is asked for at sched_mult = 1
    # whatever the checkpoint's progress, so an early checkpoint colours its mesh (with what that head has learnt so far).
    rows = appearance_rows(system, static_keys(system, 1), img_id, min(chunk, max(V, 1)))
    for r0 in range(0, V, chunk):
        R = min(chunk, V - r0)
        res = render_static(system, rays[r0:r0 + R], {k: v[:R] for k, v in rows.items()}, 1)
        out[r0:r0 + R].copy_(res[f"s_rgb_{typ}"])
    return out


# ---- depth-map fusion: a truncated signed distance volume ------------------------------------------------------------------------

WEIGHT_MODES = {"count": 0, "opacity": 1}


def _per_view(x, n, what):
    """`x` for each of n views: a list whose entries are arrays or sequences themselves holds one entry per view; anything else
    (one K as a tensor, an array or (fx, fy, cx, cy); one (W, H)) is shared by all."""
    if isinstance(x, (list, tuple)) and len(x) and (torch.is_tensor(x[0]) or isinstance(x[0], (np.ndarray, list, tuple))):
        if len(x) != n:
            raise ValueError(f"{what}: {len(x)} entries for {n} views")
        return list(x)
    return [x] * n


class TsdfVolume:
    """A truncated signed distance volume on the Nx x Ny x Nz grid points of `bounds` (the grid extract_surface meshes), on the
    device: `tsdf` [Nz, Ny, Nx] (the running mean of min(1, sdf / trunc); 1 where nothing was seen), `weight` (the summed view
    weights, 0 = never observed) and, with colour=True, `rgb` [Nz, Ny, Nx, 3] with `rgb_weight`, a weight volume of the colour's
    own (colour is fused only within `trunc` of the observed surface).  The arithmetic is defined in include/upnerf_hip.h
    (upnerf_tsdf_integrate); there is no CPU path."""

    def __init__(self, bounds, resolution: Sequence[int], trunc: float, colour: bool = True, device="cuda"):
        dev = torch.device(device)
        require_cuda("TsdfVolume", dev)
        self.bounds = box(bounds)
        Nx, Ny, Nz = (int(n) for n in resolution)
        if min(Nx, Ny, Nz) < 2:
            raise ValueError(f"resolution is the number of grid points per axis (two at least), got {tuple(resolution)}")
        self.resolution = (Nx, Ny, Nz)
        self.trunc = float(trunc)
        if not (self.trunc > 0 and np.isfinite(self.trunc)):
            raise ValueError(f"trunc must be positive and finite, got {trunc}")
        self.tsdf = torch.ones(Nz, Ny, Nx, device=dev, dtype=torch.float32)
        self.weight = torch.zeros(Nz, Ny, Nx, device=dev, dtype=torch.float32)
        self.rgb = torch.zeros(Nz, Ny, Nx, 3, device=dev, dtype=torch.float32) if colour else None
        self.rgb_weight = torch.zeros(Nz, Ny, Nx, device=dev, dtype=torch.float32) if colour else None
        self.n_views = 0

    @torch.no_grad()
    def integrate(self, depth, c2w, K, img_wh, rgb=None, opacity=None, min_opacity: float = 0.5, weight_mode: str = "count") -> None:
        """Fold one view or a list of views into the volume, in order, _lib.TSDF_MAX_VIEWS per launch (the result does not
        depend on how the list is cut).  depth: [H * W] (or [H, W]) fp32 device tensor of distances along unit rays, or a list
        of them; c2w: [3, 4] or [n, 3, 4] (or a list); K: 3 x 3 or (fx, fy, cx, cy), img_wh = (W, H): one for all views or a
        list; rgb [H * W, 3] and opacity [H * W] per view, optional.  A pixel whose opacity is below `min_opacity` is not a
        measurement; weight_mode "count": a view counts 1, "opacity": its pixel's opacity (needs the maps)."""
        if weight_mode not in WEIGHT_MODES:
            raise ValueError(f"weight_mode is one of {tuple(WEIGHT_MODES)}, got {weight_mode!r}")
        depths = list(depth) if isinstance(depth, (list, tuple)) else [depth]
        n = len(depths)
        if n < 1:
            raise ValueError("no view to integrate")
        poses = torch.as_tensor(c2w) if not isinstance(c2w, (list, tuple)) else torch.stack([torch.as_tensor(p) for p in c2w])
        poses = poses.detach().to(dtype=torch.float32).cpu().reshape(-1, 3, 4)
        if poses.shape[0] != n:
            raise ValueError(f"c2w: {poses.shape[0]} poses for {n} views")
        Ks, whs = _per_view(K, n, "K"), _per_view(img_wh, n, "img_wh")
        rgbs = list(rgb) if isinstance(rgb, (list, tuple)) else [rgb] * n
        ops = list(opacity) if isinstance(opacity, (list, tuple)) else [opacity] * n
        if len(rgbs) != n or len(ops) != n:
            raise ValueError("rgb and opacity hold one map per view")
        dev = self.tsdf.device
        views, keep = [], []
        for i in range(n):
            W, H = int(whs[i][0]), int(whs[i][1])
            maps = []
            for name, t, width in (("depth", depths[i], 1), ("opacity", ops[i], 1), ("rgb", rgbs[i], 3)):
                if t is None:
                    maps.append(None)
                    continue
                require_cuda(f"TsdfVolume.integrate: {name}", t)
                if t.dtype != torch.float32 or t.numel() != H * W * width or t.device != dev:
                    raise ValueError(f"{name} of view {i} is a fp32 tensor of {H} x {W}{' x 3' if width == 3 else ''} values on {dev}")
                maps.append(t.detach().contiguous())
            keep.append(maps)
            fx, fy, cx, cy = intrinsics(Ks[i])
            views.append(_lib.TsdfView(c2w=(C.c_float * 12)(*poses[i].reshape(-1).tolist()), fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H,
                                       depth=ptr(maps[0]), opacity=ptr(maps[1]), rgb=ptr(maps[2])))
        Nx, Ny, Nz = self.resolution
        lo, hi = self.bounds
        for v0 in range(0, n, _lib.TSDF_MAX_VIEWS):
            batch = views[v0:v0 + _lib.TSDF_MAX_VIEWS]
            a = _lib.TsdfIntegrateArgs(Nx=Nx, Ny=Ny, Nz=Nz, n_views=len(batch), lo=c_float3(lo), hi=c_float3(hi),
                                       trunc=self.trunc, min_opacity=float(min_opacity), weight_mode=WEIGHT_MODES[weight_mode],
                                       tsdf=ptr(self.tsdf), weight=ptr(self.weight), rgb=ptr(self.rgb), rgb_weight=ptr(self.rgb_weight))
            for j, v in enumerate(batch):
                a.views[j] = v
            check(TIMER.run("tsdf_integrate", lambda: lib.upnerf_tsdf_integrate(C.byref(a), stream()), units=self.tsdf.numel()),
                  "upnerf_tsdf_integrate")
        self.n_views += n

    @torch.no_grad()
    def surface_grid(self, min_weight: float = 1.0) -> torch.Tensor:
        """[Nz, Ny, Nx]: -tsdf where weight >= min_weight (positive behind the surface), NaN where too few views looked: what
        extract_surface(..., 0.0, observed_only=True) meshes (upnerf_tsdf_surface)."""
        out = torch.empty_like(self.tsdf)
        a = _lib.TsdfSurfaceArgs(n=self.tsdf.numel(), min_weight=float(min_weight), tsdf=ptr(self.tsdf), weight=ptr(self.weight),
                                 out=ptr(out))
        check(lib.upnerf_tsdf_surface(C.byref(a), stream()), "upnerf_tsdf_surface")
        return out

    @torch.no_grad()
    def sample_colour(self, points: torch.Tensor) -> torch.Tensor:
        """[V, 3] fused colour at `points` [V, 3]: trilinear over the corners that have a colour, mid-grey where none has
        (upnerf_tsdf_sample)."""
        if self.rgb is None:
            raise ValueError("this volume was built with colour=False")
        require_cuda("TsdfVolume.sample_colour", points)
        pts = points.detach().to(torch.float32).reshape(-1, 3).contiguous()
        V = pts.shape[0]
        out = torch.empty(V, 3, device=pts.device, dtype=torch.float32)
        if V == 0:
            return out
        Nx, Ny, Nz = self.resolution
        lo, hi = self.bounds
        a = _lib.TsdfSampleArgs(Nx=Nx, Ny=Ny, Nz=Nz, V=V, lo=c_float3(lo), hi=c_float3(hi), rgb=ptr(self.rgb),
                                rgb_weight=ptr(self.rgb_weight), points=ptr(pts), out=ptr(out))
        check(lib.upnerf_tsdf_sample(C.byref(a), stream()), "upnerf_tsdf_sample")
        return out

    def extract(self, min_weight: float = 1.0) -> Mesh:
        """The zero level of the fused distance as a Mesh: surface_grid, then extract_surface(..., 0.0, observed_only=True), so
        the normals point at the cameras and nothing is built where no view looked; colours from the fused colour volume."""
        mesh = extract_surface(self.surface_grid(min_weight), self.bounds, 0.0, observed_only=True)
        if self.rgb is not None:
            mesh.colours = self.sample_colour(mesh.vertices)
        return mesh


@torch.no_grad()
def fuse_views(system, bounds, resolution: Sequence[int], img_ids: Optional[Sequence[int]] = None, trunc: Optional[float] = None,
               downscale: int = 1, chunk: Optional[int] = None, min_opacity: float = 0.5) -> TsdfVolume:
    """A TsdfVolume of the scene as its training cameras see it.  For every training image of `img_ids` (default: all): the
    refined pose (as bounds_from_cameras obtains it), the rays of the whole frame at 1 / `downscale` of its size
    (novel_view.path_rays, the dataset's Ks, all_imgs_wh, nears and fars), rendered by the public render_rays as
    colour_vertices renders (sched_mult = 1, validation's sample counts, the image's own appearance row as `embed_rows`),
    `chunk` rays at a time (default val.chunk_size); depth = `s_depth_*`, colour = `s_rgb_*`, opacity = the row sum of
    `s_weights_*`; then TsdfVolume.integrate, a launch per TSDF_MAX_VIEWS views.  trunc: default 3 voxel diagonals.
    Raises while the candidate schedule has not started (sched_mult == 0), as render_path does."""
    hp, ds = system.hparams, system.train_dataset
    if system.get_schedule_mult(system._host_progress) == 0:  # (here, not in render_static: the text names the maps THIS function cannot give yet)
        raise ValueError("fuse_views renders the static depth and colour s_depth_* / s_rgb_*, which do not exist while the "
                         "candidate schedule has not started (sched_mult == 0): this checkpoint is too early in training")
    dev = next(system.parameters()).device
    require_cuda("fuse_views", dev)
    lo, hi = box(bounds)
    res = tuple(int(n) for n in resolution)
    if trunc is None:
        trunc = 3.0 * sum(((h - l) / max(n - 1, 1)) ** 2 for l, h, n in zip(lo, hi, res)) ** 0.5
    downscale, chunk = int(downscale), int(chunk or hp["val.chunk_size"])
    if downscale < 1 or chunk < 1:
        raise ValueError("downscale and chunk are positive")
    poses = refined_training_poses(system, otherwise="integrate views of your own into a TsdfVolume").to(dev)
    N = poses.shape[0]
    ids = list(range(N)) if img_ids is None else [int(i) for i in img_ids]
    if not ids or min(ids) < 0 or max(ids) >= N:
        raise ValueError(f"img_ids must be training image indices in [0, {N})")
    if getattr(ds, "Ks", None) is None or getattr(ds, "all_imgs_wh", None) is None:
        raise ValueError("the dataset carries no intrinsics / image sizes (Ks, all_imgs_wh)")
    typ = "fine" if system.fine else "coarse"
    keys = static_keys(system, 1)
    vol = TsdfVolume((lo, hi), res, trunc, colour=True, device=dev)
    pending = []  # (depth, rgb, opacity, pose, K, wh) of the views rendered and not yet folded in

    def flush():
        if pending:
            d, c, o, p, k, wh = zip(*pending)
            vol.integrate(list(d), torch.stack(p), list(k), list(wh), rgb=list(c), opacity=list(o), min_opacity=min_opacity)
            pending.clear()

    for i in ids:
        W, H = (int(x) // downscale for x in ds.all_imgs_wh[i])
        if min(W, H) < 1:
            raise ValueError(f"image {i} has no pixel left at downscale {downscale}")
        intr = tuple(v / downscale for v in intrinsics(per_image(ds, "Ks", i)))
        nf = torch.tensor([near_far(system, i)], device=dev, dtype=torch.float32)
        c2w = poses[i:i + 1].contiguous()
        n = W * H
        depth = torch.empty(n, device=dev, dtype=torch.float32)
        rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
        opacity = torch.empty(n, device=dev, dtype=torch.float32)
        rows = appearance_rows(system, keys, i, min(chunk, n))
        for r0 in range(0, n, chunk):
            R = min(chunk, n - r0)
            rays, _ = path_rays(c2w, nf, (W, H), intr, r0, R)
            out = render_static(system, rays, {k: v[:R] for k, v in rows.items()}, 1)
            depth[r0:r0 + R].copy_(out[f"s_depth_{typ}"])
            rgb[r0:r0 + R].copy_(out[f"s_rgb_{typ}"])
            opacity[r0:r0 + R].copy_(out[f"s_weights_{typ}"].reshape(R, -1).sum(1))
        pending.append((depth, rgb, opacity, poses[i], intr, (W, H)))
        if len(pending) == _lib.TSDF_MAX_VIEWS:  # (device memory: the maps of one launch's views, not of the whole scene)
            flush()
    flush()
    return vol
