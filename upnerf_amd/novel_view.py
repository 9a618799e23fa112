"""Novel views along a camera path: frames from cameras that are not in the dataset, the static scene only (TransientNet is
not evaluated), the appearance embedding moving smoothly between photographs.

    path = CameraPath.through_images(system, [3, 17, 42], n_frames=120)
    out = render_path(system, path, outputs=("rgb", "depth"), sink=ImageWriter("frames"))

The front end is two HIP kernels (csrc/path.hip): `upnerf_path_poses` turns keyframe poses into one pose per
frame (quaternion slerp, linear or Catmull-Rom translation, fp64 rounded once), `upnerf_path_rays` writes, chunk by chunk,
the [R][8] ray rows of the virtual [F][H][W] pixel list and the per-ray embedding rows as blends of two table rows.  The
rows go to `render_rays` through its `embed_rows` keyword; the pictures are built by the kernels of `visualization`.
There is no CPU path.  `plan_path` (which frame sits where, which two images it blends) is plain host arithmetic."""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream
from .ops import TIMER
from .static_scene import intrinsics, near_far, per_image, refined_training_poses, render_static, require_cuda, static_keys

__all__ = ["CameraPath", "plan_path", "path_poses", "path_rays", "render_path", "MODES"]

MODES = {"linear": _lib.PATH_LINEAR, "catmull": _lib.PATH_CATMULL}
LAST_WORKSPACE: Dict[str, tuple] = {}  # shapes of the per-chunk buffers the last render_path allocated (tests)
LAST_STATS: Dict[str, int] = {}  # rays and hits of the last render_path with an occupancy grid (empty without one)


def plan_path(n_frames: int, img_ids: Optional[Sequence[int]] = None, loop: bool = False, n_keys: Optional[int] = None,
              appearance: Optional[Tuple[int, int]] = None):
    """(u fp32 [F], i0 int32 [F], i1 int32 [F], t fp32 [F]) of a path with F = n_frames frames.

    u: the frames' path parameters, evenly spaced over [0, K - 1] with both ends (one frame: u = [0]).
    img_ids (the keyframes are images; `loop` appends the first one at the end, K = len(img_ids) [+ 1]): the appearance
    follows the path -- with k = floor(u), s = u - k a frame blends image id[k] into id[k + 1] by t = s; on a keyframe
    (integer u, the last one included) t = 0 and i0 is that keyframe's image.
    appearance = (id0, id1) (free keyframe poses, K = n_keys): one blend from id0 to id1 over the whole path, t rising
    linearly from 0 to 1 (one frame: t = 0).  (id, id) is a fixed appearance."""
    if n_frames < 1:
        raise ValueError(f"a path has at least one frame, got n_frames={n_frames}")
    if (img_ids is None) == (appearance is None):
        raise ValueError("give either img_ids (appearance follows the keyframes) or appearance=(id0, id1)")
    if img_ids is not None:
        ids = [int(i) for i in img_ids]
        if loop:
            ids = ids + ids[:1]
        if n_keys is not None and n_keys != len(ids):
            raise ValueError(f"n_keys={n_keys} but img_ids gives {len(ids)} keyframes")
        K = len(ids)
    else:
        if n_keys is None:
            raise ValueError("appearance=(id0, id1) needs n_keys")
        K = int(n_keys)
    if K < 2:
        raise ValueError(f"a path needs at least two keyframes, got {K}")
    u = np.linspace(0.0, K - 1.0, n_frames, dtype=np.float64).astype(np.float32) if n_frames > 1 else np.zeros(1, np.float32)
    u[-1] = K - 1.0 if n_frames > 1 else 0.0
    if img_ids is not None:
        k = np.minimum(np.floor(u).astype(np.int64), K - 1)
        t = (u.astype(np.float64) - k).astype(np.float32)  # exact: removing the integer part of a fp32 number
        idv = np.asarray(ids, dtype=np.int32)
        i0, i1 = idv[k], idv[np.minimum(k + 1, K - 1)]
    else:
        t = np.linspace(0.0, 1.0, n_frames, dtype=np.float64).astype(np.float32) if n_frames > 1 else np.zeros(1, np.float32)
        i0 = np.full(n_frames, int(appearance[0]), dtype=np.int32)
        i1 = np.full(n_frames, int(appearance[1]), dtype=np.int32)
    return (torch.from_numpy(u), torch.from_numpy(np.ascontiguousarray(i0)), torch.from_numpy(np.ascontiguousarray(i1)),
            torch.from_numpy(t))


@dataclass
class CameraPath:
    """Keyframes and the per-frame plan of a rendered sequence, all host tensors (render_path uploads them once)."""
    key_c2w: torch.Tensor        # [K, 3, 4] fp32
    key_near_far: torch.Tensor   # [K, 2] fp32
    u: torch.Tensor              # [F] fp32 in [0, K - 1]
    i0: torch.Tensor             # [F] int32, rows of the embedding tables
    i1: torch.Tensor             # [F] int32
    t: torch.Tensor              # [F] fp32 blend weight of i1
    img_wh: Tuple[int, int]      # (W, H)
    K: torch.Tensor              # [3, 3] intrinsics
    mode: str = "catmull"        # translation between keyframes: "linear" or "catmull"

    def __post_init__(self):
        if self.mode not in MODES:
            raise ValueError(f"mode is one of {tuple(MODES)}, got {self.mode!r}")
        self.key_c2w = torch.as_tensor(self.key_c2w, dtype=torch.float32).cpu().reshape(-1, 3, 4).contiguous()
        self.key_near_far = torch.as_tensor(self.key_near_far, dtype=torch.float32).cpu().reshape(-1, 2).contiguous()
        if self.key_c2w.shape[0] < 2 or self.key_near_far.shape[0] != self.key_c2w.shape[0]:
            raise ValueError("a path needs K >= 2 keyframe poses [K, 3, 4] and as many (near, far) pairs")
        self.u = torch.as_tensor(self.u, dtype=torch.float32).cpu().reshape(-1).contiguous()
        self.i0 = torch.as_tensor(self.i0).to(torch.int32).cpu().reshape(-1).contiguous()
        self.i1 = torch.as_tensor(self.i1).to(torch.int32).cpu().reshape(-1).contiguous()
        self.t = torch.as_tensor(self.t, dtype=torch.float32).cpu().reshape(-1).contiguous()
        F = self.u.numel()
        if F < 1 or not (self.i0.numel() == self.i1.numel() == self.t.numel() == F):
            raise ValueError("u, i0, i1 and t hold one entry per frame")
        self.img_wh = (int(self.img_wh[0]), int(self.img_wh[1]))
        if min(self.img_wh) < 1:
            raise ValueError(f"img_wh = (W, H) with W, H >= 1, got {self.img_wh}")
        self.K = torch.as_tensor(np.asarray(self.K), dtype=torch.float32).cpu().reshape(3, 3)

    @property
    def n_frames(self) -> int:
        return self.u.numel()

    @classmethod
    def through_images(cls, system, img_ids: Sequence[int], n_frames: int, mode: str = "catmull", img_wh=None, K=None,
                       loop: bool = False) -> "CameraPath":
        """A path through training images `img_ids` (indices of the training set: the rows of the per-image tables).
        Keyframes are the REFINED training poses (pose_align.refined_poses of the trained se(3) rows and the dataset's
        poses), near / far the dataset's `nears` / `fars` (hparams nerf.near / nerf.far where it has none); the appearance
        follows the path (plan_path).  `K` and `img_wh` default to those of the first keyframe image."""
        ids = [int(i) for i in img_ids]
        ds, N = system.train_dataset, system.se3_refine.weight.shape[0]
        if not ids or min(ids) < 0 or max(ids) >= N:
            raise ValueError(f"img_ids must be training image indices in [0, {N})")
        keys = refined_training_poses(system, ids, "use CameraPath.from_poses").cpu()
        nf = torch.tensor([near_far(system, i) for i in ids], dtype=torch.float32)
        if loop:
            keys, nf = torch.cat([keys, keys[:1]]), torch.cat([nf, nf[:1]])
        if K is None:
            K = per_image(ds, "Ks", ids[0])
        if img_wh is None:
            wh = getattr(ds, "all_imgs_wh", None)
            img_wh = None if wh is None else tuple(int(x) for x in wh[ids[0]])
        if K is None or img_wh is None:
            raise ValueError("the dataset carries no intrinsics / image sizes (Ks, all_imgs_wh): pass K and img_wh")
        u, i0, i1, t = plan_path(n_frames, img_ids=ids, loop=loop)
        return cls(keys, nf, u, i0, i1, t, img_wh, K, mode)

    @classmethod
    def from_poses(cls, c2w, near_far, n_frames: int, appearance: Tuple[int, int], img_wh, K, mode: str = "catmull") -> "CameraPath":
        """A path through arbitrary keyframe poses `c2w` [K, 3, 4] with `near_far` [K, 2] (or one pair for all): one
        appearance blend from image appearance[0] to appearance[1] over the whole path."""
        c2w = torch.as_tensor(c2w, dtype=torch.float32).cpu().reshape(-1, 3, 4)
        nf = torch.as_tensor(near_far, dtype=torch.float32).cpu().reshape(-1, 2)
        if nf.shape[0] == 1:
            nf = nf.expand(c2w.shape[0], 2)
        u, i0, i1, t = plan_path(n_frames, n_keys=c2w.shape[0], appearance=appearance)
        return cls(c2w, nf, u, i0, i1, t, img_wh, K, mode)


def _dev32(x: torch.Tensor, device, dtype=torch.float32) -> torch.Tensor:
    return torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()


def path_poses(key_c2w: torch.Tensor, key_nf: torch.Tensor, u: torch.Tensor, mode="catmull"):
    """(c2w [F, 3, 4], near_far [F, 2]) at path parameters `u` [F] between the keyframes (upnerf_path_poses; device tensors)."""
    require_cuda("path_poses", key_c2w)
    dev = key_c2w.device
    key_c2w, key_nf, u = _dev32(key_c2w, dev).reshape(-1, 3, 4), _dev32(key_nf, dev).reshape(-1, 2), _dev32(u, dev).reshape(-1)
    K, F = key_c2w.shape[0], u.numel()
    if key_nf.shape[0] != K:
        raise ValueError("one (near, far) pair per keyframe")
    c2w = torch.empty(F, 3, 4, device=dev, dtype=torch.float32)
    nf = torch.empty(F, 2, device=dev, dtype=torch.float32)
    a = _lib.PathPosesArgs(K=K, F=F, mode=MODES[mode] if isinstance(mode, str) else int(mode), key_c2w=ptr(key_c2w),
                           key_nf=ptr(key_nf), u=ptr(u), c2w=ptr(c2w), nf=ptr(nf))
    check(lib.upnerf_path_poses(C.byref(a), stream()), "upnerf_path_poses")
    return c2w, nf


def path_rays(c2w: torch.Tensor, nf: torch.Tensor, img_wh, K, row0: int, R: int, tables=(), i0=None, i1=None, t=None,
              rays: Optional[torch.Tensor] = None):
    """Rows [row0, row0 + R) of the frames' pixel list (upnerf_path_rays): returns (rays [R, 8], [rows [R, dim] per table]).

    c2w [F, 3, 4], nf [F, 2] device tensors; K = 3 x 3 intrinsics or (fx, fy, cx, cy); tables: (table [N, dim], out or None)
    pairs, blended between rows i0[f] and i1[f] (int32 [F]) with weight t[f] -- indices outside the table are clamped into
    it by the kernel.  `rays` / `out`: preallocated buffers with at least R rows (their first R rows are written)."""
    require_cuda("path_rays", c2w)
    dev = c2w.device
    W, H = int(img_wh[0]), int(img_wh[1])
    fx, fy, cx, cy = intrinsics(K)
    F = c2w.shape[0]
    if rays is None:
        rays = torch.empty(R, 8, device=dev, dtype=torch.float32)
    if rays.shape[0] < R or tuple(rays.shape[1:]) != (8,):
        raise ValueError(f"rays must be [>= {R}, 8]")
    if len(tables) > _lib.PATH_MAX_TABLES:
        raise ValueError(f"at most {_lib.PATH_MAX_TABLES} embedding tables per launch, got {len(tables)}")
    a = _lib.PathRaysArgs(F=F, H=H, W=W, n_tables=len(tables), row0=int(row0), R=int(R), fx=fx, fy=fy, cx=cx, cy=cy,
                          c2w=ptr(c2w), nf=ptr(nf), i0=ptr(i0), i1=ptr(i1), t=ptr(t), rays=ptr(rays))
    outs = []
    for j, (table, out) in enumerate(tables):
        if table.dim() != 2 or (i0 is None or i1 is None or t is None):
            raise ValueError("a table is [N, dim] and needs i0, i1 and t")
        for x, dt in ((i0, torch.int32), (i1, torch.int32), (t, torch.float32)):
            if x.dtype != dt or x.numel() != F:
                raise ValueError("i0, i1 are int32 [F] and t is fp32 [F]")
        dim = table.shape[1]
        if out is None:
            out = torch.empty(R, dim, device=dev, dtype=torch.float32)
        if out.shape[0] < R or tuple(out.shape[1:]) != (dim,):
            raise ValueError(f"the rows of table {j} must be [>= {R}, {dim}]")
        a.tables[j] = _lib.PathTable(table=ptr(table), dim=dim, n_rows=table.shape[0], out=ptr(out))
        outs.append(out[:R])
    check(TIMER.run("path_rays", lambda: lib.upnerf_path_rays(C.byref(a), stream()), units=R), "upnerf_path_rays")
    return rays[:R], outs


@torch.no_grad()
def render_path(system, path: CameraPath, chunk: Optional[int] = None, outputs: Sequence[str] = ("rgb",),
                depth_range: Optional[Tuple[float, float]] = None, sink: Optional[Callable] = None,
                occupancy=None, baked=None, baked_step: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """Render every frame of `path` with the static fields of `system` (perturb = 0, no gradient, validation's sample counts).

    outputs: any of "rgb" (uint8 [F, H, W, 3] of `s_rgb_fine`, `s_rgb_coarse` without a fine field), "depth" (uint8
    [F, H, W, 3], `s_depth_*` through the JET table over ONE range for the whole sequence: `depth_range`, or the min / max of
    frame 0, kept on the device), "rgb_float" (fp32 [F, H * W, 3]), "normal" (uint8 [F, H, W, 3]: the world-space normal map of
    render_rays(normals=True) through visualization.normal_image) and "normal_float" (fp32 [F, H * W, 3], unit length or zero).
    sink: called as sink("path", frame, {"rgb": ..., "depth": ...}) once per finished frame, in order (an `ImageWriter`).
    The pixel list [F][H][W] is walked in chunks of `chunk` rows (default val.chunk_size) that may straddle frames; device
    memory is the chunk's workspace, one frame of staging and the requested outputs.
    occupancy: an `occupancy.OccupancyGrid`.  Every chunk's rays are walked through it (upnerf_occ_spans), the rays that touch an
    occupied cell are compacted with their embedding rows (upnerf_occ_compact) and rendered over [t0, t1] instead of
    [near, far], and the results scattered back (upnerf_occ_scatter); a ray that touches nothing shows the BACKGROUND (1 with
    white_back, else 0) at depth `far` -- not what the full render would have composited from density below the grid's level.
    One host read per chunk (the hit count); a chunk without hits launches no field kernel.  LAST_STATS holds the sequence's
    number of rays and hits.  None: nothing of this runs.
    baked: a `baked.BakedScene`, with `baked_step` (the sample spacing in units of t; no default).  The frames come from
    `baked.render` on the rays upnerf_path_rays makes and the fields are never evaluated: no view dependence unless the scene was
    baked with sh_degree > 0 (its render then evaluates each ray's own direction: nothing to pass here), ONE appearance (the
    one the scene was baked with: the path's blend is not looked at), outputs "rgb", "depth" and "rgb_float" only.  Asking for a
    normal map, or passing `occupancy` as well (the scene carries its own bits), raises ValueError."""
    if baked is not None:
        return _render_path_baked(system, path, chunk, outputs, depth_range, sink, occupancy, baked, baked_step)
    if baked_step is not None:
        raise ValueError("baked_step belongs to baked=")
    from .visualization import depth_image, min_max_of, normal_image, rgb_image
    unknown = set(outputs) - {"rgb", "depth", "rgb_float", "normal", "normal_float"}
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)} (rgb, depth, rgb_float, normal, normal_float)")
    hp = system.hparams
    sched_mult = system.get_schedule_mult(system._host_progress)
    if sched_mult == 0:  # (here, not in render_static: the text names the outputs THIS function cannot give yet)
        raise ValueError("render_path renders the static colour s_rgb_*, which does not exist while the candidate schedule has "
                         "not started (sched_mult == 0): this checkpoint is too early in training")
    dev = next(system.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("render_path runs on the GPU only (no CPU fallback)")
    typ = "fine" if system.fine else "coarse"
    W, H = path.img_wh
    F, n = path.n_frames, W * H
    total = F * n
    chunk = int(chunk or hp["val.chunk_size"])
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    chunk = min(chunk, total)
    c2w, nf = path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode)
    i0, i1, t = path.i0.to(dev), path.i1.to(dev), path.t.to(dev)
    intr = intrinsics(path.K)
    keys = static_keys(system, sched_mult)
    weights = [system.embeddings[k].weight.detach().contiguous() for k in keys]
    # the workspace of every chunk, allocated once: 32 B of rays and sum(dim) * 4 B of rows per ray of the chunk
    ws = {"rays": torch.empty(chunk, 8, device=dev, dtype=torch.float32)}
    for k, w in zip(keys, weights):
        ws[k] = torch.empty(chunk, w.shape[1], device=dev, dtype=torch.float32)
    want_depth = "depth" in outputs
    want_normal = "normal" in outputs or "normal_float" in outputs
    LAST_STATS.clear()
    occ_ws = None
    if occupancy is not None:
        from . import occupancy as oc
        if not isinstance(occupancy, oc.OccupancyGrid) or occupancy.words.device != dev:
            raise ValueError("occupancy is an OccupancyGrid on the system's device")
        occ_ws = oc.compact_workspace(chunk, [w.shape[1] for w in weights], dev)
        occ_ws["rgb"] = torch.empty(chunk, 3, device=dev, dtype=torch.float32)
        if want_depth:
            occ_ws["depth"] = torch.empty(chunk, device=dev, dtype=torch.float32)
        for k, v in occ_ws.items():
            if k == "rows_c":
                ws.update({f"occ_{kk}": r for kk, r in zip(keys, v)})
            else:
                ws[f"occ_{k}"] = v
        LAST_STATS.update(rays=total, hits=0)
    white_back = getattr(system.train_dataset, "white_back", False)
    LAST_WORKSPACE.clear()
    LAST_WORKSPACE.update({k: tuple(v.shape) for k, v in ws.items()})
    stage_rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    stage_depth = torch.empty(n, device=dev, dtype=torch.float32) if want_depth else None
    stage_normal = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_normal else None
    out: Dict[str, torch.Tensor] = {}
    if "rgb" in outputs:
        out["rgb"] = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
    if want_depth:
        out["depth"] = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
    if "rgb_float" in outputs:
        out["rgb_float"] = torch.empty(F, n, 3, device=dev, dtype=torch.float32)
    if "normal" in outputs:
        out["normal"] = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
    if "normal_float" in outputs:
        out["normal_float"] = torch.empty(F, n, 3, device=dev, dtype=torch.float32)
    rng_dev = None  # frame 0's (min, max) depth on the device: one colour scale for the whole sequence

    def finish(f):
        nonlocal rng_dev
        images = {}
        if "rgb_float" in out:
            out["rgb_float"][f].copy_(stage_rgb)
        if "rgb" in out:
            out["rgb"][f].copy_(rgb_image(stage_rgb, (W, H)))
            images["rgb"] = out["rgb"][f]
        if want_depth:
            if depth_range is None and rng_dev is None:
                rng_dev = min_max_of(stage_depth)
            out["depth"][f].copy_(depth_image(stage_depth, (W, H), min_max=depth_range if depth_range is not None else rng_dev))
            images["depth"] = out["depth"][f]
        if "normal_float" in out:
            out["normal_float"][f].copy_(stage_normal)
        if "normal" in out:
            out["normal"][f].copy_(normal_image(stage_normal, (W, H)))
            images["normal"] = out["normal"][f]
        if sink is not None:
            sink("path", f, images)

    reuse = contextlib.ExitStack()
    if want_normal:  # parameters do not change between chunks: pack the field for upnerf_density_grad once, not per chunk
        from .normals import reuse_fragments
        reuse.enter_context(reuse_fragments())
    with reuse:
        for g0 in range(0, total, chunk):
            R = min(chunk, total - g0)
            rays, rows = path_rays(c2w, nf, (W, H), intr, g0, R, tables=[(w, ws[k]) for k, w in zip(keys, weights)], i0=i0, i1=i1,
                                   t=t, rays=ws["rays"])
            full = rays
            if occ_ws is not None:  # only the rays that touch something, over the part of the ray that does
                rays, rows, index, n_hit = oc.compact_rays(occupancy, full, rows, ws=occ_ws)
                LAST_STATS["hits"] += n_hit
            if occ_ws is None or n_hit > 0:
                res = render_static(system, rays, dict(zip(keys, rows)), sched_mult, normals=want_normal)
                rgb, depth = res[f"s_rgb_{typ}"], res[f"s_depth_{typ}"]
                normal = res[f"normal_{typ}"] if want_normal else None
            else:
                rgb = depth = normal = None
            if occ_ws is not None and want_normal:  # a ray that touches nothing has no normal: (0, 0, 0)
                full_normal = torch.zeros(R, 3, device=dev, dtype=torch.float32)
                if n_hit > 0:
                    full_normal[index[:n_hit].long()] = normal
                normal = full_normal
            if occ_ws is not None:
                rgb, depth = oc.scatter_results(index, full, rgb, depth if want_depth else None, background=1.0 if white_back else 0.0,
                                                want_depth=want_depth, out_rgb=occ_ws["rgb"], out_depth=occ_ws.get("depth"))
            g = g0
            while g < g0 + R:  # the chunk's rows, frame by frame
                f, p0 = divmod(g, n)
                cnt = min(n - p0, g0 + R - g)
                stage_rgb[p0:p0 + cnt].copy_(rgb[g - g0:g - g0 + cnt])
                if want_depth:
                    stage_depth[p0:p0 + cnt].copy_(depth[g - g0:g - g0 + cnt])
                if want_normal:
                    stage_normal[p0:p0 + cnt].copy_(normal[g - g0:g - g0 + cnt])
                g += cnt
                if p0 + cnt == n:
                    finish(f)
    return out


def _render_path_baked(system, path: CameraPath, chunk, outputs, depth_range, sink, occupancy, baked, baked_step):
    """render_path(..., baked=scene, baked_step=dt): the frames of `path` from the baked scene's grid alone (scene.render
    dispatches on scene.sh_degree: view dependence is the scene's, not an argument here)."""
    from .baked import BakedScene
    from .visualization import depth_image, min_max_of, rgb_image
    if not isinstance(baked, BakedScene):
        raise ValueError("baked is a baked.BakedScene")
    if occupancy is not None:
        raise ValueError("occupancy and baked exclude each other: a baked scene carries the bits of its own grid")
    if baked_step is None:
        raise ValueError("baked needs baked_step, the sample spacing in units of t (it has no default: it depends on the scene's scale)")
    unknown = set(outputs) - {"rgb", "depth", "rgb_float"}
    if unknown:
        raise ValueError(f"a baked scene renders rgb, depth and rgb_float only, not {sorted(unknown)}")
    dev = baked.device
    W, H = path.img_wh
    F, n = path.n_frames, W * H
    total = F * n
    chunk = int(chunk or system.hparams["val.chunk_size"])
    if chunk < 1:
        raise ValueError(f"chunk must be positive, got {chunk}")
    chunk = min(chunk, total)
    c2w, nf = path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode)
    intr = intrinsics(path.K)
    background = 1.0 if getattr(system.train_dataset, "white_back", False) else 0.0
    want_depth = "depth" in outputs
    rays_ws = torch.empty(chunk, 8, device=dev, dtype=torch.float32)
    ws = {"rgb": torch.empty(chunk, 3, device=dev), "depth": torch.empty(chunk, device=dev), "opacity": torch.empty(chunk, device=dev)}
    stage_rgb = torch.empty(n, 3, device=dev, dtype=torch.float32)
    stage_depth = torch.empty(n, device=dev, dtype=torch.float32) if want_depth else None
    out: Dict[str, torch.Tensor] = {}
    if "rgb" in outputs:
        out["rgb"] = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
    if want_depth:
        out["depth"] = torch.empty(F, H, W, 3, device=dev, dtype=torch.uint8)
    if "rgb_float" in outputs:
        out["rgb_float"] = torch.empty(F, n, 3, device=dev, dtype=torch.float32)
    rng_dev = None  # frame 0's (min, max) depth on the device: one colour scale for the whole sequence
    for g0 in range(0, total, chunk):
        R = min(chunk, total - g0)
        rays, _ = path_rays(c2w, nf, (W, H), intr, g0, R, rays=rays_ws)
        res = baked.render(rays, baked_step, background=background, out=ws)
        g = g0
        while g < g0 + R:  # the chunk's rows, frame by frame
            f, p0 = divmod(g, n)
            cnt = min(n - p0, g0 + R - g)
            stage_rgb[p0:p0 + cnt].copy_(res["rgb"][g - g0:g - g0 + cnt])
            if want_depth:
                stage_depth[p0:p0 + cnt].copy_(res["depth"][g - g0:g - g0 + cnt])
            g += cnt
            if p0 + cnt == n:
                images = {}
                if "rgb_float" in out:
                    out["rgb_float"][f].copy_(stage_rgb)
                if "rgb" in out:
                    out["rgb"][f].copy_(rgb_image(stage_rgb, (W, H)))
                    images["rgb"] = out["rgb"][f]
                if want_depth:
                    if depth_range is None and rng_dev is None:
                        rng_dev = min_max_of(stage_depth)
                    out["depth"][f].copy_(depth_image(stage_depth, (W, H), min_max=depth_range if depth_range is not None else rng_dev))
                    images["depth"] = out["depth"][f]
                if sink is not None:
                    sink("path", f, images)
    return out
