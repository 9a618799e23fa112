"""The static scene of a trained system as the scene tools see it: its training cameras (refined poses, near / far planes,
intrinsics), its fields and the one render call they share.  novel_view, geometry, normals and occupancy build on this; it is
host code only and the single copy of each piece."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["per_image", "plane", "near_far", "intrinsics", "refined_training_poses", "field_of", "box", "c_float3",
           "require_cuda", "appearance_rows", "static_keys", "render_static"]


def per_image(ds, name: str, idx: int):
    """Entry of a per-image collection of the dataset for TRAINING image `idx`: scene datasets key theirs by image id
    (`img_ids_train[idx]`), anything else is indexed by `idx`."""
    v = getattr(ds, name, None)
    if v is None:
        return None
    ids = getattr(ds, "img_ids_train", None)
    return v[ids[idx]] if (ids is not None and isinstance(v, dict)) else v[idx]


def plane(system, name: str, idx: int) -> float:
    """The "near" or "far" plane of training image `idx`: the dataset's `nears` / `fars` entry, hparams nerf.near / nerf.far
    where it has none."""
    v = per_image(system.train_dataset, f"{name}s", idx)
    return float(system.hparams[f"nerf.{name}"]) if v is None else float(v)


def near_far(system, idx: int) -> Tuple[float, float]:
    return plane(system, "near", idx), plane(system, "far", idx)


def intrinsics(K) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) as Python floats of a 3 x 3 tensor or array, or of (fx, fy, cx, cy) itself, through fp64."""
    Km = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float64)
    fx, fy, cx, cy = (Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]) if Km.shape == (3, 3) else Km
    return float(fx), float(fy), float(cx), float(cy)


def refined_training_poses(system, ids: Optional[Sequence[int]] = None, otherwise: str = "pass poses yourself") -> torch.Tensor:
    """[n, 3, 4] refined camera-to-world poses of training images `ids` (default: all): the dataset's poses composed with the
    trained se(3) rows (pose_align.refined_poses, the HIP pose kernel, which works row by row: a selection gives the rows the
    whole set gives).  otherwise: what the caller can do instead, for the error message."""
    from .pose_align import refined_poses
    ds = system.train_dataset
    w = system.se3_refine.weight.detach()
    if ids is None:
        ids = range(w.shape[0])
    else:
        w = w[torch.as_tensor(ids, device=w.device)]
    if getattr(ds, "poses_dict", None) is not None:
        raw = [per_image(ds, "poses_dict", i) for i in ids]
    elif getattr(ds, "poses", None) is not None:
        raw = [ds.poses[i] for i in ids]
    else:
        raise ValueError(f"the training dataset carries no poses (poses_dict / poses): {otherwise}")
    return refined_poses(w, torch.stack([torch.as_tensor(np.asarray(p), dtype=torch.float32).reshape(-1, 4)[:3] for p in raw]))


def field_of(system, field: str, what: str):
    """(model, device) of the `field` ("fine" or "coarse") network of `system`, for the GPU-only function `what`."""
    if field not in ("fine", "coarse"):
        raise ValueError(f"field is 'fine' or 'coarse', got {field!r}")
    model = system.models.get(f"nerf_{field}")
    if model is None:
        raise ValueError(f"the system has no {field} field")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs on the GPU only (no CPU fallback)")
    return model, dev


def box(bounds, strict: bool = False):
    """((x0, y0, z0), (x1, y1, z1)) as tuples of floats; strict: with hi > lo on every axis."""
    lo, hi = (tuple(float(v) for v in b) for b in bounds)
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("bounds is ((x0, y0, z0), (x1, y1, z1))")
    if strict and not all(h > l for l, h in zip(lo, hi)):
        raise ValueError(f"bounds must have hi > lo on every axis, got {lo} .. {hi}")
    return lo, hi


def c_float3(v):
    return (C.c_float * 3)(*v)


def require_cuda(what: str, *tensors) -> None:
    """Raise unless every one of `tensors` (tensors or torch.devices) is in device memory."""
    for t in tensors:
        dev = t if isinstance(t, torch.device) else (t.device if torch.is_tensor(t) else None)
        if dev is None or dev.type != "cuda":
            raise RuntimeError(f"libupnerf_hip operates on device memory only ({what} got a CPU tensor)")


def static_keys(system, sched_mult) -> list:
    """The embedding tables the phase reads: appearance always, candidate while the schedule has not finished."""
    return [k for k in system.embeddings if k.endswith("_a") or (k.endswith("_c") and sched_mult < 1)]


def appearance_rows(system, keys: Sequence[str], img_id: int, n: int) -> Dict[str, torch.Tensor]:
    """{key: [n, dim]}: row `img_id` of every table of `keys`, n times (the `embed_rows` of a view under one image's appearance)."""
    rows = {}
    for k in keys:
        w = system.embeddings[k].weight.detach()
        if not 0 <= int(img_id) < w.shape[0]:
            raise ValueError(f"img_id must be a training image index in [0, {w.shape[0]})")
        rows[k] = w[int(img_id)].expand(n, -1).contiguous()
    return rows


def render_static(system, rays: torch.Tensor, rows: Dict[str, torch.Tensor], sched_mult, normals: bool = False) -> dict:
    """render_rays of the static scene along `rays` [R, 8]: no dataset image behind them (`rows` are the per-ray embedding rows
    of static_keys(system, sched_mult)), perturb = 0, validation's sample counts.  The results dict of render_rays, untouched."""
    from .rendering import render_rays
    hp = system.hparams
    return render_rays(models=system.models, embeddings=system.embeddings, rays=rays, img_idx=None, sched_mult=sched_mult,
                       sched_phase=2 if sched_mult == 1 else 1, N_samples=hp["nerf.N_samples"], use_disp=hp["nerf.use_disp"], perturb=0,
                       N_importance=hp["nerf.N_importance"], white_back=getattr(system.train_dataset, "white_back", False),
                       encode_feat=hp["nerf.feat_dim"] > 0, validation=True, embed_rows=rows, normals=normals)
