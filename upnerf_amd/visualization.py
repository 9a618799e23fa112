"""The pictures of a validation (utils/visualization.py and models/nerf_system.py:276-307, nerf_system_optmize.py:179-193
of the reference): colour-mapped depth, PCA feature images and quantised colour maps, built by the HIP kernels of
csrc/viz.hip from the maps of the full-image render where they are.  The host only encodes PNG files (`ImageWriter`).

There is no CPU path: CPU tensors raise.  Nothing here calls `.cpu()` or `.item()` on a map.

Differences from the reference, all deliberate:
  * `JET` is built from OpenCV's documented construction (64 control points of the classic jet ramp, linear interpolation at
    256 evenly spaced positions, times 255, rounded half to even, saturated).  cv2 is not a dependency of this package and
    the table has NOT been compared with cv2's bits; `visualize_depth` takes any 256 x 3 uint8 table, so a user who has cv2
    can pass `cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_JET).reshape(256, 3)`.
  * The table is stored in cv2's BGR order and copied column for column: output channel c = table column c.  The reference
    hands cv2's BGR array to `Image.fromarray` unchanged, so in its logged depth pictures cv2's blue channel is displayed as
    red: small values appear dark red and large values dark blue, the mirror image of what cv2's JET shows.  That is kept
    exactly.
  * PCA images: a NaN component is left out of the min / max and written as 0 (the reference's whole image turns NaN), and
    so is every component when max == min.
  * A `val.log_image_list` name that holds none of "depth", "feat", "rgb" (`t_weight_fine`, `t_beta`, `t_alpha` in the
    shipped YAMLs): the reference logs the PREVIOUS entry's image again under that name (its `img` variable is stale).  Here a
    single-channel map becomes a grey image and anything else is skipped."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .metrics import parse_img_wh

# the classic jet ramp at 64 control points, in sixteenths (blue starts at 9/16, red ends at 8/16)
_JET_R16 = (0,) * 24 + tuple(range(1, 17)) + (16,) * 16 + tuple(range(15, 7, -1))
_JET_G16 = (0,) * 8 + tuple(range(1, 17)) + (16,) * 16 + tuple(range(15, -1, -1)) + (0,) * 8
_JET_B16 = tuple(range(9, 17)) + (16,) * 16 + tuple(range(15, -1, -1)) + (0,) * 24


def _ramp_to_u8(ctrl16) -> List[int]:
    """256 samples of the piecewise-linear curve through the 64 control points, times 255, rounded half to even -- in exact
    integer arithmetic: position i sits at i * 63 / 255 = i * 21 / 85 control-point intervals."""
    out = []
    for i in range(256):
        lo, rem = divmod(i * 21, 85)
        hi = min(lo + 1, 63)
        v = ctrl16[lo] * (85 - rem) + ctrl16[hi] * rem  # value * 16 * 85
        q, r = divmod(v * 255, 16 * 85)
        if 2 * r > 16 * 85 or (2 * r == 16 * 85 and q % 2):
            q += 1
        out.append(max(0, min(255, q)))
    return out


JET = np.stack([np.array(_ramp_to_u8(c), dtype=np.uint8) for c in (_JET_B16, _JET_G16, _JET_R16)], axis=1)  # [256, 3], BGR
JET.setflags(write=False)

_LUT_CACHE: Dict[tuple, torch.Tensor] = {}


def _lut_on(cmap, device) -> torch.Tensor:
    """The 256 x 3 uint8 table on `device`; `JET` is uploaded once per device (so a captured graph can hold its address)."""
    if cmap is JET:
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in _LUT_CACHE:
            _LUT_CACHE[key] = torch.from_numpy(np.array(JET)).to(device)
        return _LUT_CACHE[key]
    t = torch.as_tensor(cmap)
    if t.dtype != torch.uint8 or tuple(t.shape) != (256, 3):
        raise ValueError(f"a colour table is 256 x 3 uint8, got {tuple(t.shape)} {t.dtype}")
    return t.to(device).contiguous()


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"libupnerf_hip operates on device memory only ({what} is not a device tensor)")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be fp32 (got {t.dtype})")


def _pixels(t: torch.Tensor, n: int, what: str) -> Tuple[torch.Tensor, int]:
    """(tensor, element stride between pixels) of a single-channel map with n pixels, read in place where its layout is
    one stride ([n], [n, 1], a column of [n, C], [H, W] with uniform rows); anything else is made contiguous first."""
    if t.numel() != n:
        raise ValueError(f"{what} has {t.numel()} elements, the image has {n} pixels")
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() == 1:
        return t, (t.stride(0) if n > 1 else 1)
    if t.dim() == 2 and (t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1)):
        return t, (t.stride(1) if t.shape[1] > 1 else 1)
    return t.contiguous(), 1


def min_max_of(x: torch.Tensor) -> torch.Tensor:
    """Device tensor [2] = (min, max) of nan_to_num(x), reduced on the device: the `min_max` of another map's picture
    (the reference reads them back with `.item()`, nerf_system.py:285-286)."""
    _need_cuda(x, "the map")
    x, stride = _pixels(x, x.numel(), "the map")
    n = x.numel()
    ns = _lib.lib.upnerf_viz_minmax_scratch(n)
    if ns < 0:
        _lib.check(ns, "upnerf_viz_minmax_scratch")
    scratch = torch.empty(ns, dtype=torch.float32, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib.upnerf_viz_minmax(x.data_ptr(), n, stride, _lib.ptr(out), _lib.ptr(scratch), _lib.stream()),
               "upnerf_viz_minmax")
    return out


def depth_image(depth: torch.Tensor, img_wh, cmap=JET, min_max=None, depth_scale: Optional[torch.Tensor] = None,
                near: float = 0.0, far: float = 1.0, want_index: bool = False, want_value: bool = False):
    """uint8 [H, W, 3] colours of a depth map with H * W pixels (upnerf_viz_depth; include/upnerf_hip.h states every step).

    min_max: None (the map's own range), two Python numbers, or a device tensor [2] (e.g. `min_max_of(other_map)`).
    depth_scale: the image's (scale, shift) row on the device -> `depth` holds inverse depths and the picture is that of the
    reference's `pred_depths` (nerf_system.py:249-256, with `near` / `far`).
    Output channel c is table column c; with `JET` (cv2's BGR order) that reproduces the reference's red / blue swap.
    Returns the image, or (image, index uint8 [H, W] or None, value fp32 [H * W] or None) when either extra is asked for."""
    W, H = parse_img_wh(img_wh)
    _need_cuda(depth, "the depth map")
    if H < 1 or W < 1:
        raise ValueError(f"an image needs H, W >= 1, got H={H}, W={W}")
    x, stride = _pixels(depth, H * W, "the depth map")
    dev = x.device
    lut = _lut_on(cmap, dev)
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    index = torch.empty(H, W, dtype=torch.uint8, device=dev) if want_index else None
    value = torch.empty(H * W, dtype=torch.float32, device=dev) if want_value else None
    a = _lib.VizDepthArgs(H=H, W=W, pre=_lib.VIZ_PLAIN, range=_lib.VIZ_RANGE_OWN, x=x.data_ptr(), x_stride=stride,
                          lut=_lib.ptr(lut), rgb=_lib.ptr(rgb), index=_lib.ptr(index), value=_lib.ptr(value))
    keep = None
    if depth_scale is not None:
        _need_cuda(depth_scale, "depth_scale")
        keep = depth_scale.reshape(-1).contiguous()
        if keep.numel() != 2:
            raise ValueError("depth_scale is the image's (scale, shift) row")
        a.pre, a.depth_scale, a.inv_far, a.near = _lib.VIZ_PRED_DEPTH, keep.data_ptr(), 1 / float(far), float(near)
    scratch = None
    if min_max is None:
        ns = _lib.lib.upnerf_viz_depth_scratch(C.byref(a))
        if ns < 0:
            _lib.check(ns, "upnerf_viz_depth_scratch")
        scratch = torch.empty(ns, dtype=torch.float32, device=dev)
    elif torch.is_tensor(min_max):
        _need_cuda(min_max, "min_max")
        min_max = min_max.reshape(-1).contiguous()
        if min_max.numel() != 2:
            raise ValueError("a device min_max holds (min, max)")
        a.range, a.range_dev = _lib.VIZ_RANGE_DEVICE, min_max.data_ptr()
    else:
        mi, ma = min_max
        a.range, a.mi, a.ma = _lib.VIZ_RANGE_HOST, float(mi), float(ma)
    _lib.check(_lib.lib.upnerf_viz_depth(C.byref(a), _lib.ptr(scratch), _lib.stream()), "upnerf_viz_depth")
    return (rgb, index, value) if (want_index or want_value) else rgb


def visualize_depth(depth: torch.Tensor, cmap=JET, min_max=None) -> torch.Tensor:
    """visualization.py:7-23 on a device map (H, W): float (3, H, W) in [0, 1] on the device, the `ToTensor()` of the
    colour-mapped picture.  `cmap` is a 256 x 3 uint8 table (not a cv2 constant); see the module docstring for `JET`, its
    caveat and the BGR order that is kept from the reference."""
    if not torch.is_tensor(depth) or depth.dim() != 2:
        raise ValueError("depth is an (H, W) tensor")
    H, W = depth.shape
    img = depth_image(depth, (W, H), cmap=cmap, min_max=min_max)
    # ToTensor()'s uint8 / 255 through a table divided on the host: a device division by a scalar multiplies by its reciprocal
    key = ("unit", img.device.type, img.device.index)
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = (torch.arange(256, dtype=torch.float32) / 255).to(img.device)
    return _LUT_CACHE[key][img.permute(2, 0, 1).long()]


def pca_image(feat: torch.Tensor, m: torch.Tensor, c: torch.Tensor, img_wh) -> Tuple[torch.Tensor, torch.Tensor]:
    """(float [H, W, 3], uint8 [H, W, 3]) of a feature map [H * W, F] (or [H, W, F]) under the mean `m` [F] and components `c`
    [3, F] (upnerf_viz_pca): fp32 projection, ONE min and ONE max over pixels and components, normalised to [0, 1].
    Deviation from the reference: NaN components are left out of the range and come out as 0."""
    W, H = parse_img_wh(img_wh)
    for t, what in ((feat, "the feature map"), (m, "pca_m"), (c, "pca_c")):
        _need_cuda(t, what)
    F = feat.shape[-1]
    if feat.numel() != H * W * F or m.numel() != F or tuple(c.shape) != (3, F):
        raise ValueError(f"expected features [{H * W}, F], m [F], c [3, F]; got {tuple(feat.shape)}, {tuple(m.shape)}, "
                         f"{tuple(c.shape)}")
    if not 1 <= F <= 512:
        raise ValueError(f"feature width must be in [1, 512], got {F}")
    if feat.dim() == 2 and feat.stride(1) == 1 and feat.stride(0) >= F:
        rows, ld = feat, feat.stride(0)
    else:
        rows, ld = feat.contiguous().reshape(H * W, F), F
    m, c = m.reshape(-1).contiguous(), c.contiguous()
    img = torch.empty(H, W, 3, dtype=torch.float32, device=feat.device)
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=feat.device)
    a = _lib.VizPcaArgs(H=H, W=W, F=F, feat=rows.data_ptr(), feat_ld=ld, m=_lib.ptr(m), c=_lib.ptr(c), img=_lib.ptr(img),
                        rgb=_lib.ptr(rgb))
    ns = _lib.lib.upnerf_viz_pca_scratch(C.byref(a))
    if ns < 0:
        _lib.check(ns, "upnerf_viz_pca_scratch")
    scratch = torch.empty(ns, dtype=torch.float32, device=feat.device)
    _lib.check(_lib.lib.upnerf_viz_pca(C.byref(a), _lib.ptr(scratch), _lib.stream()), "upnerf_viz_pca")
    return img, rgb


def get_pca_img(feat: torch.Tensor, m: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """visualization.py:26-30 on a device map (H, W, F): float (H, W, 3) on the device.  NaN components come out as 0 (the
    reference returns an all-NaN image)."""
    if not torch.is_tensor(feat) or feat.dim() != 3:
        raise ValueError("feat is an (H, W, F) tensor")
    return pca_image(feat, m, c, (feat.shape[1], feat.shape[0]))[0]


def rgb_image(x: torch.Tensor, img_wh) -> torch.Tensor:
    """uint8 [H, W, 3] of a float map [H * W, 3], or [H * W] / [H * W, 1] replicated to three channels (upnerf_viz_rgb):
    `(uint8) clamp(255 * v, 0, 255)`, truncating; NaN -> 0."""
    W, H = parse_img_wh(img_wh)
    _need_cuda(x, "the map")
    n = H * W
    if n < 1:
        raise ValueError(f"an image needs H, W >= 1, got H={H}, W={W}")
    if x.dim() == 3 and x.shape[0] * x.shape[1] == n:
        x = x.reshape(n, x.shape[2])
    if x.dim() == 2 and tuple(x.shape) == (n, 3):
        ch, stride, cstride = 3, x.stride(0), x.stride(1)
    else:
        x, stride = _pixels(x, n, "the map")
        ch, cstride = 1, 0
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=x.device)
    a = _lib.VizRgbArgs(H=H, W=W, C=ch, x=x.data_ptr(), stride=stride, cstride=cstride, rgb=_lib.ptr(rgb))
    _lib.check(_lib.lib.upnerf_viz_rgb(C.byref(a), _lib.stream()), "upnerf_viz_rgb")
    return rgb


def normal_image(normals: torch.Tensor, img_wh, rot: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [H, W, 3] of a normal map [H * W, 3] (upnerf_viz_normals): `(n + 1) / 2` quantised as rgb_image quantises, a zero
    normal (nothing hit) drawn as mid-grey (128, 128, 128).  rot: a 3 x 3 rotation applied first, e.g. the world-to-camera
    rotation c2w[:, :3].T for a camera-space map; None: the world-space normals as they are."""
    W, H = parse_img_wh(img_wh)
    _need_cuda(normals, "the normal map")
    n = H * W
    if n < 1:
        raise ValueError(f"an image needs H, W >= 1, got H={H}, W={W}")
    if normals.numel() != 3 * n or normals.shape[-1] != 3:
        raise ValueError(f"expected normals [{n}, 3], got {tuple(normals.shape)}")
    x = normals.detach().reshape(n, 3).float().contiguous()
    if rot is not None:
        if tuple(rot.shape) != (3, 3):
            raise ValueError("rot is a 3 x 3 rotation")
        rot = torch.as_tensor(rot).detach().to(device=x.device, dtype=torch.float32).contiguous()
    rgb = torch.empty(H, W, 3, dtype=torch.uint8, device=x.device)
    a = _lib.VizNormalsArgs(H=H, W=W, n=_lib.ptr(x), rot=_lib.ptr(rot), rgb=_lib.ptr(rgb))
    _lib.check(_lib.lib.upnerf_viz_normals(C.byref(a), _lib.stream()), "upnerf_viz_normals")
    return rgb


# ---- which picture each name gets (nerf_system.py:281-305) ---------------------------------------------------------

def plan_validation_images(log_image_list, results: Mapping, typ: str, has_pca: bool, has_inv_depths: bool) -> List[tuple]:
    """[(name, kind, source)] in the reference's order; kind is "rgb", "pca", "depth", "pred_depth" or "grey", source the key of
    `results` (or of the batch for the three *_GT pictures).  `results` maps names to tensors or to their shapes.

    rgb_GT always; feat_GT when the batch carries feats, pca_m and pca_c; rescale_depth_GT when it carries inv_depths (coloured
    over the range of s_depth_{typ}).  Then every name of `val.log_image_list`, tested as the reference tests it: "depth" in
    the name, else "feat" (and PCA data present), else "rgb".  A name that is not in `results` is skipped (the reference's bare
    `except`); a name that matches none of the three becomes a grey picture when its map has one channel and is skipped
    otherwise (the reference repeats the previous picture under that name)."""
    plan = [("rgb_GT", "rgb", "rgbs")]
    if has_pca:
        plan.append(("feat_GT", "pca", "feats"))
    if has_inv_depths and f"s_depth_{typ}" in results:
        plan.append(("rescale_depth_GT", "pred_depth", "inv_depths"))
    for name in log_image_list or ():
        if name not in results:
            continue
        if "depth" in name:
            plan.append((name, "depth", name))
        elif "feat" in name and has_pca:
            plan.append((name, "pca", name))
        elif "rgb" in name:
            plan.append((name, "rgb", name))
        elif "normal" in name:  # (not a reference picture: render_rays(normals=True))
            plan.append((name, "normal", name))
        else:
            v = results[name]
            shape = tuple(getattr(v, "shape", v))
            if len(shape) == 1 or (len(shape) == 2 and shape[1] == 1):
                plan.append((name, "grey", name))
    return plan


def _is_tto(system) -> bool:
    from .nerf_system_optimize import NeRFSystemOptimize
    return isinstance(system, NeRFSystemOptimize)


def validation_images(system, batch: Mapping, results: Mapping) -> Dict[str, torch.Tensor]:
    """The pictures the reference logs for one validation image, as uint8 [H, W, 3] device tensors by the reference's names.

    `batch` is the validation batch as `validation_step` takes it (NeRFSystem: every tensor with a leading 1;
    NeRFSystemOptimize: without), `results` the maps of that step's render.  NeRFSystem: `plan_validation_images`;
    NeRFSystemOptimize (nerf_system_optmize.py:179-193): `GT` and `rgb_fine`, the latter from `s_rgb_fine`.
    `hparams["debug"]` returns {} (nerf_system.py:273-274)."""
    hp = system.hparams
    if hp.get("debug", False):
        return {}
    if batch.get("img_wh") is None:
        raise ValueError("validation images need the image size: the batch carries no img_wh")
    wh = parse_img_wh(batch["img_wh"])
    n = wh[0] * wh[1]
    device = batch["rgbs"].device
    dims = {"rgbs": 2, "feats": 2, "inv_depths": 1, "img_idx": 1, "pca_m": 1, "pca_c": 2}

    def item(key):
        """The batch entry without the DataLoader's leading 1; the PCA data of a dataset item may still be numpy arrays."""
        v = batch.get(key)
        if v is None:
            return None
        if key in ("pca_m", "pca_c") and not (torch.is_tensor(v) and v.is_cuda):
            v = torch.as_tensor(v).to(device=device, dtype=torch.float32)
        return v[0] if v.dim() == dims[key] + 1 else v

    if _is_tto(system):
        return {"GT": rgb_image(item("rgbs").reshape(n, 3), wh), "rgb_fine": rgb_image(results["s_rgb_fine"], wh)}
    typ = "fine" if "rgb_fine" in results else "coarse"
    feats, pca_m, pca_c = item("feats"), item("pca_m"), item("pca_c")
    has_pca = feats is not None and pca_m is not None and pca_c is not None
    plan = plan_validation_images(hp.get("val.log_image_list", ()), results, typ, has_pca, item("inv_depths") is not None)
    out = {}
    for name, kind, src in plan:
        if kind == "rgb":
            out[name] = rgb_image(item(src).reshape(n, 3) if name == "rgb_GT" else results[src], wh)
        elif kind == "pca":
            out[name] = pca_image(feats.reshape(n, -1) if name == "feat_GT" else results[src], pca_m, pca_c, wh)[1]
        elif kind == "depth":
            out[name] = depth_image(results[src], wh)
        elif kind == "grey":
            out[name] = rgb_image(results[src], wh)
        elif kind == "normal":
            out[name] = normal_image(results[src], wh)
        else:  # pred_depth: the depth prior under the image's learnt scale and shift, over the range of the rendered depth
            row = system.depth_scale.weight.detach()[item("img_idx").reshape(-1)[:1].long()]  # the first ray's image (:249)
            out[name] = depth_image(item(src), wh, min_max=min_max_of(results[f"s_depth_{typ}"]), depth_scale=row,
                                    near=hp["nerf.near"], far=hp["nerf.far"])
    return out


def image_tag(system, batch: Mapping) -> str:
    """The reference's logger prefix of a validation image: `val_<img_idx>` (nerf_system.py:277, 290), and
    `val_<optimize_num>` for the test-time-optimisation system (nerf_system_optmize.py:173, 192)."""
    if _is_tto(system):
        num = getattr(getattr(system, "val_dataset", None), "optimize_num", system.hparams.get("optimize_num", 0))
        return f"val_{int(num)}"
    return f"val_{int(batch['img_idx'].reshape(-1)[0])}"


class ImageWriter:
    """A sink `(tag, step, images)` that writes `root/<tag>/step_<step, 8 digits>/<name>.png`: one device-to-host copy per image
    (through a pinned staging buffer when `pinned`), PNG encoding by PIL on the host.  Tags follow the reference's logger keys:
    `val_<img_idx>` for training validation, `val_<optimize_num>` for test-time optimisation."""

    def __init__(self, root: str, pinned: bool = False):
        self.root, self.pinned = root, pinned
        self._stage: Dict[tuple, torch.Tensor] = {}
        self.written: List[str] = []

    def path(self, tag: str, step: int, name: str) -> str:
        return os.path.join(self.root, str(tag), f"step_{int(step):08d}", f"{name}.png")

    def _to_host(self, img: torch.Tensor) -> np.ndarray:
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError(f"an image is uint8 [H, W, 3], got {tuple(img.shape)} {img.dtype}")
        if not img.is_cuda:
            return img.contiguous().numpy()
        if not self.pinned:
            return img.contiguous().cpu().numpy()
        key = tuple(img.shape)
        if key not in self._stage:
            self._stage[key] = torch.empty(key, dtype=torch.uint8, pin_memory=True)
        self._stage[key].copy_(img, non_blocking=True)
        torch.cuda.current_stream(img.device).synchronize()
        return self._stage[key].numpy()

    def __call__(self, tag: str, step: int, images: Mapping[str, torch.Tensor]) -> List[str]:
        from PIL import Image
        paths = []
        for name, img in images.items():
            p = self.path(tag, step, name)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            Image.fromarray(self._to_host(img)).save(p, format="PNG")
            paths.append(p)
        self.written += paths
        return paths
