"""The reference's datasets (datasets/phototourism.py, phototourism_optimize.py, custom.py, custom_optimize.py) with their
constructor arguments, attributes and validation items, built on the device.

The host does what only it can do: parse the scene's metadata (scene.py), decode and LANCZOS-downscale the JPEGs with
PIL (a thread pool of at most 16 workers) and read the DINO / DPT `.npy` files.  Uploaded as uint8 pixels and raw maps,
everything per pixel is then built by two HIP launches per kind of buffer (csrc/scene.hip): `upnerf_scene_rays` writes
directions, ray infos, pixel coordinates and colours of all training images straight into the HBM buffers GpuRaySampler
reads, and `upnerf_resize_linear` does the cv2.resize + normalisation of the feature and depth maps.  So the train
split's buffers (`all_ray_infos`, `all_directions`, `all_rgbs`, `all_pxl_coords`, `all_inv_depths`, `feat_maps`) are
device tensors, fp32 and contiguous: GpuRaySampler.from_dataset takes them without a copy.

`use_cache` is accepted and ignored: the reference's cache step (prepare_phototourism.py, pickled CPU tensors) exists to
avoid rebuilding those buffers on the CPU; here every scene is built from its raw files.  Reading the cache pickles is
not supported.  The reference's unfinished `test` / `video` splits are not provided.  PIL is imported on first use."""
from __future__ import annotations

import ctypes as C
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .scene import custom_meta, initial_train_poses, phototourism_meta

MAX_DECODE_WORKERS = 16


# ---- host: decoding -----------------------------------------------------------------------------------------------------

def decode_image(path: str, scale: int) -> np.ndarray:
    """uint8 [H, W, 3]: PIL RGB, LANCZOS-resized to (W // scale, H // scale) when scale > 1 (phototourism.py:243-252)."""
    from PIL import Image
    img = Image.open(path).convert("RGB")
    w, h = img.size
    if scale > 1:
        img = img.resize((w // scale, h // scale), Image.LANCZOS)
    return np.ascontiguousarray(np.asarray(img, dtype=np.uint8))


def _pool_map(fn, items):
    items = list(items)
    if len(items) <= 1:
        return [fn(x) for x in items]
    with ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, len(items), os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, items))


# ---- device: the two kernels ----------------------------------------------------------------------------------------

def upload_pixels(images, device):
    """One uint8 device buffer holding every [H, W, 3] image; returns (buffer, byte offsets)."""
    offs, total = [], 0
    for im in images:
        offs.append(total)
        total += im.size
    host = np.empty(max(total, 1), dtype=np.uint8)
    for o, im in zip(offs, images):
        host[o:o + im.size] = im.reshape(-1)
    return torch.from_numpy(host).to(device), offs


def scene_rays(descs, pixels=None, pix_offs=None, device="cuda", ray_infos=True, pxl=True, rgbs=True):
    """Buffers of the images `descs` (dicts with W, H, K, near, far, img_idx and an optional window x0, x1) in one
    upnerf_scene_rays launch, rows in descriptor order: {"directions", "ray_infos", "pxl", "rgbs"} ([rows, 3] / [rows, 2]
    fp32 device tensors; absent when not asked for).  rgbs needs `pixels` (upload_pixels)."""
    n = len(descs)
    tab = (_lib.SceneImage * n)()
    row = 0
    for k, d in enumerate(descs):
        K = d["K"]
        x0, x1 = d.get("x0", 0), d.get("x1", d["W"])
        tab[k] = _lib.SceneImage(W=d["W"], H=d["H"], x0=x0, x1=x1, fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]),
                                 cy=float(K[1, 2]), near=float(d["near"]), far=float(d["far"]), img_idx=float(d["img_idx"]),
                                 row0=row, pix_off=pix_offs[k] if pix_offs is not None else 0)
        row += (x1 - x0) * d["H"]
    e = lambda c, on: torch.empty(row, c, device=device, dtype=torch.float32) if on else None
    out = {"directions": e(3, True), "ray_infos": e(3, ray_infos), "pxl": e(2, pxl), "rgbs": e(3, rgbs)}
    table = torch.empty(C.sizeof(tab), dtype=torch.uint8, device=device)
    a = _lib.SceneRaysArgs(n_images=n, rows=row, pix_bytes=pixels.numel() if pixels is not None else 0,
                           pixels=_lib.ptr(pixels), directions=_lib.ptr(out["directions"]),
                           ray_infos=_lib.ptr(out["ray_infos"]), pxl=_lib.ptr(out["pxl"]), rgbs=_lib.ptr(out["rgbs"]))
    _lib.check(_lib.lib.upnerf_scene_rays(C.byref(a), tab, _lib.ptr(table), _lib.stream()), "upnerf_scene_rays")
    return {k: v for k, v in out.items() if v is not None}


def resize_linear(src: torch.Tensor, maps, C_: int, pre: int = _lib.RESIZE_PLAIN, dst: torch.Tensor = None):
    """One upnerf_resize_linear launch.  `src` is a flat fp32 device tensor; `maps` are dicts with h, w, H, W, src_off,
    dst_off (floats) and, for the depth pre-step, near / far.  Returns `dst` (allocated flat when not given; pass
    dst=src for the in-place L2 normalisation of same-size maps)."""
    n = len(maps)
    tab = (_lib.ResizeMap * n)()
    need = 0
    for k, m in enumerate(maps):
        scale = bias = 0.0
        if pre == _lib.RESIZE_INVDEPTH:  # phototourism.py:319-320, in the reference's fp32 arithmetic
            M, mm = 1 / m["near"], 1 / m["far"]
            scale, bias = float(np.float32(M - mm)), float(np.float32(mm))
        tab[k] = _lib.ResizeMap(h=m["h"], w=m["w"], H=m["H"], W=m["W"], src_off=m["src_off"], dst_off=m["dst_off"],
                                scale=scale, bias=bias)
        need = max(need, m["dst_off"] + m["H"] * m["W"] * C_)
    if dst is None:
        dst = torch.empty(need, device=src.device, dtype=torch.float32)
    a = _lib.ResizeArgs(n_maps=n, C=C_, pre=pre, src_elems=src.numel(), dst_elems=dst.numel(), src=_lib.ptr(src),
                        dst=_lib.ptr(dst))
    nbytes = _lib.lib.upnerf_resize_scratch(C.byref(a))
    if nbytes < 0:
        _lib.check(nbytes, "upnerf_resize_scratch")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    _lib.check(_lib.lib.upnerf_resize_linear(C.byref(a), tab, _lib.ptr(scratch), _lib.stream()), "upnerf_resize_linear")
    return dst


def l2_normalize_(feat: torch.Tensor) -> torch.Tensor:
    """feat / ||feat|| over the last dimension, in place, for a contiguous [..., h, w, C] device tensor (line 287)."""
    h, w, Cc = feat.shape[-3:]
    n = feat.numel() // (h * w * Cc)
    flat = feat.view(-1)
    maps = [dict(h=h, w=w, H=h, W=w, src_off=k * h * w * Cc, dst_off=k * h * w * Cc) for k in range(n)]
    resize_linear(flat, maps, Cc, _lib.RESIZE_L2, dst=flat)
    return feat


def _as_hwc(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    return a[..., None] if a.ndim == 2 else a


def upload_maps(arrays, device):
    """[h, w(, C)] fp32 maps of one C -> (flat device tensor, map dicts with h, w and src_off)."""
    arrays = [_as_hwc(a) for a in arrays]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += a.size
    host = np.empty(total, dtype=np.float32)
    for o, a in zip(offs, arrays):
        host[o:o + a.size] = a.reshape(-1)
    return torch.from_numpy(host).to(device), [dict(h=a.shape[0], w=a.shape[1], src_off=o) for a, o in zip(arrays, offs)]


def resize_to(arrays, sizes, pre, device, nears_fars=None):
    """cv2.resize(a, (W, H)) of every map (with the pre-step), concatenated: flat [sum H * W * C] device tensor."""
    src, maps = upload_maps(arrays, device)
    Cc = _as_hwc(arrays[0]).shape[2]
    off = 0
    for k, (m, (W, H)) in enumerate(zip(maps, sizes)):
        m.update(H=H, W=W, dst_off=off)
        if nears_fars is not None:
            m["near"], m["far"] = nears_fars[k]
        off += H * W * Cc
    return resize_linear(src, maps, Cc, pre)


# ---- datasets -------------------------------------------------------------------------------------------------------

class _Timer:
    def __init__(self, device):
        self.device, self.t, self.phases = torch.device(device), time.perf_counter(), {}
        self.t0 = self.t

    def lap(self, name, sync=False):
        if sync and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.phases[name] = self.phases.get(name, 0.0) + now - self.t
        self.t = now

    def done(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.phases["total"] = time.perf_counter() - self.t0
        return self.phases


class _SceneDataset:
    """Shared by the phototourism and custom scenes: `_meta()` differs, the buffers are built alike."""
    custom = False

    def __init__(self, root_dir, scene_name, feat_dir=None, depth_dir=None, near=0.1, far=5.0, camera_noise=-1,
                 split="train", img_downscale=1, val_img_idx=(0,), use_cache=False, device="cuda"):
        self.root_dir, self.scene_name = root_dir, scene_name
        self.feat_map_dir = os.path.join(feat_dir, "feature_maps") if feat_dir is not None else None
        self.pca_info_dir = os.path.join(feat_dir, "pca_infos") if feat_dir is not None else None
        self.depth_dir = depth_dir
        self.near, self.far = near, far
        self.camera_noise = camera_noise
        self.split = split
        self.scale = max(2, img_downscale) if split == "val" else img_downscale  # the reference's guard against OOM
        self.val_img_idx = list(val_img_idx)
        self.use_cache = use_cache  # accepted, ignored (module docstring)
        self.device = torch.device(device)
        self.white_back = False
        timer = _Timer(self.device)
        self._read_meta()
        timer.lap("metadata")
        if split == "train":
            self._build_train(timer)
        elif split == "val":
            self._build_val(timer)
        else:
            raise NotImplementedError(f"split {split!r}: only train and val are provided")
        self.load_times = timer.done()

    # -- metadata
    def _read_meta(self):
        m = custom_meta(self.root_dir, self.scale) if self.custom else phototourism_meta(self.root_dir, self.scene_name,
                                                                                           self.scale)
        self.meta = m
        self.img_ids, self.image_paths, self.Ks = m.img_ids, m.image_paths, m.Ks
        self.nears, self.fars, self.xyz_world = m.nears, m.fars, m.xyz_world
        self.img_ids_train, self.img_ids_test = m.img_ids_train, m.img_ids_test
        self.N_images_train, self.N_images_test = len(m.img_ids_train), len(m.img_ids_test)
        self.id2idx = {id_: i for i, id_ in enumerate(m.img_ids_train)}
        if self.custom:  # custom.py:109-139: identities for every training image, whatever the noise
            if m.poses_dict:
                self.GT_poses_dict = m.poses_dict
            self.poses_dict = {id_: torch.eye(3, 4) for id_ in m.img_ids_train}
        else:
            self.poses_dict, self.GT_poses_dict, self.pose_noises = initial_train_poses(m, self.camera_noise, self.device)

    def _image_path(self, id_):
        return os.path.join(self.meta.image_root, self.image_paths[id_])

    def _train_near_far(self, id_):
        # line 305: `camera_noise is not None` holds for every configuration, so the rays carry the global bounds
        if self.custom or self.camera_noise is not None:
            return self.near, self.far
        return self.nears[id_], self.fars[id_]

    def _val_near_far(self, id_):
        if self.custom or self.camera_noise != 0:  # line 351
            return self.near, self.far
        return self.nears[id_], self.fars[id_]

    # -- train split: every training image's rays in the device buffers
    def _build_train(self, timer):
        ids = self.img_ids_train
        fname = self.meta.feature_name
        imgs = _pool_map(lambda i: decode_image(self._image_path(i), self.scale), ids)
        feats = _pool_map(lambda i: np.load(os.path.join(self.feat_map_dir, fname(i))), ids) if self.feat_map_dir else None
        depths = _pool_map(lambda i: np.load(os.path.join(self.depth_dir, fname(i))), ids) if self.depth_dir else None
        timer.lap("decode")
        pixels, offs = upload_pixels(imgs, self.device)
        fsrc = torch.from_numpy(np.stack([np.asarray(f, dtype=np.float32) for f in feats], 0)).to(self.device) if feats else None
        dsrc = upload_maps(depths, self.device) if depths else None
        timer.lap("upload", sync=True)
        self.all_imgs_wh = torch.tensor([[im.shape[1], im.shape[0]] for im in imgs], dtype=torch.int64)
        descs = []
        for id_, im in zip(ids, imgs):
            near, far = self._train_near_far(id_)
            descs.append(dict(W=im.shape[1], H=im.shape[0], K=self.Ks[id_], near=near, far=far, img_idx=self.id2idx[id_]))
        b = scene_rays(descs, pixels, offs, self.device)
        self.all_directions, self.all_ray_infos, self.all_pxl_coords, self.all_rgbs = b["directions"], b["ray_infos"], b["pxl"], b["rgbs"]
        self.feat_maps = l2_normalize_(fsrc) if fsrc is not None else None
        self.all_inv_depths = None
        if dsrc is not None:
            src, maps = dsrc
            off = 0
            for m, im in zip(maps, imgs):
                m.update(H=im.shape[0], W=im.shape[1], dst_off=off, near=self.near, far=self.far)
                off += im.shape[0] * im.shape[1]
            self.all_inv_depths = resize_linear(src, maps, 1, _lib.RESIZE_INVDEPTH)
        timer.lap("kernels", sync=True)

    # -- val split: full images of the training set
    def _build_val(self, timer):
        ids = [self.img_ids_train[i] for i in self.val_img_idx]
        fname = self.meta.feature_name
        imgs = _pool_map(lambda i: decode_image(self._image_path(i), self.scale), ids)
        feats = [np.load(os.path.join(self.feat_map_dir, fname(i))) for i in ids] if self.feat_map_dir else None
        pca = [(np.load(os.path.join(self.pca_info_dir, fname(i).replace(".npy", "_mean.npy"))),
                np.load(os.path.join(self.pca_info_dir, fname(i).replace(".npy", "_components.npy")))) for i in ids] \
            if self.pca_info_dir else [(None, None)] * len(ids)
        depths = [np.load(os.path.join(self.depth_dir, fname(i))) for i in ids] if self.depth_dir else None
        timer.lap("decode")
        pixels, offs = upload_pixels(imgs, self.device)
        timer.lap("upload", sync=True)
        sizes = [(im.shape[1], im.shape[0]) for im in imgs]
        nf = [self._val_near_far(i) for i in ids]
        descs = [dict(W=W, H=H, K=self.Ks[i], near=n, far=f, img_idx=self.id2idx[i]) for i, (W, H), (n, f) in zip(ids, sizes, nf)]
        b = scene_rays(descs, pixels, offs, self.device, pxl=False)
        f_all = resize_to(feats, sizes, _lib.RESIZE_L2, self.device) if feats else None
        d_all = resize_to(depths, sizes, _lib.RESIZE_INVDEPTH, self.device, nears_fars=nf) if depths else None
        self.rgbs, self.directions, self.ray_infos, self.feats, self.inv_depths = [], [], [], [], []
        self.imgs_wh, self.pca_m, self.pca_c = [], [], []
        row = foff = 0
        Cf = feats[0].shape[-1] if feats else 0
        for (W, H), (pm, pc) in zip(sizes, pca):
            n = W * H
            self.rgbs.append(b["rgbs"][row:row + n])
            self.directions.append(b["directions"][row:row + n])
            self.ray_infos.append(b["ray_infos"][row:row + n])
            self.feats.append(f_all[foff * Cf:(foff + n) * Cf].view(n, Cf) if f_all is not None else None)
            self.inv_depths.append(d_all[foff:foff + n] if d_all is not None else None)
            self.imgs_wh.append(torch.LongTensor([W, H]))
            self.pca_m.append(pm)
            self.pca_c.append(pc)
            row += n
            foff += n
        timer.lap("kernels", sync=True)

    def __len__(self):
        if self.split == "train":
            return self.all_ray_infos.shape[0]
        return len(self.val_img_idx)

    def __getitem__(self, idx):
        """val: one full image, the reference's dict (phototourism.py:456-470).  The train split is read in batches
        through GpuRaySampler.from_dataset(ds), not per ray."""
        if self.split != "val":
            raise TypeError("the train split's rays are sampled on the device: use GpuRaySampler.from_dataset(ds)")
        ri = self.ray_infos[idx]
        img_idx = ri[:, 2].long()
        id_ = self.img_ids_train[self.val_img_idx[idx]]
        return {"rgbs": self.rgbs[idx], "ray_infos": ri[:, :2].contiguous(), "directions": self.directions[idx],
                "img_idx": img_idx, "img_wh": self.imgs_wh[idx],
                "c2w": torch.as_tensor(np.asarray(self.poses_dict[id_]), dtype=torch.float32).to(self.device),
                "feats": self.feats[idx], "pca_m": self.pca_m[idx], "pca_c": self.pca_c[idx],
                "inv_depths": self.inv_depths[idx]}


class PhototourismDataset(_SceneDataset):
    custom = False


class CustomDataset(_SceneDataset):
    custom = True


class _OptimizeDataset:
    """phototourism_optimize.py / custom_optimize.py: one held-out image (`optimize_num` into the test ids) for test-time
    optimisation.  With pose_optimize the whole image is the train and the val split; otherwise the train split is the
    left half (columns [0, W // 2)) and the val split the right half ([W // 2, W)).  No feature or depth maps."""
    custom = False

    def __init__(self, root_dir, scene_name, near=0.0, far=5.0, camera_noise=-1, split="train", img_downscale=1,
                 use_cache=False, pose_optimize=True, optimize_num=None, device="cuda"):
        self.root_dir, self.scene_name = root_dir, scene_name
        self.near, self.far = near, far
        self.camera_noise = camera_noise
        self.split = split
        self.img_downscale = max(2, img_downscale) if split == "val" else img_downscale
        self.use_cache = use_cache  # accepted, ignored
        self.pose_optimize, self.optimize_num = pose_optimize, optimize_num
        self.device = torch.device(device)
        self.white_back = False
        if split not in ("train", "val"):
            raise NotImplementedError(f"split {split!r}: only train and val are provided")
        timer = _Timer(self.device)
        m = custom_meta(root_dir, self.img_downscale) if self.custom else phototourism_meta(root_dir, scene_name,
                                                                                              self.img_downscale)
        self.meta = m
        self.img_ids, self.image_paths, self.Ks = m.img_ids, m.image_paths, m.Ks
        self.nears, self.fars, self.xyz_world = m.nears, m.fars, m.xyz_world
        self.img_ids_train, self.img_ids_test = m.img_ids_train, m.img_ids_test
        self.N_images_train, self.N_images_test = len(m.img_ids_train), len(m.img_ids_test)
        if self.custom and not m.poses_dict:
            raise ValueError("test-time optimisation needs ground-truth poses (c2w in metadata.json)")
        self.GT_poses_dict = m.poses_dict
        self.poses_dict = {id_: torch.eye(3, 4) for id_ in m.img_ids_test}
        self.ray_img_ids = m.img_ids_test  # all_ray_infos[:, 2] indexes the test images (GpuRaySampler.from_dataset)
        timer.lap("metadata")
        id_ = m.img_ids_test[optimize_num]
        img = decode_image(os.path.join(m.image_root, self.image_paths[id_]), self.img_downscale)
        timer.lap("decode")
        pixels, offs = upload_pixels([img], self.device)
        timer.lap("upload", sync=True)
        H, W = img.shape[:2]
        if pose_optimize:
            x0, x1 = 0, W
        else:
            x0, x1 = (0, W // 2) if split == "train" else (W // 2, W)
        self.all_imgs_wh = [x1 - x0, H]
        b = scene_rays([dict(W=W, H=H, x0=x0, x1=x1, K=self.Ks[id_], near=near, far=far, img_idx=optimize_num)], pixels,
                       offs, self.device, pxl=False)
        self.all_directions, self.all_ray_infos, self.all_rgbs = b["directions"], b["ray_infos"], b["rgbs"]
        timer.lap("kernels", sync=True)
        self.load_times = timer.done()

    def __len__(self):
        return self.all_ray_infos.shape[0] if self.split == "train" else 1

    def __getitem__(self, idx):
        """val: the whole held-out window as one item (phototourism_optimize.py:266-276)."""
        if self.split != "val":
            raise TypeError("the train split's rays are sampled on the device: use GpuRaySampler.from_dataset(ds)")
        img_idx = self.all_ray_infos[:, 2].long()
        id_ = self.img_ids_test[self.optimize_num]
        return {"ray_infos": self.all_ray_infos[:, :2].contiguous(), "directions": self.all_directions, "img_idx": img_idx,
                "c2w": torch.as_tensor(np.asarray(self.poses_dict[id_]), dtype=torch.float32).to(self.device),
                "rgbs": self.all_rgbs, "img_wh": torch.LongTensor(self.all_imgs_wh)}


class PhototourismOptimizeDataset(_OptimizeDataset):
    custom = False


class CustomOptimizeDataset(_OptimizeDataset):
    custom = True


dataset_dict = {
    "phototourism": PhototourismDataset,
    "phototourism_optimize": PhototourismOptimizeDataset,
    "custom": CustomDataset,
    "custom_optimize": CustomOptimizeDataset,
}
