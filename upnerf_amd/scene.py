"""Scene metadata on the host: what datasets/phototourism.py:63-212 and datasets/custom.py:62-140 of the reference compute
before any pixel is touched -- image ids and file names, intrinsics, camera-to-world poses, per-image near / far bounds,
the train / test split and the initial (noised or identity) training poses.  Pure numpy / torch CPU; nothing here needs
the GPU except drawing new pose noise (the package's se(3) exponential is the HIP pose kernel).

The COLMAP readers follow COLMAP's documented binary layout (little-endian):
  cameras.bin   u64 n; n x { i32 camera_id, i32 model_id, u64 width, u64 height, f64 params[n_params(model)] }
  images.bin    u64 n; n x { i32 image_id, f64 qvec[4] (w, x, y, z), f64 tvec[3], i32 camera_id, NUL-terminated name,
                             u64 n_points2D, n_points2D x { f64 x, f64 y, i64 point3D_id } }
  points3D.bin  u64 n; n x { u64 point3D_id, f64 xyz[3], u8 rgb[3], f64 error, u64 track_length,
                             track_length x { i32 image_id, i32 point2D_idx } }
Only the fields the datasets use are kept.  A file that ends inside a record raises ValueError.

Quirks of the reference that are kept on purpose:
  * intrinsics are looked up by the IMAGE id (cameras.bin ids equal image ids in the phototourism reconstructions);
  * the full image size is (int(2 cx), int(2 cy)), not the camera's width / height fields;
  * max_far goes through float32 before scale_factor = max_far / 5;
  * the tsv's own `id` column is only used to drop rows where it is empty."""
from __future__ import annotations

import csv
import json
import os
import struct
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

# model id -> number of parameters (COLMAP's camera models)
CAMERA_MODEL_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 6: 12, 7: 5, 8: 4, 9: 5, 10: 12}
# the strings pandas.read_csv reads as a missing value by default (the reference drops rows whose id is one of them)
_NA = {"", "#N/A", "#N/A N/A", "#NA", "-1.#IND", "-1.#QNAN", "-NaN", "-nan", "1.#IND", "1.#QNAN", "<NA>", "N/A", "NA",
       "NULL", "NaN", "None", "n/a", "nan", "null"}


class Camera(NamedTuple):
    id: int
    model_id: int
    width: int
    height: int
    params: np.ndarray


class ImageMeta(NamedTuple):
    id: int
    qvec: np.ndarray
    tvec: np.ndarray
    camera_id: int
    name: str


class _Reader:
    def __init__(self, path: str):
        with open(path, "rb") as f:
            self.buf = f.read()
        self.path, self.pos = path, 0

    def take(self, fmt: str):
        n = struct.calcsize("<" + fmt)
        if self.pos + n > len(self.buf):
            raise ValueError(f"{self.path}: truncated (needs {self.pos + n} bytes, has {len(self.buf)})")
        out = struct.unpack_from("<" + fmt, self.buf, self.pos)
        self.pos += n
        return out

    def skip(self, n: int):
        if self.pos + n > len(self.buf):
            raise ValueError(f"{self.path}: truncated (needs {self.pos + n} bytes, has {len(self.buf)})")
        self.pos += n

    def cstring(self) -> str:
        end = self.buf.find(b"\0", self.pos)
        if end < 0:
            raise ValueError(f"{self.path}: truncated (image name without its terminating NUL)")
        s = self.buf[self.pos:end].decode("utf-8")
        self.pos = end + 1
        return s


def read_cameras_binary(path: str) -> Dict[int, Camera]:
    r = _Reader(path)
    (n,) = r.take("Q")
    cams = {}
    for _ in range(n):
        cid, model, width, height = r.take("iiQQ")
        if model not in CAMERA_MODEL_PARAMS:
            raise ValueError(f"{path}: unknown camera model id {model}")
        params = np.array(r.take("d" * CAMERA_MODEL_PARAMS[model]), dtype=np.float64)
        cams[cid] = Camera(cid, model, width, height, params)
    return cams


def read_images_binary(path: str) -> Dict[int, ImageMeta]:
    r = _Reader(path)
    (n,) = r.take("Q")
    images = {}
    for _ in range(n):
        vals = r.take("i7di")
        name = r.cstring()
        (n2d,) = r.take("Q")
        r.skip(24 * n2d)  # (x, y, point3D_id) per 2-D point: not used
        images[vals[0]] = ImageMeta(vals[0], np.array(vals[1:5]), np.array(vals[5:8]), vals[8], name)
    return images


def read_points3d_binary(path: str) -> np.ndarray:
    """xyz of every point, [N, 3] float64, in file order."""
    r = _Reader(path)
    (n,) = r.take("Q")
    xyz = np.empty((n, 3), dtype=np.float64)
    for k in range(n):
        vals = r.take("Q3d3BdQ")
        xyz[k] = vals[1:4]
        r.skip(8 * vals[-1])  # track: (image_id, point2D_idx) pairs
    return xyz


def qvec2rotmat(q) -> np.ndarray:
    """Rotation matrix of a unit quaternion (w, x, y, z), COLMAP's convention."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def read_tsv(path: str) -> List[dict]:
    """Rows of `<scene>.tsv` (tab-separated, header line) whose `id` is not empty, in file order."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f, delimiter="\t"))
    for k in ("filename", "id", "split"):
        if rows and k not in rows[0]:
            raise ValueError(f"{path}: no '{k}' column")
    return [r for r in rows if (r.get("id") or "").strip() not in _NA]


def scaled_K(params, scale: int) -> np.ndarray:
    """phototourism.py:100-111: fx, fy, cx, cy of a full image of (int(2 cx), int(2 cy)) pixels, rescaled to the
    integer-divided size."""
    if len(params) < 4:
        raise ValueError("the phototourism intrinsics need (fx, fy, cx, cy): a PINHOLE camera")
    img_w, img_h = int(params[2] * 2), int(params[3] * 2)
    img_w_, img_h_ = img_w // scale, img_h // scale
    K = np.zeros((3, 3), dtype=np.float32)
    K[0, 0] = params[0] * img_w_ / img_w
    K[1, 1] = params[1] * img_h_ / img_h
    K[0, 2] = params[2] * img_w_ / img_w
    K[1, 2] = params[3] * img_h_ / img_h
    K[2, 2] = 1
    return K


def w2c_matrix(im: ImageMeta) -> np.ndarray:
    return np.concatenate([np.concatenate([qvec2rotmat(im.qvec), im.tvec.reshape(3, 1)], 1),
                           np.array([[0, 0, 0, 1.0]])], 0)


def c2w_from_w2c(w2c: np.ndarray) -> np.ndarray:
    """[N,4,4] world-to-camera -> [N,3,4] camera-to-world with the axes turned from (right, down, front) to
    (right, up, back)."""
    poses = np.linalg.inv(w2c)[:, :3]
    poses[..., 1:3] *= -1
    return poses


def near_far(xyz_world: np.ndarray, w2c: np.ndarray):
    """0.1 / 99.9 percentiles of the camera-space depth of the points in front of camera w2c."""
    xyz_h = np.concatenate([xyz_world, np.ones((len(xyz_world), 1))], -1)
    z = (xyz_h @ w2c.T)[:, 2]
    z = z[z > 0]
    return np.percentile(z, 0.1), np.percentile(z, 99.9)


class SceneMeta:
    """Everything a dataset reads from a scene's metadata.  Attribute names are the reference datasets' own."""
    img_ids: list
    image_paths: dict      # id -> path relative to the image root
    image_root: str
    Ks: dict               # id -> float32 [3,3] for the requested downscale
    poses_dict: dict       # id -> [3,4] ground-truth camera-to-world (float64 numpy)
    nears: dict
    fars: dict
    img_ids_train: list
    img_ids_test: list
    xyz_world: np.ndarray
    scale_factor: Optional[float] = None

    def feature_name(self, id_) -> str:
        return os.path.basename(self.image_paths[id_]).replace(".jpg", ".npy")


def phototourism_meta(root_dir: str, scene_name: str, scale: int) -> SceneMeta:
    m = SceneMeta()
    rows = read_tsv(os.path.join(root_dir, f"{scene_name}.tsv"))
    imdata = read_images_binary(os.path.join(root_dir, "dense/sparse/images.bin"))
    by_name = {v.name: v.id for v in imdata.values()}
    m.img_ids, m.image_paths = [], {}
    for r in rows:
        if r["filename"] not in by_name:
            raise ValueError(f"{r['filename']} (in {scene_name}.tsv) is not in images.bin")
        id_ = by_name[r["filename"]]
        m.image_paths[id_] = r["filename"]
        m.img_ids.append(id_)
    m.image_root = os.path.join(root_dir, "dense/images")
    camdata = read_cameras_binary(os.path.join(root_dir, "dense/sparse/cameras.bin"))
    m.Ks = {id_: scaled_K(camdata[id_].params, scale) for id_ in m.img_ids}
    w2c = np.stack([w2c_matrix(imdata[id_]) for id_ in m.img_ids], 0)
    poses = c2w_from_w2c(w2c)
    m.xyz_world = read_points3d_binary(os.path.join(root_dir, "dense/sparse/points3D.bin"))
    m.nears, m.fars = {}, {}
    for i, id_ in enumerate(m.img_ids):
        m.nears[id_], m.fars[id_] = near_far(m.xyz_world, w2c[i])
    max_far = np.fromiter(m.fars.values(), np.float32).max()
    m.scale_factor = max_far / 5  # float32, as in the reference
    poses[..., 3] /= m.scale_factor
    for k in m.nears:
        m.nears[k] /= m.scale_factor
        m.fars[k] /= m.scale_factor
    m.xyz_world /= m.scale_factor
    m.poses_dict = {id_: poses[i] for i, id_ in enumerate(m.img_ids)}
    m.img_ids_train = [id_ for id_, r in zip(m.img_ids, rows) if r["split"] == "train"]
    m.img_ids_test = [id_ for id_, r in zip(m.img_ids, rows) if r["split"] == "test"]
    return m


def image_size(path: str):
    """(width, height) from the image file's header (PIL reads no pixels for this)."""
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def custom_meta(root_dir: str, scale: int) -> SceneMeta:
    """datasets/custom.py:62-140: `metadata.json` maps an id to {name, focal, split[, c2w]}; cx, cy are the half image
    size read from the file; no point cloud, so no per-image bounds."""
    with open(os.path.join(root_dir, "metadata.json")) as f:
        meta = json.load(f)
    m = SceneMeta()
    m.image_root = root_dir
    m.img_ids = list(meta)
    m.image_paths = {id_: v["name"] for id_, v in meta.items()}
    m.Ks = {}
    for id_, v in meta.items():
        width, height = image_size(os.path.join(root_dir, v["name"]))
        K = np.zeros((3, 3), dtype=np.float32)
        K[0, 0] = v["focal"] / scale
        K[1, 1] = v["focal"] / scale
        K[0, 2] = (width / 2) / scale
        K[1, 2] = (height / 2) / scale
        K[2, 2] = 1
        m.Ks[id_] = K
    if all("c2w" in v for v in meta.values()) and meta:
        poses = np.stack([np.asarray(v["c2w"], dtype=np.float64) for v in meta.values()], 0)
        m.poses_dict = {id_: poses[i] for i, id_ in enumerate(m.img_ids)}
    else:
        m.poses_dict = {}
    m.nears, m.fars, m.xyz_world = {}, {}, np.array([])
    m.img_ids_train, m.img_ids_test = [], []
    for id_, v in meta.items():
        if v["split"] == "train":
            m.img_ids_train.append(id_)
        elif v["split"] == "test":
            m.img_ids_test.append(id_)
        else:
            raise ValueError(f"metadata.json: image {id_} has split {v['split']!r} (train or test expected)")
    return m


def compose_pair(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """utils/camera.py compose_pair: apply pose a, then pose b ([..., 3, 4])."""
    Ra, ta, Rb, tb = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return torch.cat([Rb @ Ra, Rb @ ta + tb], -1)


def initial_train_poses(meta: SceneMeta, camera_noise, device="cuda", noise_dir: str = "noises"):
    """phototourism.py:178-211: (poses_dict, GT_poses_dict, pose_noises) for the training images.
    camera_noise None: the ground truth, unchanged.  Otherwise GT_poses_dict keeps the ground truth and poses_dict holds
    `<noise_dir>/<N>_<noise>.pt` composed onto it when that file exists; torch.eye(3, 4) when the noise is -1; or a
    fresh draw randn(N, 6) * noise through the se(3) exponential, composed onto it (not written to disk)."""
    if camera_noise is None:
        return dict(meta.poses_dict), dict(meta.poses_dict), None
    ids = meta.img_ids_train
    poses = torch.as_tensor(np.stack([meta.poses_dict[i] for i in ids], 0), dtype=torch.float32) if ids else None
    gt = meta.poses_dict
    path = os.path.join(noise_dir, f"{len(ids)}_{camera_noise}.pt")
    if os.path.isfile(path):
        noises = torch.load(path, map_location="cpu")
        composed = compose_pair(noises.float(), poses)
        return {id_: composed[i] for i, id_ in enumerate(ids)}, gt, noises
    if camera_noise == -1:
        return {id_: torch.eye(3, 4) for id_ in ids}, gt, None
    from .pose_align import refined_poses
    se3 = torch.randn(len(ids), 6) * camera_noise
    dev_se3 = se3.to(device)
    noises = refined_poses(dev_se3, torch.eye(3, 4).repeat(len(ids), 1, 1).to(device)).cpu()
    composed = refined_poses(dev_se3, poses.to(device)).cpu()
    return {id_: composed[i] for i, id_ in enumerate(ids)}, gt, noises
