"""Synthetic scenes on disk for the scene-loading tests and tools/bench_scene_load.py: COLMAP binaries packed with
`struct` from COLMAP's documented layout, a tsv split, JPEG images, DINO-like feature maps, PCA infos and DPT-like
depth maps, in the reference's directory layout (root/<scene>.tsv, root/dense/{images,sparse}, <feat_dir>/feature_maps,
<feat_dir>/pca_infos, <depth_dir>)."""
import json
import os
import struct

import numpy as np


def pack_cameras(cams):
    """cams: (camera_id, model_id, width, height, params)."""
    b = struct.pack("<Q", len(cams))
    for cid, model, w, h, params in cams:
        b += struct.pack("<iiQQ", cid, model, w, h) + struct.pack("<%dd" % len(params), *params)
    return b


def pack_images(images):
    """images: (image_id, qvec[4], tvec[3], camera_id, name, points2D [(x, y, point3D_id)])."""
    b = struct.pack("<Q", len(images))
    for iid, q, t, cid, name, pts in images:
        b += struct.pack("<i4d3di", iid, *q, *t, cid) + name.encode() + b"\0" + struct.pack("<Q", len(pts))
        for x, y, pid in pts:
            b += struct.pack("<ddq", x, y, pid)
    return b


def pack_points(points):
    """points: (point3D_id, xyz[3], rgb[3], error, track [(image_id, point2D_idx)])."""
    b = struct.pack("<Q", len(points))
    for pid, xyz, rgb, err, track in points:
        b += struct.pack("<Q3d3BdQ", pid, *xyz, *rgb, err, len(track))
        for iid, k in track:
            b += struct.pack("<ii", iid, k)
    return b


def qvec_y(theta):
    """Unit quaternion (w, x, y, z) of a rotation by theta about the y axis."""
    return (np.cos(theta / 2), 0.0, np.sin(theta / 2), 0.0)


def write_phototourism_scene(root, scene="synth", n_images=4, size=(40, 30), splits=None, feat_hw=8, feat_dim=384,
                             n_points=200, seed=0, images=True, id_base=10, quality=95):
    """A scene of n_images cameras around the origin looking at a point cloud; image ids start at id_base and are
    listed in the tsv in reverse id order (the tsv `id` column holds wrong values, as in the real files), plus one row
    with an empty id.  Returns a dict of what was written."""
    rng = np.random.default_rng(seed)
    W, H = size
    splits = splits or ["train"] * (n_images - 1) + ["test"]
    os.makedirs(os.path.join(root, "dense", "sparse"), exist_ok=True)
    os.makedirs(os.path.join(root, "dense", "images"), exist_ok=True)
    ids = [id_base + k for k in range(n_images)]
    names = [f"img_{k:03d}.jpg" for k in range(n_images)]
    cams, ims = [], []
    for k, iid in enumerate(ids):
        fx = 0.9 * W + k
        cams.append((iid, 1, W, H, (fx, fx * 1.01, W / 2, H / 2)))
        ims.append((iid, qvec_y(0.3 * k - 0.4), (0.1 * k, -0.05, 4.0 + 0.2 * k), iid, names[k], [(1.0, 2.0, -1)]))
    pts = [(p + 1, tuple(rng.uniform(-1, 1, 3)), (1, 2, 3), 0.5, [(ids[0], 0)]) for p in range(n_points)]
    with open(os.path.join(root, "dense", "sparse", "cameras.bin"), "wb") as f:
        f.write(pack_cameras(cams))
    with open(os.path.join(root, "dense", "sparse", "images.bin"), "wb") as f:
        f.write(pack_images(ims))
    with open(os.path.join(root, "dense", "sparse", "points3D.bin"), "wb") as f:
        f.write(pack_points(pts))
    order = list(range(n_images))[::-1]
    with open(os.path.join(root, f"{scene}.tsv"), "w") as f:
        f.write("filename\tid\tsplit\tdataset\n")
        for j, k in enumerate(order):
            f.write(f"{names[k]}\t{900 + j}\t{splits[k]}\t{scene}\n")
        f.write(f"unlisted.jpg\t\ttrain\t{scene}\n")
    feat_dir, depth_dir = os.path.join(root, "DINO"), os.path.join(root, "DPT")
    for d in (os.path.join(feat_dir, "feature_maps"), os.path.join(feat_dir, "pca_infos"), depth_dir):
        os.makedirs(d, exist_ok=True)
    for k in range(n_images):
        stem = names[k][:-4]
        np.save(os.path.join(feat_dir, "feature_maps", stem + ".npy"),
                rng.standard_normal((feat_hw, feat_hw, feat_dim)).astype(np.float32))
        np.save(os.path.join(feat_dir, "pca_infos", stem + "_mean.npy"), rng.standard_normal(feat_dim).astype(np.float32))
        np.save(os.path.join(feat_dir, "pca_infos", stem + "_components.npy"),
                rng.standard_normal((3, feat_dim)).astype(np.float32))
        np.save(os.path.join(depth_dir, stem + ".npy"), (rng.uniform(-0.2, 3.0, (H, W))).astype(np.float32))
        if images:
            from PIL import Image
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(
                os.path.join(root, "dense", "images", names[k]), quality=quality)
    return {"root": root, "scene": scene, "ids": ids, "names": names, "cams": cams, "images": ims,
            "xyz": np.array([p[1] for p in pts]), "splits": splits, "tsv_order": order, "feat_dir": feat_dir,
            "depth_dir": depth_dir}


def write_custom_scene(root, sizes=((41, 31), (40, 30), (39, 29)), splits=("train", "train", "test"), focal=50.0,
                       seed=0):
    """The layout of the reference's data/example: metadata.json {id: {name, focal, split, c2w}}, images under
    dense/images."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "dense", "images"), exist_ok=True)
    meta = {}
    for k, ((w, h), sp) in enumerate(zip(sizes, splits)):
        name = f"dense/images/{k + 1:03d}.jpg"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(root, name))
        c2w = np.eye(4)
        c2w[:3, 3] = (0.1 * k, 0.2, 3.0)
        meta[str(k)] = {"name": name, "focal": focal + k, "split": sp, "c2w": c2w.tolist()}
    with open(os.path.join(root, "metadata.json"), "w") as f:
        json.dump(meta, f)
    return meta
