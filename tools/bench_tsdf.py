"""Depth-map fusion on synthetic inputs (upnerf_amd/geometry.py TsdfVolume / fuse_views, csrc/tsdf.hip): one
launch of upnerf_tsdf_integrate with a full batch of views, the bytes it has to move, a plain device copy of as many bytes in
the same process (the method of tools/hbm_probe.py), and what rendering the depth map of a view costs beside it.

    python tools/bench_tsdf.py [--resolution 256] [--image 400 300] [--repeats 5] [--out profiles/tsdf_fuse.json]

The launch is timed by device events (ops.TIMER); bytes are the compulsory traffic computed from the shapes (`integrate_bytes`).
The render time per view is a host clock round fuse_views on the benchmark's synthetic system (synchronised), less its
integrate launches, divided by the views.  Prints the JSON it writes."""
import argparse
import datetime
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def integrate_bytes(N, views, pixels, colour=True):
    """Compulsory traffic of one launch: tsdf and weight (and rgb [3] and its weight) read and written once per voxel, whatever
    the number of views, plus every map (depth, opacity, rgb [3]) read once -- cached re-reads of a pixel by the voxels along
    its ray are not counted."""
    per_voxel = (2 + (4 if colour else 0)) * 4 * 2
    return N * per_voxel + views * pixels * (2 + (3 if colour else 0)) * 4


def ring_poses(n, radius, device):
    """[n, 3, 4] poses on a circle round the origin in the xz plane, looking at it (a camera looks down its -z axis)."""
    ang = torch.arange(n, dtype=torch.float32) * (2 * math.pi / n)
    c2w = torch.zeros(n, 3, 4)
    c2w[:, 0, 0] = c2w[:, 2, 2] = torch.cos(ang)
    c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 1, 1] = torch.sin(ang), -torch.sin(ang), 1.0
    c2w[:, :, 3] = radius * c2w[:, :, 2]
    return c2w.to(device)


def sphere_depth(c2w, wh, intr, radius):
    """[H * W] distance along the unit ray of every pixel to the sphere round the origin, NaN where it misses (torch, fp32)."""
    W, H = wh
    fx, fy, cx, cy = intr
    j, i = torch.meshgrid(torch.arange(H, device=c2w.device, dtype=torch.float32), torch.arange(W, device=c2w.device, dtype=torch.float32),
                          indexing="ij")
    d = torch.nn.functional.normalize(torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1).reshape(-1, 3), dim=1)
    d = d @ c2w[:, :3].T
    o = c2w[:, 3]
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    return torch.where(disc > 0, -b - disc.clamp_min(0).sqrt(), torch.full_like(b, float("nan"))).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--image", type=int, nargs=2, default=[400, 300], metavar=("W", "H"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_fuse.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf.py measures on the GPU; none is visible")
    import numpy as np
    import bench
    from upnerf_amd import _lib, geometry
    from upnerf_amd.ops import TIMER
    dev = torch.device("cuda", 0)
    n, (W, H) = a.resolution, a.image
    res, bounds = (n, n, n), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    N, views = n ** 3, _lib.TSDF_MAX_VIEWS
    intr = (0.65 * W, 0.65 * W, (W - 1) / 2, (H - 1) / 2)
    cell = (3 * (2.0 / (n - 1)) ** 2) ** 0.5

    # ---- one launch with a full batch of views: a sphere seen from a ring of cameras, colour and opacity maps present
    poses = ring_poses(views, 2.5, dev)
    depth = [sphere_depth(poses[k], (W, H), intr, 0.8) for k in range(views)]
    rgb = [torch.rand(W * H, 3, device=dev) for _ in range(views)]
    opacity = [torch.ones(W * H, device=dev) for _ in range(views)]
    vol = geometry.TsdfVolume(bounds, res, 3 * cell)
    fold = lambda: vol.integrate(depth, poses, intr, (W, H), rgb=rgb, opacity=opacity)
    fold()  # warm-up
    torch.cuda.synchronize()
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, {"tsdf_integrate"}
    for _ in range(a.repeats):
        fold()
    s = TIMER.summary()["tsdf_integrate"]
    TIMER.enabled, TIMER.only = False, None
    byts = integrate_bytes(N, views, W * H)
    launch = {"views": views, "image": [W, H], "launches": s["launches"], "ms": s["avg_ms"], "bytes": byts,
              "GB_per_s": byts / (s["avg_ms"] * 1e-3) / 1e9, "voxels_per_s": N / (s["avg_ms"] * 1e-3),
              "observed_share": float((vol.weight > 0).float().mean())}
    t0 = time.perf_counter()
    mesh = vol.extract()
    torch.cuda.synchronize()
    extract = {"ms": (time.perf_counter() - t0) * 1e3, "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0])}
    del mesh, vol

    # ---- a device copy of the same number of bytes (read + write), same process
    x = torch.empty(byts // 8, device=dev, dtype=torch.float32).normal_()
    y = torch.empty_like(x)
    y.copy_(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.repeats):
        y.copy_(x)
    torch.cuda.synchronize()
    t_copy = (time.perf_counter() - t0) / a.repeats
    copy = {"bytes": 2 * x.numel() * 4, "ms": t_copy * 1e3, "GB_per_s": 2 * x.numel() * 4 / t_copy / 1e9}
    del x, y

    # ---- what the depth renders cost beside it: fuse_views on the benchmark's system, the ring as its training cameras
    sysm = bench.build_system(dev, 0.8)
    ds = sysm.train_dataset
    n_img = sysm.se3_refine.weight.shape[0]
    ds.poses = ring_poses(views, 2.5, "cpu")[torch.arange(n_img) % views]
    ds.Ks = [np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1]])] * n_img
    ds.all_imgs_wh = torch.tensor([[W, H]] * n_img)
    ids = list(range(views))
    geometry.fuse_views(sysm, bounds, res, img_ids=ids[:1])  # warm-up
    torch.cuda.synchronize()
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, {"tsdf_integrate"}
    t0 = time.perf_counter()
    geometry.fuse_views(sysm, bounds, res, img_ids=ids)
    torch.cuda.synchronize()
    t_fuse = time.perf_counter() - t0
    s = TIMER.summary()["tsdf_integrate"]
    TIMER.enabled, TIMER.only = False, None
    hp = sysm.hparams
    fuse = {"views": views, "call_ms": t_fuse * 1e3, "integrate_launches": s["launches"], "integrate_ms": s["total_ms"],
            "render_ms_per_view": (t_fuse * 1e3 - s["total_ms"]) / views, "rays_per_view": W * H,
            "samples_per_ray": hp["nerf.N_samples"] + hp["nerf.N_importance"], "chunk": hp["val.chunk_size"]}

    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "resolution": list(res),
           "bounds": [list(bounds[0]), list(bounds[1])], "trunc": 3 * cell, "repeats": a.repeats, "integrate_launch": launch,
           "copy": copy, "extract": extract, "fuse_views": fuse, "peak_hbm_gb": torch.cuda.max_memory_allocated() / 2 ** 30}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
