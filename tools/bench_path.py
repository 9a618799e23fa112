"""Render rate of camera-path frames (upnerf_amd/novel_view.py) on a synthetic system, and the share of the frame time the path
front end (`upnerf_path_rays`) takes beside the field kernels.

    python tools/bench_path.py [--frames 8] [--width 200] [--height 200] [--keys 4] [--chunk 16384] [--progress 0.8]
                               [--images 763] [--reps 3] [--occupancy NX NY NZ --level L [--dilate K] [--out FILE]]

The system is bench.py's (two 8 x 256 fields, 64 + 128 samples, 763 images, seeded weights).  One warm-up render, then `--reps`
timed renders of the whole sequence (wall clock around a device synchronisation); a further render with the KernelTimer on gives
HIP-event times per kernel class, from which `path_rays_share` = time in upnerf_path_rays / sum of the timed kernel classes.
A `validation_step` over the same number of rays (same chunk) is timed in the same run for comparison.  One JSON line.

With --occupancy the run measures empty-space skipping instead (upnerf_amd/occupancy.py) and writes
profiles/path_occupancy.json (--out): the same system and path rendered without a grid, with the grid of the field's density at
--level, and with an ALL-FULL grid (every ray hits: the pure overhead of the three kernels), in alternating runs of one process
(`--reps` rounds of none / grid / full, the median of each).  Every rate stands next to its hit share: a random-weight field has
an arbitrary one, so no ratio means anything without it.  The box is [-2.5, 2.5]^2 x [-5.5, 0.5], in front of the cameras."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def occupancy_run(a, sysm, path, rays):
    from upnerf_amd import novel_view
    from upnerf_amd.geometry import density_grid
    from upnerf_amd.novel_view import render_path
    from upnerf_amd.occupancy import OccupancyGrid
    from upnerf_amd.ops import TIMER
    bounds = ((-2.5, -2.5, -5.5), (2.5, 2.5, 0.5))
    res = tuple(a.occupancy)
    grid = density_grid(sysm, bounds, res)
    OccupancyGrid.from_density(grid, bounds, a.level, dilate=a.dilate)  # warm-up of the build
    build_s = wall(lambda: OccupancyGrid.from_density(grid, bounds, a.level, dilate=a.dilate), a.reps)
    grid_s = wall(lambda: density_grid(sysm, bounds, res), 1)
    occs = {"none": None, "grid": OccupancyGrid.from_density(grid, bounds, a.level, dilate=a.dilate),
            "full": OccupancyGrid.from_cells(torch.ones(res[2] - 1, res[1] - 1, res[0] - 1, dtype=torch.bool, device=grid.device), bounds)}
    times = {k: [] for k in occs}
    share = {}
    for k, o in occs.items():  # warm-up of every variant
        render_path(sysm, path, outputs=("rgb",), occupancy=o)
        share[k] = novel_view.LAST_STATS["hits"] / rays if o is not None else 1.0
    for _ in range(a.reps):  # alternating: a drift of the clocks touches every variant alike
        for k, o in occs.items():
            times[k].append(wall(lambda: render_path(sysm, path, outputs=("rgb",), occupancy=o), 1))
    kern = {}
    for k in ("grid", "full"):
        TIMER.reset()
        TIMER.enabled, TIMER.only = True, {"occ_spans", "occ_compact", "occ_scatter"}
        render_path(sysm, path, outputs=("rgb",), occupancy=occs[k])
        kern[k] = {n: {"ms_per_launch": v["avg_ms"], "launches": v["launches"], "rays_per_launch": v["units_per_launch"]}
                   for n, v in sorted(TIMER.summary().items())}
        TIMER.enabled, TIMER.only = False, None
        TIMER.reset()
    F = path.n_frames
    runs = {}
    for k, ts in times.items():
        dt = statistics.median(ts)
        runs[k] = {"frames_per_s": F / dt, "rays_per_s": rays / dt, "hit_share": share[k], "seconds": sorted(ts)}
    out = {"metric": "camera-path frames with and without an occupancy grid (render_path, rgb output, no grad; random weights)",
           "frames": F, "img_wh": list(path.img_wh), "chunk": a.chunk, "progress": a.progress, "reps": a.reps,
           "resolution": list(res), "level": a.level, "dilate": a.dilate, "bounds": [list(b) for b in bounds],
           "occupied_share": occs["grid"].fraction, "sigma_min": float(grid.min()), "sigma_max": float(grid.max()),
           "runs": runs, "overhead_full_vs_none": runs["none"]["rays_per_s"] / runs["full"]["rays_per_s"] - 1.0,
           "kernels": kern, "build_ms": build_s * 1e3, "density_grid_s": grid_s}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=200)
    ap.add_argument("--height", type=int, default=200)
    ap.add_argument("--keys", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--progress", type=float, default=0.8)
    ap.add_argument("--images", type=int, default=763)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--occupancy", type=int, nargs=3, metavar=("NX", "NY", "NZ"), help="grid points of the occupancy grid")
    ap.add_argument("--level", type=float, default=None, help="density above which a cell is kept (required with --occupancy)")
    ap.add_argument("--dilate", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_occupancy.json"))
    a = ap.parse_args()
    if a.occupancy is not None and a.level is None:
        raise SystemExit("--occupancy needs --level")
    if not torch.cuda.is_available():
        raise SystemExit("bench_path.py measures on the GPU; none is visible")
    import bench
    from upnerf_amd import synth
    from upnerf_amd.novel_view import CameraPath, render_path
    from upnerf_amd.ops import TIMER
    dev = torch.device("cuda", 0)
    sysm = bench.build_system(dev, a.progress, n_images=a.images)
    sysm.hparams["val.chunk_size"] = a.chunk
    W, H, F = a.width, a.height, a.frames
    # keyframes on a small arc around the origin, looking down -z
    ang = torch.linspace(-0.3, 0.3, a.keys)
    c2w = torch.zeros(a.keys, 3, 4)
    c2w[:, 0, 0] = c2w[:, 2, 2] = torch.cos(ang)
    c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 1, 1] = torch.sin(ang), -torch.sin(ang), 1.0
    c2w[:, :, 3] = torch.stack([0.2 * torch.sin(ang), torch.zeros(a.keys), 0.2 * (1 - torch.cos(ang))], 1)
    K = torch.tensor([[0.8 * W, 0, W / 2], [0, 0.8 * W, H / 2], [0, 0, 1.0]])
    path = CameraPath.from_poses(c2w, (0.1, 5.0), F, appearance=(3, 17), img_wh=(W, H), K=K)
    rays = F * H * W
    if a.occupancy is not None:
        return occupancy_run(a, sysm, path, rays)
    render_path(sysm, path, outputs=("rgb",))  # warm-up (allocator growth, cached tables)
    dt = wall(lambda: render_path(sysm, path, outputs=("rgb",)), a.reps)
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, None
    render_path(sysm, path, outputs=("rgb",))
    kern = TIMER.summary()
    TIMER.enabled = False
    TIMER.reset()
    total_ms = sum(v["total_ms"] for v in kern.values())
    pr = kern.get("path_rays", {"total_ms": 0.0, "launches": 0, "avg_ms": 0.0})
    # the same number of rays through validation_step (dataset-style batch: stored directions, gathered rows, TransientNet, loss)
    b = synth.batch(rays, a.images, seed=7)
    b["img_idx"] = torch.full_like(b["img_idx"], 3)
    batch = {k: v.to(dev)[None] for k, v in b.items()}
    sysm.validation_step(batch)
    dv = wall(lambda: sysm.validation_step(batch), a.reps)
    print(json.dumps({
        "metric": "camera-path frames (render_path, rgb output, no grad)", "frames_per_s": F / dt, "rays_per_s": rays / dt,
        "ms_per_frame": dt / F * 1e3, "frames": F, "img_wh": [W, H], "keys": a.keys, "chunk": a.chunk, "progress": a.progress,
        "path_rays_share": pr["total_ms"] / total_ms if total_ms else None, "path_rays_ms_per_launch": pr["avg_ms"],
        "path_rays_launches": pr["launches"],
        "kernels_ms": {k: round(v["total_ms"], 4) for k, v in sorted(kern.items())},
        "validation_step_rays_per_s": rays / dv, "ratio_to_validation_step": (rays / dt) / (rays / dv),
        "peak_hbm_gb": torch.cuda.max_memory_allocated() / 2 ** 30}))


if __name__ == "__main__":
    main()
