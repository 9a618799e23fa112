"""Render rate of camera-path frames from a baked scene (upnerf_amd/baked.py) beside the two routes through the
field, on the frames of tools/bench_path.py.

    python tools/bench_baked.py [--resolution 128 128 128] [--level SIGMA] [--step 0.02] [--frames 8] [--width 200] [--height 200]
                                [--chunk 16384] [--progress 0.8] [--images 763] [--reps 3] [--out profiles/baked_render.json]
                                [--sh [--dirs 48] [--sh-out profiles/baked_sh_render.json]]

The system is bench.py's (two 8 x 256 fields, 64 + 128 samples, 763 images, seeded weights), the path and the box those of
bench_path.py --occupancy.  In one process, after a warm-up of every mode, `--reps` rounds of  plain render_path / render_path
with the occupancy grid of the same density at the same level / render_path with the baked scene  run alternately (a drift of
the clocks touches every mode alike; wall clock around a device synchronisation, the median of each).  Written: the bake time
(density, colour and packing; wall clock), frames/s and rays/s of each mode beside its hit share, the grid's bytes, the marcher's
own time per launch (HIP events), and the PSNR of the baked frames against the plain ones at this resolution, step and level.
The weights are random: the hit share and the PSNR say nothing about a trained scene.

--sh adds the baked scenes with spherical-harmonic colour, degree 1 and degree 2 baked at --dirs directions, as
two more legs of the same alternating rounds -- so the degree-0 marcher of the same build runs beside them -- and writes
--sh-out INSTEAD of --out: the rates, each scene's device bytes, the bake times (--dirs passes over the field each), the
marchers' own times per launch, and the degree-0 rate beside the one recorded in --out's file where that exists.

--sparse measures the sparse layout INSTEAD and writes --sparse-out: (1) the marcher, dense against sparse, on
the same frames through an analytic shell volume (an ellipsoid's surface, four cells thick; from_grids / from_direction_grids at 12
directions) at 128^3 and 256^3 points, degree 0 and 2, alternately in one process, medians of --reps: ms per launch, frames/s,
bytes, the occupied share of the bricks f_b and the hit share; (2) the bake, dense against sparse=True, at degree 2 and --dirs
directions on bench.py's system at --resolution, with f_b; (3) with --parent-lib PATH (the library built from the parent
commit), the times per launch of the nine marchers -- dense and sparse forward and the backward, degree 0, 1, 2 -- on the scenes
of --sh (the backward on the inputs of --tune), this build and that one alternately, the first round discarded.

--tune measures the backward march INSTEAD and writes --tune-out: the scenes of --sh (degree 0, 1, 2 at --resolution),
the --frames frames as rays in launches of --chunk, random upstream gradients, forward and backward alternately in one process,
medians of --reps (HIP events round a pass over all rays): ms per backward and per forward launch; the atomic bytes a pass
flushes -- counted here from the definition: cell changes along each ray's visited samples, times the cell's corners with a
sigma, times the floats of a point -- over the time, beside the guide's 1.3 and 0.08 TB/s; and on the first chunk the same
gradient from a restatement in torch's own ops (every sample, gather-based trilinear, autograd), its time and its distance.
Then a distill() on this system: PSNR of the baked frames against the plain ones before and after.  The weights are random.

--tune --sparse measures tuning a sparse scene in place INSTEAD and writes --pool-tune-out: on the analytic shell
of --sparse at 128^3 and 256^3 points, degree 0 and 2, one step of the dense tuner (on the dense scene: what the densify / tune /
sparsify detour runs) and one of the pool tuner (on its sparsify()), on the same --chunk rays and targets, alternately in one
process, medians of --reps (HIP events round 5 steps); beside every time the occupied share of the bricks f_b and the bytes each
tuner holds; and the new launches alone: the sparse backward, the face sum (collect and spread, over every gradient array), with
the dense backward on the same rays beside them.

--pose measures the ray gradient INSTEAD and writes --pose-out: on the analytic shell of --sparse at 128^3 points,
degree 0, 1 and 2, dense and sparse, ms per launch of upnerf_baked_ray_bwd on the --chunk rays beside the forward and the points
backward of the same scene, alternately in one process, medians of --reps (HIP events round 5 launches), the ratios, and
iterations per second of BakedLocaliser.step on two 64 x 64 photographs.

--tv measures the total variation launch INSTEAD and writes --tv-out: on the analytic shell at 128^3 and 256^3
points, degree 0 and 2, ms per upnerf_baked_tv launch on the dense grid and on the pool (the widest point array: rgbs, or the
degree-2 coefficients) beside (a) the same definition in torch ops on the dense tensors, (b) a device copy of one read of data and
one read-modify-write of grad and (c) the marcher's backward launch, alternately, medians of --reps; and the peak device bytes of
a tuner step.  --upsample measures scene.upsample() INSTEAD and writes --upsample-out: 128^3 -> 255^3 and 256^3 -> 511^3, dense
and pool to pool, seconds and peak bytes, and BakedScene.build(..., sparse=True) at 255^3, degree 2, on bench.py's weights."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUNDS = ((-2.5, -2.5, -5.5), (2.5, 2.5, 0.5))  # in front of the cameras (bench_path.py)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, nargs=3, default=(128, 128, 128), metavar=("NX", "NY", "NZ"))
    ap.add_argument("--level", type=float, default=None, help="density below which a grid point is dropped (default: the 0.75 quantile of the grid's density, a random field's scale being arbitrary)")
    ap.add_argument("--step", type=float, default=0.02, help="sample spacing of the baked render")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=200)
    ap.add_argument("--height", type=int, default=200)
    ap.add_argument("--keys", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--progress", type=float, default=0.8)
    ap.add_argument("--images", type=int, default=763)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bake-image", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baked_render.json"))
    ap.add_argument("--sh", action="store_true", help="also time the degree-1 and degree-2 spherical-harmonic scenes; writes --sh-out, not --out")
    ap.add_argument("--dirs", type=int, default=48, help="directions of the spherical-harmonic bakes")
    ap.add_argument("--sh-out", default=os.path.join(ROOT, "profiles", "baked_sh_render.json"))
    ap.add_argument("--sparse", action="store_true", help="measure the sparse layout instead; writes --sparse-out")
    ap.add_argument("--sparse-out", default=os.path.join(ROOT, "profiles", "baked_sparse_render.json"))
    ap.add_argument("--tune", action="store_true", help="measure the backward march instead; writes --tune-out")
    ap.add_argument("--tune-out", default=os.path.join(ROOT, "profiles", "baked_tune.json"))
    ap.add_argument("--tune-iters", type=int, default=200, help="with --tune: iterations of the distill")
    ap.add_argument("--pool-tune-out", default=os.path.join(ROOT, "profiles", "baked_sparse_tune.json"))
    ap.add_argument("--pose", action="store_true", help="measure the ray gradient (upnerf_baked_ray_bwd) and the localiser instead; writes --pose-out")
    ap.add_argument("--pose-out", default=os.path.join(ROOT, "profiles", "baked_pose.json"))
    ap.add_argument("--tv", action="store_true", help="measure the total variation launch (upnerf_baked_tv) instead; writes --tv-out")
    ap.add_argument("--tv-out", default=os.path.join(ROOT, "profiles", "baked_tv.json"))
    ap.add_argument("--upsample", action="store_true", help="measure the doubling of the resolution, dense and pool to pool, instead; writes --upsample-out")
    ap.add_argument("--upsample-out", default=os.path.join(ROOT, "profiles", "baked_upsample.json"))
    ap.add_argument("--env", action="store_true", help="measure the environment map (upnerf_env_composite, its backward, the bake) instead; writes --env-out")
    ap.add_argument("--env-out", default=os.path.join(ROOT, "profiles", "baked_env.json"))
    ap.add_argument("--env-ratios", default=None, help="with --env: a JSON file of the tests' worst error / gate ratios to record beside the times")
    ap.add_argument("--prune", action="store_true", help="measure the visibility march, the face max and prune() instead; writes --prune-out")
    ap.add_argument("--prune-out", default=os.path.join(ROOT, "profiles", "baked_prune.json"))
    ap.add_argument("--parent-lib", default=None, help="with --sparse: the parent commit's libupnerf_hip.so, for the nine marchers' times beside this build's")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_baked.py measures on the GPU; none is visible")
    import bench
    from upnerf_amd import novel_view
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.geometry import density_grid
    from upnerf_amd.novel_view import CameraPath, render_path
    from upnerf_amd.occupancy import OccupancyGrid
    from upnerf_amd.ops import TIMER
    dev = torch.device("cuda", 0)
    sysm = bench.build_system(dev, a.progress, n_images=a.images)
    sysm.hparams["val.chunk_size"] = a.chunk
    W, H, F = a.width, a.height, a.frames
    ang = torch.linspace(-0.3, 0.3, a.keys)  # keyframes on a small arc around the origin, looking down -z (bench_path.py)
    c2w = torch.zeros(a.keys, 3, 4)
    c2w[:, 0, 0] = c2w[:, 2, 2] = torch.cos(ang)
    c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 1, 1] = torch.sin(ang), -torch.sin(ang), 1.0
    c2w[:, :, 3] = torch.stack([0.2 * torch.sin(ang), torch.zeros(a.keys), 0.2 * (1 - torch.cos(ang))], 1)
    K = torch.tensor([[0.8 * W, 0, W / 2], [0, 0.8 * W, H / 2], [0, 0, 1.0]])
    path = CameraPath.from_poses(c2w, (0.1, 5.0), F, appearance=(a.bake_image, a.bake_image), img_wh=(W, H), K=K)  # ONE appearance: the baked one
    rays = F * H * W
    res = tuple(a.resolution)
    if a.env:
        return env_main(a, sysm, path, dev)
    if a.prune:
        return prune_main(a, path, dev)
    if a.pose:
        return pose_main(a, path, dev)
    if a.tv:
        return tv_main(a, path, dev)
    if a.upsample:
        return upsample_main(a, sysm, path, dev)
    if a.sparse and a.tune:
        return pool_tune_main(a, path, dev)
    if a.sparse:
        return sparse_main(a, sysm, path, dev)
    if a.tune:
        return tune_main(a, sysm, path, dev)
    view = (0.0, 0.0, -1.0)  # the cameras of this path look down -z; the synthetic dataset has no poses to average
    grid = density_grid(sysm, BOUNDS, res)
    if a.level is None:  # a quarter of the points kept (a stated rule, not a tuned number: the field is random)
        a.level = float(torch.quantile(grid.reshape(-1)[::max(1, grid.numel() // 1_000_000)].float(), 0.75))
    bake = lambda: BakedScene.build(sysm, BOUNDS, res, a.level, img_id=a.bake_image, view_dir=view)
    bake()  # warm-up
    bake_s = statistics.median(wall(bake) for _ in range(a.reps))
    scene = bake()
    occ = OccupancyGrid.from_density(grid, BOUNDS, a.level, dilate=1)
    modes = {"plain": {}, "occupancy": {"occupancy": occ}, "baked": {"baked": scene, "baked_step": a.step}}
    sh_scenes, sh_bake_s = {}, {}
    if a.sh:
        from upnerf_amd.baked import sphere_directions
        for degree in (1, 2):  # (one timed bake each: K passes over the field)
            bake_sh = lambda: BakedScene.build(sysm, BOUNDS, res, a.level, img_id=a.bake_image, sh_degree=degree, dirs=sphere_directions(a.dirs))
            sh_bake_s[degree] = wall(lambda: sh_scenes.__setitem__(degree, bake_sh()))
            modes[f"baked_sh{degree}"] = {"baked": sh_scenes[degree], "baked_step": a.step}
    share, frames = {}, {}
    for k, kw in modes.items():  # warm-up of every mode; the float frames for the PSNR
        frames[k] = render_path(sysm, path, outputs=("rgb_float",), **kw)["rgb_float"].clamp(0, 1)
        share[k] = novel_view.LAST_STATS["hits"] / rays if k == "occupancy" else None
    direct = scene.render(novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                               (W, H), path.K, 0, H * W)[0], a.step)
    share["baked"] = float((direct["opacity"] > 0).float().mean())  # frame 0: rays that met a kept sample
    times = {k: [] for k in modes}
    for _ in range(a.reps):
        for k, kw in modes.items():
            times[k].append(wall(lambda: render_path(sysm, path, outputs=("rgb",), **kw)))
    summary = lambda v: {"ms_per_launch": v["avg_ms"], "launches": v["launches"], "rays_per_launch": v["units_per_launch"]}
    sh_kern = {}
    for degree in sh_scenes:  # (the two SH marchers share a timer name: one pass each)
        TIMER.reset()
        TIMER.enabled, TIMER.only = True, {"baked_sh_render"}
        render_path(sysm, path, outputs=("rgb",), **modes[f"baked_sh{degree}"])
        sh_kern[degree] = summary(TIMER.summary()["baked_sh_render"])
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, {"baked_render"}
    render_path(sysm, path, outputs=("rgb",), **modes["baked"])
    kern = {n: summary(v) for n, v in TIMER.summary().items()}
    TIMER.enabled, TIMER.only = False, None
    TIMER.reset()
    psnr = lambda x, y: float(-10 * torch.log10(((x - y) ** 2).mean().clamp_min(1e-20)))
    runs = {}
    for k, ts in times.items():
        dt = statistics.median(ts)
        runs[k] = {"frames_per_s": F / dt, "rays_per_s": rays / dt, "hit_share": share[k], "seconds": sorted(ts)}
    out = {"metric": "camera-path frames: plain render_path, with an occupancy grid, from a baked scene (rgb output; random weights)",
           "frames": F, "img_wh": [W, H], "chunk": a.chunk, "progress": a.progress, "reps": a.reps, "resolution": list(res),
           "level": a.level, "step": a.step, "bounds": [list(b) for b in BOUNDS], "view_dir": list(view), "bake_image": a.bake_image,
           "bake_seconds": bake_s, "grid_bytes": scene.nbytes, "occupied_share": scene.fraction,
           "sigma_min": float(grid.min()), "sigma_max": float(grid.max()), "runs": runs, "kernels": kern,
           "psnr_baked_vs_plain_db": psnr(frames["baked"], frames["plain"]), "psnr_occupancy_vs_plain_db": psnr(frames["occupancy"], frames["plain"]),
           "baked_over_plain": runs["baked"]["rays_per_s"] / runs["plain"]["rays_per_s"],
           "baked_over_occupancy": runs["baked"]["rays_per_s"] / runs["occupancy"]["rays_per_s"]}
    if a.sh:
        recorded = None
        if os.path.exists(a.out):
            with open(a.out) as f:
                recorded = json.load(f)["runs"]["baked"]["frames_per_s"]
        out["metric"] = "camera-path frames from baked scenes: degree 0 (no view dependence) and spherical-harmonic degree 1 and 2, beside the two routes through the field (rgb output; random weights)"
        out["dirs"] = a.dirs
        out["degree0_frames_per_s_recorded"] = recorded  # (the figure of --out's file: the marcher before it was a template)
        out["degree0_over_recorded"] = runs["baked"]["frames_per_s"] / recorded if recorded else None
        for degree in (1, 2):
            sc = sh_scenes[degree]
            out[f"sh{degree}"] = {"grid_bytes": sc.nbytes, "bake_seconds": sh_bake_s[degree], "occupied_share": sc.fraction,
                                  "kernel": sh_kern[degree], "psnr_vs_plain_db": psnr(frames[f"baked_sh{degree}"], frames["plain"]),
                                  "over_degree0": runs[f"baked_sh{degree}"]["rays_per_s"] / runs["baked"]["rays_per_s"]}
        a.out = a.sh_out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def shell_grids(n, dev, dirs=None):
    """(sigma [n, n, n], rgb [n, n, n, 3] or rgb_dirs [K, n, n, n, 3]) of an ellipsoid's surface, four cells thick, in the middle of
    BOUNDS: density 40, the colour a smooth function of the position (and, with dirs, of the direction)."""
    t = torch.linspace(-1, 1, n, device=dev)
    z, y, x = t[:, None, None], t[None, :, None], t[None, None, :]
    r = (x * x + y * y + z * z).sqrt()
    sigma = torch.where((r - 0.6).abs() <= 2.0 * 2 / (n - 1), torch.full((), 40.0, device=dev), torch.zeros((), device=dev))
    base = torch.stack([(0.5 + 0.5 * x).expand(n, n, n), (0.5 + 0.5 * y).expand(n, n, n), (0.5 + 0.5 * z).expand(n, n, n)], -1)
    if dirs is None:
        return sigma, base.contiguous()
    d = torch.as_tensor(dirs, dtype=torch.float32, device=dev)
    return sigma, torch.stack([(base * (0.75 + 0.25 * (x * dk[0] + y * dk[1] + z * dk[2]))[..., None]).clamp(0, 1) for dk in d])


def torch_march(scene, params, rays, step, cells):
    """The definition in torch's own ops on `rays` [R, 8]: every lattice sample, the eight corners gathered, blended x, y, z,
    (degree > 0: the expansion at the ray's direction, clamped), composited.  Returns (rgb, depth, opacity, flushed floats): the
    last the atomic adds the backward kernel's register accumulator sends to memory for these rays, counted from the visited
    samples' cells.  `params`: the fp32 tensors of baked_tune.SceneParams (leaves for autograd)."""
    from upnerf_amd.baked import sh_basis
    degree = scene.sh_degree
    (lo, hi), (Nx, Ny, Nz) = scene.bounds, scene.resolution
    dev = rays.device
    lo_t, hi_t = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
    C = torch.tensor([Nx - 1, Ny - 1, Nz - 1], device=dev, dtype=torch.float32)
    o, d, near, far = rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    K = int(torch.ceil((far - near) / step).max())
    k = torch.arange(K, device=dev, dtype=torch.float32)
    t = near[:, None] + (k[None] + 0.5) * step
    live_k = k[None] < torch.ceil((far - near) / step)[:, None]
    g = (o[:, None] + t[..., None] * d[:, None] - lo_t) * (C / (hi_t - lo_t))
    inside = ((g >= 0) & (g <= C)).all(-1) & live_k
    gi = torch.where(inside[..., None], g, torch.zeros_like(g))
    i = torch.minimum(gi.floor(), C - 1)
    f = gi - i
    i = i.long()
    base = (i[..., 2] * Ny + i[..., 1]) * Nx + i[..., 0]
    if degree == 0:
        flat = params[0].reshape(-1, 4)
        corner = lambda off: flat[base + off]
        sig_flat, per = flat[:, 3], 4
    else:
        nb = (degree + 1) ** 2
        coef, sig_flat = params[0].reshape(-1, 3, nb), params[1].reshape(-1)
        Y = torch.as_tensor(sh_basis(d.cpu().numpy(), degree), dtype=torch.float32, device=dev)
        corner = lambda off: torch.cat([torch.einsum("rkcj,rj->rkc", coef[base + off], Y), sig_flat[base + off][..., None]], -1)
        per = 3 * nb + 1
    offs = [dx + dy * Nx + dz * Nx * Ny for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    c = [corner(off) for off in offs]
    fx, fy, fz = f[..., 0:1], f[..., 1:2], f[..., 2:3]
    x00, x10, x01, x11 = c[0] + fx * (c[1] - c[0]), c[2] + fx * (c[3] - c[2]), c[4] + fx * (c[5] - c[4]), c[6] + fx * (c[7] - c[6])
    y0, y1 = x00 + fy * (x10 - x00), x01 + fy * (x11 - x01)
    v = (y0 + fz * (y1 - y0)) * inside[..., None]
    col = v[..., :3].clamp(0, 1) if degree else v[..., :3]
    delta = step * d.norm(dim=1, keepdim=True)
    alpha = 1 - torch.exp(-delta * v[..., 3])
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], 1), 1)
    w = T * alpha
    opacity = w.sum(1)
    rgb = (w[..., None] * col).sum(1)
    depth = (w * t).sum(1) + (1 - opacity) * far
    with torch.no_grad():  # the flushes: a visited sample (inside, its cell's bit set) whose cell differs from the last visited one's
        cell = (i[..., 2] * (Ny - 1) + i[..., 1]) * (Nx - 1) + i[..., 0]
        visited = inside & cells.reshape(-1)[cell]
        key = torch.where(visited, cell, torch.full_like(cell, -1))
        last = torch.cummax(torch.where(visited, torch.arange(K, device=dev)[None].expand_as(cell), torch.full_like(cell, -1)), 1)[0]
        prev = torch.cat([torch.full_like(last[:, :1], -1), last[:, :-1]], 1)
        prev_cell = torch.where(prev >= 0, torch.gather(key, 1, prev.clamp(min=0)), torch.full_like(cell, -2))
        flush = visited & (key != prev_cell)
        n_live = sum((sig_flat[base + off] != 0).long() for off in offs)
        floats = int((flush * n_live).sum()) * per
    return rgb, depth, opacity, floats


def tune_main(a, sysm, path, dev):
    import statistics as st
    from upnerf_amd import baked_tune, novel_view
    from upnerf_amd.baked import BakedScene, sphere_directions
    from upnerf_amd.geometry import density_grid
    from upnerf_amd.novel_view import render_path
    F, W, H = a.frames, a.width, a.height
    res = tuple(a.resolution)
    rays = novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                (W, H), path.K, 0, F * H * W)[0]
    R = rays.shape[0]
    grid = density_grid(sysm, BOUNDS, res)
    if a.level is None:
        a.level = float(torch.quantile(grid.reshape(-1)[::max(1, grid.numel() // 1_000_000)].float(), 0.75))
    gen = torch.Generator(device="cpu").manual_seed(5)
    g_rgb, g_depth, g_op = (torch.randn(*shape, generator=gen).to(dev) for shape in ((R, 3), (R,), (R,)))
    chunks = [(r0, min(a.chunk, R - r0)) for r0 in range(0, R, a.chunk)]
    out = {"metric": "the baked marcher's backward pass (upnerf_baked_render_bwd) beside its forward, per degree; random weights, random upstream gradients",
           "resolution": list(res), "level": a.level, "step": a.step, "rays": R, "rays_per_launch": a.chunk, "launches": len(chunks),
           "guide_atomic_TBps": {"shaped_and_spread": 1.3, "one_lane_per_row_or_one_row": 0.08}, "degrees": {}}
    scenes = {}
    for degree in (0, 1, 2):
        kw = dict(sh_degree=degree, dirs=sphere_directions(a.dirs)) if degree else dict(view_dir=(0.0, 0.0, -1.0))
        scenes[degree] = BakedScene.build(sysm, BOUNDS, res, a.level, img_id=a.bake_image, **kw)

    def passes(degree):
        scene = scenes[degree]
        nb = (degree + 1) ** 2
        shape = tuple(reversed(scene.resolution))
        bufs = torch.zeros(shape + (4,), device=dev) if degree == 0 else (torch.zeros(shape + (3, nb), device=dev), torch.zeros(shape, device=dev))
        fwd = lambda: [scene.render(rays[r0:r0 + n], a.step) for r0, n in chunks]
        bwd = lambda: [baked_tune.backward(scene.grid, degree, scene.occupancy, scene.bounds, rays[r0:r0 + n], a.step, 0.0, 0.0, g_rgb[r0:r0 + n],
                                           g_depth[r0:r0 + n], g_op[r0:r0 + n], out=bufs) for r0, n in chunks]
        return fwd, bwd

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    fns = {d_: passes(d_) for d_ in scenes}
    for fwd, bwd in fns.values():  # warm-up
        fwd(), bwd()
    ms = {d_: {"fwd": [], "bwd": []} for d_ in scenes}
    for _ in range(a.reps):
        for d_, (fwd, bwd) in fns.items():
            ms[d_]["fwd"].append(event_ms(fwd))
            ms[d_]["bwd"].append(event_ms(bwd))
    for degree, scene in scenes.items():
        cells = scene.occupancy.cells()
        params = baked_tune.SceneParams.of(scene)
        floats = 0
        sub = max(1, 2048 if degree else 16384)  # (rows of the torch restatement at a time: it materialises every sample)
        with torch.no_grad():
            for r0 in range(0, R, sub):
                floats += torch_march(scene, [p.detach() for p in params.tensors], rays[r0:r0 + sub], a.step, cells)[3]
        # the same gradient from torch's autograd on the first rows
        n = sub
        torch_fn = lambda: torch.autograd.grad((lambda o: (o[0] * g_rgb[:n]).sum() + (o[1] * g_depth[:n]).sum() + (o[2] * g_op[:n]).sum())(
            torch_march(scene, params.tensors, rays[:n], a.step, cells)), params.tensors)
        torch_fn()
        t_ms = st.median(event_ms(torch_fn) for _ in range(a.reps))
        want = torch_fn()
        ours_fn = lambda: baked_tune.backward(scene.grid, degree, scene.occupancy, scene.bounds, rays[:n], a.step, 0.0, 0.0, g_rgb[:n], g_depth[:n], g_op[:n])
        ours_fn()
        k_ms = st.median(event_ms(ours_fn) for _ in range(a.reps))
        got = ours_fn()
        got = (got,) if degree == 0 else got
        live = (params.tensors[-1][..., 3] if degree == 0 else params.tensors[1]) != 0  # (autograd also fills the dead corners: not parameters here)
        dist = max(float(((g_ - w_) * (live[..., None] if g_.dim() == 4 else live[..., None, None] if g_.dim() == 5 else live)).abs().max() / w_.abs().max())
                   for g_, w_ in zip(got, want))
        b_ms, f_ms = st.median(ms[degree]["bwd"]), st.median(ms[degree]["fwd"])
        out["degrees"][str(degree)] = {
            "bwd_ms_per_launch": b_ms / len(chunks), "fwd_ms_per_launch": f_ms / len(chunks), "bwd_over_fwd": b_ms / f_ms,
            "bwd_rays_per_s": R / (b_ms * 1e-3), "atomic_bytes_per_pass": floats * 4, "atomic_TBps": floats * 4 / (b_ms * 1e-3) / 1e12,
            "torch_autograd": {"rays": n, "torch_ms": t_ms, "kernel_ms": k_ms, "torch_over_kernel": t_ms / k_ms, "max_abs_diff_over_max": dist},
            "hit_share_frame0": float((scene.render(rays[:H * W], a.step)["opacity"] > 0).float().mean())}
    # distill on this system: the degree-0 scene against the field's own renders of the path's keyframe cameras
    plain = render_path(sysm, path, outputs=("rgb_float",))["rgb_float"].clamp(0, 1)
    psnr = lambda sc: float(-10 * torch.log10(((render_path(sysm, path, outputs=("rgb_float",), baked=sc, baked_step=a.step)["rgb_float"].clamp(0, 1) - plain) ** 2).mean()))
    out["distill"] = {}
    for degree in (0, 2):
        before = psnr(scenes[degree])
        t0 = time.perf_counter()
        tuned, curve = baked_tune.distill(sysm, scenes[degree], path, iters=a.tune_iters, batch=a.chunk, baked_step=a.step, seed=0, lr=1e-2, img_id=a.bake_image)
        torch.cuda.synchronize()
        out["distill"][str(degree)] = {"iters": a.tune_iters, "batch": a.chunk, "lr": 1e-2, "seconds": time.perf_counter() - t0, "loss_first": curve[0],
                                       "loss_last": curve[-1], "psnr_db_before": before, "psnr_db_after": psnr(tuned),
                                       "note": "targets: the keyframe cameras; PSNR: all frames of the path; random weights, no trained scene"}
    os.makedirs(os.path.dirname(os.path.abspath(a.tune_out)), exist_ok=True)
    with open(a.tune_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def pool_tune_main(a, path, dev):
    import statistics as st
    from upnerf_amd import baked_sparse_tune, baked_tune, novel_view
    from upnerf_amd.baked import BakedScene, sphere_directions
    W, H = a.width, a.height
    rays = novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                (W, H), path.K, 0, H * W)[0][:a.chunk].contiguous()
    R = rays.shape[0]
    gen = torch.Generator(device="cpu").manual_seed(5)
    g_rgb = torch.randn(R, 3, generator=gen).to(dev)
    STEPS = 5

    def event_ms(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    rows = []
    for n in (128, 256):
        for degree in (0, 2):
            if degree == 0:
                dense = BakedScene.from_grids(*shell_grids(n, dev), BOUNDS, 1.0)
            else:
                dirs = sphere_directions(12)
                sigma, rgb_dirs = shell_grids(n, dev, dirs)
                dense = BakedScene.from_direction_grids(sigma, rgb_dirs, dirs, BOUNDS, 1.0, sh_degree=2)
                del sigma, rgb_dirs
            sparse = dense.sparsify()
            target = (dense.render(rays, a.step)["rgb"] + 0.05 * torch.randn(R, 3, generator=gen).to(dev)).clamp(0, 1)
            tuners = {"dense": dense.tune(1e-2), "pool": sparse.tune_pool(1e-2)}
            params = baked_sparse_tune.PoolParams.of(sparse, requires_grad=False)
            grads = tuners["pool"].grads
            legs = {f"{k}_step": (lambda t=t: t.step(rays, target, a.step)) for k, t in tuners.items()}
            legs["sparse_bwd"] = lambda: baked_sparse_tune.backward(sparse.pool, params, rays, a.step, 0.0, 0.0, g_rgb, out=grads[0] if degree == 0 else grads,
                                                                    face_sum=False)
            legs["face_sum"] = lambda: [baked_sparse_tune.face_sum(t, sparse) for t in grads]
            dgrads = tuners["dense"].grads
            legs["dense_bwd"] = lambda: baked_tune.backward(dense.grid, degree, dense.occupancy, dense.bounds, rays, a.step, 0.0, 0.0, g_rgb,
                                                            out=dgrads[0] if degree == 0 else dgrads)
            for fn in legs.values():  # warm-up
                fn()
            ms = {k: [] for k in legs}
            for _ in range(a.reps):
                for k, fn in legs.items():
                    ms[k].append(event_ms(fn, STEPS))
            med = {k: st.median(v) for k, v in ms.items()}
            rows.append({"resolution": n, "degree": degree, "occupied_bricks": sparse.n_bricks, "f_b": sparse.brick_fraction,
                         "hit_share": float((dense.render(rays, a.step)["opacity"] > 0).float().mean()),
                         "dense": {"step_ms": med["dense_step"], "tuner_bytes": tuners["dense"].nbytes, "scene_bytes": dense.nbytes, "step_ms_all": sorted(ms["dense_step"])},
                         "pool": {"step_ms": med["pool_step"], "tuner_bytes": tuners["pool"].nbytes, "scene_bytes": sparse.nbytes, "step_ms_all": sorted(ms["pool_step"])},
                         "dense_step_over_pool_step": med["dense_step"] / med["pool_step"],
                         "dense_bytes_over_pool_bytes": tuners["dense"].nbytes / tuners["pool"].nbytes,
                         "launches_ms": {"baked_sparse_render_bwd": med["sparse_bwd"], "brick_face_sum_collect_and_spread": med["face_sum"],
                                         "baked_render_bwd_dense": med["dense_bwd"]}})
            del dense, sparse, tuners, params, grads, dgrads, legs
            torch.cuda.empty_cache()
    out = {"metric": "one tuner step, dense (BakedTuner on the dense scene) against in place on the brick pool (PoolTuner), and the new launches alone; analytic shell, random targets",
           "rays": R, "step": a.step, "reps": a.reps, "steps_per_timing": STEPS, "bounds": [list(b) for b in BOUNDS], "rows": rows,
           "note": "an analytic shell, not a trained scene: f_b and the hit share are the shell's"}
    os.makedirs(os.path.dirname(os.path.abspath(a.pool_tune_out)), exist_ok=True)
    with open(a.pool_tune_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def _event_ms(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _shell_scene(n, degree, dev):
    from upnerf_amd.baked import BakedScene, sphere_directions
    if degree == 0:
        return BakedScene.from_grids(*shell_grids(n, dev), BOUNDS, 1.0)
    dirs = sphere_directions(12)
    sigma, rgb_dirs = shell_grids(n, dev, dirs)
    return BakedScene.from_direction_grids(sigma, rgb_dirs, dirs, BOUNDS, 1.0, sh_degree=2)


def torch_tv(data, sigma, cells, w, eps, out):
    """The definition of upnerf_baked_tv in torch ops on the same dense tensors: value, and the gradient added into `out`."""
    a = data[:-1, :-1, :-1]
    dx, dy, dz = data[:-1, :-1, 1:] - a, data[:-1, 1:, :-1] - a, data[1:, :-1, :-1] - a
    t = (eps + dx * dx + dy * dy + dz * dz).sqrt()
    on = cells[..., None].to(data.dtype) * w
    live = (sigma != 0)[..., None].to(data.dtype)
    r = on / t
    g = torch.zeros_like(data)
    g[:-1, :-1, :-1] -= (dx + dy + dz) * r
    g[:-1, :-1, 1:] += dx * r
    g[:-1, 1:, :-1] += dy * r
    g[1:, :-1, :-1] += dz * r
    out += g * live
    return (t * on).sum()


def tv_main(a, path, dev):
    """upnerf_baked_tv on the pool and on the dense grid of the analytic shell, beside (a) the same definition in torch ops on the
    dense tensors, (b) a device copy of the bytes the launch must move at least and (c) the marcher's backward launch of the same
    tuner step; alternately in one process, medians of --reps."""
    import statistics as st
    from upnerf_amd import baked_reg, baked_sparse_tune, baked_tune, novel_view
    W, H = a.width, a.height
    rays = novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                (W, H), path.K, 0, H * W)[0][:a.chunk].contiguous()
    R = rays.shape[0]
    g_rgb = torch.randn(R, 3, generator=torch.Generator(device="cpu").manual_seed(5)).to(dev)
    STEPS, rows = 5, []
    for n in (128, 256):
        for degree in (0, 2):
            dense = _shell_scene(n, degree, dev)
            sparse = dense.sparsify()
            target = dense.render(rays, a.step)["rgb"].clone()
            tuners, peak = {}, {}
            for k, make in (("dense", lambda: dense.tune(1e-2, tv_sigma=1e-3, tv_colour=1e-3)),
                            ("pool", lambda: sparse.tune_pool(1e-2, tv_sigma=1e-3, tv_colour=1e-3))):
                # each tuner alone: its construction and one step, above what was allocated before it (the scenes, the other tuner)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                tuners[k] = make()
                tuners[k].step(rays, target, a.step)
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() - base
            td, tp = tuners["dense"], tuners["pool"]
            data = {"dense": td.masters[0], "pool": tp.masters[0]}  # rgbs [.., 4], or the coefficients [.., 3, 9]
            sig = {k: (t.masters[0][..., 3] if degree == 0 else t.masters[1]) for k, t in tuners.items()}
            F = data["dense"].numel() // sig["dense"].numel()
            w = [1e-6] * F
            cells = dense.occupancy.cells()
            wt = torch.tensor(w, device=dev)
            flat = data["dense"].reshape(tuple(sig["dense"].shape) + (F,))
            gflat = td.grads[0].reshape(flat.shape)
            legs = {"tv_dense": lambda: baked_reg.tv_backward(data["dense"], sig["dense"], td.occupancy, w, 1e-8, out=td.grads[0]),
                    "tv_pool": lambda: baked_reg.tv_backward(data["pool"], sig["pool"], tp.occupancy, w, 1e-8, layout=tp.params, out=tp.grads[0], face_sum=False),
                    "torch_dense": lambda: torch_tv(flat, sig["dense"], cells, wt, 1e-8, gflat),
                    # one read of data, one read-modify-write of grad, in one launch: grad += data
                    "copy_dense": lambda: td.grads[0].add_(data["dense"]),
                    "copy_pool": lambda: tp.grads[0].add_(data["pool"]),
                    "bwd_dense": lambda: baked_tune.backward(td.points, degree, td.occupancy, td.bounds, rays, a.step, 0.0, 0.0, g_rgb,
                                                             out=td.grads[0] if degree == 0 else td.grads),
                    "bwd_pool": lambda: baked_sparse_tune.backward(tp.points, tp.params, rays, a.step, 0.0, 0.0, g_rgb,
                                                                   out=tp.grads[0] if degree == 0 else tp.grads, face_sum=False)}
            for fn in legs.values():
                fn()
            ms = {k: [] for k in legs}
            for _ in range(a.reps):
                for k, fn in legs.items():
                    ms[k].append(_event_ms(fn, STEPS))
            med = {k: st.median(v) for k, v in ms.items()}
            rows.append({"resolution": n, "degree": degree, "floats_per_point": F, "occupied_bricks": sparse.n_bricks, "f_b": sparse.brick_fraction,
                         "ms": med, "ms_all": {k: sorted(v) for k, v in ms.items()}, "torch_over_hip_dense": med["torch_dense"] / med["tv_dense"],
                         "hip_over_copy_dense": med["tv_dense"] / med["copy_dense"], "hip_over_copy_pool": med["tv_pool"] / med["copy_pool"],
                         "tuner_peak_bytes_construction_and_step": peak, "tuner_bytes": {k: t.nbytes for k, t in tuners.items()}})
            del dense, sparse, tuners, td, tp, data, sig, cells, flat, gflat, legs
            torch.cuda.empty_cache()
    out = {"metric": "one upnerf_baked_tv launch on the point array of widest F (rgbs, or the degree-2 coefficients) beside the same definition in torch ops, "
                     "a device copy of one read of data and one read-modify-write of grad, and the marcher's backward launch; analytic shell",
           "rays": R, "step": a.step, "reps": a.reps, "launches_per_timing": STEPS, "bounds": [list(b) for b in BOUNDS], "rows": rows,
           "note": "an analytic shell, not a trained scene; torch_dense runs on the dense tensors only (the torch form of the pool would need the dense round trip)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.tv_out)), exist_ok=True)
    with open(a.tv_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def _two_shells(n, degree, dev):
    """_shell_scene with a second shell of half the radius inside it: what lies behind the first shell a ray meets is the hidden one."""
    from upnerf_amd.baked import BakedScene, sphere_directions
    dirs = sphere_directions(12) if degree else None
    sigma, colour = shell_grids(n, dev, dirs)
    t = torch.linspace(-1, 1, n, device=dev)
    r = (t[None, None, :] ** 2 + t[None, :, None] ** 2 + t[:, None, None] ** 2).sqrt()
    sigma = torch.where((r - 0.3).abs() <= 2.0 * 2 / (n - 1), torch.full((), 40.0, device=dev), sigma)
    if degree == 0:
        return BakedScene.from_grids(sigma, colour, BOUNDS, 1.0)
    return BakedScene.from_direction_grids(sigma, colour, dirs, BOUNDS, 1.0, sh_degree=2)


def prune_main(a, path, dev):
    """upnerf_baked_visibility beside the forward launch of the same scene, dense and pool, degree 0 and 2, on two analytic shells
    at 128^3 points; the face max; and pool bytes, bricks and forward ms before and after prune().  Alternately in one process,
    medians of --reps."""
    import statistics as st
    from upnerf_amd import baked_prune, novel_view
    W, H = a.width, a.height
    rays = novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                (W, H), path.K, 0, H * W)[0][:a.chunk].contiguous()
    R, n, STEPS, rows = rays.shape[0], 128, 5, []
    for degree in (0, 2):
        dense = _two_shells(n, degree, dev)
        sparse = dense.sparsify()
        vis_d = torch.zeros(dense.resolution[::-1], device=dev)
        vis_p = torch.zeros(sparse.n_bricks, 9, 9, 9, device=dev)
        pruned = {w: sparse.prune(rays, a.step, min_weight=w) for w in (None, 1e-2)}
        out = {k: torch.empty(R, 3 if k == "rgb" else 1, device=dev).squeeze(-1) for k in ("rgb", "depth", "opacity")}
        legs = {"forward_dense": lambda: dense.render(rays, a.step, out=out),
                "forward_pool": lambda: sparse.render(rays, a.step, out=out),
                "visibility_dense": lambda: baked_prune.march_visibility(dense, rays, a.step, 0.0, vis_d),
                "visibility_pool": lambda: baked_prune.march_visibility(sparse, rays, a.step, 0.0, vis_p),
                "face_max": lambda: baked_prune.face_max(vis_p, sparse),
                "forward_pool_pruned": lambda: pruned[None].render(rays, a.step, out=out),
                "forward_pool_pruned_1e-2": lambda: pruned[1e-2].render(rays, a.step, out=out)}
        for fn in legs.values():
            fn()

        def cold_ms(fn, buf):
            # what a caller pays: visibility() and prune() start from a zeroed buffer, so every atomic of the launch is issued.  (In
            # the legs above the buffer holds the maxima of the launch before and the load in front of the atomic skips them all.)
            total = 0.0
            for _ in range(STEPS):
                buf.zero_()  # untimed
                total += _event_ms(fn)
            return total / STEPS

        cold = {"visibility_dense_cold": lambda: cold_ms(legs["visibility_dense"], vis_d),
                "visibility_pool_cold": lambda: cold_ms(legs["visibility_pool"], vis_p)}
        ms = {k: [] for k in list(legs) + list(cold)}
        for _ in range(a.reps):
            for k, fn in legs.items():
                ms[k].append(_event_ms(fn, STEPS))
            for k, fn in cold.items():
                ms[k].append(fn())
        med = {k: st.median(v) for k, v in ms.items()}
        same = all(torch.equal(sparse.render(rays, a.step)[k], pruned[None].render(rays, a.step)[k]) for k in ("rgb", "depth", "opacity"))
        size = lambda s: {"pool_bytes": s.pool.numel() * s.pool.element_size(), "n_bricks": s.n_bricks, "f_b": s.brick_fraction, "nbytes": s.nbytes}
        rows.append({"resolution": n, "degree": degree, "ms": med, "ms_all": {k: sorted(v) for k, v in ms.items()},
                     "visibility_over_forward_dense": med["visibility_dense_cold"] / med["forward_dense"],
                     "visibility_over_forward_pool": med["visibility_pool_cold"] / med["forward_pool"],
                     "warm_visibility_over_forward_dense": med["visibility_dense"] / med["forward_dense"],
                     "warm_visibility_over_forward_pool": med["visibility_pool"] / med["forward_pool"],
                     "before": size(sparse), "after_default": size(pruned[None]), "after_1e-2": size(pruned[1e-2]),
                     "points_seen_share": float((dense.visibility(rays, a.step) > 0).float().mean()),
                     "pruned_renders_the_rays_to_the_same_bits": same})
        del dense, sparse, pruned, vis_d, vis_p, legs
        torch.cuda.empty_cache()
    res = {"metric": "one upnerf_baked_visibility launch into a zeroed buffer (_cold: the zeroing untimed; the legs without the suffix max into the "
                     "buffer of the launch before, so their atomics are all skipped) beside the forward launch of the same scene in the same process; upnerf_brick_face_max on the "
                     "pool-shaped visibility; a sparse scene before and after prune() for the same rays (default weight, and 1e-2); two analytic shells",
           "rays": R, "step": a.step, "reps": a.reps, "launches_per_timing": STEPS, "bounds": [list(b) for b in BOUNDS], "rows": rows,
           "note": "analytic shells, not a trained scene: what share of a trained scene a prune removes, and which min_weight serves, is unchecked"}
    os.makedirs(os.path.dirname(os.path.abspath(a.prune_out)), exist_ok=True)
    with open(a.prune_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def upsample_main(a, sysm, path, dev):
    """scene.upsample() 128^3 -> 255^3 and 256^3 -> 511^3 on the analytic shell, dense and pool to pool: time and peak device bytes;
    for degree 2 at 128^3 -> 255^3, BakedScene.build(..., sparse=True) at the target size on bench.py's seeded weights beside them."""
    import statistics as st
    from upnerf_amd.baked import BakedScene, sphere_directions
    rows = []

    def measure(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ts = []
        for _ in range(a.reps):
            ts.append(wall(fn))
        return {"seconds": st.median(ts), "seconds_all": sorted(ts), "peak_bytes": torch.cuda.max_memory_allocated() - base}

    for n in (128, 256):
        for degree in (0, 2):
            if n == 256 and degree == 2:
                dense = None  # 511^3 records of 64 bytes are 8.5 GB beside their parents: the pool route alone
                sparse = _shell_scene(n, degree, dev).sparsify()
            else:
                dense = _shell_scene(n, degree, dev)
                sparse = dense.sparsify()
            row = {"resolution": n, "target": 2 * n - 1, "degree": degree, "parent_bricks": sparse.n_bricks, "parent_f_b": sparse.brick_fraction,
                   "parent_bytes": {"dense": dense.nbytes if dense is not None else None, "sparse": sparse.nbytes}}
            if dense is not None:
                row["dense"] = measure(lambda: dense.upsample())
            row["sparse"] = measure(lambda: sparse.upsample())
            child = sparse.upsample()
            row["child_bricks"], row["child_f_b"], row["child_bytes_sparse"] = child.n_bricks, child.brick_fraction, child.nbytes
            del child, dense, sparse
            torch.cuda.empty_cache()
            rows.append(row)
    level = None
    n = 255
    from upnerf_amd.geometry import density_grid
    grid = density_grid(sysm, BOUNDS, (64, 64, 64))
    level = float(torch.quantile(grid.reshape(-1).float(), 0.95))  # a twentieth of the points kept: a stated rule, the field is random
    del grid
    dirs = sphere_directions(12)
    bake = measure(lambda: BakedScene.build(sysm, BOUNDS, (n, n, n), level, img_id=a.bake_image, sh_degree=2, dirs=dirs, sparse=True))
    # the loop working, not a fidelity figure: the weights are random.  A fixed-resolution distill against one with TV and one upsampling
    from upnerf_amd import baked_tune
    coarse = BakedScene.build(sysm, BOUNDS, (64, 64, 64), level, img_id=a.bake_image, view_dir=(0.0, 0.0, -1.0))
    kw = dict(iters=60, batch=4096, baked_step=a.step, seed=0, lr=0.01, img_id=a.bake_image)
    fixed = baked_tune.distill(sysm, coarse, path, **kw)
    c2f = baked_tune.distill(sysm, coarse, path, tv=(1e-3, 1e-3), upsample_at=(30,), **kw)
    curves = {"resolution": [64, 64, 64], "iters": 60, "batch": 4096, "lr": 0.01, "tv": [1e-3, 1e-3], "upsample_at": [30],
              "fixed_resolution": {"final_resolution": list(fixed[0].resolution), "loss_every_5": fixed[1][::5] + fixed[1][-1:]},
              "tv_and_one_upsampling": {"final_resolution": list(c2f[0].resolution), "loss_every_5": c2f[1][::5] + c2f[1][-1:]},
              "note": "random weights: the loop working, not a fidelity figure; the loss is the batch's MSE before each update, without the penalty"}
    out = {"metric": "scene.upsample(): wall seconds round a device synchronisation (median of --reps) and peak device bytes above the parent's",
           "reps": a.reps, "bounds": [list(b) for b in BOUNDS], "rows": rows, "distill_curves": curves,
           "bake_sparse_degree2_at_255": dict(bake, level=level, dirs=12, note="BakedScene.build(sparse=True) on bench.py's seeded (random) weights at the target size"),
           "note": "an analytic shell, not a trained scene"}
    os.makedirs(os.path.dirname(os.path.abspath(a.upsample_out)), exist_ok=True)
    with open(a.upsample_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def torch_env(env, rays, opacity, rgb):
    """The definition of upnerf_env_composite in torch ops (tools/torch_ops.py style: the same arithmetic on the same tensors, one
    op per step): face, cell, bilinear blend, composite.  Differentiable in rays, opacity and rgb through autograd."""
    E = env.shape[1] - 1
    d = rays[:, 3:6]
    mag = d.abs()
    m = torch.zeros(d.shape[0], dtype=torch.long, device=d.device)
    m = torch.where(mag[:, 1] > mag.gather(1, m[:, None])[:, 0], torch.ones_like(m), m)
    m = torch.where(mag[:, 2] > mag.gather(1, m[:, None])[:, 0], torch.full_like(m, 2), m)
    a_, b_ = torch.where(m == 0, 1, 0), torch.where(m == 2, 1, 2)
    pick = lambda i: d.gather(1, i[:, None])[:, 0]
    dm = pick(m)
    face = 2 * m + (dm < 0).long()
    u, v = pick(a_) / dm.abs(), pick(b_) / dm.abs()
    gu, gv = (u + 1) * (E / 2), (v + 1) * (E / 2)
    iu, iv = gu.detach().floor().clamp(max=E - 1).long(), gv.detach().floor().clamp(max=E - 1).long()
    fu, fv = (gu - iu)[:, None], (gv - iv)[:, None]
    n00, n10, n01, n11 = env[face, iv, iu, :3], env[face, iv, iu + 1, :3], env[face, iv + 1, iu, :3], env[face, iv + 1, iu + 1, :3]
    x0, x1 = torch.addcmul(n00, fu, n10 - n00), torch.addcmul(n01, fu, n11 - n01)
    return torch.addcmul(rgb, (1 - opacity)[:, None], torch.addcmul(x0, fv, x1 - x0))


def env_main(a, sysm, path, dev):
    """--env: ms per launch of upnerf_env_composite and upnerf_env_composite_bwd on one chunk of rays (E = 64) beside the forward
    march of the same rays through a 128^3 analytic shell and beside the same definition in torch ops (forward, and forward +
    autograd backward), alternately in one process, medians of --reps; and the seconds of Environment.build at E = 64 and 256."""
    import datetime
    import statistics as st
    from upnerf_amd import baked_env, novel_view
    W, H = a.width, a.height
    c2w, nf = novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode)
    rays = novel_view.path_rays(c2w, nf, (W, H), path.K, 0, H * W)[0][:a.chunk].contiguous()
    R = rays.shape[0]
    gen = torch.Generator(device="cpu").manual_seed(5)
    g_out = torch.randn(R, 3, generator=gen).to(dev)
    scene = _shell_scene(128, 0, dev)
    bake_s = {}
    for E in (64, 256):
        baked_env.Environment.build(sysm, BOUNDS, E, img_id=a.bake_image)  # warm-up
        bake_s[E] = st.median(wall(lambda: baked_env.Environment.build(sysm, BOUNDS, E, img_id=a.bake_image)) for _ in range(a.reps))
    env = baked_env.Environment.build(sysm, BOUNDS, 64, img_id=a.bake_image)
    march = scene.render(rays, a.step)
    rgb, opacity = march["rgb"].clone(), march["opacity"].clone()
    out = torch.empty_like(rgb)

    def torch_both():
        r, o, c = rays.clone().requires_grad_(True), opacity.clone().requires_grad_(True), rgb.clone().requires_grad_(True)
        torch_env(env.env, r, o, c).backward(g_out)

    legs = {"march_forward": lambda: scene.render(rays, a.step),
            "composite": lambda: baked_env._composite(env.env, rays, opacity, rgb, out),
            "composite_bwd": lambda: baked_env.composite_backward(env.env, rays, opacity, g_out),
            "torch_composite": lambda: torch_env(env.env, rays, opacity, rgb),
            "torch_composite_and_bwd": torch_both}
    STEPS = 5
    for fn in legs.values():
        fn()
    ms = {k: [] for k in legs}
    for _ in range(a.reps):  # alternately: every leg sees the same clocks
        for k, fn in legs.items():
            ms[k].append(_event_ms(fn, STEPS))
    got = baked_env._composite(env.env, rays, opacity, rgb, torch.empty_like(rgb))
    ratios = None
    if a.env_ratios:
        with open(a.env_ratios) as f:
            ratios = json.load(f)
    res = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "rays": R, "E": 64, "step": a.step, "reps": a.reps,
           "launches_per_sample": STEPS, "ms": {k: st.median(v) for k, v in ms.items()}, "ms_all": ms,
           "max_abs_difference_to_torch_ops": float((got - torch_env(env.env, rays, opacity, rgb)).abs().max()),
           "opacity_mean": float(opacity.mean()), "bake_seconds": {str(E): s for E, s in bake_s.items()},
           "bake_node_rays": {str(E): 6 * (E + 1) ** 2 for E in bake_s}, "test_worst_err_over_gate": ratios,
           "note": "random synthetic field and an analytic shell, not a trained scene: fidelity is unchecked; the map has no parallax"}
    os.makedirs(os.path.dirname(os.path.abspath(a.env_out)), exist_ok=True)
    with open(a.env_out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def pose_main(a, path, dev):
    """--pose: ms per launch of upnerf_baked_ray_bwd on one chunk of rays beside the forward and the points backward of the same
    scene (128^3 analytic shell, degree 0, 1, 2, dense and sparse), alternately in one process, medians of --reps; and
    iterations per second of BakedLocaliser.step on two 64 x 64 photographs of the degree-0 scene."""
    import statistics as st
    from upnerf_amd import baked_pose, baked_sparse_tune, baked_tune, novel_view
    from upnerf_amd.baked import BakedScene, sphere_directions
    W, H = a.width, a.height
    c2w, nf = novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode)
    rays = novel_view.path_rays(c2w, nf, (W, H), path.K, 0, H * W)[0][:a.chunk].contiguous()
    R = rays.shape[0]
    gen = torch.Generator(device="cpu").manual_seed(5)
    g_rgb = torch.randn(R, 3, generator=gen).to(dev)
    STEPS = 5

    def event_ms(fn, n=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    rows, n = [], 128
    for degree in (0, 1, 2):
        if degree == 0:
            dense = BakedScene.from_grids(*shell_grids(n, dev), BOUNDS, 1.0)
        else:
            dirs = sphere_directions(12)
            sigma, rgb_dirs = shell_grids(n, dev, dirs)
            dense = BakedScene.from_direction_grids(sigma, rgb_dirs, dirs, BOUNDS, 1.0, sh_degree=degree)
            del sigma, rgb_dirs
        sparse = dense.sparsify()
        for layout, scene in (("dense", dense), ("sparse", sparse)):
            out = torch.empty(R, 8, device=dev)
            legs = {"forward": lambda: scene.render(rays, a.step),
                    "ray_bwd": lambda: baked_pose.ray_backward(scene, rays, a.step, 0.0, 0.0, g_rgb, out=out)}
            if layout == "dense":
                grads = baked_tune.backward(dense.grid, degree, dense.occupancy, dense.bounds, rays, a.step, 0.0, 0.0, g_rgb)
                legs["points_bwd"] = lambda: baked_tune.backward(dense.grid, degree, dense.occupancy, dense.bounds, rays, a.step, 0.0, 0.0, g_rgb, out=grads)
            else:
                params = baked_sparse_tune.PoolParams.of(sparse, requires_grad=False)
                grads = baked_sparse_tune.backward(sparse.pool, params, rays, a.step, 0.0, 0.0, g_rgb, face_sum=False)
                legs["points_bwd"] = lambda: baked_sparse_tune.backward(sparse.pool, params, rays, a.step, 0.0, 0.0, g_rgb, out=grads, face_sum=False)
            for fn in legs.values():  # warm-up
                fn()
            ms = {k: [] for k in legs}
            for _ in range(a.reps):
                for k, fn in legs.items():
                    ms[k].append(event_ms(fn, STEPS))
            med = {k: st.median(v) for k, v in ms.items()}
            rows.append({"resolution": n, "degree": degree, "layout": layout, "ms_per_launch": med, "ms_all": {k: sorted(v) for k, v in ms.items()},
                         "ray_bwd_over_points_bwd": med["ray_bwd"] / med["points_bwd"], "ray_bwd_over_forward": med["ray_bwd"] / med["forward"],
                         "hit_share": float((scene.render(rays, a.step)["opacity"] > 0).float().mean())})
            del legs, grads
        if degree == 0:  # the localiser: two photographs rendered by the marcher itself, poses a little off
            w = 64
            Kc = (0.8 * w, 0.8 * w, w / 2, w / 2)
            yy, xx = torch.meshgrid(torch.arange(w, device=dev), torch.arange(w, device=dev), indexing="ij")
            dirs_c = baked_pose.pixel_directions(xx.reshape(-1), yy.reshape(-1), Kc)
            from upnerf_amd.camera import get_rays
            poses = c2w[[0, c2w.shape[0] - 1]].contiguous()
            targets = []
            for p in poses:
                o, d = get_rays(dirs_c, p)
                targets.append(dense.render(torch.cat([o, d, nf[:1].expand(w * w, 2)], 1).contiguous(), a.step)["rgb"].view(w, w, 3))
            init = poses.clone()
            init[:, :, 3] += 0.01
            loc = baked_pose.BakedLocaliser(dense, torch.stack(targets), Kc, init, nf[0].tolist(), lr=1e-3)
            lgen = torch.Generator(device="cpu").manual_seed(7)
            one = lambda: loc.step(4096, a.step, lgen)
            one()
            its = [1e3 / event_ms(one, 20) for _ in range(a.reps)]
            localiser = {"images": 2, "pixels_per_image": w * w, "batch": 4096, "iterations_per_s": st.median(its), "all": sorted(its)}
        del dense, sparse
        torch.cuda.empty_cache()
    out = {"metric": "the baked marcher's ray gradient (upnerf_baked_ray_bwd) beside the forward and the points backward of the same scene, and one localiser step; analytic shell, random upstream gradients",
           "rays": R, "step": a.step, "reps": a.reps, "launches_per_timing": STEPS, "bounds": [list(b) for b in BOUNDS], "rows": rows, "localiser": localiser,
           "note": "an analytic shell, not a trained scene: the hit share is the shell's"}
    os.makedirs(os.path.dirname(os.path.abspath(a.pose_out)), exist_ok=True)
    with open(a.pose_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def sparse_main(a, sysm, path, dev):
    import ctypes as C
    import statistics as st
    from upnerf_amd import _lib, baked as bk, novel_view
    from upnerf_amd.baked import BakedScene, sphere_directions
    from upnerf_amd.geometry import density_grid
    from upnerf_amd.novel_view import render_path
    from upnerf_amd.ops import TIMER
    F, W, H = a.frames, a.width, a.height
    rays = F * H * W
    frame0 = novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                  (W, H), path.K, 0, H * W)[0]

    def kernel_ms(scene, name):
        TIMER.reset()
        TIMER.enabled, TIMER.only = True, {name}
        render_path(sysm, path, outputs=("rgb",), baked=scene, baked_step=a.step)
        v = TIMER.summary()[name]
        TIMER.enabled, TIMER.only = False, None
        TIMER.reset()
        return v["avg_ms"]

    marcher = []
    for n in (128, 256):
        for degree in (0, 2):
            if degree == 0:
                dense = BakedScene.from_grids(*shell_grids(n, dev), BOUNDS, 1.0)
            else:
                dirs = sphere_directions(12)
                sigma, rgb_dirs = shell_grids(n, dev, dirs)
                dense = BakedScene.from_direction_grids(sigma, rgb_dirs, dirs, BOUNDS, 1.0, sh_degree=2)
                del sigma, rgb_dirs
            sparse = dense.sparsify()
            legs = {"dense": dense, "sparse": sparse}
            frames = {k: render_path(sysm, path, outputs=("rgb_float",), baked=sc, baked_step=a.step)["rgb_float"] for k, sc in legs.items()}  # warm-up
            times, ms = {k: [] for k in legs}, {k: [] for k in legs}
            for _ in range(a.reps):
                for k, sc in legs.items():
                    times[k].append(wall(lambda: render_path(sysm, path, outputs=("rgb",), baked=sc, baked_step=a.step)))
                for k, sc in legs.items():
                    ms[k].append(kernel_ms(sc, "baked_sparse_render" if sc.sparse else ("baked_sh_render" if degree else "baked_render")))
            row = {"resolution": n, "degree": degree, "occupied_bricks": sparse.n_bricks, "f_b": sparse.brick_fraction,
                   "occupied_cells": sparse.fraction, "same_picture": bool(torch.equal(frames["dense"], frames["sparse"])),
                   "hit_share": float((dense.render(frame0, a.step)["opacity"] > 0).float().mean())}
            for k, sc in legs.items():
                row[k] = {"bytes": sc.nbytes, "ms_per_launch": st.median(ms[k]), "frames_per_s": F / st.median(times[k]), "seconds": sorted(times[k])}
            row["sparse_over_dense"] = row["sparse"]["frames_per_s"] / row["dense"]["frames_per_s"]
            row["dense_ms_over_sparse_ms"] = row["dense"]["ms_per_launch"] / row["sparse"]["ms_per_launch"]
            marcher.append(row)
            del dense, sparse, legs, frames
            torch.cuda.empty_cache()
    # the bake, on bench.py's system (random weights: the density is nearly uniform, so f_b says what this number can show)
    res = tuple(a.resolution)
    grid = density_grid(sysm, BOUNDS, res)
    if a.level is None:
        a.level = float(torch.quantile(grid.reshape(-1)[::max(1, grid.numel() // 1_000_000)].float(), 0.75))
    dirs = sphere_directions(a.dirs)
    made = {}
    bake = lambda sparse: made.__setitem__(sparse, BakedScene.build(sysm, BOUNDS, res, a.level, img_id=a.bake_image, sh_degree=2, dirs=dirs, sparse=sparse))
    bake_s = {k: wall(lambda: bake(k)) for k in (False, True)}
    f_b = made[True].brick_fraction
    bake_out = {"resolution": list(res), "degree": 2, "dirs": a.dirs, "level": a.level, "dense_seconds": bake_s[False], "sparse_seconds": bake_s[True],
                "f_b": f_b, "expected_colour_work_ratio": f_b * (729 / 512) * (32 / 9), "dense_bytes": made[False].nbytes, "sparse_bytes": made[True].nbytes,
                "same_pool": bool(torch.equal(made[True].pool, made[False].sparsify().pool)),
                "pool_records": made[True].pool[..., 0].numel(), "pool_records_that_differ": int((made[True].pool != made[False].sparsify().pool).any(-1).sum()),
                "largest_coefficient_difference": float((made[True].pool[..., :54].contiguous().view(torch.float16).float() -
                                                         made[False].sparsify().pool[..., :54].contiguous().view(torch.float16).float()).abs().max()),
                "note": "random weights: above f_b = 0.20 this shows the cost side only; a trained scene is unchecked"}
    parent = None
    if a.parent_lib:  # the marchers of the parent commit's library beside this build's, on the scenes of --sh: nine instantiations
        from upnerf_amd import baked_tune
        old = C.CDLL(a.parent_lib)
        for name, cls in (("upnerf_baked_render", _lib.BakedRenderArgs), ("upnerf_baked_sh_render", _lib.BakedShRenderArgs),
                          ("upnerf_baked_sparse_render", _lib.BakedSparseRenderArgs), ("upnerf_baked_render_bwd", _lib.BakedRenderBwdArgs)):
            getattr(old, name).argtypes, getattr(old, name).restype = [C.POINTER(cls), C.c_void_p], C.c_int
        scenes = {0: BakedScene.build(sysm, BOUNDS, res, a.level, img_id=a.bake_image, view_dir=(0.0, 0.0, -1.0)),
                  1: BakedScene.build(sysm, BOUNDS, res, a.level, img_id=a.bake_image, sh_degree=1, dirs=dirs), 2: made[False]}
        # the backward on the inputs of --tune: every ray of the path in launches of --chunk, random upstream gradients
        all_rays = novel_view.path_rays(*novel_view.path_poses(path.key_c2w.to(dev), path.key_near_far.to(dev), path.u.to(dev), path.mode),
                                        (W, H), path.K, 0, rays)[0]
        gen = torch.Generator(device="cpu").manual_seed(5)
        g_rgb, g_depth, g_op = (torch.randn(*shape, generator=gen).to(dev) for shape in ((rays, 3), (rays,), (rays,)))
        chunks = [(r0, min(a.chunk, rays - r0)) for r0 in range(0, rays, a.chunk)]

        def bwd_ms(d):
            sc, nb = scenes[d], (d + 1) ** 2
            shape = tuple(reversed(sc.resolution))
            bufs = torch.zeros(shape + (4,), device=dev) if d == 0 else (torch.zeros(shape + (3, nb), device=dev), torch.zeros(shape, device=dev))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r0, n in chunks:
                baked_tune.backward(sc.grid, d, sc.occupancy, sc.bounds, all_rays[r0:r0 + n], a.step, 0.0, 0.0, g_rgb[r0:r0 + n], g_depth[r0:r0 + n],
                                    g_op[r0:r0 + n], out=bufs)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / len(chunks)

        legs = {}
        for d, sc in scenes.items():
            sp = sc.sparsify()
            legs[f"dense{d}"] = lambda sc=sc, d=d: kernel_ms(sc, "baked_sh_render" if d else "baked_render")
            legs[f"sparse{d}"] = lambda sp=sp: kernel_ms(sp, "baked_sparse_render")
            legs[f"bwd{d}"] = lambda d=d: bwd_ms(d)
        new, ms = bk.lib, {(k, w): [] for k in legs for w in ("parent", "this")}
        for _ in range(a.reps + 1):  # (the first round warms up)
            for k, leg in legs.items():
                for w, library in (("parent", old), ("this", new)):
                    bk.lib = baked_tune.lib = library
                    ms[k, w].append(leg())
        bk.lib = baked_tune.lib = new
        parent = {k: {"parent_ms_per_launch": st.median(ms[k, "parent"][1:]), "this_ms_per_launch": st.median(ms[k, "this"][1:]),
                      "parent_over_this": st.median(ms[k, "parent"][1:]) / st.median(ms[k, "this"][1:]),
                      "parent_ms_all": sorted(ms[k, "parent"][1:]), "this_ms_all": sorted(ms[k, "this"][1:])} for k in legs}
    out = {"metric": "sparse baked scenes: the marcher dense against sparse on an analytic shell, the degree-2 bake dense against sparse, the nine marchers against the parent commit's",
           "frames": F, "img_wh": [W, H], "chunk": a.chunk, "step": a.step, "reps": a.reps, "bounds": [list(b) for b in BOUNDS],
           "marcher": marcher, "bake": bake_out, "marchers_vs_parent": parent}
    os.makedirs(os.path.dirname(os.path.abspath(a.sparse_out)), exist_ok=True)
    with open(a.sparse_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
