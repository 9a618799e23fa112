"""Render the frames of a camera path through training images of a trained scene: novel views of the static scene, the
appearance moving from photograph to photograph (upnerf_amd/novel_view.py).

    python tools/render_path.py --config scene.yaml --ckpt last.ckpt --images 3 17 42 --frames 120 --out DIR
                                [--mode linear|catmull] [--downscale N] [--depth] [--normals] [--loop] [--chunk ROWS]
                                [--occupancy NX NY NZ --level SIGMA [--dilate K] [--bounds X0 Y0 Z0 X1 Y1 Z1 | --margin M]]
                                [--baked NX NY NZ --level SIGMA --step DT [--bake-image ID] [--save-baked F | --load-baked F]
                                 [--baked-sh {1,2} [--baked-dirs K]] [--baked-sparse] [--baked-tune ITERS [--baked-tune-lr LR] [--baked-tune-pool]
                                  [--baked-tv LS LC] [--baked-upsample-at I [I ...]]
                                  [--baked-prune-at I [I ...] [--baked-prune-weight W]]] [--baked-env E [--baked-env-far T]]]

--occupancy skips empty space: the fine field's density is sampled on NX x NY x NZ grid points over the box (--bounds, or the
box round the refined cameras and their far points grown by --margin), cells with a corner >= --level (grown by --dilate
rounds) are kept, and only the rays that touch such a cell are rendered, over the part of the ray that does.  A skipped pixel
shows the background, NOT what the full render would have composited from density below --level: --level (no default, as in
tools/extract_mesh.py) and --dilate trade speed for that.

--baked renders a PREVIEW without the field: the fine field is sampled once into a colour-density grid of NX x NY x NZ points over
the same box (points below --level are dropped), with the appearance of training image --bake-image (default: the first of
--images) and for ONE viewing direction, the mean optical axis of the training cameras -- a baked scene has no view dependence
and one appearance -- and every frame is marched from that grid with samples --step apart (upnerf_amd/baked.py).
--baked-sh 1 | 2 gives the preview its view dependence back: the colour head is sampled for --baked-dirs directions (default 48,
a Fibonacci lattice on the whole sphere: that many passes over the field), a spherical-harmonic expansion of that degree is
fitted per grid point, and each ray evaluates it for its own direction (32 or 64 bytes a point instead of 16).
--baked-sparse stores only the occupied 8 x 8 x 8-cell bricks of that grid and evaluates the colour only there (the picture is
bit for bit the dense scene's; the colour passes cost about 5.06 times the occupied share of the bricks of the dense bake's, so
it pays below a share of 0.20, which is what a fine grid of a real scene has).
--baked-tune ITERS fits the baked grid, before it is rendered or saved, to the field's own renders of the path's keyframe cameras
under the baked appearance: ITERS iterations of Adam through the marcher's backward pass (upnerf_amd/baked_tune.py).
A --baked-sparse scene is made dense for that and stored sparse again, unless --baked-tune-pool is given: then the pool is tuned in
place, with no buffer the size of the grid (upnerf_amd/baked_sparse_tune.py; the bricks stay the bake's).
--baked-tv LS LC adds a total variation penalty to --baked-tune (weights of sigma and of the colour, per occupied cell), and
--baked-upsample-at I [I ...] doubles the grid's resolution before each listed iteration, dense to dense or pool to pool
(upnerf_amd/baked_reg.py): the rendered and saved scene has the final resolution.
--baked-prune-at I [I ...] drops, before each listed iteration (and before an upsampling of the same iteration), the grid points
to which the keyframe cameras' rays give a compositing weight below --baked-prune-weight W (default: the points none of them sees
at all), and with them the bricks of a pool that are left empty (upnerf_amd/baked_prune.py).
--baked-env E also bakes an environment: a cube map of E cells per face side of what the field shows from the box centre outwards
(to --baked-env-far, default the training images' largest far plane), composited behind the march instead of the flat backdrop
(upnerf_amd/baked_env.py); it has no parallax.  The tuners keep it frozen and it is saved with the grid.
--save-baked writes the grid to an .npz, --load-baked renders from one (then NX NY NZ, --level, the degree and the layout are those
of the file).
--depth works, --normals and --occupancy do not.

Writes PNG files only -- DIR/path/step_<frame, 8 digits>/rgb.png (and depth.png with --depth, normal.png with
--normals: the world-space normal map, (n + 1) / 2, mid-grey where nothing was hit).  No video encoder is installed
with this package: turn the frames into a film with a tool of your own (e.g. ffmpeg -i DIR/path/step_%08d/rgb.png)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="the scene's YAML configuration (as given to training)")
    ap.add_argument("--ckpt", required=True, help="checkpoint of the trained system")
    ap.add_argument("--images", type=int, nargs="+", required=True, help="training image indices the path goes through, in order (at least two)")
    ap.add_argument("--frames", type=int, required=True, help="number of frames, both end keyframes included")
    ap.add_argument("--out", required=True, help="output directory (PNG files only; no video encoder is installed)")
    ap.add_argument("--mode", default="catmull", choices=("linear", "catmull"), help="translation between keyframes")
    ap.add_argument("--downscale", type=int, default=1, help="render at 1/N of the first keyframe image's size")
    ap.add_argument("--depth", action="store_true", help="also write the colour-mapped depth of every frame (one range: frame 0's)")
    ap.add_argument("--normals", action="store_true", help="also write the world-space normal map of every frame")
    ap.add_argument("--loop", action="store_true", help="close the path on the first image")
    ap.add_argument("--chunk", type=int, default=None, help="rows per render chunk (default: val.chunk_size)")
    ap.add_argument("--occupancy", type=int, nargs=3, metavar=("NX", "NY", "NZ"), help="skip empty space with an occupancy grid of this many grid points")
    ap.add_argument("--level", type=float, default=None, help="density above which a cell is kept (required with --occupancy; no default)")
    ap.add_argument("--dilate", type=int, default=1, help="rounds of 26-neighbour dilation of the kept cells")
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"), help="box of the occupancy grid")
    ap.add_argument("--margin", type=float, default=0.5, help="without --bounds: the box round the cameras and their far points, grown by this")
    ap.add_argument("--baked", type=int, nargs=3, metavar=("NX", "NY", "NZ"), help="render from a colour-density grid of this many grid points instead of the field")
    ap.add_argument("--step", type=float, default=None, help="sample spacing of the baked render along a ray (required with --baked / --load-baked; no default)")
    ap.add_argument("--bake-image", type=int, default=None, help="training image whose appearance is baked (default: the first of --images)")
    ap.add_argument("--baked-sh", type=int, choices=(1, 2), default=None, help="bake a spherical-harmonic expansion of this degree of the colour over the viewing direction (with --baked)")
    ap.add_argument("--baked-dirs", type=int, default=None, help="directions the colour head is sampled for with --baked-sh (default 48)")
    ap.add_argument("--baked-sparse", action="store_true", help="store and bake only the occupied bricks of the grid (with --baked)")
    ap.add_argument("--baked-tune", type=int, default=None, metavar="ITERS", help="after baking, fit the grid to the field's own renders of the path's keyframe cameras for this many Adam iterations (with --baked)")
    ap.add_argument("--baked-tune-lr", type=float, default=None, metavar="LR", help="learning rate of --baked-tune (default 0.01)")
    ap.add_argument("--baked-tune-pool", action="store_true", help="tune a --baked-sparse scene in place on its brick pool instead of through the dense layout (with --baked-sparse and --baked-tune)")
    ap.add_argument("--baked-tv", type=float, nargs=2, default=None, metavar=("LS", "LC"), help="total variation weights of sigma and of the colour in --baked-tune")
    ap.add_argument("--baked-upsample-at", type=int, nargs="+", default=None, metavar="I", help="double the grid's resolution before these iterations of --baked-tune")
    ap.add_argument("--baked-prune-at", type=int, nargs="+", default=None, metavar="I", help="prune the grid by what the keyframe cameras see before these iterations of --baked-tune")
    ap.add_argument("--baked-prune-weight", type=float, default=None, metavar="W", help="the compositing weight below which --baked-prune-at drops a point (default: only what no ray sees)")
    ap.add_argument("--baked-env", type=int, default=None, metavar="E", help="also bake an environment map of E cells per cube face side and show it behind the grid (with --baked)")
    ap.add_argument("--baked-env-far", type=float, default=None, metavar="T", help="far end of the environment's rays (default: the largest far plane of the training images)")
    ap.add_argument("--save-baked", default=None, help="write the baked grid to this .npz")
    ap.add_argument("--load-baked", default=None, help="render from the baked grid of this .npz instead of baking")
    return ap


def check_args(a):
    if a.occupancy is not None and a.level is None:
        raise SystemExit("--occupancy needs --level: the useful density threshold depends on the scene's scale")
    baked = a.baked is not None or a.load_baked is not None
    if a.baked is not None and a.load_baked is not None:
        raise SystemExit("--baked bakes a grid, --load-baked reads one: give one of them")
    if a.baked is not None and a.level is None:
        raise SystemExit("--baked needs --level: the useful density threshold depends on the scene's scale")
    if baked and a.step is None:
        raise SystemExit("a baked render needs --step: the sample spacing depends on the scene's scale")
    if baked and (a.occupancy is not None or a.normals):
        raise SystemExit("a baked render has no --normals and carries its own occupancy bits (no --occupancy)")
    if not baked and (a.step is not None or a.bake_image is not None or a.save_baked is not None):
        raise SystemExit("--step, --bake-image and --save-baked belong to --baked")
    if a.baked is None and (a.baked_sh is not None or a.baked_dirs is not None):
        raise SystemExit("--baked-sh and --baked-dirs belong to --baked (a file read with --load-baked carries its own degree)")
    if a.baked is None and a.baked_sparse:
        raise SystemExit("--baked-sparse belongs to --baked (a file read with --load-baked carries its own layout)")
    if a.baked is None and (a.baked_tune is not None or a.baked_tune_lr is not None):
        raise SystemExit("--baked-tune and --baked-tune-lr belong to --baked (the targets are rendered under the appearance the grid is baked with)")
    if a.baked_tune_lr is not None and a.baked_tune is None:
        raise SystemExit("--baked-tune-lr is the learning rate of --baked-tune")
    if a.baked_tune_pool and (a.baked is None or not a.baked_sparse or a.baked_tune is None):
        raise SystemExit("--baked-tune-pool tunes the brick pool of a sparse bake in place: it needs --baked-sparse and --baked-tune")
    if (a.baked_tv is not None or a.baked_upsample_at is not None) and a.baked_tune is None:
        raise SystemExit("--baked-tv and --baked-upsample-at belong to --baked-tune")
    if a.baked_upsample_at is not None and any(not 0 <= i < a.baked_tune for i in a.baked_upsample_at):
        raise SystemExit("--baked-upsample-at lists iterations of --baked-tune: 0 .. ITERS - 1")
    if a.baked_prune_at is not None and a.baked_tune is None:
        raise SystemExit("--baked-prune-at belongs to --baked-tune")
    if a.baked_prune_at is not None and any(not 0 <= i < a.baked_tune for i in a.baked_prune_at):
        raise SystemExit("--baked-prune-at lists iterations of --baked-tune: 0 .. ITERS - 1")
    if a.baked_prune_weight is not None and a.baked_prune_at is None:
        raise SystemExit("--baked-prune-weight is the weight of --baked-prune-at")
    if a.baked_tune is not None and a.baked_tune < 1:
        raise SystemExit("--baked-tune counts iterations: one at least")
    if a.baked is None and (a.baked_env is not None or a.baked_env_far is not None):
        raise SystemExit("--baked-env and --baked-env-far belong to --baked (a file read with --load-baked carries its own environment)")
    if a.baked_env_far is not None and a.baked_env is None:
        raise SystemExit("--baked-env-far is the far end of --baked-env's rays")
    if a.baked_dirs is not None and a.baked_sh is None:
        raise SystemExit("--baked-dirs counts the directions of --baked-sh")
    if a.load_baked is not None and (a.save_baked is not None or a.level is not None or a.bounds is not None):
        raise SystemExit("--load-baked takes the grid, its box and its level from the file")
    if a.occupancy is None and a.baked is None and (a.level is not None or a.bounds is not None):
        raise SystemExit("--level and --bounds belong to --occupancy or --baked")
    return a


def main(argv=None):
    a = check_args(parser().parse_args(argv))
    if not torch.cuda.is_available():
        raise SystemExit("render_path.py renders on the GPU; none is visible")
    from _system import load_system
    from upnerf_amd.novel_view import CameraPath, render_path
    from upnerf_amd.visualization import ImageWriter
    system = load_system(a.config, a.ckpt)
    path = CameraPath.through_images(system, a.images, a.frames, mode=a.mode, loop=a.loop)
    if a.downscale > 1:
        n = a.downscale
        K = path.K.clone()
        K[:2] /= n  # fx, fy, cx, cy of the smaller pixel grid
        path = CameraPath(path.key_c2w, path.key_near_far, path.u, path.i0, path.i1, path.t,
                          (max(1, path.img_wh[0] // n), max(1, path.img_wh[1] // n)), K, path.mode)
    writer = ImageWriter(a.out)
    occ, extra = None, {}
    if a.occupancy is not None:
        from upnerf_amd import geometry, novel_view
        from upnerf_amd.occupancy import OccupancyGrid
        bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:])) if a.bounds else geometry.bounds_from_cameras(system, a.margin)
        tb = time.perf_counter()
        occ = OccupancyGrid.build(system, bounds, a.occupancy, a.level, dilate=a.dilate)
        extra = {"occupied_share": occ.fraction, "bounds": [list(bounds[0]), list(bounds[1])], "level": a.level, "dilate": a.dilate,
                 "occupancy_seconds": time.perf_counter() - tb}
    scene = None
    if a.baked is not None or a.load_baked is not None:
        from upnerf_amd import geometry
        from upnerf_amd.baked import BakedScene, sphere_directions
        tb = time.perf_counter()
        if a.load_baked is not None:
            scene = BakedScene.load(a.load_baked, next(system.parameters()).device)
        else:
            bounds = (tuple(a.bounds[:3]), tuple(a.bounds[3:])) if a.bounds else geometry.bounds_from_cameras(system, a.margin)
            sh = {} if a.baked_sh is None else {"sh_degree": a.baked_sh, "dirs": sphere_directions(48 if a.baked_dirs is None else a.baked_dirs)}
            scene = BakedScene.build(system, bounds, a.baked, a.level, img_id=a.images[0] if a.bake_image is None else a.bake_image, sparse=a.baked_sparse,
                                     env_size=a.baked_env, env_far=a.baked_env_far, **sh)
            if a.baked_tune is not None:  # distil on the path's own keyframe cameras; a sparse scene is tuned dense and stored sparse again
                if a.baked_tune_pool:  # ... unless the pool itself is tuned, in place
                    from upnerf_amd.baked_sparse_tune import distill
                else:
                    from upnerf_amd.baked_tune import distill
                tt = time.perf_counter()
                tuned, curve = distill(system, scene if a.baked_tune_pool else scene.densify(), path, iters=a.baked_tune, batch=a.chunk or system.hparams["val.chunk_size"], baked_step=a.step,
                                       seed=0, lr=0.01 if a.baked_tune_lr is None else a.baked_tune_lr, img_id=a.images[0] if a.bake_image is None else a.bake_image,
                                       tv=tuple(a.baked_tv or (0.0, 0.0)), upsample_at=tuple(a.baked_upsample_at or ()),
                                       prune_at=tuple(a.baked_prune_at or ()), prune_weight=a.baked_prune_weight)
                scene = tuned.sparsify() if a.baked_sparse else tuned  # (a tuned pool is sparse already: sparsify() returns it)
                tune_extra = {"tune_iters": a.baked_tune, "tune_loss_first": curve[0], "tune_loss_last": curve[-1], "tune_seconds": time.perf_counter() - tt}
            if a.save_baked is not None:
                scene.save(a.save_baked)
        torch.cuda.synchronize()
        extra = {"baked_resolution": list(scene.resolution), "bounds": [list(scene.bounds[0]), list(scene.bounds[1])], "level": scene.level,
                 "sh_degree": scene.sh_degree, "sparse": scene.sparse, "occupied_bricks": scene.n_bricks, "brick_share": scene.brick_fraction, "step": a.step, "occupied_share": scene.fraction, "baked_bytes": scene.nbytes,
                 "env_size": scene.env.E if scene.env is not None else None, "env_bytes": scene.env.nbytes if scene.env is not None else 0, "bake_seconds": time.perf_counter() - tb}
        if a.baked_tune is not None:
            extra.update(tune_extra)
    t0 = time.perf_counter()
    render_path(system, path, chunk=a.chunk, outputs=("rgb",) + (("depth",) if a.depth else ()) + (("normal",) if a.normals else ()), sink=writer, occupancy=occ,
                baked=scene, baked_step=a.step)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if occ is not None:
        extra["hit_share"] = novel_view.LAST_STATS["hits"] / max(novel_view.LAST_STATS["rays"], 1)
    print(json.dumps({"frames": path.n_frames, "img_wh": list(path.img_wh), "files": len(writer.written), "out": a.out,
                      "seconds": dt, "frames_per_s": path.n_frames / dt, **extra}))


if __name__ == "__main__":
    main()
