"""Register photographs against a baked scene: refine their camera poses by gradient descent through the baked marcher
(upnerf_amd/baked_pose.py).  No field and no checkpoint is needed, only the scene's .npz.

    python tools/localise.py --load-baked scene.npz --images DIR | FILE [FILE ...] --init poses.npy --K FX FY CX CY
                             --near-far N F --step DT --out poses.npy [--iters 200] [--batch 4096] [--lr 0.01] [--seed 0]
                             [--downscale N] [--background G]

--images: a directory (its .png / .jpg / .jpeg files in sorted order) or the files themselves, all of one size, decoded as the
datasets decode them (upnerf_amd/datasets.py: decode_image); --downscale N shrinks them N times, and K with them.  --init: a .npy
[N, 3, 4] (or [3, 4] for one photograph) of camera-to-world poses in the scene's frame and the project's camera convention (x
right, y up, looking down -z), one per photograph, in the order of the images.  --K: the pinhole intrinsics of the photographs
at full size.  --step: the marcher's sample spacing (no default: it depends on the scene's scale).

Writes --out, a .npy [N, 3, 4] of the refined poses, and prints one JSON line with the first and last loss.  How far off a pose
may start and still be pulled in depends on the scene and the photograph; the loss curve says whether it was."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

EXTENSIONS = (".png", ".jpg", ".jpeg")


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--load-baked", required=True, help="the baked scene's .npz (tools/render_path.py --save-baked)")
    ap.add_argument("--images", nargs="+", required=True, help="a directory of photographs, or the files")
    ap.add_argument("--init", required=True, help=".npy [N, 3, 4]: the poses to start from")
    ap.add_argument("--K", type=float, nargs=4, required=True, metavar=("FX", "FY", "CX", "CY"), help="intrinsics of the photographs at full size")
    ap.add_argument("--near-far", type=float, nargs=2, required=True, metavar=("N", "F"))
    ap.add_argument("--step", type=float, required=True, help="sample spacing of the marcher along a ray")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=4096, help="pixels per iteration, drawn over all photographs")
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--downscale", type=int, default=1, help="work at 1/N of the photographs' size")
    ap.add_argument("--background", type=float, default=0.0, help="grey level of what the scene does not cover (not looked at where the loaded scene carries an environment map: that is shown instead)")
    ap.add_argument("--out", required=True, help=".npy [N, 3, 4]: the refined poses")
    return ap


def image_files(args):
    if len(args) == 1 and os.path.isdir(args[0]):
        files = sorted(os.path.join(args[0], f) for f in os.listdir(args[0]) if f.lower().endswith(EXTENSIONS))
    else:
        files = list(args)
    if not files:
        raise SystemExit("--images names no photograph")
    return files


def main(argv=None):
    a = parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("localise.py runs on the GPU; none is visible")
    if a.iters < 1 or a.batch < 1 or a.downscale < 1:
        raise SystemExit("--iters, --batch and --downscale are positive")
    from upnerf_amd.baked import BakedScene
    from upnerf_amd.baked_pose import localise
    from upnerf_amd.datasets import decode_image
    dev = torch.device("cuda", 0)
    files = image_files(a.images)
    images = [decode_image(f, a.downscale) for f in files]
    if len({im.shape for im in images}) != 1:
        raise SystemExit("the photographs are not all of one size")
    init = np.load(a.init).astype(np.float32)
    init = init[None] if init.ndim == 2 else init
    if init.shape != (len(files), 3, 4):
        raise SystemExit(f"--init holds poses of shape {init.shape}; {len(files)} photographs need [{len(files)}, 3, 4]")
    scene = BakedScene.load(a.load_baked, dev)
    targets = torch.from_numpy(np.stack(images)).to(dev).to(torch.float32) / 255.0
    K = [k / a.downscale for k in a.K]
    t0 = time.perf_counter()
    poses, curve = localise(scene, targets, K, torch.from_numpy(init).to(dev), tuple(a.near_far), iters=a.iters, batch=a.batch,
                            baked_step=a.step, seed=a.seed, lr=a.lr, background=a.background)
    dt = time.perf_counter() - t0
    np.save(a.out, poses.cpu().numpy())
    print(json.dumps({"photographs": len(files), "img_wh": [int(targets.shape[2]), int(targets.shape[1])], "iters": a.iters, "batch": a.batch,
                      "env_size": scene.env.E if scene.env is not None else None, "loss_first": curve[0], "loss_last": curve[-1], "seconds": dt, "iterations_per_s": a.iters / dt, "out": a.out}))


if __name__ == "__main__":
    main()
