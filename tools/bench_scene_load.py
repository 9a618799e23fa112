"""Time the scene loader (upnerf_amd/datasets.py) on a synthetic phototourism scene written to a temporary directory:
COLMAP binaries, N JPEGs of W x H, 64 x 64 x 384 feature maps and full-resolution depth maps.  Prints one JSON line with
the phases of the train split (metadata, decode = JPEG decode + LANCZOS + .npy reads, upload, kernels, total, in
seconds) and the buffer sizes.

    python tools/bench_scene_load.py --images 100 --width 1000 --height 750 --downscale 2
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--height", type=int, default=750)
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=2, help="loads of the same scene; the first one warms up")
    args = ap.parse_args()
    import torch
    import scene_synth
    from upnerf_amd.datasets import PhototourismDataset
    tmp = tempfile.mkdtemp(prefix="scene_bench_")
    try:
        t = time.perf_counter()
        info = scene_synth.write_phototourism_scene(tmp, n_images=args.images, size=(args.width, args.height), feat_hw=64,
                                                    splits=["train"] * args.images, n_points=20000)
        write_s = time.perf_counter() - t
        runs = []
        for _ in range(args.repeat):
            ds = PhototourismDataset(tmp, "synth", feat_dir=info["feat_dir"], depth_dir=info["depth_dir"], near=0.1,
                                     far=5.0, camera_noise=-1, split="train", img_downscale=args.downscale)
            runs.append({k: round(v, 4) for k, v in ds.load_times.items()})
            rays = len(ds)
            del ds
            torch.cuda.empty_cache()
        print(json.dumps({"images": args.images, "size": [args.width, args.height], "downscale": args.downscale,
                          "rays": rays, "scene_write_s": round(write_s, 2), "cpus": len(os.sched_getaffinity(0)),
                          "runs": runs}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
