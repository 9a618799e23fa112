"""Render the frames of a camera path through training images of a trained scene: novel views of the static scene, the
appearance moving from photograph to photograph (upnerf_amd/novel_view.py).

    python tools/render_path.py --config scene.yaml --ckpt last.ckpt --images 3 17 42 --frames 120 --out DIR
                                [--mode linear|catmull] [--downscale N] [--depth] [--loop] [--chunk ROWS]

Writes PNG files only -- DIR/path/step_<frame, 8 digits>/rgb.png (and depth.png with --depth).  No video encoder is installed
with this package: turn the frames into a film with a tool of your own (e.g. ffmpeg -i DIR/path/step_%08d/rgb.png)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True, help="the scene's YAML configuration (as given to training)")
    ap.add_argument("--ckpt", required=True, help="checkpoint of the trained system")
    ap.add_argument("--images", type=int, nargs="+", required=True, help="training image indices the path goes through, in order (at least two)")
    ap.add_argument("--frames", type=int, required=True, help="number of frames, both end keyframes included")
    ap.add_argument("--out", required=True, help="output directory (PNG files only; no video encoder is installed)")
    ap.add_argument("--mode", default="catmull", choices=("linear", "catmull"), help="translation between keyframes")
    ap.add_argument("--downscale", type=int, default=1, help="render at 1/N of the first keyframe image's size")
    ap.add_argument("--depth", action="store_true", help="also write the colour-mapped depth of every frame (one range: frame 0's)")
    ap.add_argument("--loop", action="store_true", help="close the path on the first image")
    ap.add_argument("--chunk", type=int, default=None, help="rows per render chunk (default: val.chunk_size)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("render_path.py renders on the GPU; none is visible")
    from upnerf_amd import checkpoint, config
    from upnerf_amd.nerf_system import NeRFSystem
    from upnerf_amd.novel_view import CameraPath, render_path
    from upnerf_amd.visualization import ImageWriter
    hparams = config.get_from_path(a.config)
    system = NeRFSystem(hparams)
    system.setup()
    checkpoint.load_checkpoint(system, a.ckpt, resume=False)
    system.cuda()
    path = CameraPath.through_images(system, a.images, a.frames, mode=a.mode, loop=a.loop)
    if a.downscale > 1:
        n = a.downscale
        K = path.K.clone()
        K[:2] /= n  # fx, fy, cx, cy of the smaller pixel grid
        path = CameraPath(path.key_c2w, path.key_near_far, path.u, path.i0, path.i1, path.t,
                          (max(1, path.img_wh[0] // n), max(1, path.img_wh[1] // n)), K, path.mode)
    writer = ImageWriter(a.out)
    t0 = time.perf_counter()
    render_path(system, path, chunk=a.chunk, outputs=("rgb", "depth") if a.depth else ("rgb",), sink=writer)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"frames": path.n_frames, "img_wh": list(path.img_wh), "files": len(writer.written), "out": a.out,
                      "seconds": dt, "frames_per_s": path.n_frames / dt}))


if __name__ == "__main__":
    main()
