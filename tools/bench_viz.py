"""Cost of the validation pictures (csrc/viz.hip) for one synthetic H x W image with F-wide features, against a plain torch-ops
restatement of the reference's formulas (utils/visualization.py) on the same device, in the same run.

    python tools/bench_viz.py [--height 350] [--width 500] [--feat 384] [--reps 50]

Each product is warmed up, then timed `--reps` times with HIP events around one call each, the two implementations alternating;
the median is reported.  Prints one JSON line: per product the median ms of the kernels and of the torch ops, the bytes the
product must read and write (from the shapes), the GB/s that gives, and `image_set_ms`: the sum over the pictures one
validation image of the shipped `val.log_image_list` needs (3 colour + 3 grey + 3 depth + 2 PCA)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=350)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--feat", type=int, default=384)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_viz.py measures on the GPU; none is visible")
    from upnerf_amd import visualization as viz
    H, W, F = a.height, a.width, a.feat
    n, wh = H * W, (a.width, a.height)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    depth = torch.rand(n, device=dev, generator=g) * 4.4 + 0.1
    rgb = torch.rand(n, 3, device=dev, generator=g)
    grey = torch.rand(n, device=dev, generator=g)
    feat = torch.nn.functional.normalize(torch.randn(n, F, device=dev, generator=g), dim=-1)
    m = torch.randn(F, device=dev, generator=g) * 0.02
    c = torch.nn.functional.normalize(torch.randn(3, F, device=dev, generator=g), dim=-1)
    lut = torch.from_numpy(viz.JET.copy()).to(dev)

    def torch_depth():  # visualization.py:7-23 without the host: nan_to_num, range, normalise, clip, quantise, table look-up
        x = torch.nan_to_num(depth)
        mi, ma = x.min(), x.max()
        t = ((x - mi) / (ma - mi + 1e-8)).clamp_(0, 1)
        return lut[(255 * t).to(torch.uint8).long()].view(H, W, 3)

    def torch_pca():  # visualization.py:26-30, then .mul(255).clamp(0, 255).byte()
        pc = (feat - m[None, :]) @ c.T
        mx, mn = pc.max(), pc.min()
        pc = (pc - mn) / (mx - mn)
        return pc.view(H, W, 3), pc.mul(255).clamp_(0, 255).byte().view(H, W, 3)

    def torch_rgb():
        return rgb.mul(255).clamp_(0, 255).byte().view(H, W, 3)

    def torch_grey():
        return grey.mul(255).clamp_(0, 255).byte()[:, None].expand(n, 3).contiguous().view(H, W, 3)

    products = {
        # name: (kernels, torch ops, bytes read + written)
        "depth": (lambda: viz.depth_image(depth, wh), torch_depth, 2 * 4 * n + 3 * n),  # read twice: range, then colours
        "pca": (lambda: viz.pca_image(feat, m, c, wh), torch_pca, 4 * n * F + 2 * 12 * n + 12 * n + 3 * n),
        "rgb": (lambda: viz.rgb_image(rgb, wh), torch_rgb, 12 * n + 3 * n),
        "grey": (lambda: viz.rgb_image(grey, wh), torch_grey, 4 * n + 3 * n),
    }
    out = {"metric": "validation pictures, ms per product (median of HIP-event timings)", "H": H, "W": W, "F": F, "reps": a.reps}
    for name, (hip, ref, nbytes) in products.items():
        for _ in range(3):
            hip(), ref()
        torch.cuda.synchronize()
        th, tr = [], []
        for _ in range(a.reps):
            th.append(timed(hip))
            tr.append(timed(ref))
        mh, mr = statistics.median(th), statistics.median(tr)
        out[name] = {"hip_ms": mh, "torch_ms": mr, "bytes": nbytes, "hip_gbps": nbytes / mh * 1e-6,
                     "torch_gbps": nbytes / mr * 1e-6, "hip_min_ms": min(th), "torch_min_ms": min(tr)}
    out["image_set_ms"] = 3 * out["rgb"]["hip_ms"] + 3 * out["grey"]["hip_ms"] + 3 * out["depth"]["hip_ms"] + 2 * out["pca"]["hip_ms"]
    out["image_set_torch_ms"] = (3 * out["rgb"]["torch_ms"] + 3 * out["grey"]["torch_ms"] + 3 * out["depth"]["torch_ms"]
                                 + 2 * out["pca"]["torch_ms"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
