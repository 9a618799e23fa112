"""LPIPS (AlexNet) of N image pairs on random weights (upnerf_amd/lpips.py): the whole call and the split over
its twelve library calls, at the reference's validation size and at a full-resolution photo.

    python tools/bench_lpips.py [--sizes 350x500 1200x1600] [--pairs 1] [--repeats 10] [--out profiles/lpips.json]

The call is timed with a host clock round `repeats` calls that end in a synchronise; the split with device events round each
library call (ops.TIMER), one extra pass.  FLOP counts are 2 * C_out * C_in * k * k per output pixel.  Prints the JSON it
writes."""
import argparse
import datetime
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_model(seed=0):
    """He-scaled convolutions, small biases, lin weights in [0, 1): the arithmetic of a real checkpoint without its file."""
    from upnerf_amd.lpips import CONVS, LpipsAlex
    g = torch.Generator().manual_seed(seed)
    convs = [(torch.randn(co, ci, k, k, generator=g) * (2.0 / (ci * k * k)) ** 0.5, 0.1 * torch.randn(co, generator=g))
             for _, co, ci, k, _, _ in CONVS]
    return LpipsAlex(convs, [torch.rand(c[1], generator=g) for c in CONVS])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["350x500", "1200x1600"], help="HxW")
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py measures on the GPU; none is visible")
    from upnerf_amd.metrics import ssim
    from upnerf_amd.ops import TIMER
    model = random_model().to("cuda")
    results = []
    for size in a.sizes:
        H, W = (int(v) for v in size.lower().split("x"))
        g = torch.Generator().manual_seed(H + W)
        pred = torch.rand(a.pairs, 3, H, W, generator=g).cuda()
        gt = (pred + 0.05 * torch.randn(a.pairs, 3, H, W, generator=g).cuda()).contiguous()

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.repeats):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.repeats * 1e3

        call_ms = timed(lambda: model(pred, gt))
        ssim_ms = timed(lambda: ssim(pred, gt))
        TIMER.reset()
        TIMER.enabled = True
        TIMER.only = {f"lpips_{kind}{i}" for kind in ("conv", "pool", "dist") for i in range(5)}
        value = model(pred, gt)
        split = TIMER.summary()
        TIMER.enabled, TIMER.only = False, None
        kernels = {}
        for name in sorted(split):
            s = split[name]
            kernels[name] = {"ms": s["total_ms"]}
            if name.startswith("lpips_conv"):
                kernels[name].update(GFLOP=s["units_per_launch"] / 1e9, TFLOP_per_s=s["units_per_launch"] / (s["total_ms"] * 1e-3) / 1e12)
        results.append({"H": H, "W": W, "pairs": a.pairs, "call_ms": call_ms, "ssim_call_ms": ssim_ms,
                        "kernels_ms": sum(k["ms"] for k in kernels.values()), "kernels": kernels,
                        "lpips": [float(v) for v in value]})
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "weights": "random (seed 0)", "results": results, "peak_hbm_gb": torch.cuda.max_memory_allocated() / 2 ** 30}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
