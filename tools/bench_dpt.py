"""DPT-Large inverse depth of one image on seeded random dpt_large-shaped weights (upnerf_amd/dpt.py): the whole
image, the split over its library calls, and the same definition in torch's own fp32 operators (ATen / MIOpen: the fp32
evaluation of tests/dpt_ref.py on the device) alternating with it in the same run.

    python tools/bench_dpt.py [--size 384x512] [--repeats 5] [--out profiles/dpt.json]

The image is timed with a host clock round calls that end in a synchronise, the two routes alternating; the split with device
events round each library call (ops.TIMER), one extra pass.  FLOP counts are 2 * C_out * 9 * C_in per output pixel for the
3 x 3 convolutions, against the 157.3 TFLOP/s fp32-MFMA peak.  Prints the JSON it writes."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_TFLOPS = 157.3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="384x512", help="network input HxW")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--depth", type=int, default=24, help="blocks in the random weights (24: dpt_large)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpt.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_dpt.py measures on the GPU; none is visible")
    import dpt_ref as R
    from upnerf_amd.dpt import MODEL, DptDepth
    from upnerf_amd.ops import TIMER
    H, W = (int(v) for v in a.size.lower().split("x"))
    hooks = MODEL["hooks"] if a.depth == 24 else tuple((k + 1) * a.depth // 4 - 1 for k in range(4))
    cfg = dict(D=MODEL["width"], heads=MODEL["heads"], depth=a.depth, hooks=hooks, stage_widths=MODEL["stage_widths"],
               fusion=MODEL["fusion"], head=MODEL["head"], P=24, seed=0)
    sd = R.make_params(**cfg)
    model = DptDepth.from_state_dict(sd, **R.model_kwargs(cfg)).to("cuda")
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    x = R.make_input(H, W, 0, torch.float32).cuda()

    def hip():
        return model.forward_net(x)

    def aten():
        with torch.no_grad():
            return R.forward_net(sd_dev, x, dtype=torch.float32, **cfg)[0]

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out_hip, out_aten = hip().clone(), aten()  # (warm-up of both routes: code objects, MIOpen's choice of algorithms)
    once(hip), once(aten)
    t_hip, t_aten = [], []
    for _ in range(a.repeats):
        t_hip.append(once(hip))
        t_aten.append(once(aten))
    diff = float((out_hip - out_aten).abs().max())
    TIMER.reset()
    TIMER.enabled = True
    hip()
    split = TIMER.summary()
    TIMER.enabled = False
    kernels, conv_flop, conv_ms = {}, 0.0, 0.0
    for name in sorted(split):
        s = split[name]
        kernels[name] = {"launches": s["launches"], "ms": s["total_ms"]}
        if s["units_per_launch"]:
            flop = s["units_per_launch"] * s["launches"]
            kernels[name].update(GFLOP=flop / 1e9, TFLOP_per_s=flop / (s["total_ms"] * 1e-3) / 1e12)
            if name.startswith("dpt_conv3x3"):
                conv_flop, conv_ms = conv_flop + flop, conv_ms + s["total_ms"]
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "H": H, "W": W, "depth": a.depth,
           "weights": "random dpt_large-shaped (seed 0)", "repeats": a.repeats,
           "hip_image_ms": statistics.median(t_hip), "hip_image_ms_all": t_hip,
           "aten_image_ms": statistics.median(t_aten), "aten_image_ms_all": t_aten,
           "max_abs_diff_hip_vs_aten": diff, "map_max_abs": float(out_aten.abs().max()),
           "finite": bool(torch.isfinite(out_hip).all()),
           "kernels_ms": sum(k["ms"] for k in kernels.values()), "kernels": kernels,
           "conv3x3": {"GFLOP": conv_flop / 1e9, "ms": conv_ms, "TFLOP_per_s": conv_flop / (conv_ms * 1e-3) / 1e12 if conv_ms else None,
                       "share_of_fp32_mfma_peak": conv_flop / (conv_ms * 1e-3) / 1e12 / PEAK_TFLOPS if conv_ms else None},
           "peak_hbm_gb": torch.cuda.max_memory_allocated() / 2 ** 30}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
