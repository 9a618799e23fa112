"""Cost of the DINO descriptor extractor (upnerf_amd/dino.py, csrc/dino.hip) for one image, split by kernel, against the same
definition evaluated by torch's own ops (ATen GEMMs, scaled_dot_product_attention, fp32) on the same device in the same run.

    python tools/bench_dino.py [--size 448] [--reps 3] [--out profiles/dino.json]

Seeded random dino_vits8-shaped weights (no pretrained file is needed: the cost does not depend on the values).  Writes one JSON
object: ms per image of both routes (median of `--reps` after one warm-up, the two alternating), the per-kernel split of the HIP
route through ops.TIMER (HIP events around each launch), the attention kernel's achieved fraction of the fp32 MFMA peak
(4 N^2 D FLOP per layer), the PCA fit, and the largest difference between the two routes' maps."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3  # 256 CUs x 256 FLOP/clk x 2.4 GHz (the figure bench.py uses)


def random_state_dict(D=384, depth=12, P=28, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    sd = {"cls_token": 0.5 * n(1, 1, D), "pos_embed": 0.5 * n(1, 1 + P * P, D),
          "patch_embed.proj.weight": n(D, 3, 8, 8) * 192 ** -0.5, "patch_embed.proj.bias": 0.1 * n(D)}
    for i in range(depth):
        b = f"blocks.{i}."
        sd[b + "norm1.weight"], sd[b + "norm1.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)
        sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"] = 1.5 * n(3 * D, D) * D ** -0.5, 0.1 * n(3 * D)
        sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"] = n(D, D) * D ** -0.5, 0.1 * n(D)
        sd[b + "norm2.weight"], sd[b + "norm2.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)
        sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = n(4 * D, D) * D ** -0.5, 0.1 * n(4 * D)
        sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = n(D, 4 * D) * (4 * D) ** -0.5, 0.1 * n(D)
    return sd


def aten_descriptors(sd, model, image):
    """The table of upnerf_amd/dino.py in torch ops, fp32, on the image's device."""
    from upnerf_amd.dino import PREPROCESS, key_rows
    D, heads, layer, stride = model.D, model.heads, model.layer, model.stride
    H, W = image.shape[:2]
    h0, w0 = model.grid(H, W)
    x = image.float() / 255
    x = (x - x.new_tensor(PREPROCESS["mean"])) / x.new_tensor(PREPROCESS["std"])
    x = F.conv2d(x.permute(2, 0, 1)[None], sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=stride)
    x = x.flatten(2).transpose(1, 2)[0]
    x = torch.cat([sd["cls_token"].reshape(1, D), x], 0) + model._pos_rows(H, W, image.device)
    N = x.shape[0]
    for i in range(layer):
        b = f"blocks.{i}."
        y = F.layer_norm(x, (D,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], 1e-6)
        qkv = F.linear(y, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]).reshape(N, 3, heads, 64).permute(1, 2, 0, 3)
        a = F.scaled_dot_product_attention(qkv[0][None], qkv[1][None], qkv[2][None])[0].permute(1, 0, 2).reshape(N, D)
        x = x + F.linear(a, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
        y = F.layer_norm(x, (D,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], 1e-6)
        x = x + F.linear(F.gelu(F.linear(y, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"])), sd[b + "mlp.fc2.weight"],
                         sd[b + "mlp.fc2.bias"])
    b = f"blocks.{layer}."
    y = F.layer_norm(x, (D,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], 1e-6)[1:]
    rows = key_rows(D, heads).to(image.device)
    return F.linear(y, sd[b + "attn.qkv.weight"][rows], sd[b + "attn.qkv.bias"][rows]).reshape(h0, w0, D)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dino.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino.py measures on the GPU; none is visible")
    torch.backends.cuda.matmul.allow_tf32 = False
    from upnerf_amd.dino import DinoViT
    from upnerf_amd.ops import TIMER
    sd = random_state_dict()
    model = DinoViT.from_state_dict(sd).to("cuda")
    dsd = {k: v.cuda() for k, v in sd.items()}
    image = torch.randint(0, 256, (a.size, a.size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).cuda()
    h0, w0 = model.grid(a.size, a.size)
    N = h0 * w0 + 1
    with torch.no_grad():
        _, hip = timed(lambda: model.descriptors(image))  # warm-up of both
        _, ref = timed(lambda: aten_descriptors(dsd, model, image))
        diff = float((hip - ref).abs().max() / ref.abs().max())
        t_hip, t_aten, t_pca = [], [], []
        for _ in range(a.reps):
            t_hip.append(timed(lambda: model.descriptors(image))[0])
            t_aten.append(timed(lambda: aten_descriptors(dsd, model, image))[0])
            t_pca.append(timed(lambda: model.fit_pca(hip))[0])
        TIMER.enabled = True
        TIMER.reset()
        model.descriptors(image)
        model.pca_moments(hip)
        kern = TIMER.summary()
        TIMER.enabled = False
    att = kern["dino_attention"]
    att_tflops = att["units_per_launch"] / (att["avg_ms"] * 1e-3) / 1e12
    res = {"image": [a.size, a.size], "tokens": N, "layers_run": model.layer, "reps": a.reps,
           "hip_ms_per_image": statistics.median(t_hip), "aten_ms_per_image": statistics.median(t_aten),
           "fit_pca_ms_per_image_with_host_eigh": statistics.median(t_pca),
           "max_abs_diff_hip_vs_aten_rel_to_max_abs": diff,
           "kernels_ms_per_image": {k: round(v["total_ms"], 4) for k, v in sorted(kern.items())},
           "kernel_launches": {k: v["launches"] for k, v in sorted(kern.items())},
           "attention": {"avg_launch_ms": att["avg_ms"], "tflops": att_tflops, "peak_fp32_mfma_tflops": PEAK_FP32_MFMA_TFLOPS,
                         "frac_of_peak": att_tflops / PEAK_FP32_MFMA_TFLOPS, "flop_per_launch": att["units_per_launch"]},
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
