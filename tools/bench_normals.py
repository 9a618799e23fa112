"""Time the two routes to the density gradient at a million points and write profiles/normals.json.

    python tools/bench_normals.py [--points 1048576] [--reps 11] [--out profiles/normals.json]

Route "fused": upnerf_density_grad, one launch, nothing of size M x W in HBM.
Route "train": what a user had before -- upnerf_field_fwd with everything a training pass stores (x0, every layer's
activations, the mask words), then upnerf_field_bwd with a unit seed on d_sigma_s, need_dxyz = 1 and no heads, which also
writes the weight-gradient operands gz_h / gz_e that nobody reads.  Both are fp32 MFMA, both called at the C ABI on the same
points, alternating in one process; the figure is the median HIP-event time.  W = 256: the fine field of bench.py's synthetic
system; W = 64: a field of the same depth with synth.nerf_state weights.  The byte counts are what each route must move,
counted from the shapes (weights, re-read from L2 by every workgroup, are left out of both)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hbm_bytes(M, W, D):
    """Bytes per route, from the shapes: fp32 everywhere, mask words 8 B per thread, 256 threads per 64-point tile and layer."""
    tiles = (M + 63) // 64
    masks = D * tiles * 256 * 8
    fused = M * 12 + M * 4 + M * 12                                   # points in; sigma, grad out
    fwd = M * (12 + 12 + 4) + M * 4 + M * 64 * 4 + D * M * W * 4 + masks   # o, d, z in; sigma, x0, h, masks out
    fwd += M * 64 * 4                                                # the skip layer re-reads x0
    bwd = M * 4 * 2 + masks + M * 4 + D * M * W * 4 + M * W * 4 + M * 64 * 4 + M * 12   # seed, sigma, masks in; dpre, gz_h, gz_e out; x0 in; dxyz out
    return {"fused": fused, "train": fwd + bwd}


def routes(model, pts):
    from upnerf_amd import _lib
    from upnerf_amd._lib import lib, ptr
    from upnerf_amd.rendering import band_weights
    pk, L = model.packer, model.packer.L
    W, D, M, dev = pk.W, pk.D, pts.shape[0], pts.device
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    P = model.packed().detach().contiguous()
    PF, PT = pk.frag_hip(P), pk.frag_t_hip(P)
    wk = (C.c_float * 10)(*band_weights(model.xyz_L, 0.3, model.c2f))
    st = torch.cuda.current_stream().cuda_stream
    sigma, grad = f(M), f(M, 3)
    ga = _lib.DensityGradArgs(M=M, points=ptr(pts), P=ptr(PF), PT=ptr(PT), wk_xyz=wk, sigma=ptr(sigma), grad=ptr(grad))
    d, z = torch.zeros(M, 3, device=dev), torch.zeros(M, 1, device=dev)
    sig2, x0, h = f(M), f(M, _lib.X0), f(D, M, W)
    hmask = torch.empty((D + 1) * ((M + 127) // 128) * 512, device=dev, dtype=torch.int64)
    fa = _lib.FieldFwdArgs(R=M, S=1, use_cand=0, use_rgb=0, rays_o=ptr(pts), rays_d=ptr(d), z=ptr(z), wk_xyz=wk, P=ptr(PF),
                           sigma_s=ptr(sig2), x0=ptr(x0), h=ptr(h), hmask=ptr(hmask))
    ones, gz_h, gz_e, dpre, dxyz = torch.ones(M, device=dev), f(D, M, W), f(M, W), f(M), f(M, 3)
    fb = _lib.FieldBwdArgs(R=M, S=1, use_cand=0, use_rgb=0, need_dxyz=1, PT=ptr(PT), P=ptr(PF), d_sigma_s=ptr(ones),
                           sigma_s=ptr(sig2), x0=ptr(x0), h=ptr(h), hmask=ptr(hmask), gz_h=ptr(gz_h), gz_e=ptr(gz_e),
                           dpre_sig_s=ptr(dpre), dxyz=ptr(dxyz))
    keep = (PF, PT, d, z, ones, pts)  # (the structs hold raw pointers)

    def fused():
        rc = lib.upnerf_density_grad(C.byref(L), C.byref(ga), st)
        if rc:
            raise RuntimeError(f"upnerf_density_grad: {rc}")

    def train():
        rc = lib.upnerf_field_fwd(C.byref(L), C.byref(fa), st) or lib.upnerf_field_bwd(C.byref(L), C.byref(fb), st)
        if rc:
            raise RuntimeError(f"upnerf_field_fwd / bwd: {rc}")
    return fused, train, (grad, dxyz), keep


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals.py runs on the GPU; none is visible")
    import bench
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    dev = torch.device("cuda", 0)
    M = a.points
    pts = (synth.uniform("bench_normals.points", (M, 3), 1)).to(dev).contiguous()
    m64 = NeRF("fine", D=8, W=64, skips=[4], xyz_L=10, dir_L=4, c2f=(0.1, 0.5))
    m64.load_state_dict(synth.nerf_state("fine", D=8, W=64, seed=0, trunk_gain=2.5))
    models = {256: bench.build_system(dev, 0.3).models["nerf_fine"], 64: m64.to(dev)}
    result = {"points": M, "reps": a.reps, "device": torch.cuda.get_device_name(0), "fields": {}}
    for W, model in models.items():
        fused, train, (g1, g2), keep = routes(model, pts)
        for _ in range(2):
            fused(), train()
        torch.cuda.synchronize()
        t = {"fused": [], "train": []}
        for _ in range(a.reps):  # alternating, one process
            t["fused"].append(timed(fused))
            t["train"].append(timed(train))
        ms = {k: statistics.median(v) for k, v in t.items()}
        by = hbm_bytes(M, W, model.packer.D)
        diff = float((g1 - g2).abs().max() / g2.norm(dim=1).max())
        result["fields"][f"W{W}"] = {"W": W, "D": model.packer.D, "ms": ms, "hbm_bytes": by, "speedup_fused_over_train": ms["train"] / ms["fused"],
                                     "bytes_ratio_train_over_fused": by["train"] / by["fused"], "max_rel_difference_of_the_routes": diff}
        del keep
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
