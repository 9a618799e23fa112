"""Mesh extraction on synthetic weights (upnerf_amd/geometry.py): the density pass of a grid, the extraction
passes, and beside them the two rates they are held against -- the fine pass of a validation render (the same field kernel with
its heads) and a plain device copy (the method of tools/hbm_probe.py).  All in one process on one GPU.

    python tools/bench_mesh.py [--resolution 256] [--chunk COLUMNS] [--repeats 3] [--out profiles/mesh_extract.json]

Times are device events round the launches (ops.TIMER) or a host clock round work that ends in a synchronise; bytes are the
compulsory traffic computed from the shapes (formulas in `extraction_bytes`).  Prints the JSON it writes."""
import argparse
import datetime
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def extraction_bytes(N, V, F, levels):
    """Compulsory HBM traffic of the two entry points for N grid points, V vertices, F faces (cached re-reads of neighbours not
    counted).  count: the flags kernel reads the grid (4 N) and writes a mask and a count per point (2 N); each of the two scans
    reads a byte and writes an int per point (5 N) and, above one block, adds the block offsets in place (8 N).  emit: the vertex
    kernel reads masks, scan and grid (9 N) and writes 24 B per vertex; the face kernel reads counts, scan, grid, masks and the
    vertex scan (14 N) and writes 12 B per face."""
    scan = 5 * N + (8 * N if levels > 1 else 0)
    return {"count": 6 * N + 2 * scan, "emit": 23 * N + 24 * V + 12 * F}


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=None, help="grid columns per field launch (default: density_grid's)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pixels", type=int, default=65536, help="rays of the validation render the fine pass is timed in")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU; none is visible")
    import bench
    from upnerf_amd import geometry, rendering, synth
    from upnerf_amd.ops import TIMER
    dev = torch.device("cuda", 0)
    sysm = bench.build_system(dev, 0.8)
    n = a.resolution
    res, bounds = (n, n, n), ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    N = n ** 3

    # ---- density pass: whole call (host clock, synchronised) and the field launches alone (device events)
    grid = geometry.density_grid(sysm, bounds, res, chunk=a.chunk)  # warm-up at the timed shapes
    t_call = timed(lambda: geometry.density_grid(sysm, bounds, res, chunk=a.chunk), a.repeats)
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, {"density_grid"}
    geometry.density_grid(sysm, bounds, res, chunk=a.chunk)
    s = TIMER.summary()["density_grid"]
    density = {"samples": N, "call_ms": t_call * 1e3, "samples_per_s_call": N / t_call, "field_launches": s["launches"],
               "field_kernel_ms": s["total_ms"], "samples_per_s_field_kernel": N / (s["total_ms"] * 1e-3),
               "samples_per_launch": s["units_per_launch"], "field_mode": rendering.FIELD_MODE}

    # ---- the fine pass of a validation render: field_fwd launches with N_samples + N_importance samples per ray
    hp = sysm.hparams
    S_fine = hp["nerf.N_samples"] + hp["nerf.N_importance"]
    b = synth.batch(a.pixels, 763, seed=7)
    b["img_idx"] = torch.full_like(b["img_idx"], 3)
    batch = {k: v.to(dev)[None] for k, v in b.items()}
    TIMER.enabled = False
    sysm.validation_step(batch)  # warm-up
    torch.cuda.synchronize()
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, {"field_fwd"}
    sysm.validation_step(batch)
    torch.cuda.synchronize()
    recs = [(e0.elapsed_time(e1), u) for e0, e1, u in TIMER.records.get("field_fwd", [])]
    TIMER.enabled, TIMER.only = False, None
    chunk_rays = min(hp["val.chunk_size"], a.pixels)
    fine = [(ms, u) for ms, u in recs if u == chunk_rays * S_fine]
    fine_pass = {"launches": len(fine), "samples_per_launch": chunk_rays * S_fine, "samples_per_ray": S_fine,
                 "kernel_ms": sum(ms for ms, _ in fine),
                 "samples_per_s": (sum(u for _, u in fine) / (sum(ms for ms, _ in fine) * 1e-3)) if fine else None}

    # ---- extraction passes on that grid at its median
    level = float(grid.median())
    mesh = geometry.extract_surface(grid, bounds, level)  # warm-up
    V, F = int(mesh.vertices.shape[0]), int(mesh.faces.shape[0])
    del mesh
    t_extract = timed(lambda: geometry.extract_surface(grid, bounds, level), a.repeats)
    TIMER.reset()
    TIMER.enabled, TIMER.only = True, {"mtet_count", "mtet_emit"}
    for _ in range(a.repeats):
        geometry.extract_surface(grid, bounds, level)
    s = TIMER.summary()
    TIMER.enabled, TIMER.only = False, None
    levels = 1 if N <= 1024 else 2 if N <= 1024 ** 2 else 3
    byts = extraction_bytes(N, V, F, levels)
    passes = {k: {"ms": s[f"mtet_{k}"]["avg_ms"], "bytes": byts[k], "GB_per_s": byts[k] / (s[f"mtet_{k}"]["avg_ms"] * 1e-3) / 1e9}
              for k in ("count", "emit")}

    # ---- the copy rate of this box (tools/hbm_probe.py: y.copy_(x), read + write)
    x = torch.empty(1 << 28, device=dev, dtype=torch.float32).normal_()  # 1 GiB
    y = torch.empty_like(x)
    t_copy = timed(lambda: y.copy_(x), 5)
    copy = {"bytes": 2 * x.numel() * 4, "GB_per_s": 2 * x.numel() * 4 / t_copy / 1e9}
    del x, y

    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "resolution": list(res),
           "bounds": [list(bounds[0]), list(bounds[1])], "repeats": a.repeats, "density_pass": density,
           "render_fine_pass": fine_pass, "level": level, "vertices": V, "faces": F, "extract_call_ms": t_extract * 1e3,
           "extract_passes": passes, "copy": copy, "peak_hbm_gb": torch.cuda.max_memory_allocated() / 2 ** 30}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
