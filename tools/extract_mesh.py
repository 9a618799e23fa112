"""Write the surface of a trained scene as a coloured triangle mesh (upnerf_amd/geometry.py).

    python tools/extract_mesh.py --ckpt last.ckpt [--config scene.yaml] --level SIGMA --out scene.ply
                                 (--bounds X0 Y0 Z0 X1 Y1 Z1 | --from-cameras MARGIN) [--resolution 256 | NX NY NZ]
                                 [--img-id 0] [--slab S] [--field fine|coarse] [--chunk COLUMNS] [--analytic-normals]
    python tools/extract_mesh.py --config scene.yaml --ckpt last.ckpt --fuse-depth --out scene.ply (--bounds ... | --from-cameras MARGIN)
                                 [--resolution ...] [--images I J ...] [--trunc T] [--downscale N] [--min-weight W] [--chunk RAYS]

--level is the density (sigma, after the softplus) of the surface and has NO default: the useful value depends on the scale of
the scene, so look at the histogram of a coarse grid first (--level with a low --resolution is quick).  With --config the
scene's dataset is loaded, which --from-cameras needs (the box round the refined cameras and their far points); with --ckpt
alone the hyper-parameters come from the checkpoint and the box from --bounds.  Colours are the static colour under the
appearance of training image --img-id, rendered over a slab of thickness 2 S round every vertex (default: one cell diagonal).
--fuse-depth is the alternative to --level (exactly one of the two is given) and needs no threshold: the depth maps rendered from
the refined training poses (all images, or --images; at 1 / --downscale of their size) are fused into a truncated signed distance
volume whose zero level is the surface, kept where at least --min-weight views agree, and the colours are the fused colours of
those renders (geometry.fuse_views).  --trunc is the truncation distance (default: three voxel diagonals);
--chunk is then the number of rays per render call.  It needs the dataset (--config): the poses, intrinsics and image sizes.
--analytic-normals replaces the grid's central-difference normals by the field's own, -grad sigma / |grad sigma| at the vertices
(geometry.refine_normals), before the colouring aims its rays along them.
Prints one JSON line."""
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
    ap.add_argument("--config", help="the scene's YAML configuration (as given to training); loads the dataset")
    ap.add_argument("--ckpt", help="checkpoint of the trained system")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--level", type=float, help="density of the surface (no default: it depends on the scene's scale)")
    how.add_argument("--fuse-depth", action="store_true", help="fuse rendered depth maps into a TSDF and mesh its zero level instead")
    ap.add_argument("--images", type=int, nargs="+", default=None, help="--fuse-depth: training images to fuse (default: all)")
    ap.add_argument("--trunc", type=float, default=None, help="--fuse-depth: truncation distance (default: three voxel diagonals)")
    ap.add_argument("--downscale", type=int, default=1, help="--fuse-depth: render the depth maps at 1 / N of the image size")
    ap.add_argument("--min-weight", type=float, default=1.0, help="--fuse-depth: views that must have seen a voxel")
    ap.add_argument("--out", required=True, help="the PLY file to write")
    box = ap.add_mutually_exclusive_group(required=True)
    box.add_argument("--bounds", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    box.add_argument("--from-cameras", type=float, metavar="MARGIN", help="box round the refined cameras and their far points, grown by MARGIN")
    ap.add_argument("--resolution", type=int, nargs="+", default=[256], help="grid points per axis: one number or NX NY NZ")
    ap.add_argument("--img-id", type=int, default=0, help="training image whose appearance colours the mesh")
    ap.add_argument("--slab", type=float, default=None, help="half thickness of the slab rendered round a vertex (default: a cell diagonal)")
    ap.add_argument("--field", default="fine", choices=("fine", "coarse"))
    ap.add_argument("--chunk", type=int, default=None, help="grid columns per field launch (default: about a million samples)")
    ap.add_argument("--analytic-normals", action="store_true", help="vertex normals from the field's analytic gradient, not the grid's differences")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    if not a.config and not a.ckpt:
        raise SystemExit("give --ckpt, --config or both")
    if len(a.resolution) not in (1, 3):
        raise SystemExit("--resolution takes one number or three")
    res = tuple(a.resolution * 3 if len(a.resolution) == 1 else a.resolution)
    if not torch.cuda.is_available():
        raise SystemExit("extract_mesh.py runs on the GPU; none is visible")
    from _system import load_system
    from upnerf_amd import geometry
    system = load_system(a.config, a.ckpt, need_dataset=a.from_cameras is not None)
    t0 = time.perf_counter()
    bounds = (geometry.bounds_from_cameras(system, a.from_cameras) if a.from_cameras is not None
              else (tuple(a.bounds[:3]), tuple(a.bounds[3:])))
    if a.fuse_depth:
        if not a.config:
            raise SystemExit("--fuse-depth renders the training views: give --config (poses, intrinsics, image sizes)")
        vol = geometry.fuse_views(system, bounds, res, img_ids=a.images, trunc=a.trunc, downscale=a.downscale, chunk=a.chunk)
        mesh = vol.extract(min_weight=a.min_weight)
        if a.analytic_normals and mesh.vertices.shape[0]:
            mesh = geometry.refine_normals(system, mesh, field=a.field)
        mesh.write_ply(a.out)
        torch.cuda.synchronize()
        print(json.dumps({"out": a.out, "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]),
                          "resolution": list(res), "bounds": [list(bounds[0]), list(bounds[1])], "fuse_depth": True,
                          "views": vol.n_views, "trunc": vol.trunc, "min_weight": a.min_weight, "downscale": a.downscale,
                          "observed": float((vol.weight >= a.min_weight).float().mean()),
                          "analytic_normals": bool(a.analytic_normals), "seconds": time.perf_counter() - t0}))
        return
    grid = geometry.density_grid(system, bounds, res, field=a.field, chunk=a.chunk)
    mesh = geometry.extract_surface(grid, bounds, a.level)
    slab = a.slab
    if slab is None:
        slab = sum(((h - l) / max(n - 1, 1)) ** 2 for l, h, n in zip(bounds[0], bounds[1], res)) ** 0.5
    if a.analytic_normals and mesh.vertices.shape[0]:
        mesh = geometry.refine_normals(system, mesh, field=a.field)
    if mesh.vertices.shape[0]:
        mesh.colours = geometry.colour_vertices(system, mesh, a.img_id, slab)
    mesh.write_ply(a.out)
    torch.cuda.synchronize()
    print(json.dumps({"out": a.out, "vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0]),
                      "resolution": list(res), "bounds": [list(bounds[0]), list(bounds[1])], "level": a.level, "slab": slab, "analytic_normals": bool(a.analytic_normals),
                      "sigma_min": float(grid.min()), "sigma_max": float(grid.max()), "seconds": time.perf_counter() - t0}))


if __name__ == "__main__":
    main()
