"""DINO feature maps and their PCA for a directory of images, from a dino_vits8 checkpoint the user supplies: the
arguments and outputs of the reference's preprocess/save_dino_feature.py, computed by upnerf_amd/dino.py on the GPU.

    python tools/extract_features.py --image_dir D --save_dir S --weights dino_vits8.pth [--tsv_path T] [--resize 448]

writes S/feature_maps/<stem>.npy ([h0][w0][384] fp32) and S/pca_infos/<stem>_{mean,components}.npy.  Files: the TSV's rows
with an id (the rows training uses), else every file of the directory.  <stem> is the file name without its last four
characters, as in the reference."""
import argparse
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def select_files(image_dir, tsv_path=None):
    """The reference's selection: the `filename` column of the TSV's rows whose `id` is not empty, in file order; without a
    TSV every entry of the directory."""
    if tsv_path is None:
        return sorted(os.listdir(image_dir))
    with open(tsv_path, newline="") as f:
        return [r["filename"] for r in csv.DictReader(f, delimiter="\t") if (r.get("id") or "").strip()]


def write_features(save_dir, name, feature, mean, components):
    """One image's three files; `name` is the image's file name."""
    stem = name[:-4]
    for sub in ("feature_maps", "pca_infos"):
        os.makedirs(os.path.join(save_dir, sub), exist_ok=True)
    np.save(os.path.join(save_dir, "feature_maps", stem + ".npy"), np.asarray(feature, dtype=np.float32))
    np.save(os.path.join(save_dir, "pca_infos", stem + "_mean.npy"), np.asarray(mean, dtype=np.float32))
    np.save(os.path.join(save_dir, "pca_infos", stem + "_components.npy"), np.asarray(components, dtype=np.float32))


def run(image_dir, save_dir, extract, tsv_path=None, progress=None):
    """extract(path) -> (feature [h0][w0][D], mean [D], components [3][D]) for every selected file.  Returns the names."""
    names = select_files(image_dir, tsv_path)
    for n in names:
        write_features(save_dir, n, *extract(os.path.join(image_dir, n)))
        if progress:
            progress(n)
    return names


def make_extractor(weights, resize, device="cuda"):
    from upnerf_amd.dino import DinoViT, load_image
    model = DinoViT.load(weights).to(device)

    def extract(path):
        desc = model.descriptors(load_image(path, resize).to(device))
        mean, comps = model.fit_pca(desc)
        return desc.cpu().numpy(), mean.cpu().numpy(), comps.cpu().numpy()
    return extract


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--image_dir", required=True, help="directory of data")
    ap.add_argument("--save_dir", required=True, help="save directory")
    ap.add_argument("--weights", required=True, help="the dino_vits8 checkpoint (a state dict)")
    ap.add_argument("--tsv_path", default=None, help="save only the features that will be used for training")
    ap.add_argument("--resize", type=int, default=448, help="image resize")
    args = ap.parse_args(argv)
    names = run(args.image_dir, args.save_dir, make_extractor(args.weights, args.resize), args.tsv_path,
                progress=lambda n: print(n, flush=True))
    print(f"{len(names)} images -> {args.save_dir}")


if __name__ == "__main__":
    main()
