"""DPT-Large inverse-depth maps for a directory of images, from the dpt_large checkpoint the user supplies: the arguments and
outputs of the reference's preprocess/save_dpt_depth.py, computed by upnerf_amd/dpt.py on the GPU.

    python tools/extract_depth.py -i IMAGES -o DEPTH_DIR -m dpt_large-midas-2f21e586.pt [-t dpt_large] [--tsv_path T]

writes DEPTH_DIR/<stem>.npy ([h][w] fp32 at the photograph's size; the reference writes float16 from an fp16 network).  Files:
the TSV's rows with an id (the rows training uses), else every file of the directory, as tools/extract_features.py selects
them.  <stem> is the file name without its extension.  --optimize / --no-optimize are accepted and ignored (everything here is
fp32); --kitti_crop and every model type but dpt_large raise."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from extract_features import select_files  # noqa: E402


def write_depth(save_dir, name, depth):
    os.makedirs(save_dir, exist_ok=True)
    np.save(os.path.join(save_dir, os.path.splitext(name)[0] + ".npy"), np.asarray(depth, dtype=np.float32))


def run(image_dir, save_dir, extract, tsv_path=None, progress=None):
    """extract(path) -> inverse depth [h][w] for every selected file.  Returns the names."""
    names = select_files(image_dir, tsv_path)
    for n in names:
        write_depth(save_dir, n, extract(os.path.join(image_dir, n)))
        if progress:
            progress(n)
    return names


def make_extractor(weights, model_type="dpt_large", device="cuda", **model_kwargs):
    from upnerf_amd.dpt import DptDepth, load_image
    model = DptDepth.load(weights, model_type, **model_kwargs).to(device)
    return lambda path: model.inverse_depth(load_image(path).to(device)).cpu().numpy()


def main(argv=None, model_kwargs=None):
    """model_kwargs: structure overrides of DptDepth for a weight file that is not dpt_large-shaped (the tests' stub)."""
    from upnerf_amd.dpt import check_model_type
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-i", "--input_path", required=True, help="folder with input images")
    ap.add_argument("-o", "--output_path", required=True, help="folder for the output maps")
    ap.add_argument("--tsv_path", default=None, help="save only the maps that will be used for training")
    ap.add_argument("-m", "--model_weights", required=True, help="the dpt_large checkpoint (a state dict)")
    ap.add_argument("-t", "--model_type", default="dpt_large", help="dpt_large (nothing else is built here)")
    ap.add_argument("--kitti_crop", dest="kitti_crop", action="store_true")
    ap.add_argument("--optimize", dest="optimize", action="store_true", help="accepted, ignored: the network runs in fp32")
    ap.add_argument("--no-optimize", dest="optimize", action="store_false", help="accepted, ignored")
    ap.set_defaults(optimize=True, kitti_crop=False)
    args = ap.parse_args(argv)
    check_model_type(args.model_type)
    if args.kitti_crop:
        raise NotImplementedError("--kitti_crop is not built here")
    extract = make_extractor(args.model_weights, args.model_type, **(model_kwargs or {}))
    names = run(args.input_path, args.output_path, extract, args.tsv_path, progress=lambda n: print(n, flush=True))
    print(f"{len(names)} images -> {args.output_path}")
    return names


if __name__ == "__main__":
    main()
