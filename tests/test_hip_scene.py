"""upnerf_scene_rays / upnerf_resize_linear (csrc/scene.hip) against CPU torch and an fp64 numpy restatement of OpenCV's
INTER_LINEAR resize, and the datasets built on them (upnerf_amd/datasets.py) end to end: the sampler's batches against
ones assembled on the CPU from the same files by the reference's rules, NeRFSystem / fit_from_config / TTO without
datasets passed in."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import scene_synth

pytestmark = pytest.mark.gpu


# ---- references -----------------------------------------------------------------------------------------------------

def cv_resize_linear(src, W, H):
    """cv2.resize(src, (W, H)) with INTER_LINEAR, restated in fp64 from OpenCV's float coefficients: half-pixel centres,
    edge clamping with a zero weight, horizontal then vertical blend; a same-size resize copies."""
    src = np.asarray(src, dtype=np.float64)
    sq = src.ndim == 2
    if sq:
        src = src[..., None]
    h, w = src.shape[:2]
    if (h, w) == (H, W):
        out = src.copy()
    else:
        def coef(n_dst, n_src):
            # OpenCV's coefficients: scale = 1 / (n_dst / n_src) in double, the source coordinate rounded to float
            # (near x = 64 that rounding is 4e-6 of a pixel, so it is part of what cv2.resize computes)
            f = ((np.arange(n_dst) + 0.5) * (1.0 / (n_dst / n_src)) - 0.5).astype(np.float32)
            s = np.floor(f).astype(np.int64)
            f = (f - s.astype(np.float32)).astype(np.float64)
            lo = s < 0
            f[lo], s[lo] = 0, 0
            hi = s >= n_src - 1
            f[hi], s[hi] = 0, n_src - 1
            return s, np.minimum(s + 1, n_src - 1), f
        x0, x1, fx = coef(W, w)
        y0, y1, fy = coef(H, h)
        hr = lambda rows: rows[:, x0] * (1 - fx)[None, :, None] + rows[:, x1] * fx[None, :, None]
        out = hr(src[y0]) * (1 - fy)[:, None, None] + hr(src[y1]) * fy[:, None, None]
    return out[..., 0] if sq else out


def ref_rays(W, H, K, near, far, idx, x0=0, x1=None, pixels=None):
    """The reference's CPU tensors for one image window: get_ray_directions on kornia's integer grid, ray infos,
    pxl = linspace / (n - 1), ToTensor colours."""
    x1 = W if x1 is None else x1
    xs, ys = torch.linspace(0, W - 1, W), torch.linspace(0, H - 1, H)
    j, i = torch.meshgrid(ys, xs, indexing="ij")
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    d = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)[:, x0:x1].reshape(-1, 3)
    n = d.shape[0]
    ri = torch.cat([near * torch.ones(n, 1), far * torch.ones(n, 1), idx * torch.ones(n, 1)], 1)
    hp, wp = torch.linspace(0, H - 1, H) / (H - 1), torch.linspace(0, W - 1, W) / (W - 1)
    h_, w_ = torch.meshgrid(hp, wp, indexing="ij")
    pxl = torch.stack((h_, w_), -1)[:, x0:x1].reshape(-1, 2)
    out = {"directions": d, "ray_infos": ri, "pxl": pxl}
    if pixels is not None:
        out["rgbs"] = (torch.from_numpy(pixels.copy()).permute(2, 0, 1).float().div(255))[:, :, x0:x1].reshape(3, -1).t()
    return out


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- upnerf_scene_rays ------------------------------------------------------------------------------------------------

def _rand_K(W, H, g):
    K = np.zeros((3, 3), dtype=np.float32)
    K[0, 0], K[1, 1] = np.float32(W * (0.7 + 0.3 * g.random())), np.float32(H * (0.9 + 0.3 * g.random()))
    K[0, 2], K[1, 2] = np.float32(W / 2 + g.random() - 0.5), np.float32(H / 2 + g.random() - 0.5)
    K[2, 2] = 1
    return K


CASES = {
    "odd_one": [(37, 29, None)],
    "2x2": [(2, 2, None)],
    "one_column": [(9, 7, (4, 5))],
    "tto_halves": [(31, 17, (0, 15)), (31, 17, (15, 31))],
    "several": [(40, 30, None), (2, 3, None), (33, 21, (0, 16)), (64, 48, None), (17, 2, (3, 17))],
}


@pytest.mark.parametrize("case", list(CASES))
def test_scene_rays_bit_for_bit(case):
    from upnerf_amd.datasets import scene_rays, upload_pixels
    g = np.random.default_rng(len(case))
    descs, pix, refs = [], [], []
    for k, (W, H, win) in enumerate(CASES[case]):
        x0, x1 = win if win else (0, W)
        K = _rand_K(W, H, g)
        near, far = float(g.uniform(0.01, 1)), float(g.uniform(2, 9))
        p = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        p[0, 0] = (0, 255, 128)
        descs.append(dict(W=W, H=H, x0=x0, x1=x1, K=K, near=near, far=far, img_idx=3 * k + 1))
        pix.append(p)
        refs.append(ref_rays(W, H, K, near, far, 3 * k + 1, x0, x1, p))
    pixels, offs = upload_pixels(pix, "cuda")
    out = scene_rays(descs, pixels, offs, "cuda")
    rows = sum(r["directions"].shape[0] for r in refs)
    for key in ("directions", "ray_infos", "pxl", "rgbs"):
        want = torch.cat([r[key] for r in refs], 0)
        assert out[key].shape[0] == rows and _bits_equal(out[key], want), key
    again = scene_rays(descs, pixels, offs, "cuda")
    for key in out:
        assert _bits_equal(out[key], again[key])


def test_scene_rays_rows_outside_windows_stay_untouched():
    from upnerf_amd import _lib
    W, H, cap = 13, 5, 200
    K = _rand_K(W, H, np.random.default_rng(1))
    tab = (_lib.SceneImage * 2)()
    tab[0] = _lib.SceneImage(W=W, H=H, x0=2, x1=6, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near=0.1, far=5.0,
                             img_idx=0.0, row0=7, pix_off=0)
    tab[1] = _lib.SceneImage(W=W, H=H, x0=6, x1=13, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near=0.1, far=5.0,
                             img_idx=1.0, row0=100, pix_off=W * H * 3)
    pixels = torch.randint(0, 256, (2 * W * H * 3,), dtype=torch.uint8, device="cuda")
    bufs = {k: torch.full((cap, c), float("nan"), device="cuda") for k, c in (("d", 3), ("r", 3), ("p", 2), ("c", 3))}
    table = torch.empty(C.sizeof(tab), dtype=torch.uint8, device="cuda")
    a = _lib.SceneRaysArgs(n_images=2, rows=cap, pix_bytes=pixels.numel(), pixels=_lib.ptr(pixels),
                           directions=_lib.ptr(bufs["d"]), ray_infos=_lib.ptr(bufs["r"]), pxl=_lib.ptr(bufs["p"]),
                           rgbs=_lib.ptr(bufs["c"]))
    assert _lib.lib.upnerf_scene_rays(C.byref(a), tab, _lib.ptr(table), _lib.stream()) == 0
    written = torch.zeros(cap, dtype=torch.bool)
    written[7:7 + 4 * H] = True
    written[100:100 + 7 * H] = True
    for k, b in bufs.items():
        b = b.cpu()
        assert not torch.isnan(b[written]).any(), k
        assert torch.isnan(b[~written]).all(), k
    # refused: a window past the capacity, past the image, H < 2, pixels too short
    for field, val in (("row0", cap - 4 * H + 1), ("x1", W + 1), ("H", 1), ("pix_off", W * H * 3 + 1)):
        bad = (_lib.SceneImage * 2)(tab[0], tab[1])
        setattr(bad[0] if field != "pix_off" else bad[1], field, val)
        assert _lib.lib.upnerf_scene_rays(C.byref(a), bad, _lib.ptr(table), _lib.stream()) == -1, field


# ---- upnerf_resize_linear -------------------------------------------------------------------------------------------

def _resize_dev(arrays, sizes, pre, nears_fars=None):
    from upnerf_amd.datasets import resize_to
    return resize_to(arrays, sizes, pre, "cuda", nears_fars).cpu().numpy()


def _check(got, want, tol=2e-6):
    assert got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30)
    assert err < tol, err


@pytest.mark.parametrize("name,srcs,sizes", [
    ("up_64_to_375x500_c384", [(64, 64, 384)], [(500, 375)]),
    ("two_maps_c384", [(64, 64, 384), (32, 48, 384)], [(500, 375), (21, 13)]),
    ("depth_exact_half", [(60, 80, 1)], [(40, 30)]),
    ("depth_odd_down", [(61, 83, 1), (75, 100, 1)], [(27, 19), (33, 25)]),
    ("one_pixel_wide", [(17, 1, 1), (1, 9, 1), (1, 1, 1)], [(6, 40), (20, 3), (4, 4)]),
    ("one_pixel_wide_c5", [(1, 7, 5), (1, 1, 5)], [(3, 9), (4, 4)]),
    ("c3_scalar_path", [(10, 12, 3)], [(25, 21)]),
])
def test_resize_plain_matches_opencv_restatement(name, srcs, sizes):
    from upnerf_amd import _lib
    g = np.random.default_rng(len(name))
    Cs = {s[2] for s in srcs}
    arrays = [g.standard_normal(s).astype(np.float32) for s in srcs]
    if Cs == {1}:
        arrays = [a[..., 0] for a in arrays]
    got = _resize_dev(arrays, sizes, _lib.RESIZE_PLAIN)
    want = np.concatenate([cv_resize_linear(a, W, H).reshape(-1) for a, (W, H) in zip(arrays, sizes)])
    _check(got, want)
    assert np.array_equal(got, _resize_dev(arrays, sizes, _lib.RESIZE_PLAIN))  # two launches agree bitwise


def test_resize_l2_prestep():
    from upnerf_amd import _lib
    g = np.random.default_rng(7)
    arrays = [g.standard_normal((64, 64, 384)).astype(np.float32), g.standard_normal((8, 8, 384)).astype(np.float32) * 40]
    sizes = [(500, 375), (8, 8)]
    got = _resize_dev(arrays, sizes, _lib.RESIZE_L2)
    want = np.concatenate([cv_resize_linear(a / np.linalg.norm(a.astype(np.float64), axis=-1, keepdims=True), W, H).reshape(-1)
                           for a, (W, H) in zip(arrays, sizes)])
    _check(got, want)
    # same-size maps in place (the train split's feature maps)
    from upnerf_amd.datasets import l2_normalize_
    f = torch.from_numpy(np.stack([arrays[0], g.standard_normal((64, 64, 384)).astype(np.float32)])).cuda()
    ref = f.cpu() / torch.norm(f.cpu(), dim=-1, keepdim=True)
    l2_normalize_(f)
    assert torch.allclose(f.cpu(), ref, rtol=0, atol=2e-7)


def test_resize_invdepth_prestep():
    from upnerf_amd import _lib
    g = np.random.default_rng(9)
    arrays = [g.uniform(-0.5, 3.0, (75, 100)).astype(np.float32), g.uniform(-1, 7.0, (60, 80)).astype(np.float32)]
    sizes = [(50, 37), (40, 30)]
    nf = [(0.1, 5.0), (0.37, 4.2)]
    got = _resize_dev(arrays, sizes, _lib.RESIZE_INVDEPTH, nf)
    want = []
    for a, (W, H), (near, far) in zip(arrays, sizes, nf):
        d = a.copy()
        d[d < 0] = 0
        M, m = 1 / near, 1 / far
        d = d / d.max() * (M - m) + m  # the reference's numpy line, in fp32
        want.append(cv_resize_linear(d, W, H).reshape(-1))
    _check(got, np.concatenate(want))


def test_resize_refuses_bad_tables():
    from upnerf_amd import _lib
    src = torch.zeros(64 * 64 * 4, device="cuda")
    dst = torch.zeros(10 * 10 * 4, device="cuda")
    scratch = torch.empty(256, dtype=torch.uint8, device="cuda")

    def call(C_, m, d=dst):
        tab = (_lib.ResizeMap * 1)(_lib.ResizeMap(**m))
        a = _lib.ResizeArgs(n_maps=1, C=C_, pre=0, src_elems=src.numel(), dst_elems=d.numel(), src=_lib.ptr(src),
                            dst=_lib.ptr(d))
        return _lib.lib.upnerf_resize_linear(C.byref(a), tab, _lib.ptr(scratch), _lib.stream())
    ok = dict(h=64, w=64, H=10, W=10, src_off=0, dst_off=0)
    assert call(4, ok) == 0
    assert call(4, dict(ok, H=11)) == -1          # destination past its capacity
    assert call(4, dict(ok, src_off=4)) == -1     # source past its capacity
    assert call(513, dict(ok, h=1, w=1, H=1, W=1)) == -1
    assert call(4, ok, d=src) == -1               # in place with a size change


# ---- datasets end to end ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    pytest.importorskip("PIL")
    root = str(tmp_path_factory.mktemp("scene"))
    info = scene_synth.write_phototourism_scene(root, n_images=5, size=(41, 31), feat_hw=8, feat_dim=384)
    return info


def _cpu_train_buffers(ds, info):
    """The reference's train buffers (phototourism.py:238-323), assembled on the CPU from the same files."""
    from upnerf_amd.datasets import decode_image
    d, ri, rgb, pxl, feats, invd = [], [], [], [], [], []
    for id_ in ds.img_ids_train:
        im = decode_image(os.path.join(info["root"], "dense/images", ds.image_paths[id_]), ds.scale)
        H, W = im.shape[:2]
        r = ref_rays(W, H, ds.Ks[id_], ds.near, ds.far, ds.id2idx[id_], pixels=im)
        d.append(r["directions"]), ri.append(r["ray_infos"]), rgb.append(r["rgbs"]), pxl.append(r["pxl"])
        f = torch.from_numpy(np.load(os.path.join(info["feat_dir"], "feature_maps", ds.image_paths[id_].replace(".jpg", ".npy"))))
        feats.append(f / torch.norm(f, dim=-1, keepdim=True))
        dm = np.load(os.path.join(info["depth_dir"], ds.image_paths[id_].replace(".jpg", ".npy"))).astype(np.float32)
        dm[dm < 0] = 0
        M, m = 1 / ds.near, 1 / ds.far
        dm = dm / dm.max() * (M - m) + m
        invd.append(torch.from_numpy(cv_resize_linear(dm, W, H).reshape(-1)))
    return {"directions": torch.cat(d), "ray_infos": torch.cat(ri), "rgbs": torch.cat(rgb), "pxl": torch.cat(pxl),
            "feat_maps": torch.stack(feats), "inv_depths": torch.cat(invd)}


def _cpu_batch(ref, ds, idx):
    """phototourism.py:420-454 for every index, collated."""
    fm = ref["feat_maps"]
    h = fm.shape[1]
    out = {"ray_infos": [], "directions": [], "img_idx": [], "c2w": [], "rgbs": [], "feats": [], "inv_depths": []}
    for i in idx.tolist():
        img_idx = ref["ray_infos"][i, 2].long()
        out["ray_infos"].append(ref["ray_infos"][i, :2])
        out["directions"].append(ref["directions"][i])
        out["img_idx"].append(img_idx)
        out["c2w"].append(torch.as_tensor(np.asarray(ds.poses_dict[ds.img_ids_train[img_idx]]), dtype=torch.float32))
        out["rgbs"].append(ref["rgbs"][i])
        pm = ref["pxl"][i] * (h - 1)
        y, x = pm
        y1, x1 = torch.floor(pm).long()
        y2, x2 = min(h - 1, y1 + 1), min(h - 1, x1 + 1)
        f = fm[img_idx]
        out["feats"].append((y2 - y) * (x2 - x) * f[y1, x1] + (y2 - y) * (x - x1) * f[y1, x2]
                            + (y - y1) * (x2 - x) * f[y2, x1] + (y - y1) * (x - x1) * f[y2, x2])
        out["inv_depths"].append(ref["inv_depths"][i])
    return {k: torch.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("downscale", [1, 2])
def test_phototourism_train_buffers_and_sampler(scene_dir, downscale):
    from upnerf_amd.datasets import PhototourismDataset
    from upnerf_amd.ray_sampler import GpuRaySampler
    info = scene_dir
    ds = PhototourismDataset(info["root"], "synth", feat_dir=info["feat_dir"], depth_dir=info["depth_dir"], near=0.1,
                             far=5.0, camera_noise=-1, split="train", img_downscale=downscale)
    assert ds.N_images_train == 4 and ds.N_images_test == 1 and ds.white_back is False
    assert set(ds.load_times) == {"metadata", "decode", "upload", "kernels", "total"}
    ref = _cpu_train_buffers(ds, info)
    for k, name in (("directions", "all_directions"), ("ray_infos", "all_ray_infos"), ("rgbs", "all_rgbs"),
                    ("pxl", "all_pxl_coords")):
        t = getattr(ds, name)
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert _bits_equal(t, ref[k]), name
    assert torch.allclose(ds.feat_maps.cpu(), ref["feat_maps"], rtol=0, atol=2e-7)
    _check(ds.all_inv_depths.cpu().numpy(), ref["inv_depths"].numpy())
    W, H = 41 // downscale, 31 // downscale
    assert ds.all_imgs_wh.tolist() == [[W, H]] * 4 and len(ds) == 4 * W * H

    s = GpuRaySampler.from_dataset(ds)
    assert s.directions.data_ptr() == ds.all_directions.data_ptr()  # taken without a copy
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1))[:300]
    idx[:3] = torch.tensor([0, len(ds) - 1, W * H - 1])
    got = s.sample(idx.cuda())
    want = _cpu_batch(ref, ds, idx)
    for k in ("ray_infos", "directions", "img_idx", "c2w", "rgbs"):
        assert torch.equal(got[k].cpu(), want[k]), k
    assert torch.allclose(got["feats"].cpu(), want["feats"], rtol=0, atol=1e-6)
    _check(got["inv_depths"].cpu().numpy(), want["inv_depths"].numpy())


def test_phototourism_val_items(scene_dir):
    from upnerf_amd.datasets import PhototourismDataset, decode_image
    info = scene_dir
    ds = PhototourismDataset(info["root"], "synth", feat_dir=info["feat_dir"], depth_dir=info["depth_dir"], near=0.1,
                             far=5.0, camera_noise=-1, split="val", img_downscale=1, val_img_idx=[0, 2])
    assert ds.scale == 2 and len(ds) == 2
    for k, vi in enumerate([0, 2]):
        item = ds[k]
        assert set(item) == {"rgbs", "ray_infos", "directions", "img_idx", "img_wh", "c2w", "feats", "pca_m", "pca_c",
                             "inv_depths"}
        id_ = ds.img_ids_train[vi]
        im = decode_image(os.path.join(info["root"], "dense/images", ds.image_paths[id_]), 2)
        H, W = im.shape[:2]
        r = ref_rays(W, H, ds.Ks[id_], 0.1, 5.0, vi, pixels=im)
        assert item["img_wh"].tolist() == [W, H]
        assert _bits_equal(item["rgbs"], r["rgbs"]) and _bits_equal(item["directions"], r["directions"])
        assert _bits_equal(item["ray_infos"], r["ray_infos"][:, :2])
        assert torch.equal(item["img_idx"].cpu(), torch.full((W * H,), vi, dtype=torch.int64))
        assert torch.equal(item["c2w"].cpu(), torch.eye(3, 4))
        stem = ds.image_paths[id_].replace(".jpg", "")
        f = np.load(os.path.join(info["feat_dir"], "feature_maps", stem + ".npy"))
        _check(item["feats"].cpu().numpy(),
               cv_resize_linear(f / np.linalg.norm(f.astype(np.float64), axis=-1, keepdims=True), W, H).reshape(W * H, -1))
        assert np.array_equal(item["pca_m"], np.load(os.path.join(info["feat_dir"], "pca_infos", stem + "_mean.npy")))
        assert item["inv_depths"].shape == (W * H,)


def _scene_hparams(info, tmp_path, **over):
    """A scene YAML of the reference's layout pointed at the synthetic scene, small enough for a few steps."""
    from upnerf_amd.nerf_system import default_hparams
    hp = default_hparams(**{"nerf.N_samples": 16, "nerf.N_importance": 16, "train.batch_size": 256, "max_steps": 3,
                            "val.chunk_size": 512, "val.log_interval": 1.0})
    hp.update({"dataset_name": "phototourism", "scene_name": "synth", "root_dir": info["root"], "feat_dir": info["feat_dir"],
               "depth_dir": info["depth_dir"], "phototourism.img_downscale": 2, "phototourism.use_cache": True,
               "val.img_idx": (1,), "out_dir": str(tmp_path / "out"), "exp_name": "scene"})
    hp.update(over)
    return hp


def test_nerf_system_setup_builds_the_datasets(scene_dir, tmp_path):
    from upnerf_amd.datasets import PhototourismDataset
    from upnerf_amd.nerf_system import NeRFSystem
    s = NeRFSystem(_scene_hparams(scene_dir, tmp_path))
    s.setup()
    assert isinstance(s.train_dataset, PhototourismDataset) and s.train_dataset.split == "train"
    assert s.val_dataset.split == "val" and len(s.val_dataset) == 1
    assert s.se3_refine.weight.shape[0] == 4 and s.embedding_coarse_a.weight.shape[0] == 4
    with pytest.raises(NotImplementedError):
        NeRFSystem(_scene_hparams(scene_dir, tmp_path, dataset_name="blender")).setup()


def test_fit_from_config_without_datasets(scene_dir, tmp_path):
    from upnerf_amd.trainer import fit_from_config
    seen = []
    system, tr = fit_from_config(_scene_hparams(scene_dir, tmp_path), None, None, log=seen.append)
    assert system.global_step == 6 and len(tr.history) >= 1
    assert all(np.isfinite(h["val/psnr"]) and np.isfinite(h["val/loss"]) for h in tr.history)
    assert torch.isfinite(system.logged["train/loss"])


@pytest.mark.parametrize("pose_optimize", [True, False], ids=["pose", "appearance"])
def test_optimize_split_halves_and_tto_ssim(scene_dir, tmp_path, pose_optimize):
    from upnerf_amd.datasets import PhototourismOptimizeDataset, decode_image
    from upnerf_amd.nerf_system_optimize import NeRFSystemOptimize, run_stage
    from upnerf_amd.ray_sampler import GpuRaySampler
    info = scene_dir
    kw = dict(near=0.0, far=5.0, camera_noise=-1, img_downscale=1, pose_optimize=pose_optimize, optimize_num=0)
    tr = PhototourismOptimizeDataset(info["root"], "synth", split="train", **kw)
    va = PhototourismOptimizeDataset(info["root"], "synth", split="val", **kw)
    id_ = tr.img_ids_test[0]
    assert set(tr.poses_dict) == {id_} and torch.equal(tr.poses_dict[id_], torch.eye(3, 4))
    assert np.array_equal(tr.GT_poses_dict[id_], tr.meta.poses_dict[id_])
    im_tr = decode_image(os.path.join(info["root"], "dense/images", tr.image_paths[id_]), 1)
    im_va = decode_image(os.path.join(info["root"], "dense/images", va.image_paths[id_]), 2)
    for ds, im, split in ((tr, im_tr, "train"), (va, im_va, "val")):
        H, W = im.shape[:2]
        x0, x1 = (0, W) if pose_optimize else ((0, W // 2) if split == "train" else (W // 2, W))
        assert ds.all_imgs_wh == [x1 - x0, H]
        r = ref_rays(W, H, ds.Ks[id_], 0.0, 5.0, 0, x0, x1, im)
        for k, name in (("directions", "all_directions"), ("ray_infos", "all_ray_infos"), ("rgbs", "all_rgbs")):
            assert _bits_equal(getattr(ds, name), r[k]), (split, name)
    item = va[0]
    assert item["img_wh"].tolist() == va.all_imgs_wh

    hp = _scene_hparams(info, tmp_path, **{"optimize_num": 0, "pose_optimize": pose_optimize, "nerf.perturb": 0.0,
                                            "phototourism.img_downscale": 1})
    torch.manual_seed(0)
    t = NeRFSystemOptimize(hp, pose_optimize=pose_optimize)
    t.setup()
    assert isinstance(t.train_dataset, PhototourismOptimizeDataset) and t.se3_refine.weight.shape[0] == 1
    t = t.cuda()
    smp = GpuRaySampler.from_dataset(t.train_dataset)
    val = [{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in t.val_dataset[0].items()}]
    hist = run_stage(t, lambda e, start=0: smp.batches(256, seed=0, epoch=e, start=start), smp.n_batches(256), 1,
                     val_batches=val).history
    assert len(hist) == 1 and np.isfinite(hist[0]["val/psnr"]) and np.isfinite(hist[0]["val/ssim"])
