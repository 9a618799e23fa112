"""Scene metadata on the host (upnerf_amd/scene.py) against hand-packed COLMAP files and independent numpy restatements
of the reference's rules (datasets/phototourism.py:63-212, datasets/custom.py:62-140).  No GPU."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import scene_synth
from upnerf_amd import scene


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


def test_colmap_readers_hand_packed(tmp_path):
    cams = _write(str(tmp_path / "cameras.bin"),
                  struct.pack("<QiiQQ4d", 1, 7, 1, 640, 480, 500.0, 510.0, 320.5, 240.25))
    c = scene.read_cameras_binary(cams)
    assert list(c) == [7] and c[7].model_id == 1 and (c[7].width, c[7].height) == (640, 480)
    assert c[7].params.tolist() == [500.0, 510.0, 320.5, 240.25]

    b = struct.pack("<Q", 2)
    b += struct.pack("<i4d3di", 3, 1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0, 7) + b"a.jpg\0" + struct.pack("<Q", 2)
    b += struct.pack("<ddq", 1.5, 2.5, 4) + struct.pack("<ddq", 3.5, 4.5, -1)
    b += struct.pack("<i4d3di", 5, 0.5, 0.5, 0.5, 0.5, -1.0, 0.0, 0.25, 7) + b"dir/b.jpg\0" + struct.pack("<Q", 0)
    ims = scene.read_images_binary(_write(str(tmp_path / "images.bin"), b))
    assert list(ims) == [3, 5]
    assert ims[3].name == "a.jpg" and ims[5].name == "dir/b.jpg" and ims[5].camera_id == 7
    assert ims[3].qvec.tolist() == [1, 0, 0, 0] and ims[5].tvec.tolist() == [-1.0, 0.0, 0.25]

    p = struct.pack("<Q", 3)
    for pid, xyz, track in ((1, (0.5, 1.0, 2.0), [(3, 0)]), (9, (-1.0, 0.0, 4.0), []), (4, (2.0, 2.0, 2.0), [(3, 1), (5, 0)])):
        p += struct.pack("<Q3d3BdQ", pid, *xyz, 10, 20, 30, 0.75, len(track))
        for t in track:
            p += struct.pack("<ii", *t)
    xyz = scene.read_points3d_binary(_write(str(tmp_path / "points3D.bin"), p))
    assert xyz.dtype == np.float64 and xyz.tolist() == [[0.5, 1.0, 2.0], [-1.0, 0.0, 4.0], [2.0, 2.0, 2.0]]

    # the same bytes through the test helper's packers
    assert scene_synth.pack_points([(1, (0.5, 1.0, 2.0), (10, 20, 30), 0.75, [(3, 0)]),
                                    (9, (-1.0, 0.0, 4.0), (10, 20, 30), 0.75, []),
                                    (4, (2.0, 2.0, 2.0), (10, 20, 30), 0.75, [(3, 1), (5, 0)])]) == p


@pytest.mark.parametrize("which", ["cameras", "images", "points"])
def test_truncated_files_are_refused(tmp_path, which):
    if which == "cameras":
        data, fn = scene_synth.pack_cameras([(1, 1, 4, 4, (1.0, 1.0, 2.0, 2.0))]), scene.read_cameras_binary
    elif which == "images":
        data, fn = scene_synth.pack_images([(1, (1, 0, 0, 0), (0, 0, 0), 1, "x.jpg", [(0.0, 0.0, 1)])]), scene.read_images_binary
    else:
        data, fn = scene_synth.pack_points([(1, (0, 0, 1), (1, 2, 3), 0.1, [(1, 0)])]), scene.read_points3d_binary
    path = _write(str(tmp_path / "f.bin"), data)
    fn(path)  # complete: fine
    for cut in (4, len(data) // 2, len(data) - 1):
        _write(path, data[:cut])
        with pytest.raises(ValueError, match="truncated"):
            fn(path)


def test_qvec2rotmat_identity_and_quarter_turns():
    assert np.allclose(scene.qvec2rotmat((1, 0, 0, 0)), np.eye(3))
    s = np.sqrt(0.5)
    want = {"x": [[1, 0, 0], [0, 0, -1], [0, 1, 0]],
            "y": [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],
            "z": [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}
    for k, axis in enumerate("xyz"):
        q = [s, 0, 0, 0]
        q[1 + k] = s
        R = scene.qvec2rotmat(q)
        assert np.allclose(R, want[axis], atol=1e-15), axis
        assert np.allclose(R @ R.T, np.eye(3))


def test_c2w_axis_flip():
    R = scene.qvec2rotmat(scene_synth.qvec_y(0.7))
    t = np.array([0.3, -0.2, 4.0])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, t
    c2w = scene.c2w_from_w2c(w2c[None])[0]
    assert c2w.shape == (3, 4)
    assert np.allclose(c2w[:, 0], R.T[:, 0]) and np.allclose(c2w[:, 1:3], -R.T[:, 1:3])
    assert np.allclose(c2w[:, 3], -R.T @ t)


def test_scene_metadata_bounds_and_scale(tmp_path):
    info = scene_synth.write_phototourism_scene(str(tmp_path), n_images=5, images=False, n_points=300)
    m = scene.phototourism_meta(str(tmp_path), "synth", 1)
    order = [info["ids"][k] for k in info["tsv_order"]]
    assert m.img_ids == order  # tsv order, ids from images.bin by name, the empty-id row dropped
    assert m.image_paths == {info["ids"][k]: info["names"][k] for k in range(5)}
    assert m.img_ids_train == [i for i in order if i != info["ids"][4]] and m.img_ids_test == [info["ids"][4]]

    # independent restatement: world-to-camera from the packed qvec / tvec, fp64 percentiles, float32 max_far
    xyz = info["xyz"]
    nears, fars, w2cs = {}, {}, {}
    for iid, q, t, *_ in info["images"]:
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        zc = (xyz @ R.T + np.asarray(t))[:, 2]
        zc = zc[zc > 0]
        nears[iid], fars[iid] = np.percentile(zc, 0.1), np.percentile(zc, 99.9)
        w2cs[iid] = (R, np.asarray(t))
    max_far = np.float32(max(np.float32(fars[i]) for i in m.img_ids))
    sf = max_far / 5
    assert isinstance(m.scale_factor, np.float32) and m.scale_factor == sf
    for i in m.img_ids:
        assert m.nears[i] == nears[i] / sf and m.fars[i] == fars[i] / sf
        R, t = w2cs[i]
        c2w = np.concatenate([R.T, (-R.T @ t)[:, None]], 1)
        c2w[:, 1:3] *= -1
        c2w[:, 3] /= sf
        assert np.allclose(m.poses_dict[i], c2w, atol=1e-12)
    assert np.allclose(m.xyz_world, xyz / sf)
    assert max(m.fars.values()) == pytest.approx(5.0, rel=1e-6)


@pytest.mark.parametrize("scale", [1, 2, 3])
@pytest.mark.parametrize("cx,cy", [(320.0, 240.0), (333.5, 250.5), (100.7, 61.2)])
def test_K_rescaling(scale, cx, cy):
    params = (412.3, 415.9, cx, cy)
    K = scene.scaled_K(params, scale)
    w, h = int(cx * 2), int(cy * 2)  # odd sizes for the .5 centres
    w_, h_ = w // scale, h // scale
    assert K.dtype == np.float32
    assert K[0, 0] == np.float32(412.3 * w_ / w) and K[1, 1] == np.float32(415.9 * h_ / h)
    assert K[0, 2] == np.float32(cx * w_ / w) and K[1, 2] == np.float32(cy * h_ / h) and K[2, 2] == 1
    assert K[0, 1] == K[1, 0] == K[2, 0] == K[2, 1] == 0
    with pytest.raises(ValueError):
        scene.scaled_K((500.0, 320.0, 240.0), scale)


def test_tsv_drops_empty_ids(tmp_path):
    p = tmp_path / "s.tsv"
    p.write_text("filename\tid\tsplit\tdataset\n"
                 "a.jpg\t12\ttrain\ts\n"
                 "b.jpg\t\ttrain\ts\n"
                 "c.jpg\t7\ttest\ts\n"
                 "d.jpg\tNaN\ttest\ts\n"
                 "e.jpg\t3\ttrain\ts\n")
    rows = scene.read_tsv(str(p))
    assert [(r["filename"], r["split"]) for r in rows] == [("a.jpg", "train"), ("c.jpg", "test"), ("e.jpg", "train")]


def test_custom_metadata(tmp_path):
    pytest.importorskip("PIL")
    meta = scene_synth.write_custom_scene(str(tmp_path))
    for s in (1, 2, 4):
        m = scene.custom_meta(str(tmp_path), s)
        assert m.img_ids == ["0", "1", "2"] and m.img_ids_train == ["0", "1"] and m.img_ids_test == ["2"]
        assert m.image_paths["1"] == "dense/images/002.jpg" and m.image_root == str(tmp_path)
        for k, (w, h) in zip("012", ((41, 31), (40, 30), (39, 29))):
            K = m.Ks[k]
            f = meta[k]["focal"]
            assert K[0, 0] == np.float32(f / s) and K[1, 1] == np.float32(f / s)
            assert K[0, 2] == np.float32(w / 2 / s) and K[1, 2] == np.float32(h / 2 / s)
            assert np.array_equal(m.poses_dict[k], np.asarray(meta[k]["c2w"]))
        assert m.nears == {} and m.fars == {}
    data = json.loads((tmp_path / "metadata.json").read_text())
    data["1"]["split"] = "val"
    (tmp_path / "metadata.json").write_text(json.dumps(data))
    with pytest.raises(ValueError):
        scene.custom_meta(str(tmp_path), 1)


def test_pose_noise_minus_one_gives_identities(tmp_path, monkeypatch):
    scene_synth.write_phototourism_scene(str(tmp_path), n_images=4, images=False)
    m = scene.phototourism_meta(str(tmp_path), "synth", 2)
    monkeypatch.chdir(tmp_path)  # no noises/ directory here
    poses, gt, noises = scene.initial_train_poses(m, -1, device="cpu")
    assert noises is None and list(poses) == m.img_ids_train
    for i in m.img_ids_train:
        assert torch.equal(poses[i], torch.eye(3, 4))
    assert gt is m.poses_dict
    poses, gt, _ = scene.initial_train_poses(m, None, device="cpu")
    assert all(np.array_equal(poses[i], m.poses_dict[i]) for i in m.img_ids)


def test_pose_noise_file_is_composed(tmp_path, monkeypatch):
    scene_synth.write_phototourism_scene(str(tmp_path), n_images=4, images=False)
    m = scene.phototourism_meta(str(tmp_path), "synth", 1)
    N = len(m.img_ids_train)
    g = torch.Generator().manual_seed(3)
    R, _ = torch.linalg.qr(torch.randn(N, 3, 3, generator=g))
    noise = torch.cat([R, torch.randn(N, 3, 1, generator=g)], -1)
    os.makedirs(tmp_path / "noises")
    torch.save(noise, tmp_path / "noises" / f"{N}_0.15.pt")
    monkeypatch.chdir(tmp_path)
    poses, gt, loaded = scene.initial_train_poses(m, 0.15, device="cpu")
    assert torch.equal(loaded, noise)
    for k, i in enumerate(m.img_ids_train):
        P = torch.as_tensor(m.poses_dict[i], dtype=torch.float32)
        want = torch.cat([P[:, :3] @ noise[k, :, :3], P[:, :3] @ noise[k, :, 3:] + P[:, 3:]], -1)
        assert torch.allclose(poses[i], want, atol=1e-6)
