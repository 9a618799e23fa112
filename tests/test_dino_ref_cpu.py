"""The fp64 restatement of the DINO key-descriptor extractor (tests/dino_ref.py) against itself and in fp32, and the host side
of upnerf_amd/dino.py and tools/extract_features.py.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import dino_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    return R.make_params(D=128, heads=2, depth=3, P=3, seed=3), R.make_image(32, 32, 1)


def test_key_row_permutation_equals_permuting_the_output(small):
    sd, img = small
    for layer in (0, 2):
        a = R.descriptors(sd, img, heads=2, stride=8, layer=layer)
        b = R.descriptors(sd, img, heads=2, stride=8, layer=layer, permute_rows=True)
        assert a.shape == (4, 4, 128) and torch.allclose(a, b, rtol=0, atol=1e-12)
    from upnerf_amd.dino import key_rows
    c = torch.arange(128)
    assert torch.equal(key_rows(128, 2), 128 + (c % 2) * 64 + c // 2)


def test_blocks_past_layer_change_nothing(small):
    sd, img = small
    cut = {k: v for k, v in sd.items() if not k.startswith("blocks.2.")}
    assert torch.equal(R.descriptors(sd, img, heads=2, stride=8, layer=1), R.descriptors(cut, img, heads=2, stride=8, layer=1))


def test_layer_0_runs_no_full_block(small):
    sd, img = small
    only = {k: v for k, v in sd.items() if not k.startswith("blocks.") or k.startswith(("blocks.0.norm1", "blocks.0.attn.qkv"))}
    d = R.descriptors(only, img, heads=2, stride=8, layer=0)  # (a KeyError if anything else of a block were touched)
    assert torch.equal(d, R.descriptors(sd, img, heads=2, stride=8, layer=0))


@pytest.mark.parametrize("cfg", R.E2E)
def test_fp32_evaluation_stays_within_1e_5_of_max_abs(cfg):
    D, heads, depth, layer, H, W, stride = cfg
    sd = R.make_params(D=D, heads=heads, depth=depth, P=5, seed=D + layer)
    img = R.make_image(H, W, H + W)
    want = R.descriptors(sd, img, heads=heads, stride=stride, layer=layer)
    got = R.descriptors(sd, img, heads=heads, stride=stride, layer=layer, dtype=torch.float32)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"fp32 vs fp64: {err:.2e} of max-abs {float(want.abs().max()):.2f}")
    assert err < 1e-5


@pytest.mark.parametrize("H,W,stride,want", [(40, 40, 4, (9, 9)), (36, 52, 4, (8, 12)), (43, 41, 4, (9, 9)), (45, 47, 4, (10, 10)),
                                             (32, 32, 8, (4, 4)), (39, 33, 8, (4, 4)), (448, 448, 4, (111, 111)), (8, 8, 4, (1, 1))])
def test_token_grid(H, W, stride, want):
    from upnerf_amd.dino import token_grid
    assert token_grid(H, W, 8, stride) == want == R.token_grid(H, W, 8, stride)
    with pytest.raises(ValueError):
        token_grid(7, 40, 8, stride)


def test_pos_embed_resize_matches_the_restatement_and_keeps_the_pretraining_grid():
    from upnerf_amd.dino import resize_pos_embed
    pos = R.make_params(D=128, heads=2, depth=1, P=5)["pos_embed"]
    got = resize_pos_embed(pos, 8, 12, 36, 52)
    want = R.pos_rows(pos.double(), 8, 12, False)
    assert got.shape == (97, 128) and torch.equal(got[0], pos[0, 0])
    assert float((got.double() - want).abs().max()) < 1e-6
    assert torch.equal(resize_pos_embed(pos, 5, 5, 24, 24), pos[0])
    assert not torch.equal(resize_pos_embed(pos, 5, 5, 24, 26)[1:], pos[0, 1:])  # same grid, not square: resized


def test_loader_errors(tmp_path):
    from upnerf_amd.dino import DinoViT
    sd = R.make_params(D=128, heads=2, depth=3, P=3)
    m = DinoViT.from_state_dict(sd, heads=2, stride=8, layer=2)
    assert (m.D, m.depth, m.layer, len(m.blocks)) == (128, 3, 2, 3) and set(m.blocks[2]) == {"norm1.weight", "norm1.bias"}
    assert m.key_w.shape == (128, 128) and torch.equal(m.key_w[3], sd["blocks.2.attn.qkv.weight"][128 + 64 + 1])
    for key in ("cls_token", "pos_embed", "patch_embed.proj.weight", "blocks.0.mlp.fc1.bias", "blocks.2.attn.qkv.weight"):
        with pytest.raises(ValueError, match="missing key"):
            DinoViT.from_state_dict({k: v for k, v in sd.items() if k != key}, heads=2, layer=2)
    bad = dict(sd)
    bad["blocks.1.mlp.fc2.weight"] = torch.zeros(128, 256)
    with pytest.raises(ValueError, match=r"blocks.1.mlp.fc2.weight: expected shape \(128, 512\), got \(128, 256\)"):
        DinoViT.from_state_dict(bad, heads=2, layer=2)
    with pytest.raises(ValueError, match="head dim"):
        DinoViT.from_state_dict(sd, heads=4, layer=2)  # 128 / 4 = 32
    with pytest.raises(ValueError, match="layer=3"):
        DinoViT.from_state_dict(sd, heads=2, layer=3)
    # blocks past `layer` are not needed, and a checkpoint file round-trips through load()
    m1 = DinoViT.from_state_dict({k: v for k, v in sd.items() if not k.startswith("blocks.2.mlp")}, heads=2, layer=2)
    assert m1.depth == 3
    path = tmp_path / "w.pth"
    torch.save(sd, path)
    m2 = DinoViT.load(str(path), heads=2, stride=8, layer=1)
    assert torch.equal(m2.pe_w, sd["patch_embed.proj.weight"].reshape(128, 192))
    with pytest.raises(RuntimeError, match="device memory"):
        m2.descriptors(torch.zeros(32, 32, 3, dtype=torch.uint8))


def test_pca_components_sign_rule_and_order():
    from upnerf_amd.dino import pca_components
    x = R.planted_descriptors(81, 128)
    m, comps, val = R.pca(x)
    xn = x.double() / x.double().norm(dim=-1, keepdim=True)
    c = xn - xn.mean(0)
    got = pca_components(c.T @ c)
    assert torch.allclose(got, comps, rtol=0, atol=1e-10)
    for row in got:
        assert row[row.abs().argmax()] > 0
    assert val[0] > val[1] > val[2] > val[3]


def test_tool_file_naming_and_tsv_filter(tmp_path):
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import extract_features as T
    img_dir, out_all, out_tsv = tmp_path / "images", tmp_path / "all", tmp_path / "tsv"
    img_dir.mkdir()
    names = ["a_01.jpg", "b.png", "c.0.jpg"]
    for k, n in enumerate(names):
        Image.fromarray(np.full((9, 11, 3), 40 * k, np.uint8)).save(img_dir / n)
    tsv = tmp_path / "scene.tsv"
    tsv.write_text("filename\tid\tsplit\tdataset\nc.0.jpg\t7\ttrain\ts\nb.png\t\ttrain\ts\na_01.jpg\t3\ttest\ts\n")
    seen = []

    def stub(path):  # stands in for the network: the map's first value says which file it came from
        seen.append(os.path.basename(path))
        v = float(np.asarray(Image.open(path))[0, 0, 0])
        return np.full((2, 3, 8), v, np.float32), np.full(8, v + 1, np.float64), np.full((3, 8), v + 2, np.float32)

    assert T.run(str(img_dir), str(out_all), stub) == sorted(names)
    assert sorted(os.listdir(out_all / "feature_maps")) == ["a_01.npy", "b.npy", "c.0.npy"]
    assert sorted(os.listdir(out_all / "pca_infos")) == ["a_01_components.npy", "a_01_mean.npy", "b_components.npy", "b_mean.npy",
                                                         "c.0_components.npy", "c.0_mean.npy"]
    f = np.load(out_all / "feature_maps" / "b.npy")
    assert f.shape == (2, 3, 8) and f.dtype == np.float32 and f[0, 0, 0] == 40
    mean = np.load(out_all / "pca_infos" / "b_mean.npy")
    assert mean.dtype == np.float32 and mean[0] == 41 and np.load(out_all / "pca_infos" / "b_components.npy").shape == (3, 8)
    seen.clear()
    assert T.run(str(img_dir), str(out_tsv), stub, str(tsv)) == ["c.0.jpg", "a_01.jpg"] == seen  # the row without an id is left out
    assert sorted(os.listdir(out_tsv / "feature_maps")) == ["a_01.npy", "c.0.npy"]
