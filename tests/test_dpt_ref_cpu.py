"""Host-only checks of the DPT definition: the size rule, the pos-embed resize, the load-time errors and the weight re-layouts
of upnerf_amd/dpt.py, and the fp64 restatement (tests/dpt_ref.py) against itself: evaluated in fp32 it stays inside the
project's gate at every returned stage, and each planted defect lands outside it.

Measured on the host (worst stage, error over the reference map's max-abs; the gate is 1e-4):
    fp32 restatement: configuration a 2.0e-6, b 1.2e-6
    planted defects on configuration a, at the head: align_corners 5.6e-1, no_pre_relu 4.6e-1, no_cls 8.5e-1, dydx 5.1e-1,
    rn_bias 1.1e-1, final_norm 6.2e-1"""
import functools

import pytest
import torch
import torch.nn.functional as F

import dpt_ref as R

REL_GATE = 1e-4  # README: "<=1e-4 rel, fp32", taken against the reference map's max-abs


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg = R.CONFIGS[name]
    sd = R.make_params(**cfg)
    x = R.make_input(cfg["H"], cfg["W"], cfg["seed"])
    out, stages = R.forward_net(sd, x, **cfg)
    return cfg, sd, x, out, stages


# ---- the size rule -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,size,want", [
    (768, 1024, 384, (384, 512)),   # landscape: scales 0.5 / 0.375, 0.5 is nearer 1; 384 / 32 = 12, 512 / 32 = 16
    (1024, 768, 384, (512, 384)),   # portrait: the width's scale 0.5 for both axes
    (384, 384, 384, (384, 384)),
    (256, 768, 384, (384, 1152)),   # a tie: |1 - 1.5| = |1 - 0.5|; the strict `<` keeps the height's scale 1.5: 768 * 1.5 / 32 = 36
    (768, 1056, 384, (384, 512)),   # half to even: scale 0.5, 1056 * 0.5 / 32 = 16.5 -> 16
    (768, 1120, 384, (384, 576)),   # half to even: 1120 * 0.5 / 32 = 17.5 -> 18
    (80, 64, 64, (64, 64)),         # scales 0.8 / 1.0: the width's; 80 / 32 = 2.5 -> 2
    (112, 64, 64, (128, 64)),       # portrait, scale 1.0: 112 / 32 = 3.5 -> 4
    (50, 70, 64, (32, 64)),         # scales 1.28 / 0.914: the width's; 50 * 0.914 / 32 = 1.43 -> 1
])
def test_net_size_hand_worked(h, w, size, want):
    from upnerf_amd.dpt import net_size
    assert net_size(h, w, size) == want == R.net_size(h, w, size)


def test_pos_embed_resize():
    from upnerf_amd.dpt import resize_pos_embed
    g = torch.Generator().manual_seed(0)
    pos = torch.randn(1, 1 + 9, 8, generator=g)
    same = resize_pos_embed(pos, 3, 3)
    assert torch.allclose(same, pos[0], atol=1e-6)  # the pretraining grid comes back
    got = resize_pos_embed(pos, 2, 6)
    assert got.shape == (13, 8) and torch.equal(got[0], pos[0, 0])
    want = F.interpolate(pos[0, 1:].T.reshape(1, 8, 3, 3), size=(2, 6), mode="bilinear", align_corners=False)
    assert torch.equal(got[1:], want[0].reshape(8, 12).T)
    assert torch.allclose(got.double(), R.pos_rows(pos.double(), 2, 6), atol=1e-6)


# ---- load-time errors ----------------------------------------------------------------------------------------------------

def test_load_time_shape_and_key_errors():
    from upnerf_amd.dpt import DptDepth, check_model_type
    cfg, sd, *_ = _case("b")
    kw = R.model_kwargs(cfg)
    DptDepth.from_state_dict(sd, **kw)
    for key in ("pretrained.model.pos_embed", "scratch.layer2_rn.weight", "pretrained.act_postprocess1.4.bias",
                "scratch.refinenet1.resConfUnit1.conv2.weight", "scratch.output_conv.4.weight",
                "pretrained.act_postprocess3.0.project.0.weight", "pretrained.model.blocks.1.mlp.fc2.bias"):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            DptDepth.from_state_dict(bad, **kw)
        bad[key] = torch.zeros(*sd[key].shape, 2)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            DptDepth.from_state_dict(bad, **kw)
    ok = dict(sd)
    for u in (1, 2):  # refinenet4's resConfUnit1 is never read, and no bias of layerK_rn either
        del ok[f"scratch.refinenet4.resConfUnit1.conv{u}.weight"]
    ok["scratch.layer1_rn.bias"] = torch.zeros(3)
    DptDepth.from_state_dict(ok, **kw)
    with pytest.raises(ValueError, match="hooks"):
        DptDepth.from_state_dict(sd, **{**kw, "hooks": (0, 1, 2, 3)})  # two blocks in the weights
    with pytest.raises(ValueError, match="multiples of 32"):
        DptDepth.from_state_dict(sd, **{**kw, "fusion": 48})
    with pytest.raises(ValueError, match="head dim"):
        DptDepth.from_state_dict(sd, **{**kw, "heads": 4})
    for t in ("dpt_hybrid", "dpt_hybrid_kitti", "midas_v21"):
        with pytest.raises(NotImplementedError, match="dpt_large"):
            check_model_type(t)
    check_model_type("dpt_large")


# ---- weight re-layouts -----------------------------------------------------------------------------------------------------

def test_conv3x3_relayout_against_conv2d():
    from upnerf_amd.dpt import relay_conv3x3
    g = torch.Generator().manual_seed(1)
    w, x = torch.randn(5, 4, 3, 3, generator=g, dtype=torch.float64), torch.randn(6, 7, 4, generator=g, dtype=torch.float64)
    wr = relay_conv3x3(w)
    assert wr.shape == (5, 3, 3, 4) and wr.is_contiguous()
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    got = torch.stack([torch.stack([(xp[y:y + 3, c:c + 3].reshape(-1) * wr.reshape(5, -1)).sum(1) for c in range(7)]) for y in range(6)])
    assert torch.allclose(got, R.conv3x3(x, w), atol=1e-12)


@pytest.mark.parametrize("s", [2, 4])
def test_conv_transpose_relayout_against_conv_transpose2d(s):
    from upnerf_amd.dpt import relay_conv_transpose
    g = torch.Generator().manual_seed(s)
    ci, co, H, W = 3, 5, 2, 3
    w, b = torch.randn(ci, co, s, s, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
    x = torch.randn(H, W, ci, generator=g, dtype=torch.float64)
    wide = x.reshape(H * W, ci) @ relay_conv_transpose(w).T  # [(y, x)][(dy, dx, c_out)]
    got = wide.reshape(H, W, s, s, co).permute(0, 2, 1, 3, 4).reshape(H * s, W * s, co) + b
    want = F.conv_transpose2d(x.permute(2, 0, 1)[None], w, b, stride=s)[0].permute(1, 2, 0)
    assert torch.allclose(got, want, atol=1e-12)


# ---- the restatement against itself -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a", "b"])
def test_fp32_restatement_meets_the_gate_at_every_stage(name):
    cfg, sd, x, out, stages = _case(name)
    assert out.shape == (cfg["H"], cfg["W"]) and out.dtype == torch.float64
    _, s32 = R.forward_net(sd, x, dtype=torch.float32, **cfg)
    worst = 0.0
    for (stage, want), (_, got) in zip(R.stage_list(stages), R.stage_list(s32)):
        assert got.shape == want.shape and float(want.abs().max()) > 0, stage
        err = _rel(got, want)
        worst = max(worst, err)
        print(f"fp32 restatement, configuration {name}, {stage} {tuple(want.shape)}: {err:.2e} of max-abs")
        assert err < REL_GATE, stage
    print(f"fp32 restatement, configuration {name}: worst {worst:.2e}")
    assert float((out > 0).double().mean()) > 0.25
    if name == "b":
        assert stages["reassembled"][3].shape[:2] == (1, 1)  # the in = 1 edge of the upsample


@pytest.mark.parametrize("defect", ["align_corners", "no_pre_relu", "no_cls", "dydx", "rn_bias", "final_norm"])
def test_planted_defects_land_outside_the_gate(defect):
    cfg, sd, x, out, stages = _case("a")
    bad, _ = R.forward_net(sd, x, defect=defect, **cfg)
    err = _rel(bad, out)
    print(f"planted {defect}: {err:.2e} of max-abs at the head")
    assert err > REL_GATE


def test_inverse_depth_route_shapes():
    cfg, sd, *_ = _case("b")
    photo = R.make_photo(50, 70, 1)
    assert R.net_size(50, 70, 64) == (32, 64)
    out = R.inverse_depth(sd, photo, 64, cfg)
    assert out.shape == (50, 70) and torch.isfinite(out).all() and float(out.max()) > 0
