"""fp64 restatement of DPT-Large's inverse-depth network (the definition in the issue behind upnerf_amd/dpt.py: ViT backbone with
four hooks, reassemble with readout="project", RefineNet fusion, the head, and the two resizes around it) in plain torch CPU
ops on checkpoint-layout weights (F.conv2d, F.conv_transpose2d, F.interpolate), and a seeded weight maker.  CPU only;
tests/test_dpt_ref_cpu.py checks it against itself, in fp32 and against planted defects, tests/test_hip_dpt.py holds the HIP
kernels to it."""
import math

import torch
import torch.nn.functional as F

import dino_ref as V  # layernorm, gelu, attention: the same block arithmetic

PATCH = 16
SCALES = (4, 2, 1, -2)  # per stage: ConvTranspose of this kernel and stride; 1: nothing; -2: Conv k3 s2 p1

# the two seeded configurations of the GPU test: small enough for seconds of fp64 on the host
CFG_A = dict(D=128, heads=2, depth=4, hooks=(0, 1, 2, 3), stage_widths=(32, 64, 128, 128), fusion=64, head=(32, 32), H=64, W=96,
             P=3, seed=11)
CFG_B = dict(D=192, heads=3, depth=2, hooks=(0, 0, 1, 1), stage_widths=(32, 64, 96, 96), fusion=32, head=(32, 32), H=32, W=32,
             P=3, seed=12)  # (the last stage is a 1 x 1 map: the in = 1 edge of the upsample)
CONFIGS = {"a": CFG_A, "b": CFG_B}


def model_kwargs(cfg):
    return dict(heads=cfg["heads"], hooks=cfg["hooks"], stage_widths=cfg["stage_widths"], fusion=cfg["fusion"], head=cfg["head"])


def make_params(D, heads, depth, hooks, stage_widths, fusion, head, P=3, seed=0, dtype=torch.float32, **_):
    """randn / sqrt(fan_in) weights, 0.1 randn biases, LayerNorm gains 1 + 0.2 n; the last bias positive (4: the head's inputs are post-ReLU, so
    its pre-activation has an offset of a few units of either sign) so that the final ReLU leaves most of the map alive.  Keys and shapes of the checkpoint."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    fan = lambda *s: n(*s) / math.sqrt(s[1] * (s[2] * s[3] if len(s) == 4 else 1))
    m = "pretrained.model."
    sd = {m + "cls_token": 0.5 * n(1, 1, D), m + "pos_embed": 0.5 * n(1, 1 + P * P, D),
          m + "patch_embed.proj.weight": fan(D, 3, PATCH, PATCH), m + "patch_embed.proj.bias": 0.1 * n(D)}
    for i in range(depth):
        b = f"{m}blocks.{i}."
        sd[b + "norm1.weight"], sd[b + "norm1.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)
        sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"] = 1.5 * fan(3 * D, D), 0.1 * n(3 * D)
        sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"] = fan(D, D), 0.1 * n(D)
        sd[b + "norm2.weight"], sd[b + "norm2.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)
        sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"] = fan(4 * D, D), 0.1 * n(4 * D)
        sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"] = fan(D, 4 * D), 0.1 * n(D)
    sd[m + "norm.weight"], sd[m + "norm.bias"] = 1 + 0.2 * n(D), 0.1 * n(D)  # (ignored: the hooks are raw block outputs)
    for k, (S, sc) in enumerate(zip(stage_widths, SCALES), 1):
        p = f"pretrained.act_postprocess{k}."
        sd[p + "0.project.0.weight"], sd[p + "0.project.0.bias"] = fan(D, 2 * D), 0.1 * n(D)
        sd[p + "3.weight"], sd[p + "3.bias"] = fan(S, D, 1, 1), 0.1 * n(S)
        if sc > 1:  # ConvTranspose2d: [C_in][C_out][s][s]; every output pixel has ONE tap: fan_in = C_in
            sd[p + "4.weight"], sd[p + "4.bias"] = n(S, S, sc, sc) / math.sqrt(S), 0.1 * n(S)
        elif sc < 0:
            sd[p + "4.weight"], sd[p + "4.bias"] = fan(S, S, 3, 3), 0.1 * n(S)
        sd[f"scratch.layer{k}_rn.weight"] = fan(fusion, S, 3, 3)
        for u in (1, 2):  # (refinenet4.resConfUnit1 exists in the file and is ignored)
            for c in (1, 2):
                q = f"scratch.refinenet{k}.resConfUnit{u}.conv{c}."
                sd[q + "weight"], sd[q + "bias"] = fan(fusion, fusion, 3, 3), 0.1 * n(fusion)
        q = f"scratch.refinenet{k}.out_conv."
        sd[q + "weight"], sd[q + "bias"] = fan(fusion, fusion, 1, 1), 0.1 * n(fusion)
    h0, h1 = head
    sd["scratch.output_conv.0.weight"], sd["scratch.output_conv.0.bias"] = fan(h0, fusion, 3, 3), 0.1 * n(h0)
    sd["scratch.output_conv.2.weight"], sd["scratch.output_conv.2.bias"] = fan(h1, h0, 3, 3), 0.1 * n(h1)
    sd["scratch.output_conv.4.weight"], sd["scratch.output_conv.4.bias"] = fan(1, h1, 1, 1), 4.0 + 0.1 * n(1).abs()
    sd["scratch.unused.weight"] = n(3)  # (anything else is ignored)
    return {k: v.to(dtype) for k, v in sd.items()}


def make_input(H, W, seed=0, dtype=torch.float64):
    """A normalised network-size input in [-1, 1], [H][W][3]."""
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.rand(H, W, 3, generator=g, dtype=torch.float64) * 2 - 1).to(torch.float32).to(dtype)


def make_photo(h, w, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)


def net_size(h, w, size=384, multiple=32):
    import numpy as np
    sh, sw = size / h, size / w
    if abs(1 - sw) < abs(1 - sh):
        sh = sw
    else:
        sw = sh
    return int(np.round(sh * h / multiple) * multiple), int(np.round(sw * w / multiple) * multiple)


def pos_rows(pos, gh, gw):
    n = pos.shape[1] - 1
    P = int(round(math.sqrt(n)))
    D = pos.shape[-1]
    grid = F.interpolate(pos[0, 1:].reshape(1, P, P, D).permute(0, 3, 1, 2), size=(gh, gw), mode="bilinear", align_corners=False)
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


def rcu(x, p, key, pre_relu=True):
    y = F.relu(x) if pre_relu else x
    y = F.conv2d(y, p[key + "conv1.weight"], p[key + "conv1.bias"], padding=1)
    y = F.conv2d(F.relu(y), p[key + "conv2.weight"], p[key + "conv2.bias"], padding=1)
    return y + x


def forward_net(sd, x, *, heads, hooks, fusion=None, dtype=torch.float64, defect=None, **_):
    """x: [H][W][3] normalised input.  Returns (inverse depth [H][W], stages) with stages = dict(reassembled = four [h][w][S]
    maps, fusion = the outputs of refinenet4, 3, 2, 1 as [h][w][F], head = the output).  `defect` plants one deviation from the
    definition (tests/test_dpt_ref_cpu.py): "align_corners", "no_pre_relu", "no_cls", "dydx", "rn_bias", "final_norm"."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    m = "pretrained.model."
    x = x.to(dtype)
    H, W = x.shape[:2]
    gh, gw = H // PATCH, W // PATCH
    D = p[m + "cls_token"].shape[-1]
    ac = defect != "align_corners"
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=ac)
    tok = F.conv2d(x.permute(2, 0, 1)[None], p[m + "patch_embed.proj.weight"], p[m + "patch_embed.proj.bias"], stride=PATCH)
    tok = tok[0].reshape(D, gh * gw).T
    tok = torch.cat([p[m + "cls_token"].reshape(1, D), tok], 0) + pos_rows(p[m + "pos_embed"], gh, gw)
    acts = {}
    for i in range(max(hooks) + 1):
        b = f"{m}blocks.{i}."
        y = V.layernorm(tok, p[b + "norm1.weight"], p[b + "norm1.bias"])
        qkv = y @ p[b + "attn.qkv.weight"].T + p[b + "attn.qkv.bias"]
        tok = tok + V.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], heads) @ p[b + "attn.proj.weight"].T + p[b + "attn.proj.bias"]
        y = V.layernorm(tok, p[b + "norm2.weight"], p[b + "norm2.bias"])
        tok = tok + V.gelu(y @ p[b + "mlp.fc1.weight"].T + p[b + "mlp.fc1.bias"]) @ p[b + "mlp.fc2.weight"].T + p[b + "mlp.fc2.bias"]
        acts[i] = V.layernorm(tok, p[m + "norm.weight"], p[m + "norm.bias"]) if defect == "final_norm" else tok
    maps, rn = [], []
    for k, sc in enumerate(SCALES, 1):
        a = acts[hooks[k - 1]]
        q = f"pretrained.act_postprocess{k}."
        cls = torch.zeros_like(a[1:]) if defect == "no_cls" else a[:1].expand(gh * gw, D)
        t = V.gelu(torch.cat([a[1:], cls], 1) @ p[q + "0.project.0.weight"].T + p[q + "0.project.0.bias"])
        t = t.T.reshape(1, D, gh, gw)
        t = F.conv2d(t, p[q + "3.weight"], p[q + "3.bias"])
        if sc > 1:
            wt = p[q + "4.weight"]
            t = F.conv_transpose2d(t, wt.transpose(2, 3) if defect == "dydx" else wt, p[q + "4.bias"], stride=sc)
        elif sc < 0:
            t = F.conv2d(t, p[q + "4.weight"], p[q + "4.bias"], stride=2, padding=1)
        maps.append(t)
        bias = 0.1 * torch.ones(p[f"scratch.layer{k}_rn.weight"].shape[0], dtype=dtype) if defect == "rn_bias" else None
        rn.append(F.conv2d(t, p[f"scratch.layer{k}_rn.weight"], bias, padding=1))
    paths, path = [], None
    for k in (4, 3, 2, 1):
        q = f"scratch.refinenet{k}."
        out = rn[k - 1] if path is None else path + rcu(rn[k - 1], p, q + "resConfUnit1.")
        out = rcu(out, p, q + "resConfUnit2.", pre_relu=defect != "no_pre_relu")
        path = F.conv2d(up(out), p[q + "out_conv.weight"], p[q + "out_conv.bias"])
        paths.append(path)
    t = F.conv2d(path, p["scratch.output_conv.0.weight"], p["scratch.output_conv.0.bias"], padding=1)
    t = F.relu(F.conv2d(up(t), p["scratch.output_conv.2.weight"], p["scratch.output_conv.2.bias"], padding=1))
    out = F.relu(F.conv2d(t, p["scratch.output_conv.4.weight"], p["scratch.output_conv.4.bias"]))[0, 0]
    nhwc = lambda t: t[0].permute(1, 2, 0)
    return out, dict(reassembled=[nhwc(t) for t in maps], fusion=[nhwc(t) for t in paths], head=out)


def stage_list(stages):
    """(name, map) pairs of everything forward_net returns, in network order."""
    return ([(f"reassembled{k + 1}", t) for k, t in enumerate(stages["reassembled"])] +
            [(f"refinenet{4 - j}", t) for j, t in enumerate(stages["fusion"])] + [("head", stages["head"])])


def cubic(x, H, W):
    """[h][w][C] -> [H][W][C]: F.interpolate(mode="bicubic", align_corners=False) (A = -0.75, half-pixel centres, clamped taps)."""
    return F.interpolate(x.permute(2, 0, 1)[None], size=(H, W), mode="bicubic", align_corners=False)[0].permute(1, 2, 0)


def inverse_depth(sd, photo, size, cfg, dtype=torch.float64):
    """The whole route for an [h][w][3] uint8 photograph: / 255, bicubic to the net size, (x - 0.5) / 0.5, the network, bicubic
    back to (h, w)."""
    h, w = photo.shape[:2]
    H, W = net_size(h, w, size)
    x = (cubic(photo.to(dtype) / 255, H, W) - 0.5) / 0.5
    out, _ = forward_net(sd, x, dtype=dtype, **cfg)
    return cubic(out[:, :, None], h, w)[:, :, 0]


def conv3x3(x, w, bias=None, res=None, stride=1, pre_relu=False, relu=False):
    """x: [H][W][C_in], w: checkpoint layout [C_out][C_in][3][3], res: [Ho][Wo][C_out] -> [Ho][Wo][C_out]."""
    t = x.permute(2, 0, 1)[None]
    y = F.conv2d(F.relu(t) if pre_relu else t, w, bias, stride=stride, padding=1)[0].permute(1, 2, 0)
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def upsample2x(x):
    return F.interpolate(x.permute(2, 0, 1)[None], scale_factor=2, mode="bilinear", align_corners=True)[0].permute(1, 2, 0)
