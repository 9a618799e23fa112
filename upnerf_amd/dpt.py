"""DPT-Large monocular inverse-depth maps from weights the user supplies: the `<depth_dir>/<stem>.npy` files that datasets.py
reads into `all_inv_depths` and the depth prior of the loss reads, which the reference makes with preprocess/save_dpt_depth.py
`-t dpt_large` (a DPT checkout, timm, cv2).

The arithmetic runs in HIP: the backbone is the ViT block loop of vit.py (csrc/dino.hip, `upnerf_linear`), the decoder and the
two resizes are csrc/dpt.hip (`upnerf_conv3x3`, `upnerf_upsample2x`, `upnerf_depth_to_space`, `upnerf_resize_cubic`,
`upnerf_vit_patches16`); every 1 x 1 convolution and the readout are `upnerf_linear` on NHWC maps, and the 32 -> 1 head is an
`upnerf_linear` with N = 1 and its ReLU.  There is no CPU path and no pretrained file in this repository.  The user has the
file: `dpt_large-midas-2f21e586.pt`; `DptDepth.load` reads it.

Everything this module knows about the network, its state-dict keys and its preprocessing is in the table below (MODEL, KEYS,
PREPROCESS, `net_size`, `resize_pos_embed`).  It is written from memory of intel-isl/DPT (dpt/models.py, dpt/vit.py,
dpt/blocks.py, dpt/transforms.py) and of timm's vit_large_patch16_384 and has NOT been compared with either: neither is
installed where this was written, nor are the pretrained weights.  Real weights, DPT's own output and the key names are
unchecked; a user who finds a mismatch changes this one table.

One stated deviation: the reference runs the network in fp16 (`optimize=True`) and saves float16 maps; here everything is fp32
on the fp32-input MFMA and the maps are fp32."""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn.functional as F

from . import _lib, vit
from .ops import TIMER

# ---- the network: dpt_large (DPTDepthModel(backbone="vitl16_384", non_negative=True, invert=False)) ---------------------------
#   backbone ViT-L/16: patch 16 (a 16 x 16 convolution at stride 16), width 1024, 24 pre-norm blocks, 16 heads of 64, MLP ratio
#   4, qkv_bias, LayerNorm eps 1e-6, exact-erf GELU; hooks = the RAW outputs of blocks 5, 11, 17, 23 (no final `norm`)
#   reassemble (readout="project"), per hook k = 1..4 with stage width S_k:
#       t_n <- GELU(W [t_n ; t_cls] + b) for the patch tokens; the (H/16, W/16) grid; Conv 1 x 1 1024 -> S_k; then
#       k = 1: ConvTranspose k4 s4;  k = 2: ConvTranspose k2 s2;  k = 3: nothing;  k = 4: Conv k3 s2 p1
#   decoder: layerK_rn = Conv k3 p1 WITHOUT bias S_k -> F; refinenet4..1 (FeatureFusionBlock_custom, no batch norm):
#       out = x0; with a second input out += RCU1(x1); out = RCU2(out); bilinear x 2 align_corners=True; 1 x 1 out_conv
#       RCU(x) = conv2(relu(conv1(relu(x)))) + x, both k3 p1 with bias; refinenet4 has one input (its resConfUnit1 is ignored)
#   head: Conv F -> head[0] k3 p1; bilinear x 2 align_corners=True; Conv head[0] -> head[1] k3 p1; ReLU; Conv head[1] -> 1 k1; ReLU
MODEL = dict(patch=16, width=1024, depth=24, heads=16, head_dim=64, mlp_ratio=4, ln_eps=1e-6, hooks=(5, 11, 17, 23),
             stage_widths=(256, 512, 1024, 1024), fusion=256, head=(128, 32), net_size=384)
REASSEMBLE_SCALE = (4, 2, 1, -2)  # per stage: transposed convolution of this kernel and stride; 1: nothing; -2: Conv k3 s2 p1
# state-dict keys ({k}: stage 1..4, {i}: block); anything else is ignored
KEYS = dict(cls="pretrained.model.cls_token",                                # [1, 1, D]
            pos="pretrained.model.pos_embed",                                # [1, 1 + P * P, D], P = 24
            pe_w="pretrained.model.patch_embed.proj.weight",                 # [D, 3, 16, 16]
            pe_b="pretrained.model.patch_embed.proj.bias",                   # [D]
            block="pretrained.model.blocks.{i}.",                            # + vit.BLOCK_KEYS
            readout="pretrained.act_postprocess{k}.0.project.0.",            # Linear(2 D -> D): weight [D, 2 D], bias [D]
            project="pretrained.act_postprocess{k}.3.",                      # Conv 1 x 1: weight [S_k, D, 1, 1], bias [S_k]
            resample="pretrained.act_postprocess{k}.4.",                     # k = 1, 2: ConvTranspose weight [S_k, S_k, s, s];
                                                                             # k = 4: Conv weight [S_k, S_k, 3, 3]; bias [S_k]
            layer_rn="scratch.layer{k}_rn.weight",                           # [F, S_k, 3, 3], no bias
            rcu="scratch.refinenet{k}.resConfUnit{u}.conv{c}.",              # weight [F, F, 3, 3], bias [F]
            out_conv="scratch.refinenet{k}.out_conv.",                       # weight [F, F, 1, 1], bias [F]
            head="scratch.output_conv.{j}.")                                 # j = 0, 2: k3; j = 4: k1
# ---- preprocessing (save_dpt_depth.py:96-110 and DPT's Resize(384, 384, keep_aspect_ratio=True, ensure_multiple_of=32,
#      resize_method="minimal", image_interpolation_method=cv2.INTER_CUBIC), NormalizeImage(0.5, 0.5)) and postprocessing
#      (F.interpolate(mode="bicubic", align_corners=False) to the photograph's size) --------------------------------------------
PREPROCESS = dict(multiple=32, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))
UNSUPPORTED = ("dpt_hybrid", "dpt_hybrid_kitti", "dpt_hybrid_nyu", "midas_v21")


def check_model_type(model_type):
    """dpt_hybrid* has a ResNetV2 stem (weight-standardised convolutions, group norm) and midas_v21 is a convolutional network:
    neither is built here."""
    if model_type != "dpt_large":
        raise NotImplementedError(f"model type {model_type!r} is not built here; only dpt_large is")


def net_size(h, w, size=MODEL["net_size"], multiple=PREPROCESS["multiple"]):
    """The network input size (H, W) for an h x w photograph: scales size / h and size / w, both axes take the one whose
    |1 - s| is smaller (a tie takes the height's), each side round(s * side / multiple) * multiple with numpy's round (half
    to even, which Python's round is too)."""
    sh, sw = size / h, size / w
    if abs(1 - sw) < abs(1 - sh):
        sh = sw
    else:
        sw = sh
    return int(round(sh * h / multiple) * multiple), int(round(sw * w / multiple) * multiple)


def resize_pos_embed(pos, gh, gw):
    """timm / DPT's _resize_pos_embed: the P x P grid part of pos_embed [1, 1 + P * P, D] resized to (gh, gw) with
    F.interpolate(mode="bilinear", align_corners=False); the class row is kept.  Returns [1 + gh * gw, D]."""
    n = pos.shape[1] - 1
    P = int(round(math.sqrt(n)))
    if P * P != n:
        raise ValueError(f"pos_embed: {n} patch rows are not a square grid")
    D = pos.shape[-1]
    grid = pos[0, 1:].reshape(1, P, P, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(gh, gw), mode="bilinear", align_corners=False)
    return torch.cat([pos[0, :1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


# ---- weight re-layouts (once, at load time, on the host) ------------------------------------------------------------------

def relay_conv3x3(w):
    """[C_out][C_in][3][3] -> [C_out][3][3][C_in]: K = (ky, kx, ci) runs along contiguous channels of an NHWC map."""
    return w.permute(0, 2, 3, 1).contiguous()


def relay_conv_transpose(w):
    """ConvTranspose2d weight [C_in][C_out][s][s] (kernel = stride) -> [(dy, dx, c_out)][c_in]: the product with a pixel's
    channels gives that pixel's s x s block of outputs, which upnerf_depth_to_space scatters."""
    ci, co, s, s2 = w.shape
    return w.permute(2, 3, 1, 0).reshape(s * s2 * co, ci).contiguous()


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class DptDepth:
    """The weights as fp32 tensors in the layouts the kernels take, plus buffers per network size.  A plain object."""

    def __init__(self, params, *, heads=MODEL["heads"], hooks=MODEL["hooks"], stage_widths=MODEL["stage_widths"],
                 fusion=MODEL["fusion"], head=MODEL["head"], net_size=MODEL["net_size"], patch=MODEL["patch"]):
        def want(key, shape):
            if key not in params:
                raise ValueError(f"missing key {key!r}")
            t = params[key]
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
            return _f32(t)

        if KEYS["cls"] not in params:
            raise ValueError(f"missing key {KEYS['cls']!r}")
        cls = params[KEYS["cls"]]
        if cls.dim() != 3 or tuple(cls.shape[:2]) != (1, 1):
            raise ValueError(f"{KEYS['cls']}: expected shape (1, 1, D), got {tuple(cls.shape)}")
        D = int(cls.shape[-1])
        if heads < 1 or D % heads or D // heads != MODEL["head_dim"]:
            raise ValueError(f"width {D} with {heads} heads is a head dim of {D / max(heads, 1):g}; the attention kernel is "
                             f"built for {MODEL['head_dim']}")
        if D > 1024:
            raise ValueError(f"width {D}: the layer norm kernel takes at most 1024")
        depth = 0
        while KEYS["block"].format(i=depth) + "norm1.weight" in params:
            depth += 1
        if len(hooks) != 4 or len(stage_widths) != 4 or len(head) != 2:
            raise ValueError("hooks and stage_widths have four entries, head two")
        if any(not 0 <= h < depth for h in hooks) or list(hooks) != sorted(hooks):
            raise ValueError(f"hooks={tuple(hooks)} with {depth} blocks in the weights")
        for name, widths in (("stage_widths", stage_widths), ("fusion", (fusion,)), ("head", head)):
            if any(c < 32 or c % 32 or c > 1024 for c in widths):
                raise ValueError(f"{name}={widths}: upnerf_conv3x3 takes channel counts in multiples of 32 up to 1024")
        if (3 * patch * patch) % 8 or net_size % (2 * patch):
            raise ValueError(f"patch={patch}, net_size={net_size}: the net size must be a multiple of twice the patch")
        if KEYS["pos"] not in params:
            raise ValueError(f"missing key {KEYS['pos']!r}")
        pos = _f32(params[KEYS["pos"]])
        P = int(round(math.sqrt(max(pos.shape[1] - 1, 0)))) if pos.dim() == 3 else 0
        if pos.dim() != 3 or pos.shape[0] != 1 or pos.shape[2] != D or P < 1 or P * P != pos.shape[1] - 1:
            raise ValueError(f"{KEYS['pos']}: expected shape (1, 1 + P * P, {D}), got {tuple(pos.shape)}")
        self.D, self.heads, self.depth, self.patch, self.hidden = D, heads, depth, patch, MODEL["mlp_ratio"] * D
        self.hooks, self.stage_widths, self.fusion, self.head, self.net = tuple(hooks), tuple(stage_widths), fusion, tuple(head), net_size
        self.pos = pos  # resized per grid on the host at setup, resize_pos_embed
        self.w = w = {}
        w["cls"] = _f32(cls.reshape(D))
        w["pe_w"] = want(KEYS["pe_w"], (D, 3, patch, patch)).reshape(D, 3 * patch * patch)
        w["pe_b"] = want(KEYS["pe_b"], (D,))
        dims = {"D": D, "3D": 3 * D, "4D": self.hidden}
        self.blocks = []
        for i in range(hooks[-1] + 1):  # blocks past the last hook never run and are not kept
            self.blocks.append({name: want(KEYS["block"].format(i=i) + name, [dims[s] for s in shape.split(",")])
                                for name, shape in vit.BLOCK_KEYS})
        Fw = fusion
        for k, (S, scale) in enumerate(zip(stage_widths, REASSEMBLE_SCALE), 1):
            ro = KEYS["readout"].format(k=k)
            rw = want(ro + "weight", (D, 2 * D))
            w[f"ro{k}_tok"], w[f"ro{k}_cls"] = rw[:, :D].contiguous(), rw[:, D:].contiguous()  # W [t_n ; t_cls] = W_tok t_n + W_cls t_cls
            w[f"ro{k}_b"] = want(ro + "bias", (D,))
            pj = KEYS["project"].format(k=k)
            w[f"pj{k}_w"], w[f"pj{k}_b"] = want(pj + "weight", (S, D, 1, 1)).reshape(S, D), want(pj + "bias", (S,))
            rs = KEYS["resample"].format(k=k)
            if scale > 1:
                w[f"rs{k}_w"] = relay_conv_transpose(want(rs + "weight", (S, S, scale, scale)))
                w[f"rs{k}_b"] = want(rs + "bias", (S,))
            elif scale < 0:
                w[f"rs{k}_w"], w[f"rs{k}_b"] = relay_conv3x3(want(rs + "weight", (S, S, 3, 3))), want(rs + "bias", (S,))
            w[f"rn{k}_w"] = relay_conv3x3(want(KEYS["layer_rn"].format(k=k), (Fw, S, 3, 3)))
            for u in ((2,) if k == 4 else (1, 2)):  # refinenet4 takes one input: its resConfUnit1 is not read
                for c in (1, 2):
                    key = KEYS["rcu"].format(k=k, u=u, c=c)
                    w[f"f{k}u{u}c{c}_w"], w[f"f{k}u{u}c{c}_b"] = relay_conv3x3(want(key + "weight", (Fw, Fw, 3, 3))), want(key + "bias", (Fw,))
            oc = KEYS["out_conv"].format(k=k)
            w[f"f{k}o_w"], w[f"f{k}o_b"] = want(oc + "weight", (Fw, Fw, 1, 1)).reshape(Fw, Fw), want(oc + "bias", (Fw,))
        h0, h1 = head
        hk = lambda j: KEYS["head"].format(j=j)
        w["h0_w"], w["h0_b"] = relay_conv3x3(want(hk(0) + "weight", (h0, Fw, 3, 3))), want(hk(0) + "bias", (h0,))
        w["h2_w"], w["h2_b"] = relay_conv3x3(want(hk(2) + "weight", (h1, h0, 3, 3))), want(hk(2) + "bias", (h1,))
        w["h4_w"], w["h4_b"] = want(hk(4) + "weight", (1, h1, 1, 1)).reshape(1, h1), want(hk(4) + "bias", (1,))
        self._pos_cache, self._bufs = {}, {}

    @classmethod
    def from_state_dict(cls, sd, **kw):
        return cls(sd, **kw)

    @classmethod
    def load(cls, path, model_type="dpt_large", **kw):
        check_model_type(model_type)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        for wrap in ("state_dict", "model"):  # (a training checkpoint keeps the weights one level down)
            if isinstance(sd, dict) and KEYS["cls"] not in sd and wrap in sd and isinstance(sd[wrap], dict):
                sd = sd[wrap]
        return cls.from_state_dict(sd, **kw)

    def to(self, device):
        self.w = {k: v.to(device) for k, v in self.w.items()}
        self.blocks = [{k: v.to(device) for k, v in b.items()} for b in self.blocks]
        self._pos_cache, self._bufs = {}, {}
        return self

    def cuda(self):
        return self.to("cuda")

    @property
    def device(self):
        return self.w["cls"].device

    def net_size(self, h, w):
        return net_size(h, w, self.net)

    def _pos_rows(self, gh, gw, device):
        key = (gh, gw, str(device))
        if key not in self._pos_cache:
            self._pos_cache[key] = resize_pos_embed(self.pos, gh, gw).contiguous().to(device)
        return self._pos_cache[key]

    def _buf(self, size, name, *shape):
        """A buffer of the network size `size`, allocated on first use and kept."""
        key = (size, name, str(self.device))
        if key not in self._bufs:
            self._bufs[key] = torch.empty(*shape, dtype=torch.float32, device=self.device)
        return self._bufs[key]

    # -- single launches (maps are [H * W][C] tensors: NHWC with the row stride C) -----------------------------------------
    def _conv(self, name, x, H, W, wk, bk, y, stride=1, pre_relu=0, relu=0, res=None):
        w = self.w[wk]
        co, ci = int(w.shape[0]), int(w.shape[3])
        a = _lib.Conv3x3Args(H=H, W=W, C_in=ci, C_out=co, stride=stride, pre_relu=pre_relu, relu=relu, x=_lib.ptr(x), ldx=ci,
                             w=_lib.ptr(w), bias=_lib.ptr(self.w[bk]) if bk else None, res=_lib.ptr(res), ldr=co, y=_lib.ptr(y),
                             ldy=co)
        st = _lib.stream()
        M = ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        # (timed per shape: the small maps fill few CUs, tools/bench_dpt.py records what that costs)
        _lib.check(TIMER.run(f"{name}_{H}x{W}_{ci}to{co}", lambda: _lib.lib.upnerf_conv3x3(C.byref(a), st), units=2 * M * co * 9 * ci),
                   "upnerf_conv3x3")

    def _upsample(self, x, H, W, Cn, y):
        a = _lib.Upsample2xArgs(H=H, W=W, C=Cn, x=_lib.ptr(x), ldx=Cn, y=_lib.ptr(y), ldy=Cn)
        st = _lib.stream()
        _lib.check(TIMER.run("dpt_upsample2x", lambda: _lib.lib.upnerf_upsample2x(C.byref(a), st)), "upnerf_upsample2x")

    def _rcu(self, size, key, x, H, W, out):
        """out = conv2(relu(conv1(relu(x)))) + x: two launches, the ReLUs on the operand load, the residual in the epilogue."""
        t = self._buf(size, f"rcu_t{H}x{W}", H * W, self.fusion)
        self._conv("dpt_conv3x3_rcu", x, H, W, key + "c1_w", key + "c1_b", t, pre_relu=1)
        self._conv("dpt_conv3x3_rcu", t, H, W, key + "c2_w", key + "c2_b", out, pre_relu=1, res=x)

    def forward_net(self, x: torch.Tensor, return_stages: bool = False):
        """x: the normalised network-size input, [H][W][3] fp32 on the device, H and W multiples of twice the patch.  Returns the
        inverse depth [H][W]; with return_stages also a dict: `reassembled` (the four maps [h][w][S_k] before layerK_rn),
        `fusion` (the outputs of refinenet4, 3, 2, 1, [h][w][F]) and `head`.  The returned tensors are this object's buffers:
        the next call of the same size overwrites them."""
        if x.dim() != 3 or x.shape[2] != 3:
            raise ValueError(f"expected an [H][W][3] input, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
        if x.dtype != torch.float32:
            raise TypeError(f"forward_net takes the normalised fp32 input (got {x.dtype})")
        if self.device != x.device:
            raise RuntimeError(f"DptDepth weights are on {self.device}, the input on {x.device}; call .to()")
        H, W, P, D, Fw, w = int(x.shape[0]), int(x.shape[1]), self.patch, self.D, self.fusion, self.w
        if H % (2 * P) or W % (2 * P) or H < 2 * P or W < 2 * P:
            raise ValueError(f"the network input ({H} x {W}) must be a multiple of {2 * P} on both sides")
        x = x.contiguous()
        size = (H, W)
        gh, gw = H // P, W // P
        T, N, Kp = gh * gw, gh * gw + 1, 3 * P * P
        lib, st = _lib.lib, _lib.stream()
        buf = lambda name, *shape: self._buf(size, name, *shape)
        rows, tok, xn, qkv, att, hid = (buf("rows", T, Kp), buf("tok", N, D), buf("xn", N, D), buf("qkv", N, 3 * D), buf("att", N, D),
                                        buf("hid", N, self.hidden))
        pos = self._pos_rows(gh, gw, x.device)

        # -- backbone
        pa = _lib.VitPatches16Args(H=H, W=W, patch=P, image=_lib.ptr(x), rows=_lib.ptr(rows))
        _lib.check(TIMER.run("dpt_patches", lambda: lib.upnerf_vit_patches16(C.byref(pa), st)), "upnerf_vit_patches16")
        vit.linear("dpt_patch_proj", T, D, Kp, _lib.ptr(rows), Kp, w["pe_w"], w["pe_b"], tok.data_ptr() + 4 * D, D)
        _lib.check(TIMER.run("dpt_embed", lambda: lib.upnerf_vit_embed(N, D, _lib.ptr(w["cls"]), _lib.ptr(pos), _lib.ptr(tok), st)),
                   "upnerf_vit_embed")
        hooked = [buf(f"hook{k}", N, D) for k in range(4)]

        def after(i):
            for k, h in enumerate(self.hooks):
                if h == i:
                    hooked[k].copy_(tok)  # (a device-to-device copy of the raw block output)

        vit.run_blocks(self.blocks, N, D, self.heads, self.hidden, tok, xn, qkv, att, hid, "dpt", after=after)

        # -- reassemble: readout, the token grid as an NHWC map, 1 x 1 projection, resample; then layerK_rn
        maps, dims, rn = [], [], []
        for k, (S, scale) in enumerate(zip(self.stage_widths, REASSEMBLE_SCALE), 1):
            act = hooked[k - 1]
            clsb, ro, pj = buf(f"clsb{k}", D), buf("ro", T, D), buf(f"pj{k}", T, S)
            # W [t_n ; t_cls] + b = W_tok t_n + (W_cls t_cls + b): the class half is one M = 1 product, the bias of the other
            vit.linear("dpt_readout_cls", 1, D, D, _lib.ptr(act), D, w[f"ro{k}_cls"], w[f"ro{k}_b"], _lib.ptr(clsb), D)
            vit.linear("dpt_readout", T, D, D, act.data_ptr() + 4 * D, D, w[f"ro{k}_tok"], clsb, _lib.ptr(ro), D)
            vit.gelu("dpt_gelu", ro, T * D)
            vit.linear("dpt_project", T, S, D, _lib.ptr(ro), D, w[f"pj{k}_w"], w[f"pj{k}_b"], _lib.ptr(pj), S)
            if scale > 1:
                wide, m = buf(f"wide{k}", T, scale * scale * S), buf(f"map{k}", T * scale * scale, S)
                vit.linear("dpt_conv_transpose", T, scale * scale * S, S, _lib.ptr(pj), S, w[f"rs{k}_w"], None, _lib.ptr(wide),
                           scale * scale * S)
                da = _lib.DepthToSpaceArgs(H=gh, W=gw, C=S, s=scale, x=_lib.ptr(wide), ldx=scale * scale * S,
                                           bias=_lib.ptr(w[f"rs{k}_b"]), y=_lib.ptr(m), ldy=S)
                _lib.check(TIMER.run("dpt_depth_to_space", lambda: lib.upnerf_depth_to_space(C.byref(da), st)),
                           "upnerf_depth_to_space")
                mh, mw = gh * scale, gw * scale
            elif scale < 0:
                mh, mw = (gh - 1) // 2 + 1, (gw - 1) // 2 + 1
                m = buf(f"map{k}", mh * mw, S)
                self._conv("dpt_conv3x3_s2", pj, gh, gw, f"rs{k}_w", f"rs{k}_b", m, stride=2)
            else:
                m, mh, mw = pj, gh, gw
            maps.append(m)
            dims.append((mh, mw))
            r = buf(f"rn{k}", mh * mw, Fw)
            self._conv("dpt_conv3x3_rn", m, mh, mw, f"rn{k}_w", None, r)
            rn.append(r)

        # -- fusion: refinenet4 (one input), then 3, 2, 1 (the path so far and layerK_rn)
        paths, path = [], None
        for k in (4, 3, 2, 1):
            mh, mw = dims[k - 1]
            if path is None:
                cur = rn[k - 1]
            else:
                cur = buf(f"sum{k}", mh * mw, Fw)
                self._rcu(size, f"f{k}u1", rn[k - 1], mh, mw, cur)
                vit.residual("dpt_add", cur, path, mh * mw * Fw)  # out = x0 + RCU1(x1)
            r2, up, path = buf(f"rcu2_{k}", mh * mw, Fw), buf(f"up{k}", 4 * mh * mw, Fw), buf(f"path{k}", 4 * mh * mw, Fw)
            self._rcu(size, f"f{k}u2", cur, mh, mw, r2)
            self._upsample(r2, mh, mw, Fw, up)
            vit.linear("dpt_out_conv", 4 * mh * mw, Fw, Fw, _lib.ptr(up), Fw, w[f"f{k}o_w"], w[f"f{k}o_b"], _lib.ptr(path), Fw)
            paths.append(path)

        # -- head
        h0, h1 = self.head
        ph, pw = 2 * dims[0][0], 2 * dims[0][1]
        a0, a1, a2, out = buf("head0", ph * pw, h0), buf("head1", 4 * ph * pw, h0), buf("head2", 4 * ph * pw, h1), buf("out", 2 * ph, 2 * pw)
        self._conv("dpt_conv3x3_head0", path, ph, pw, "h0_w", "h0_b", a0)
        self._upsample(a0, ph, pw, h0, a1)
        self._conv("dpt_conv3x3_head2", a1, 2 * ph, 2 * pw, "h2_w", "h2_b", a2, relu=1)
        vit.linear("dpt_head4", 4 * ph * pw, 1, h1, _lib.ptr(a2), h1, w["h4_w"], w["h4_b"], _lib.ptr(out), 1, act=1)
        if not return_stages:
            return out
        return out, dict(reassembled=[m.view(d[0], d[1], -1) for m, d in zip(maps, dims)],
                         fusion=[p.view(2 * dims[k - 1][0], 2 * dims[k - 1][1], Fw) for p, k in zip(paths, (4, 3, 2, 1))], head=out)

    def _resize(self, name, x, h, w, H, W, Cn, y, u8=0, affine=False):
        a = _lib.ResizeCubicArgs(h=h, w=w, H=H, W=W, C=Cn, u8=u8, affine=int(affine), x=_lib.ptr(x), y=_lib.ptr(y))
        a.mean[:], a.std[:] = PREPROCESS["mean"], PREPROCESS["std"]
        st = _lib.stream()
        _lib.check(TIMER.run(name, lambda: _lib.lib.upnerf_resize_cubic(C.byref(a), st)), "upnerf_resize_cubic")

    def inverse_depth(self, image: torch.Tensor) -> torch.Tensor:
        """image: the photograph [h][w][3] on the device, uint8 (divided by 255 on the way in) or fp32 already in [0, 1].  Returns
        the inverse depth [h][w] fp32 (a new tensor), in the network's own unnormalised units."""
        if image.dim() != 3 or image.shape[2] != 3:
            raise ValueError(f"expected an [h][w][3] image, got {tuple(image.shape)}")
        if not image.is_cuda:
            raise RuntimeError("libupnerf_hip operates on device memory only (got a CPU tensor)")
        if image.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"inverse_depth takes uint8 or fp32 images (got {image.dtype})")
        if self.device != image.device:
            raise RuntimeError(f"DptDepth weights are on {self.device}, the image on {image.device}; call .to()")
        image = image.contiguous()
        h, w = int(image.shape[0]), int(image.shape[1])
        H, W = self.net_size(h, w)
        x = self._buf((H, W), "input", H, W, 3)
        self._resize("dpt_resize_in", image, h, w, H, W, 3, x, u8=int(image.dtype == torch.uint8), affine=True)
        net = self.forward_net(x)
        out = torch.empty(h, w, dtype=torch.float32, device=image.device)
        self._resize("dpt_resize_out", net, H, W, h, w, 1, out)
        return out


def load_image(path) -> torch.Tensor:
    """An image file as the uint8 [h][w][3] RGB array `inverse_depth` takes: decoded in PIL on the host."""
    import numpy as np
    from PIL import Image
    return torch.from_numpy(np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8).copy())
