"""Parameter packing for the fused field kernels.

The HIP kernels read every matrix of one NeRF from ONE flat fp32 buffer `P` (row-major [N][Kp], K padded to a
multiple of 8, see include/upnerf_hip.h:upnerf_layout) and the backward chain reads transposed copies from `PT`.
`pack()` builds P from the module's parameters with differentiable torch ops (pad / cat / one small matmul for the
folded colour layer), so the gradient the kernels write in P's layout flows back to parameters that keep the
reference's names and shapes (models/nerf.py:39-78) -- state_dicts stay interchangeable with the reference.

Folding: rgb_share_layer.0 consumes cat[s_feat, PE(dir), a] with s_feat = W_f e + b_f, so
  W_r1[:, :F] s_feat = (W_r1[:, :F] W_f) e + W_r1[:, :F] b_f
and the kernels only ever see the [W/2][W] product; autograd differentiates the product."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Dict

import torch
import torch.nn.functional as F

from . import zero_pool
from ._lib import CK, MAX_D, Frag16Desc, FragDesc, Layout, PackDesc
from .pass_plan import (EXP_C1, EXP_C2, EXP_FINAL, EXP_HEAD_T, EXP_R1, block_offset, block_size, blocks_by_field, layout_offsets,
                        param_blocks, t_blocks)

# One copy of the pack launch: `rows` x `cols` floats from column col0 of the parameter `name` (row pitch src_ld) to column
# dst_col0 of `block` (None: the scratch area behind P); form: "both", or the one direction ("fwd" / "bwd") it belongs to
_Copy = namedtuple("_Copy", "name col0 rows cols src_ld block dst_col0 form")


class _PackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packer, names, *tensors):
        from ._lib import check, lib, ptr, stream
        L, W, W2, Fd, ldr = packer.L, packer.W, packer.W2, packer.feat_dim, packer.block["wr1"].ld
        p = {n: t.detach().contiguous() for n, t in zip(names, tensors)}
        dev = tensors[0].device
        if not packer.encode_feat:  # no feature layer to fold into the colour head: the pack launch is the whole job
            buf = zero_pool.zeros(L.total, dev)
            arr = packer._pack_descs(lambda n: p[n].data_ptr())
            check(lib.upnerf_pack(ptr(buf), arr, len(arr), 0, stream()), "upnerf_pack")
            ctx.packer, ctx.names, ctx.buf = packer, names, None
            ctx.shapes = [tuple(t.shape) for t in tensors]
            return buf
        buf = zero_pool.zeros(L.total + W2 * Fd, dev)  # P followed by a copy of W_r1[:, :F]
        st = stream()
        arr = packer._pack_descs(lambda n: p[n].data_ptr(), L.total)
        check(lib.upnerf_pack(ptr(buf), arr, len(arr), 0, st), "upnerf_pack")
        base = buf.data_ptr()
        wrF = base + 4 * L.total
        # folded colour layer: W_r1[:, :F] . W_feat -> wr1[:, :W];  W_r1[:, :F] . b_feat + b_r1 -> br1
        check(lib.upnerf_linear(W2, W, Fd, wrF, Fd, ptr(p["feat_share_layer.weight"]), W, None, base + 4 * L.wr1, ldr, 2,
                                st), "upnerf_linear")
        # W_r1[:, :F] . b_feat + b_r1 -> br1: one small matrix-vector launch straight into P (r3 ADVICE: rocBLAS gemv made the
        # summation order -- and with it the bitwise replay == eager contract -- depend on the rocBLAS version, and created its
        # handle inside a capture)
        check(lib.upnerf_matvec(W2, Fd, wrF, Fd, ptr(p["feat_share_layer.bias"]), ptr(p["rgb_share_layer.0.bias"]), base + 4 * L.br1, 0,
                                st), "upnerf_matvec")
        ctx.packer, ctx.names, ctx.buf = packer, names, buf
        ctx.save_for_backward(p["feat_share_layer.weight"], p["feat_share_layer.bias"])
        ctx.shapes = [tuple(t.shape) for t in tensors]
        return buf[:L.total]

    @staticmethod
    def backward(ctx, dP):
        from ._lib import check, lib, ptr, stream
        from .ops import wgrad_blocks_into, wgrad_into
        packer, names, buf = ctx.packer, ctx.names, ctx.buf
        L, W, W2, Fd, ldr = packer.L, packer.W, packer.W2, packer.feat_dim, packer.block["wr1"].ld
        dP = dP.contiguous()
        dev = dP.device
        st = stream()
        # one flat buffer for all parameter gradients
        sizes = [math.prod(s) for s in ctx.shapes]
        flat = zero_pool.zeros(sum(sizes), dev)
        grads, off = {}, 0
        for n, s_, k in zip(names, ctx.shapes, sizes):
            grads[n] = flat[off:off + k].view(s_)
            off += k
        arr = packer._pack_descs(lambda n: grads[n].data_ptr())
        check(lib.upnerf_pack(ptr(dP), arr, len(arr), 1, st), "upnerf_pack")
        if not packer.encode_feat:
            return (None, None) + tuple(grads[n] for n in names)
        feat_w, feat_b = ctx.saved_tensors
        base = dP.data_ptr()
        gbr1 = dP[L.br1:L.br1 + W2]
        g_wr = grads["rgb_share_layer.0.weight"]          # [W2][F + 27 + A]
        in_rgb = g_wr.shape[1]
        # d W_r1[:, :F] = gfold . W_feat^T + gbr1 (x) b_feat
        check(lib.upnerf_linear(W2, Fd, W, base + 4 * L.wr1, ldr, ptr(feat_w), W, None, ptr(g_wr), in_rgb, 0, st),
              "upnerf_linear")
        # (the second term, g_wr[:, :F] += gbr1 (x) b_feat, rides on the matrix-vector launch below: upnerf_matvec_rank1)
        # d W_feat = W_r1[:, :F]^T . gfold ; d b_feat = W_r1[:, :F]^T . gbr1 ; d b_r1 = gbr1
        wrF = buf[L.total:].view(W2, Fd)
        g_fw = grads["feat_share_layer.weight"]
        if Fd > 256:
            wgrad_blocks_into(W2, wrF, Fd, Fd, dP, ldr, W, g_fw.data_ptr(), W, None, dev, b_off=L.wr1)
        else:
            wgrad_into(W2, wrF, Fd, Fd, dP, ldr, W, g_fw.data_ptr(), W, None, dev, b_off=L.wr1)
        check(lib.upnerf_matvec_rank1(W2, Fd, ptr(wrF), Fd, ptr(gbr1), ptr(grads["feat_share_layer.bias"]), ptr(g_wr), in_rgb,
                                      ptr(feat_b), st), "upnerf_matvec_rank1")
        return (None, None) + tuple(grads[n] for n in names)


class NerfPacker:
    def __init__(self, W: int, D: int, skips, in_xyz: int, in_dir: int, feat_dim: int, appearance_dim: int,
                 candidate_dim: int, encode_feat: bool = True):
        # encode_feat = False (models/nerf.py:52-56, 110-123): the colour head reads xyz_encoding_final itself, so the
        # "folded" first colour matrix of the layout is W_r1[:, :W] as it stands -- same layout, no fold launches
        self.encode_feat = bool(encode_feat)
        if W not in (64, 256):
            raise ValueError(f"HIP field kernels support W in (64, 256), got {W}")
        if not 1 <= D <= MAX_D:
            raise ValueError(f"HIP field kernels support 1 <= D <= {MAX_D}, got {D}")
        if in_xyz != 63:
            raise ValueError("HIP field kernels are specialised for N_emb_xyz = 10 (63-wide encoding)")
        if in_dir != 27:
            raise ValueError("HIP field kernels are specialised for N_emb_dir = 4 (27-wide encoding)")
        if appearance_dim not in (0, 48) or candidate_dim not in (0, CK):
            raise ValueError("HIP field kernels support appearance_dim in (0, 48) and candidate_dim in (0, 16)")
        active = [s for s in skips if 0 < s < D]
        if len(active) > 1:
            raise ValueError("at most one active skip connection is supported")
        self.W, self.D, self.W2 = W, D, W // 2
        self.skip = active[0] if active else -1
        self.feat_dim, self.A, self.C, self.in_dir = feat_dim, appearance_dim, candidate_dim, in_dir
        self.has_cand = candidate_dim > 0
        # the blocks of P and of the transposed set (pass_plan states them once), their offsets as plain integers
        # (pass_plan.wgrad_schedule reads these), and the same in the struct the kernels take
        self.blocks, self.tblocks, self.block = (f(W, D, self.skip) for f in (param_blocks, t_blocks, blocks_by_field))
        self.offsets = layout_offsets(W, D, self.skip)
        L = Layout()
        for k, v in self.offsets._asdict().items():
            if isinstance(v, tuple):  # one per layer
                getattr(L, k)[:D] = v
            else:
                setattr(L, k, v)
        self.L = L
        self._copies = self._source_map()
        self._pack_forms, self._frag_descs = {f: self._pack_template(f) for f in ("fwd", "bwd")}, self._make_frag_descs()

    # layout field -> the reference parameter a block is a plain copy of (w, b: per layer; wr1, br1: _source_map)
    PARAM = {"we": "xyz_encoding_final.weight", "be": "xyz_encoding_final.bias", "wsig": "share_sigma.0.weight",
             "bsig": "share_sigma.0.bias", "wc1": "candidate_encoding.0.weight", "bc1": "candidate_encoding.0.bias",
             "wc2": "candidate_encoding.2.weight", "bc2": "candidate_encoding.2.bias", "wcsig": "candidate_sigma.0.weight",
             "bcsig": "candidate_sigma.0.bias", "wr2": "rgb_share_layer.2.weight", "br2": "rgb_share_layer.2.bias"}

    def _source_map(self):
        """Which columns of which reference parameter are copied where: [_Copy] in the order of the pack launch's descriptors (a
        layer's matrix and bias together, then block order).  form "fwd": the contiguous copy of W_r1[:, :F] the fold reads, to a
        scratch area behind P (block None); "bwd": d b_r1 = d br1, which forward is the mat-vec's output, not a copy."""
        wr, naux = "rgb_share_layer.0.weight", self.in_dir + self.A
        Fd = self.feat_dim if self.encode_feat else self.W  # columns of W_r1 in front of [PE(dir) | appearance]
        out = []
        for b in sorted(self.blocks, key=lambda b: self.D if b.layer is None else b.layer):
            if b.field == "wr1" and self.encode_feat:  # the side columns; [:, :W] is the fold's
                out += [_Copy(wr, Fd, b.rows, naux, Fd + naux, b, b.part("dir").col0, "both"),
                        _Copy(wr, 0, b.rows, Fd, Fd + naux, None, 0, "fwd")]
            elif b.field == "wr1":  # W_r1 = [W | PE(dir) | appearance] as it stands
                out.append(_Copy(wr, 0, b.rows, Fd + naux, Fd + naux, b, 0, "both"))
            elif b.field == "br1":
                out.append(_Copy("rgb_share_layer.0.bias", 0, 1, b.cols, b.cols, b, 0, "bwd" if self.encode_feat else "both"))
            elif self.has_cand or not self.PARAM.get(b.field, "").startswith("candidate"):  # its parts, side by side
                name = self.PARAM.get(b.field) or f"xyz_encoding_{b.layer + 1}.0.{'weight' if b.field == 'w' else 'bias'}"
                c0 = 0
                for part in b.parts:
                    if c0 and out[-1].dst_col0 + out[-1].cols == part.col0:  # no padding between the two: one copy
                        out[-1] = out[-1]._replace(cols=out[-1].cols + part.cols)
                    else:
                        out.append(_Copy(name, c0, b.used_rows, part.cols, b.cols, b, part.col0, "both"))
                    c0 += part.cols
        return out

    # ------------------------------------------------------------------ forward-form buffer
    def pack(self, p: Dict[str, torch.Tensor]) -> torch.Tensor:
        """p: name -> parameter (reference names, e.g. 'xyz_encoding_1.0.weight').  Returns P [L.total]."""
        dev = p["xyz_encoding_1.0.weight"].device
        folded = {}
        if self.encode_feat:  # the fold (module docstring): [W/2][W] in front of wr1's side columns, and br1
            wrF = p["rgb_share_layer.0.weight"][:, :self.feat_dim]
            folded = {"wr1": wrF @ p["feat_share_layer.weight"],
                      "br1": (wrF @ p["feat_share_layer.bias"] + p["rgb_share_layer.0.bias"])[None]}
        pieces = []
        for b in self.blocks:
            cols = [(0, folded[b.field])] if b.field in folded else []
            cols += [(c.dst_col0, p[c.name].reshape(-1, c.src_ld)[:, c.col0:c.col0 + c.cols])
                     for c in self._copies if c.block is b and c.form != "bwd"]
            if not cols:  # a head the model does not have
                pieces.append(torch.zeros(block_size(b), device=dev, dtype=torch.float32))
                continue
            row, end = [], 0
            for c0, t in cols:  # (in column order) zero columns between the parts, behind the last one, then zero rows
                row.append(F.pad(t, (c0 - end, 0)))
                end = c0 + t.shape[1]
            m = F.pad(torch.cat(row, 1), (0, b.ld - end)).reshape(-1)
            pieces.append(F.pad(m, (0, block_size(b) - m.numel())))
        P = torch.cat(pieces)
        assert P.numel() == self.L.total
        return P

    # ------------------------------------------------------------------ HIP pack (product path on the GPU)
    def _pack_template(self, form):
        """One direction's copy descriptors as bytes (the packer stays copyable), pointers as byte offsets; what fills them per call."""
        cs = [c for c in self._copies if c.form in ("both", form)]
        arr = (PackDesc * len(cs))(*[
            PackDesc(4 * c.col0, c.rows, c.cols, c.src_ld, block_offset(self.L, c.block) + c.dst_col0 if c.block else 0,
                     c.block.ld if c.block else c.cols, 0) for c in cs])
        return bytes(arr), [(i, c.name, 4 * c.col0) for i, c in enumerate(cs)], [i for i, c in enumerate(cs) if c.block is None]

    def _pack_descs(self, base_of, scratch_off=None):
        """Copy descriptors of pack() as the array upnerf_pack takes.  `base_of(name)` gives the device pointer a descriptor starts
        from (the parameter, or its gradient buffer for the backward); `scratch_off`: where the contiguous copy of W_r1[:, :F]
        goes (forward only; its gradient comes from the fold, not from a copy)."""
        tmpl, fill, scratch = self._pack_forms["bwd" if scratch_off is None else "fwd"]
        arr = (PackDesc * len(fill)).from_buffer_copy(tmpl)
        for i, name, byte0 in fill:
            arr[i].ptr = base_of(name) + byte0
        for i in scratch:
            arr[i].dst_off = scratch_off
        return arr

    PACK_NAMES_BASE = ["share_sigma.0.weight", "share_sigma.0.bias", "xyz_encoding_final.weight", "xyz_encoding_final.bias",
                       "feat_share_layer.weight", "feat_share_layer.bias", "rgb_share_layer.0.weight",
                       "rgb_share_layer.0.bias", "rgb_share_layer.2.weight", "rgb_share_layer.2.bias"]

    def pack_names(self):
        base = [n for n in self.PACK_NAMES_BASE if self.encode_feat or not n.startswith("feat_share_layer")]
        names = [f"xyz_encoding_{l + 1}.0.{k}" for l in range(self.D) for k in ("weight", "bias")] + base
        return names + [n for n in self.PARAM.values() if n.startswith("candidate") and self.has_cand]

    def pack_hip(self, p: Dict[str, torch.Tensor]) -> torch.Tensor:
        """pack() with HIP kernels and a hand-written backward: 4 launches instead of ~45 (and ~10 instead of ~50 in the
        backward).  Same layout; the folded colour matrix is produced by upnerf_linear (exact fp32 MFMA)."""
        names = self.pack_names()
        return _PackFn.apply(self, names, *[p[n] for n in names])

    # ------------------------------------------------------------------ one-launch HIP re-layout (product path)
    EXP_FINAL, EXP_C1, EXP_C2, EXP_R1, EXP_HEAD_T = EXP_FINAL, EXP_C1, EXP_C2, EXP_R1, EXP_HEAD_T  # (pass_plan's; trunk layer l: id l)

    def _make_frag_descs(self):
        """(forward descriptors, n, transposed descriptors, n) for upnerf_frag_copy and, with the exponent ids, for upnerf_frag16.
        Forward: every matrix block onto itself.  Transposed: every feed of every block of PT, the trunk's by layer and source
        column (a skip layer's encoding columns first) and then the struct's order -- the kernels index the row norms
        upnerf_frag16 returns by descriptor."""
        L = self.L
        fwd = [(block_offset(L, b), b.ld, 0, b.rows, b.ld, block_offset(L, b), b.ld, 0, b.exp) for b in self.blocks if b.matrix]
        feeds = sorted(((t, f) for t in self.tblocks for f in t.feeds),
                       key=lambda tf: (self.D, 0) if tf[1].src.layer is None else (tf[1].src.layer, tf[1].col0))
        bwd = [(block_offset(L, f.src) + f.col0, f.src.ld, 1, f.cols, f.src.rows, block_offset(L, t), t.ld, f.dst_col0, f.exp)
               for t, f in feeds]
        mk = lambda T, lst, n: (T * len(lst))(*[T(*d[:n]) for d in lst])
        return {T: (mk(T, fwd, n), len(fwd), mk(T, bwd, n), len(bwd)) for T, n in ((FragDesc, 8), (Frag16Desc, 9))}

    def _descs(self):
        return self._frag_descs[FragDesc]

    def _descs16(self):
        return self._frag_descs[Frag16Desc]

    @torch.no_grad()
    def frag_hip(self, P: torch.Tensor) -> torch.Tensor:
        """Kernel-side copy of P (matrices in fragment order) with one HIP launch."""
        from ._lib import check, lib, ptr, stream
        fd, nf, _, _ = self._descs()
        out = P.clone()
        check(lib.upnerf_frag_copy(ptr(P), ptr(out), fd, nf, stream()), "upnerf_frag_copy")
        return out

    @torch.no_grad()
    def frag_t_hip(self, P: torch.Tensor) -> torch.Tensor:
        """Fragment-ordered transposed copies (layout t_*) straight from the row-major P, one HIP launch."""
        from ._lib import check, lib, ptr, stream
        _, _, bd, nb = self._descs()
        out = torch.zeros(self.L.t_total, device=P.device, dtype=P.dtype)
        check(lib.upnerf_frag_copy(ptr(P), ptr(out), bd, nb, stream()), "upnerf_frag_copy")
        return out

    # ------------------------------------------------------------------ f16x3 re-layout (product path, W = 256)
    @torch.no_grad()
    def frag16_hip(self, P: torch.Tensor, perm: bool = False):
        """(P16, PT16, wexp, wnorm): every matrix of P (and its transposed copy) as scaled fp16 (hi, lo) MFMA fragments with
        one power-of-two exponent per matrix id -- what upnerf_field_fwd_f16x3 / upnerf_field_bwd_f16x3 read.  perm: both
        sets in the k order of the register-resident kernels (csrc/field16rr.hip: include/upnerf_hip.h, tile_rows = 256), plus
        the row 1-norms they bound their exponents with (wnorm [64]: forward matrices at 0.., transposed ones at 32..)."""
        from ._lib import check, lib, ptr, stream
        fd, nf, bd, nb = self._descs16()
        t0 = (self.L.total + 63) // 64 * 64  # the transposed set starts on a 256-byte boundary
        both = zero_pool.zeros(t0 + self.L.t_total, P.device)  # one fill for the two sets
        P16, PT16 = both[:self.L.total], both[t0:]
        scratch = torch.empty(16, device=P.device, dtype=torch.float32)
        wexp = torch.empty(16, device=P.device, dtype=torch.int32)
        wnorm = torch.empty(64, device=P.device, dtype=torch.float32) if perm else None
        check(lib.upnerf_frag16(ptr(P), ptr(P16), ptr(PT16), fd, nf, bd, nb, ptr(scratch), ptr(wexp), int(perm), int(perm),
                                ptr(wnorm), stream()), "upnerf_frag16")
        return P16, PT16, wexp, wnorm

    # ------------------------------------------------------------------ MFMA fragment order (no grad)
    @staticmethod
    def _frag_into(dst, src, off, n, kp):
        """dst[off:off+n*kp] = fragment-ordered copy of the row-major [n][kp] matrix at src[off:]:
        [n/32][kp/8][half(2)][lane%32][4]  (csrc/common.cuh:mma_lds)."""
        v = src[off:off + n * kp].view(n // 32, 32, kp // 8, 2, 4).permute(0, 2, 3, 1, 4)
        dst[off:off + n * kp].view(n // 32, kp // 8, 2, 32, 4).copy_(v)

    @torch.no_grad()
    def frag(self, P: torch.Tensor) -> torch.Tensor:
        """Kernel-side copy of P: matrices in fragment order, vectors (biases, 1/3-wide heads) unchanged."""
        out = P.clone()
        for b in self.blocks:
            if b.matrix:
                self._frag_into(out, P, block_offset(self.L, b), b.rows, b.ld)
        return out

    @torch.no_grad()
    def frag_t(self, PT: torch.Tensor) -> torch.Tensor:
        out = PT.clone()
        for t in self.tblocks:
            self._frag_into(out, PT, block_offset(self.L, t), t.rows, t.ld)
        return out

    # ------------------------------------------------------------------ transposed copies (no grad)
    @torch.no_grad()
    def pack_t(self, P: torch.Tensor) -> torch.Tensor:
        PT = torch.empty(self.L.t_total, device=P.device, dtype=P.dtype)
        for t in self.tblocks:
            o = block_offset(self.L, t)
            dst = PT[o:o + t.rows * t.ld].view(t.rows, t.ld)
            if not t.feeds:
                dst.zero_()
            for f in t.feeds:
                so = block_offset(self.L, f.src)
                src = P[so:so + f.src.rows * f.src.ld].view(f.src.rows, f.src.ld)
                dst[:, f.dst_col0:f.dst_col0 + f.src.rows] = src[:, f.col0:f.col0 + f.cols].t()
        return PT
