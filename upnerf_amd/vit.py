"""The pre-norm transformer block loop shared by the DINO extractor (dino.py) and the DPT backbone (dpt.py): single launches of
`upnerf_linear`, `upnerf_layernorm`, `upnerf_vit_attention`, `upnerf_vit_gelu` and `upnerf_vit_residual` (csrc/dino.hip) on the
caller's buffers.  A block is
    x += proj(attn(norm1 x));  x += fc2(gelu(fc1(norm2 x)))
with LayerNorm eps 1e-6, GELU in its exact erf form, heads of 64 and softmax scale 64 ** -0.5.  `prefix` names the launches in
ops.TIMER (`dino_qkv`, `dpt_qkv`, ...)."""
from __future__ import annotations

import ctypes as C

from . import _lib
from .ops import TIMER

HEAD_DIM = 64
LN_EPS = 1e-6
# per block: state-dict key under `blocks.i.` and its shape in terms of the width D
BLOCK_KEYS = (("norm1.weight", "D"), ("norm1.bias", "D"), ("attn.qkv.weight", "3D,D"), ("attn.qkv.bias", "3D"),
              ("attn.proj.weight", "D,D"), ("attn.proj.bias", "D"), ("norm2.weight", "D"), ("norm2.bias", "D"),
              ("mlp.fc1.weight", "4D,D"), ("mlp.fc1.bias", "4D"), ("mlp.fc2.weight", "D,4D"), ("mlp.fc2.bias", "D"))


def linear(name, M, N, K, A, lda, W, b, Cout, ldc, act=0):
    """Cout[M][N] = act(A[M][K] . W[N][K]^T + b): A and Cout are device addresses (row strides lda, ldc), W and b tensors."""
    st = _lib.stream()
    _lib.check(TIMER.run(name, lambda: _lib.lib.upnerf_linear(M, N, K, A, lda, _lib.ptr(W), K, _lib.ptr(b), Cout, ldc, act, st),
                         units=2 * M * N * K), "upnerf_linear")  # (units: FLOP)


def layernorm(name, M, D, x, w, b, y, eps=LN_EPS):
    st = _lib.stream()
    _lib.check(TIMER.run(name, lambda: _lib.lib.upnerf_layernorm(
        M, D, _lib.ptr(x), D, _lib.ptr(w), _lib.ptr(b), eps, _lib.ptr(y), D, st)), "upnerf_layernorm")


def attention(name, N, D, heads, qkv, out):
    a = _lib.VitAttentionArgs(N=N, heads=heads, head_dim=HEAD_DIM, q=qkv.data_ptr(), k=qkv.data_ptr() + 4 * D,
                              v=qkv.data_ptr() + 8 * D, ldq=3 * D, ldk=3 * D, ldv=3 * D, scale=HEAD_DIM ** -0.5,
                              out=_lib.ptr(out), ldo=D)
    st = _lib.stream()
    _lib.check(TIMER.run(name, lambda: _lib.lib.upnerf_vit_attention(C.byref(a), st), units=4 * N * N * D),
               "upnerf_vit_attention")


def gelu(name, x, n):
    st = _lib.stream()
    _lib.check(TIMER.run(name, lambda: _lib.lib.upnerf_vit_gelu(_lib.ptr(x), n, st)), "upnerf_vit_gelu")


def residual(name, x, y, n):
    st = _lib.stream()
    _lib.check(TIMER.run(name, lambda: _lib.lib.upnerf_vit_residual(_lib.ptr(x), _lib.ptr(y), n, st)), "upnerf_vit_residual")


def run_blocks(blocks, N, D, heads, hidden, tok, xn, qkv, att, hid, prefix, after=None):
    """Runs `blocks` (dicts of the BLOCK_KEYS tensors) in place on tok [N][D]; xn, att [N][D], qkv [N][3 D] and hid [N][hidden]
    are work buffers.  after(i) is called behind block i (the DPT hooks)."""
    for i, blk in enumerate(blocks):
        layernorm(prefix + "_layernorm", N, D, tok, blk["norm1.weight"], blk["norm1.bias"], xn)
        linear(prefix + "_qkv", N, 3 * D, D, _lib.ptr(xn), D, blk["attn.qkv.weight"], blk["attn.qkv.bias"], _lib.ptr(qkv), 3 * D)
        attention(prefix + "_attention", N, D, heads, qkv, att)
        linear(prefix + "_proj", N, D, D, _lib.ptr(att), D, blk["attn.proj.weight"], blk["attn.proj.bias"], _lib.ptr(xn), D)
        residual(prefix + "_residual", tok, xn, N * D)
        layernorm(prefix + "_layernorm", N, D, tok, blk["norm2.weight"], blk["norm2.bias"], xn)
        linear(prefix + "_fc1", N, hidden, D, _lib.ptr(xn), D, blk["mlp.fc1.weight"], blk["mlp.fc1.bias"], _lib.ptr(hid), hidden)
        gelu(prefix + "_gelu", hid, N * hidden)
        linear(prefix + "_fc2", N, D, hidden, _lib.ptr(hid), hidden, blk["mlp.fc2.weight"], blk["mlp.fc2.bias"], _lib.ptr(att), D)
        residual(prefix + "_residual", tok, att, N * D)
        if after is not None:
            after(i)
