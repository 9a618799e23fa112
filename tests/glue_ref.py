"""Plain restatements and case tables of the training step's glue kernels (upnerf_amd/csrc/gemm.hip: upnerf_pack in both directions,
upnerf_add_pairs, upnerf_zero, upnerf_adam_gather, upnerf_set_scalars, upnerf_scale_exponents).  CPU only, numpy and torch:
tests/test_glue_ref_cpu.py shows that the tables hit the edges they name and that the restatements agree with torch,
tests/test_hip_glue.py holds the kernels to them.

The copy kernels move 32-bit words, so everything here is int32 bit patterns; only `accumulate` and the pair sums view the words
as fp32.  Every comparison is exact.  Nothing here is computed from a kernel's output.

Canary: a destination is pre-filled with CANARY, a NaN bit pattern that no input holds (inputs() replaces it where a random
word happens to equal it), and GUARD words of it stand before and behind every buffer's used range, so a word written outside the
described elements -- a padding column, a gap between descriptors, the neighbourhood of the buffer -- shows as a lost canary.

upnerf_scale_exponents: the exact exponent is integer arithmetic on the fp32 maximum, v = max(m, 1e-30f), k the integer with
2^(k-1) < v <= 2^k (math.frexp), e* = 14 - k.  The kernel's contract is fp32 log2f, whose value for |log2 v| <= 128 has an ulp of
up to 2^-17; a few ulps of that, times ln 2, stay below 2^-15 relative, so only a v within 2^-14 relative ABOVE a power of two
may come out one binade early: e in {e*, e* + 1} there (the scaled maximum is then at most 2^14 (1 + 2^-14)), e == e* everywhere
else and at every exact power of two.
"""
import math
from collections import namedtuple

import numpy as np
import torch

import dense_ref as dr

CANARY = 0x7FC5A5A5  # a quiet NaN with a payload; as int32 it is positive
GUARD = 64           # canary words in front of and behind every buffer's used range
BLOCK = 256          # threads per workgroup of the descriptor-driven kernels (one element each)
MAX_PACK_DESC, MAX_ADD_PAIRS, MAX_ADAM_DESC, MAX_SCALARS, MAX_EXPONENTS = 48, 8, 96, 96, 64
ADAM_BLOCK = 1024    # elements per workgroup of adam_gather_kernel (256 threads x 4)

# words that a float pipeline could damage: signalling and quiet NaNs with payloads, +-0, denormals, +-inf, the smallest negative
# denormal, and the largest / smallest normal numbers
SPECIAL_WORDS = (0x7F800001, 0x7FA00123, 0xFF8ABCDE, 0x7FC00000, 0xFFC00001, 0x7FFFFFFF, 0xFFFFFFFF, 0x00000000, 0x80000000,
                 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x00800000, 0x3F800000)

Desc = namedtuple("Desc", "rows cols src_ld dst_off dst_ld accumulate")

# (rows, cols, src_ld, dst_ld) per descriptor; one table = one launch
PACK_TABLES = {
    "one": [(1, 1, 1, 1)],
    "edges256": [(1, 255, 255, 255), (1, 256, 256, 256), (1, 257, 257, 257)],          # boundaries at elements 255 and 511
    "strided": [(7, 3, 5, 8), (1, 1, 1, 1), (33, 65, 65, 72), (2, 300, 300, 300), (64, 1, 1, 4)],
    "max48": [(1, n, n, n) for n in range(1, MAX_PACK_DESC + 1)],
}
ADD_SIZES = (1, 255, 256, 257, 70001)
# 4096 * 256 * 4 + 3 fills the 4096-workgroup cap exactly (one trip per thread, and the tail); one quad more makes a second trip
ZERO_SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4096 * 256 * 4 + 3, (4096 * 256 + 1) * 4 + 3)
ZERO_BLOCK_CAP = 4096
ADAM_PIECES = (1, 1023, 1024, 1025, 4097)
SCALAR_COUNTS = (1, 63, 64, 65, 95, 96)
EXPONENT_COUNTS = (1, 63, 64)


def i32(words):
    """Bit patterns (Python ints in [0, 2^32)) as an int32 array."""
    return np.array(words, dtype=np.uint32).view(np.int32)


def words(n, seed):
    """n int32 words: the special patterns first (as many as fit, rotated by the seed), random words behind; never CANARY."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    sp = np.roll(np.array(SPECIAL_WORDS, dtype=np.uint32), seed)
    k = min(n, len(sp))
    w[:k] = sp[:k]
    w[w == CANARY] = 0x12345678
    return w.view(np.int32)


def finite(n, seed):
    """n finite fp32 values as int32 words: magnitudes in [0.5, 1] at scales 2^-3 .. 2^3, a few denormals, zeros of both signs."""
    x = (dr.flat((n,), seed) * 2.0 ** torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(seed))).numpy().copy()
    for j, v in enumerate((0.0, -0.0, 1e-40, -1e-42)):
        if 4 * j < n:
            x[4 * j] = np.float32(v)
    return x.view(np.int32)


def canary(n):
    return np.full(n, CANARY, dtype=np.uint32).view(np.int32)


def layout(table, flags=None, gap=lambda j: 3 + 5 * (j % 4)):
    """Descriptors of a table placed into one destination buffer, descriptor j `gap(j)` words behind the end of descriptor
    j - 1.  Returns (descriptors, words used).  The destinations are disjoint by construction."""
    descs, off = [], 0
    for j, (rows, cols, src_ld, dst_ld) in enumerate(table):
        off += gap(j)
        descs.append(Desc(rows, cols, src_ld, off, dst_ld, 0 if flags is None else int(flags[j])))
        off += (rows - 1) * dst_ld + cols  # (the last row ends at its last column: nothing behind it belongs to the descriptor)
    return descs, off


def src_words(d):
    """Words a descriptor's parameter spans: rows * src_ld (the padding of the last row included)."""
    return d.rows * d.src_ld


def dst_index(d):
    """Indices (into the destination buffer) of the elements a descriptor describes, in the kernels' element order."""
    r, c = np.divmod(np.arange(d.rows * d.cols), d.cols)
    return d.dst_off + r * d.dst_ld + c


def src_index(d):
    r, c = np.divmod(np.arange(d.rows * d.cols), d.cols)
    return r * d.src_ld + c


def starts(descs):
    """Prefix sums of rows * cols: element boundaries of the descriptors inside one launch."""
    return np.concatenate([[0], np.cumsum([d.rows * d.cols for d in descs])])


# -------------------------------------------------------------------------------------------------------------- restatements
def pack(P, descs, srcs, base=0):
    """upnerf_pack, unpack = 0, on int32 words: P[base + dst_off + r dst_ld + c] (=|+=) src[r src_ld + c], descriptor by descriptor
    and row by row.  Returns a new P."""
    P = P.copy()
    for d, s in zip(descs, srcs):
        for r in range(d.rows):
            lo = base + d.dst_off + r * d.dst_ld
            row = s[r * d.src_ld:r * d.src_ld + d.cols]
            if d.accumulate:
                P[lo:lo + d.cols] = (P[lo:lo + d.cols].view(np.float32) + row.view(np.float32)).view(np.int32)
            else:
                P[lo:lo + d.cols] = row
    return P


def unpack(P, descs, dsts, base=0):
    """upnerf_pack, unpack = 1: dst[r src_ld + c] = P[base + dst_off + r dst_ld + c].  Returns new destinations."""
    out = []
    for d, t in zip(descs, dsts):
        t = t.copy()
        for r in range(d.rows):
            lo = base + d.dst_off + r * d.dst_ld
            t[r * d.src_ld:r * d.src_ld + d.cols] = P[lo:lo + d.cols]
        out.append(t)
    return out


def add_pairs(a_list, b_list):
    """upnerf_add_pairs on int32 words viewed as fp32: out_j = a_j + b_j, pair by pair (numpy's fp32 addition; the bits of a NaN
    result are the adder's business, so callers compare those by position)."""
    with np.errstate(all="ignore"):
        return [(a.view(np.float32) + b.view(np.float32)).view(np.int32) for a, b in zip(a_list, b_list)]


def add_inputs(n, seed):
    """Two operands of n fp32 values with the planted rows in front: +-inf (and inf - inf), NaN, a pair summing to -0, denormals
    (sum of two denormals, a denormal result of two normals), a sum that overflows."""
    a, b = finite(n, seed).view(np.float32).copy(), finite(n, seed + 1).view(np.float32).copy()
    inf, nan, tiny = np.float32(np.inf), np.float32(np.nan), np.float32(1e-45)
    plant = [(inf, 1.0), (-inf, -inf), (inf, -inf), (nan, 1.0), (2.0, nan), (-0.0, -0.0), (0.0, -0.0), (1.5, -1.5), (tiny, tiny),
             (1e-40, -3e-41), (np.float32(2.0 ** -126), -np.float32(2.0 ** -126) * np.float32(0.75)), (3e38, 3e38)]
    for j, (x, y) in enumerate(plant[:n]):
        a[j], b[j] = np.float32(x), np.float32(y)
    return a.view(np.int32), b.view(np.int32)


def adam_gather(p, m, v, pieces, b1, b2, eps, step_size, bc2_sqrt, dtype=torch.float32):
    """upnerf_adam_gather: piece (off, g) updates elements [off, off + len(g)) of p / m / v by dense_ref.adam_formula, piece by
    piece; everything else is left as it is.  Returns new (p, m, v) in `dtype`."""
    p, m, v = p.to(dtype).clone(), m.to(dtype).clone(), v.to(dtype).clone()
    for off, g in pieces:
        s = slice(off, off + g.numel())
        p[s], m[s], v[s] = dr.adam_formula(p[s], g, m[s], v[s], b1, b2, eps, step_size, bc2_sqrt, dtype)[:3]
    return p, m, v


def adam_layout(sizes, gap=lambda j: 5 + 3 * (j % 7)):
    """Offsets of pieces of the given sizes inside flat buffers with gaps in front of each; returns (offsets, floats used)."""
    offs, off = [], 0
    for j, n in enumerate(sizes):
        off += gap(j)
        offs.append(off)
        off += n
    return offs, off + 7


# ---------------------------------------------------------------------------------------------------- upnerf_scale_exponents
FLOOR = float(np.float32(1e-30))  # the kernel's clamp, as the fp32 number it is


def _f32(x):
    return float(np.float32(x))


def _next(x, up):
    return float(np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf)))


def exponent_maxima():
    """The maxima of the issue: 2^p for p in [-100, 127] with their fp32 neighbours one ulp above and below, 0, a denormal, 1e-30,
    the values just above and below 1e-30, FLT_MAX."""
    out = []
    for p in range(-100, 128):
        x = 2.0 ** p
        out += [x, _next(x, True), _next(x, False)]
    out += [0.0, 1e-40, FLOOR, _next(FLOOR, True), _next(FLOOR, False), float(np.finfo(np.float32).max)]
    return [_f32(x) for x in out]


def exact_exponent(mx):
    """(e*, exact): e* = 14 - k with 2^(k-1) < v <= 2^k for v = max(mx, 1e-30f), in integer arithmetic on the fp32 number;
    exact = False only in the band 2^(k-1) < v <= 2^(k-1) (1 + 2^-14), where e* + 1 is accepted as well."""
    v = max(_f32(mx), FLOOR)
    f, ex = math.frexp(v)  # v = f 2^ex, 0.5 <= f < 1
    k = ex - 1 if f == 0.5 else ex
    in_band = f != 0.5 and f <= 0.5 * (1.0 + 2.0 ** -14)  # (both sides exact in fp64)
    return 14 - k, not in_band
