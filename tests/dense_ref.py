"""fp64 references, seeded input families and derived per-element error bounds of the dense kernels (upnerf_wgrad, upnerf_wgrad16 on
fp32 rows, upnerf_vec_wgrad, upnerf_linear, upnerf_frag16, upnerf_adam).  CPU only: tests/test_dense_ref_cpu.py proves the bounds
on emulations of the kernels' arithmetic, tests/test_hip_dense.py holds the kernels to them.  No bound is computed from a kernel's
output.

Notation: u = 2^-24 (unit roundoff of fp32), S[n][k] = sum_m |A[m][n]| |B[m][k]| in fp64, L = number of terms of a sum.

fp32 kernels (products exact or fused into the addition, any summation order; Higham, Accuracy and Stability, (3.5)):
    |kernel - fp64| <= L u S                      column sums / bias: L u sum_m |a|.

f16x3 (upnerf_wgrad16 on fp32 rows, planes 0 and 2: both name the 3-term split -- include/upnerf_hip.h "0 / 2 (f16x3) = split on
load", and the launcher sends every planes != 1 to the NP = 2 kernel).  a' = 2^ea a, b' = 2^eb b are exact (powers of two).
ah = fl16(a'), al = fl16(a' - ah); the kernel sums ah bh + ah bl + al bh = (ah + al)(bh + bl) - al bl with exact products (11 x 11
bits) in fp32 and multiplies by 2^-(ea+eb).  With da = a' - (ah + al):
    r = a' - ah is exact in fp32, |r| <= 2^-11 |a'|  (fp16 normal range; |r| <= 2^-25 below it: spacing 2^-24),
    |da| = |r - fl16(r)| <= 2^-11 |r| <= 2^-22 |a'|  where r is a normal fp16, <= 2^-25 where it is subnormal:
    |da| <= 2^-22 |a'| + 2^-25,      |al| <= 2^-11 |a'| (1 + 2^-11) + 2^-25.
    a'b' - (ah bh + ah bl + al bh) = da b' + a' db - da db + al bl
      relative parts:  (2^-22 + 2^-22 + 2^-22 (1 + 2^-11)^2 + 2^-44) |a'b'|  <=  c 2^-22 |a'b'|,   c = 3 + 2^-8   (C_SPLIT)
      absolute parts:  2^-25 (|a'| + |b'|) (1 + 2^-10)  [first order 2^-25 each; from al bl and da db: 2^-36 + 2^-47 each]
                       + 2 * 2^-50                      [both residues in the subnormal range at once: (2^-25)^2 twice]
    gate = (M u + c 2^-22) S + 2^-25 (1 + 2^-10) (2^-ea sum_m |B[m][k]| + 2^-eb sum_m |A[m][n]|) + M 2^-49 2^-(ea+eb)
M u S and not 3 M u S for the fp32 accumulation: a 16-deep MFMA step adds its sixteen exact products to the accumulator with one
rounding, so a chain has 3 M / 16 roundings on the matrix cores; and counted product by product, the two lo products of a row
are 2^-11 of its hi product, so the M hi products carry the sum: M (1 + 2^-10) u S at the very most, inside c's slack.
The last term is 2^-77 of a peak-sized product and only matters where everything else vanishes.  The bound is not 0 for an
all-zero operand (the floor of the OTHER operand remains), so the exact zeros of that family are asserted on their own.
planes = 1 (operands rounded to fp16, one product): |a' - ah| <= 2^-11 |a'| resp. 2^-25, so
    a'b' - ah bh = da b' + a' db - da db:  (2^-10 + 2^-22) |a'b'| + 2^-25 (|a'| + |b'|)(1 + 2^-10) + 2^-50     (C_F16 = 2^12 + 1)
Column sums (db) and the riding vector head are fp32 sums of the unscaled rows: the fp32 bound.

upnerf_adam: 4 e32 + 2^-22 scale per element as in tests/test_hip_perray.py, e32 = |formula in fp32 - formula in fp64| on the
CPU, scale = summed magnitudes of the output's summands (p - step * m / denom cancels).

upnerf_frag16: x' = 2^e x; hi = fl16(x'), lo = fl16(x' - hi) as above, so |x - 2^-e (hi + lo)| <= max(2^-22 |x|, 2^-25 2^-e).
"""
import math

import torch

U = 2.0 ** -24
C_SPLIT = 3.0 + 2.0 ** -8
C_F16 = 2.0 ** 12 + 1.0  # in units of 2^-22
FLOOR16 = 2.0 ** -25 * (1.0 + 2.0 ** -10)
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def flat(shape, seed):
    """Random signs, magnitudes in [0.5, 1]."""
    g = _gen(seed)
    mag = torch.rand(*shape, generator=g) * 0.5 + 0.5
    sgn = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return (mag * sgn).float().clamp(-1.0, 1.0)


def below(x):
    """Largest float below the positive float x."""
    return float(torch.nextafter(torch.tensor(x, dtype=torch.float32), torch.tensor(0.0)))


FAMILIES = ("flat", "cols", "rows12", "zeroA", "pow2_m3", "pow2_0", "pow2_5", "below_m3", "below_0", "below_5", "tiny40", "tiny60",
            "huge40")


def family(name, M, N, K, seed):
    """(A [M][N], B [M][K]) fp32 CPU tensors of one input family (module docstring of tests/test_hip_dense.py)."""
    A, B = flat((M, N), seed), flat((M, K), seed + 1)
    if name == "flat":
        pass
    elif name == "cols":
        # even columns: 2^0 .. 2^-20; odd columns 2^-29 .. 2^-38: scaled by 2^ea (maximum ~2^14) they land in [2^-25, 2^-14), the
        # subnormal range of fp16
        n = torch.arange(N)
        e = torch.where(n % 2 == 0, -((n // 2) % 21), -(29 + (n // 2) % 10))
        A = A * torch.pow(torch.tensor(2.0), e.float())[None, :]
    elif name == "rows12":
        rows = sorted({0, M // 2, M - 1})
        A[rows] *= 4096.0
        B[rows] *= 4096.0
    elif name == "zeroA":
        A = torch.zeros(M, N)
    elif name.startswith("pow2_") or name.startswith("below_"):
        p = {"m3": -3, "0": 0, "5": 5}[name.split("_")[1]]
        A = A * 2.0 ** p
        top = 2.0 ** p if name.startswith("pow2_") else below(2.0 ** p)
        A = A.clamp(-below(top), below(top))
        A[M // 2, N // 3] = -top
    elif name == "tiny40":
        A, B = A * 2.0 ** -40, B * 2.0 ** -40
    elif name == "tiny60":
        A, B = A * 2.0 ** -60, B * 2.0 ** -60
    elif name == "huge40":
        A = A * 2.0 ** 40
    else:
        raise KeyError(name)
    return A.float().contiguous(), B.float().contiguous()


def host_exponent(x):
    """14 - ceil(log2(max(max|x|, 1e-30))): the formula of ops.scale_exponents / upnerf_scale_exponents, in fp64 on the host."""
    mx = max(float(x.abs().max()) if x.numel() else 0.0, float(torch.tensor(1e-30, dtype=torch.float32)))
    return 14 - math.ceil(math.log2(mx))


# ------------------------------------------------------------------------------------------------------------ references
def wgrad_ref(A, B):
    """fp64: dW [N][K], db [N], S = |A|^T |B|, column 1-norms of A and of B."""
    a, b = A.double(), B.double()
    return dict(dW=a.t() @ b, db=a.sum(0), S=a.abs().t() @ b.abs(), sa=a.abs().sum(0), sb=b.abs().sum(0))


def gate_fp32(L, S):
    return L * U * S


def gate_f16(ref, M, ea, eb, planes):
    """Per-element bound of upnerf_wgrad16 on fp32 rows (module docstring); planes 0 / 2: three-term split, 1: rounded operands."""
    c = C_F16 if planes == 1 else C_SPLIT
    tail = (1 if planes == 1 else 2) * 2.0 ** -50
    return ((M * U + c * 2.0 ** -22) * ref["S"] + FLOOR16 * (2.0 ** -ea * ref["sb"][None, :] + 2.0 ** -eb * ref["sa"][:, None])
            + M * tail * 2.0 ** -(ea + eb))


def ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound; a bound of 0 asks for an error of exactly 0 (inf otherwise); a NaN anywhere
    gives NaN, which fails `<= 1`."""
    got, ref, bound = got.detach().cpu().double(), ref.detach().cpu().double(), torch.as_tensor(bound).detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = bound.expand_as(ref)
    err = (got - ref).abs()
    if torch.isnan(got).any() or torch.isnan(err).any() or torch.isnan(bound).any():
        return NAN
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------- emulations of the kernels' arithmetic
def split16(x):
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def emulate_f16(A, B, ea, eb, planes, drop=None, zero_col=None):
    """upnerf_wgrad16's arithmetic on fp32 rows in torch: operands scaled by 2^ea / 2^eb in fp32, split with x.half() and
    (x - hi).half(), the products summed in fp64, unscaled, rounded to fp32.  drop = (m, n, k): that one term left out;
    zero_col = k: column k of B staged as zeros (a ragged column lost)."""
    a, b = A * 2.0 ** ea, B * 2.0 ** eb
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    ah, al = split16(a)
    bh, bl = split16(b)
    ah, al, bh, bl = ah.double(), al.double(), bh.double(), bl.double()
    if planes == 1:
        al, bl = torch.zeros_like(al), torch.zeros_like(bl)
    if zero_col is not None:
        bh, bl = bh.clone(), bl.clone()
        bh[:, zero_col] = 0
        bl[:, zero_col] = 0
    acc = ah.t() @ bh + ah.t() @ bl + al.t() @ bh
    if drop is not None:
        m, n, k = drop
        acc[n, k] -= ah[m, n] * bh[m, k] + ah[m, n] * bl[m, k] + al[m, n] * bh[m, k]
    return (acc * 2.0 ** -(ea + eb)).float()


def emulate_fp32(A, B, drop=None):
    """The fp32 kernels' arithmetic: a row-by-row fp32 accumulation (one rounding per row, as a chain of fused multiply-adds)."""
    acc = torch.zeros(A.shape[1], B.shape[1], dtype=torch.float32)
    for m in range(A.shape[0]):
        t = A[m].double()[:, None] * B[m].double()[None, :]
        if drop is not None and drop[0] == m:
            t[drop[1], drop[2]] = 0
        acc = (acc.double() + t).float()
    return acc


# ------------------------------------------------------------------------------------------------------------------ linear
def linear_ref(x, w, bias):
    """fp64 pre-activation x . w^T + bias (w [N][K]) and S = |x| |w|^T + |bias|."""
    pre = x.double() @ w.double().t()
    S = x.double().abs() @ w.double().abs().t()
    if bias is not None:
        pre = pre + bias.double()[None, :]
        S = S + bias.double().abs()[None, :]
    return pre, S


# -------------------------------------------------------------------------------------------------------------------- Adam
def adam_formula(p, g, m, v, b1, b2, eps, step_size, bc2_sqrt, dtype):
    """The update in the kernel's comment (csrc/gemm.hip: adam_update), operation by operation, in `dtype`; the scalars are the
    fp32 numbers the kernel receives.  Returns p, m, v and the summed magnitudes of each output's summands (the gate's scale)."""
    f = lambda x: torch.tensor(float(torch.tensor(x, dtype=torch.float32)), dtype=dtype)
    b1, b2, eps, step_size, bc2_sqrt = f(b1), f(b2), f(eps), f(step_size), f(bc2_sqrt)
    one = torch.tensor(1.0, dtype=dtype)
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    dm = (g - m) * (one - b1)
    mi = m + dm
    t1, t2 = v * b2, ((one - b2) * g) * g
    vi = t1 + t2
    denom = torch.sqrt(vi) / bc2_sqrt + eps
    upd = step_size * (mi / denom)
    return p - upd, mi, vi, (p.abs() + upd.abs(), m.abs() + dm.abs(), t1.abs() + t2.abs())


def adam_bias_scalars(lr, b1, b2, step):
    """(step_size, bc2_sqrt) as the host forms them: in double precision (include/upnerf_hip.h)."""
    return lr / (1.0 - b1 ** step), math.sqrt(1.0 - b2 ** step)


def torch_adam(p, g, m, v, lr, b1, b2, eps, step):
    """One step of torch.optim.Adam on the CPU from the given state."""
    q = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[q] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
    q.grad = g.clone()
    opt.step()
    st = opt.state[q]
    return q.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()


ADAM_G = (0.0, 1e-20, -1e-20, 1e-8, -1e-8, 1.0, -1.0, 1e4, -1e4, 1e19, 1e20, 1e25)  # 1e25: (1 - beta2) g g overflows fp32
ADAM_V = (0.0, 1e-30, 1.0)


def adam_table(seed):
    """Planted (p, g, m, v): every g x v x sign of m."""
    rows = [(g, v, s) for g in ADAM_G for v in ADAM_V for s in (-1.0, 1.0)]
    gen = _gen(seed)
    n = len(rows)
    p = flat((n,), seed)
    g = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    v = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    m = torch.tensor([r[2] for r in rows], dtype=torch.float32) * (torch.rand(n, generator=gen) * 0.5 + 0.5) * 1e-3
    return p, g, m, v


# ------------------------------------------------------------------------------------------------------------------ frag16
def frag16_exponent(mx):
    """14 - frexp exponent of the maximum, 0 for an all-zero matrix (csrc/gemm.hip: frag16_exp, without its +-100 clamp)."""
    return 0 if not mx > 0 else 14 - math.frexp(mx)[1]


def frag16_byte(r, k, kp, plane, perm):
    """Byte offset of element (r, k) of a [rows][kp] matrix inside its fragment image (include/upnerf_hip.h, upnerf_frag16)."""
    kk = k % 16
    if perm:
        half, j = (kk // 4) % 2, (kk // 8) * 4 + kk % 4
    else:
        half, j = kk // 8, kk % 8
    return (((r // 32) * (kp // 16) + k // 16) * 2 + plane) * 1024 + (half * 32 + r % 32) * 16 + j * 2
