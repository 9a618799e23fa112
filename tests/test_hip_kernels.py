"""GPU parity tests, kernel by kernel: every C-ABI entry point of libupnerf_hip.so against the CPU oracle
(oracle/upnerf_oracle.py) or, for the fused kernels' internals, against the torch restatement of the kernels'
arithmetic (tests/kernel_space.py, itself pinned to the oracle by tests/test_packing_cpu.py).

Tolerances (max-normalised error, golden_util.rel_err): fp32 MFMA vs fp32 CPU BLAS differ only in summation order:
1e-5 on activations and per-ray maps, 1e-4 on gradients (the bar BASELINE.json states is 1e-4)."""
import ctypes as C

import numpy as np
import os

import pytest
import torch

import field_cases
import kernel_space as ks
from field_cases import TOL_ACT, TOL_GRAD, check_field_pass
from golden_util import GOLDEN, Case, orc, rel_err
from prologue_ref import philox_uniform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib, camera, ops, pass_plan, rendering
    return dict(lib=_lib, camera=camera, ops=ops, rendering=rendering, pass_plan=pass_plan)


def cpu(t):
    return t.detach().cpu()


def gen(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def wg_desc(hip, M, A, N, B, K, ea, eb, dW, ldo, db, ws, ns, **kw):
    """upnerf_wgrad_desc of dW [N][ldo] = A^T B; A / B: the fields of ops.WgOp (tensor, ld[, kind, exp, lo]); ea / eb: addresses;
    kw: n2 / dW2 / ldo2 / db2, v / dv / dbv, planes (tensors where the descriptor holds a pointer)."""
    L, ops = hip["lib"], hip["ops"]
    kw = {k: (t.data_ptr() if isinstance(t, torch.Tensor) else t) for k, t in kw.items()}
    return L.WgradDesc(M=M, N=N, K=K, planes=kw.pop("planes", 2), A=ops.WgOp(*A).c(), B=ops.WgOp(*B).c(), expo_a=ea, expo_b=eb,
                       dW=dW.data_ptr(), ldo=ldo, db=db.data_ptr(), slabs=L.ptr(ws), nsplit=ns, **kw)


# ------------------------------------------------------------------------------------------ a2-a4
@pytest.mark.parametrize("identity", [True, False])
def test_pose_rays_fwd_bwd(hip, identity):
    R = 67
    se3 = gen((R, 6), 1) * 0.3
    se3[0] = 0.0          # zero-initialised table entry (nerf_system.py:407)
    se3[1, :3] = 0.0
    se3[2] *= 5.0         # large rotation, exercises the high Taylor terms
    if identity:
        c2w = torch.eye(3, 4).repeat(R, 1, 1)
    else:
        q, _ = torch.linalg.qr(gen((R, 3, 3), 2))
        c2w = torch.cat([q, gen((R, 3, 1), 3)], -1)
    dirs = gen((R, 3), 4)
    dirs[:, 2] = -1.0
    go, gd = gen((R, 3), 5), gen((R, 3), 6)
    s_ref = se3.clone().requires_grad_(True)
    o_ref, d_ref = orc.get_rays(dirs, orc.compose_pair(orc.se3_exp(s_ref), c2w))
    ((o_ref * go).sum() + (d_ref * gd).sum()).backward()
    s_gpu = se3.cuda().requires_grad_(True)
    o, d = hip["camera"].refine_and_get_rays(s_gpu, c2w.cuda(), dirs.cuda())
    ((o * go.cuda()).sum() + (d * gd.cuda()).sum()).backward()
    assert rel_err(cpu(o), o_ref.detach()) < 1e-6 and rel_err(cpu(d), d_ref.detach()) < 1e-6
    assert torch.isfinite(s_gpu.grad).all()
    assert rel_err(cpu(s_gpu.grad), s_ref.grad) < 2e-5
    # no refinement = plain get_rays, both calling conventions of utils/ray.py:30-67
    o2, d2 = hip["camera"].get_rays(dirs.cuda(), c2w.cuda())
    o2r, d2r = orc.get_rays(dirs, c2w)
    assert rel_err(cpu(o2), o2r) < 1e-6 and rel_err(cpu(d2), d2r) < 1e-6
    o3, d3 = hip["camera"].get_rays(dirs.cuda(), c2w[0].cuda())
    o3r, d3r = orc.get_rays(dirs, c2w[0])
    assert rel_err(cpu(o3), o3r) < 1e-6 and rel_err(cpu(d3), d3r) < 1e-6


# ------------------------------------------------------------------------------------------ a5
@pytest.mark.parametrize("S,perturb,disp", [(64, 0.0, False), (64, 1.0, False), (48, 0.5, True), (128, 1.0, False)])
def test_sample_coarse(hip, S, perturb, disp):
    L = hip["lib"]
    R = 33
    nf = torch.stack([gen((R,), 7, 0.05, 0.3), gen((R,), 8, 3.0, 6.0)], 1)
    u = gen((R, S), 9, 0.0, 1.0)
    ref = orc.coarse_depths(nf[:, :1], nf[:, 1:], S, disp, perturb, u if perturb > 0 else None)
    z = torch.empty(R, S, device="cuda")
    steps = torch.linspace(0, 1, S).cuda()
    ud, nfd = u.cuda(), nf.cuda()
    L.check(L.lib.upnerf_sample_coarse(R, S, L.ptr(nfd), L.ptr(steps), L.ptr(ud) if perturb > 0 else None,
                                       perturb, int(disp), L.ptr(z), L.stream()), "sample_coarse")
    assert np.array_equal(cpu(z).numpy(), ref.numpy())  # same op order, no contraction: bit exact


# ------------------------------------------------------------------------------------------ a11, a12
def _run_pdf(hip, z, w_full, n, det, u):
    R, S = z.shape
    out = torch.zeros(R, n + 3, device="cuda")
    hip["rendering"].sample_pdf(z.cuda(), w_full.cuda(), n, det, out, 3, None if det else u.cuda())
    return cpu(out)[:, 3:]


def test_sample_pdf_matches_oracle(hip):
    R, S, n = 29, 64, 128
    z = torch.sort(gen((R, S), 10, 0.1, 5.0), -1)[0]
    w = gen((R, S), 11, 0.0, 1.0) ** 6
    w[3] = 0.0                       # all-zero weights: uniform pdf from the eps
    w[4, 10:50] = 0.0                # empty bins inside
    mid = 0.5 * (z[:, :-1] + z[:, 1:])
    u = gen((R, n), 12, 0.0, 1.0)
    u[5, 0], u[5, 1] = 0.0, 1.0 - 1e-7
    # A 1-ulp difference in the pdf normalisation moves a sample by (bin width / bin mass) * 1e-7, and bins lighter
    # than eps are, by the reference's `denom < eps -> 1` rule, collapsed onto their lower edge, so the inverse cdf
    # jumps there.  Gate: |dz| <= 1e-6 * local slope, for every sample whose u is not within 1e-6 of a cdf knot.
    pdf = (w[:, 1:-1] + 1e-5) / (w[:, 1:-1] + 1e-5).sum(1, keepdim=True)
    cdf = torch.cat([torch.zeros(R, 1), torch.cumsum(pdf, -1)], -1)
    B = pdf.shape[1]
    for det in (False, True):
        uu = torch.linspace(0, 1, n).expand(R, n).contiguous() if det else u
        hi = torch.searchsorted(cdf, uu, right=True)
        lo, hi = (hi - 1).clamp_min(0), hi.clamp_max(B)
        den = cdf.gather(1, hi) - cdf.gather(1, lo)
        den = torch.where(den < 1e-5, torch.ones_like(den), den)
        slope = (mid.gather(1, hi) - mid.gather(1, lo)) / den
        away = ((uu[:, :, None] - cdf[:, None, :]).abs().min(-1)[0] > 1e-6)
        ref = orc.sample_pdf(mid, w[:, 1:-1], n, det, None if det else u)
        got = _run_pdf(hip, z, w, n, det, None if det else u)
        assert bool((((got - ref).abs() <= 1e-6 * slope + 2e-6) | ~away).all())
        assert float(((got - ref).abs() < 2e-6).float().mean()) > 0.97
    # well-conditioned rows (every bin heavier than eps): plain absolute gate
    w2 = gen((R, S), 14, 0.2, 1.0)
    ref = orc.sample_pdf(mid, w2[:, 1:-1], n, False, u)
    got = _run_pdf(hip, z, w2, n, False, u)
    assert float((got - ref).abs().max()) < 5e-6


def test_sample_pdf_reference_edge_fixture(hip):
    """searchsorted(right=True) knots, u == 1, zero-weight bins: vectors produced by the reference itself."""
    g = np.load(f"{GOLDEN}/leaf.npz")
    bins, w, u = (torch.from_numpy(g[k]) for k in ("pdf_edge_bins", "pdf_edge_w", "pdf_edge_u"))
    # rebuild a z whose mid-points are the fixture's bins: z_{j+1} = 2 b_j - z_j
    z = torch.zeros(bins.shape[0], bins.shape[1] + 1)
    z[:, 0] = bins[:, 0] - 0.5
    for j in range(bins.shape[1]):
        z[:, j + 1] = 2 * bins[:, j] - z[:, j]
    wf = torch.cat([torch.zeros(2, 1), w, torch.zeros(2, 1)], 1)
    got = _run_pdf(hip, z, wf, u.shape[1], False, u)
    assert float((got - torch.from_numpy(g["pdf_edge_out"])).abs().max()) < 2e-6


@pytest.mark.parametrize("S", [64, 192, 256, 7])
def test_sort_rows(hip, S):
    L = hip["lib"]
    R = 41
    z = gen((R, S), 13)
    z[0, : S // 2] = z[0, S // 2: 2 * (S // 2)]  # duplicates
    zd = z.cuda().contiguous()
    L.check(L.lib.upnerf_sort_rows(R, S, L.ptr(zd), L.stream()), "sort_rows")
    assert np.array_equal(cpu(zd).numpy(), torch.sort(z, -1)[0].numpy())


@pytest.mark.parametrize("Nc,na,nb,mode", [(64, 128, 0, "keyed"), (64, 90, 38, "keyed"), (64, 0, 128, "keyed"), (128, 128, 0, "buf"),
                                           (64, 38, 90, "buf"), (64, 128, 0, "det"), (64, 64, 64, "det"), (5, 3, 0, "keyed")])
def test_fused_resample_and_sort_equals_the_launch_per_piece_sequence(hip, Nc, na, nb, mode):
    """upnerf_resample_sort (round 6: coarse depths | inverse-CDF set A | set B -> sorted fine depths in one launch, keyed uniforms
    generated in the kernel) against the sequence it replaces -- strided copy, upnerf_uniform_keyed + upnerf_sample_pdf per set,
    upnerf_sort_rows -- bit for bit; sets of width zero keep their draw number (the reference draws rand(R, 0) too)."""
    L = hip["lib"]
    lib, ptr, st = L.lib, L.ptr, L.stream
    R, S = 333, Nc + na + nb
    g = torch.Generator().manual_seed(Nc * 1000 + na)
    z = torch.sort(torch.rand(R, Nc, generator=g) * 4 + 0.1, -1)[0].cuda().contiguous()
    wa = (torch.rand(R, Nc, generator=g) ** 4).cuda().contiguous()
    wb = (torch.rand(R, Nc, generator=g) ** 8).cuda().contiguous()
    wa[3] = 0.0  # an all-eps cdf row
    seed, step, row0, stride = 0x1234567887654321, 17, 5, 3
    # set A sits BEHIND set B in the row, as render_rays places the candidate-weight samples (rendering.py:283-290)
    col_a, col_b = Nc + nb, Nc
    draws = {}
    ref = torch.empty(R, S, device="cuda")
    ref[:, :Nc] = z
    for d, (w, n, col) in enumerate(((wa, na, col_a), (wb, nb, col_b)), start=1):
        if n == 0:
            continue
        if mode == "det":
            u, rows = torch.linspace(0, 1, n, device="cuda"), 1
        elif mode == "buf":
            u, rows = torch.rand(R, n, generator=g).cuda().contiguous(), R
        else:
            u, rows = torch.empty(R, n, device="cuda"), R
            L.check(lib.upnerf_uniform_keyed(R, n, seed, step, None, row0, stride, d, ptr(u), st()), "uniform_keyed")
        draws[d] = u
        L.check(lib.upnerf_sample_pdf(R, Nc, ptr(z), ptr(w), ptr(u), rows, n, ref.data_ptr() + 4 * col, S, st()), "sample_pdf")
    L.check(lib.upnerf_sort_rows(R, S, ptr(ref), st()), "sort_rows")
    got = torch.full((R, S), float("nan"), device="cuda")
    rng = L.Rng(seed=seed, step=step, row0=row0, row_stride=stride, step_dev=None)
    ua, ub = (draws.get(1), draws.get(2)) if mode != "keyed" else (None, None)
    L.check(lib.upnerf_resample_sort(R, Nc, ptr(z), ptr(wa), na, col_a, ptr(ua), 1, ptr(wb), nb, col_b, ptr(ub), 2,
                                     1 if mode == "det" else R, C.byref(rng) if mode == "keyed" else None, ptr(got), st()), "resample_sort")
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    # ... and the step counter from device memory (graph replay) draws the same numbers
    if mode == "keyed":
        sd = torch.tensor([float(step)], device="cuda")
        rng2 = L.Rng(seed=seed, step=0, row0=row0, row_stride=stride, step_dev=sd.data_ptr())
        got2 = torch.empty_like(got)
        L.check(lib.upnerf_resample_sort(R, Nc, ptr(z), ptr(wa), na, col_a, None, 1, ptr(wb), nb, col_b, None, 2, R, C.byref(rng2),
                                         ptr(got2), st()), "resample_sort")
        assert torch.equal(got2, ref)


@pytest.mark.parametrize("disp", [0, 1])
def test_coarse_depths_with_the_jitter_generated_in_the_kernel(hip, disp):
    """upnerf_sample_coarse_keyed == upnerf_sample_coarse fed by upnerf_uniform_keyed(draw 0), bit for bit."""
    L = hip["lib"]
    lib, ptr, st = L.lib, L.ptr, L.stream
    R, S = 517, 64
    g = torch.Generator().manual_seed(3)
    nf = torch.stack([0.1 + torch.rand(R, generator=g), 4 + torch.rand(R, generator=g)], 1).cuda().contiguous()
    steps = torch.linspace(0, 1, S, device="cuda")
    seed, step, row0, stride = 77, 123456, 2, 8
    u = torch.empty(R, S, device="cuda")
    L.check(lib.upnerf_uniform_keyed(R, S, seed, step, None, row0, stride, 0, ptr(u), st()), "uniform_keyed")
    ref, got = torch.empty(R, S, device="cuda"), torch.empty(R, S, device="cuda")
    L.check(lib.upnerf_sample_coarse(R, S, ptr(nf), ptr(steps), ptr(u), 1.0, disp, ptr(ref), st()), "sample_coarse")
    rng = L.Rng(seed=seed, step=step, row0=row0, row_stride=stride, step_dev=None)
    L.check(lib.upnerf_sample_coarse_keyed(R, S, ptr(nf), ptr(steps), C.byref(rng), 1.0, disp, ptr(got), st()), "sample_coarse_keyed")
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("M", [64 * 37, 64 * 512])
def test_weight_gradient_from_producer_split_planes_staged_by_lds_dma(hip, M):
    """upnerf_wgrad16 on UPNERF_WG_PLANES operands (round 6; measured, not wired into the step: DESIGN.md 4.9): both operands as the (hi, lo) fp16 planes
    + per-64-row exponents the f16x3 field kernels hold in LDS, staged by LDS-DMA.  Against fp64 on the values the planes decode to,
    and against the UPNERF_WG_F32 kind on the fp32 rows (= hi + lo exactly): the same products, so 1e-6 of the maximum."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_wgrad_planes import split_planes, tensor_exp
    L, ops = hip["lib"], hip["ops"]
    lib, ptr, st = L.lib, L.ptr, L.stream
    dev = "cuda"
    g = torch.Generator().manual_seed(M)
    A = (torch.randn(M, 256, generator=g) * torch.rand(M, 1, generator=g) ** 3 * (torch.rand(M, 256, generator=g) > 0.5)).to(dev)
    B = torch.relu(torch.randn(M, 256, generator=g)).to(dev)
    A[64:128] *= 1e-6  # a tile far below the tensor's maximum: its exponent gap exceeds what fp16 holds after the rescale
    Ah, Al, aexp, Ad = split_planes(A, False)
    Bh, Bl, bexp, Bd = split_planes(B, True)
    ea = torch.tensor([tensor_exp(Ad)], dtype=torch.int32, device=dev)
    eb = torch.tensor([tensor_exp(Bd)], dtype=torch.int32, device=dev)
    ns = ops.nsplit_for(M)
    res = []
    for planes in (True, False):
        dW, db = torch.full((256, 260), 7.0, device=dev), torch.full((256,), 7.0, device=dev)
        ws = torch.empty(ns * (256 * 256 + 256 + 260), device=dev)
        pend = L.WgradPending()
        a_op, b_op = ((Ah, 256, L.WG_PLANES, aexp, Al), (Bh, 256, L.WG_PLANES, bexp, Bl)) if planes else ((Ad, 256), (Bd, 256))
        desc = wg_desc(hip, M, a_op, 256, b_op, 256, ptr(ea), ptr(eb), dW, 260, db, ws, ns)
        L.check(lib.upnerf_wgrad16(C.byref(desc), C.byref(pend), st()), "wgrad")
        L.check(lib.upnerf_wgrad_finish(C.byref(pend), st()), "finish")
        torch.cuda.synchronize()
        assert float(dW[:, 256:].min()) == 7.0 and float(dW[:, 256:].max()) == 7.0  # the padding columns of the destination stay untouched
        res.append((dW[:, :256].clone(), db.clone()))
    ref, refb = Ad.double().t() @ Bd.double(), Ad.double().sum(0)
    for dW, db in res:
        assert float((dW.double() - ref).abs().max() / ref.abs().max()) < 2e-6
        assert float((db.double() - refb).abs().max() / refb.abs().max()) < 2e-6
    assert float((res[0][0] - res[1][0]).abs().max() / res[1][0].abs().max()) < 1e-6
    # not a multiple of 64 rows: refused, the caller keeps the fp32 rows
    a_op, b_op = (Ah, 256, L.WG_PLANES, aexp, Al), (Bh, 256, L.WG_PLANES, bexp, Bl)
    bad = wg_desc(hip, M + 16, a_op, 256, b_op, 256, ptr(ea), ptr(eb), dW, 260, db, ws, ns)
    assert lib.upnerf_wgrad16(C.byref(bad), C.byref(L.WgradPending()), st()) == -2  # UPNERF_EUNSUP


def test_fanout_sums_the_gradients_of_all_pairs_in_one_launch(hip):
    """ops.fanout: two aliases per tensor; the backward adds every pair with ONE upnerf_add_pairs launch -- the bits of autograd's own
    a + b -- and passes a lone gradient through."""
    ops = hip["ops"]
    xs = [gen(s_, 40 + i).cuda().requires_grad_(True) for i, s_ in enumerate([(300, 3), (300, 3), (384, 257), (384,)])]
    frozen = gen((5,), 50).cuda()
    launches = []
    real = ops.lib.upnerf_add_pairs

    def counted(*a):
        launches.append(a[1])
        return real(*a)

    ops.lib.upnerf_add_pairs = counted
    try:
        A, B = ops.fanout(*xs, frozen)
        assert A[4] is frozen and B[4] is frozen
        ws = [gen(tuple(x.shape), 60 + i).cuda() for i, x in enumerate(xs)]
        vs = [gen(tuple(x.shape), 70 + i).cuda() for i, x in enumerate(xs)]
        loss = sum((a * w).sum() for a, w in zip(A[:3], ws)) + sum((b * b * v).sum() for b, v in zip(B[:4], vs))  # xs[3]: one consumer only
        loss.backward()
    finally:
        ops.lib.upnerf_add_pairs = real
    assert launches == [3]
    for i, x in enumerate(xs):
        ref = (ws[i] if i < 3 else 0) + 2 * x.detach() * vs[i]
        assert torch.equal(x.grad, ref if i < 3 else 2 * x.detach() * vs[i]), i


def test_matvec_with_the_rank_one_update_riding_along(hip):
    """upnerf_matvec_rank1: y = A^T x exactly as upnerf_matvec(trans = 1) and R += x (x) v -- the bias fold's backward in one launch."""
    L = hip["lib"]
    lib, ptr, st = L.lib, L.ptr, L.stream
    M, K, ldr = 128, 384, 459
    A, x, v = gen((M, K), 1).cuda(), gen((M,), 2).cuda(), gen((K,), 3).cuda()
    R0 = gen((M, ldr), 4).cuda()
    y_ref, y = torch.empty(K, device="cuda"), torch.empty(K, device="cuda")
    L.check(lib.upnerf_matvec(M, K, ptr(A), K, ptr(x), None, ptr(y_ref), 1, st()), "matvec")
    Rg = R0.clone()
    L.check(lib.upnerf_matvec_rank1(M, K, ptr(A), K, ptr(x), ptr(y), ptr(Rg), ldr, ptr(v), st()), "matvec_rank1")
    torch.cuda.synchronize()
    assert torch.equal(y, y_ref)
    want = R0.clone()
    want[:, :K] += x[:, None] * v[None, :]
    assert torch.equal(Rg[:, K:], R0[:, K:])
    assert rel_err(cpu(Rg[:, :K]), cpu(want[:, :K])) < 1e-6


@pytest.mark.parametrize("R,N,dim", [(4096, 763, 48), (100, 7, 6), (5000, 1200, 128), (64, 3, 2), (300, 10, 200)])
def test_embedding_gradient_kernel(hip, R, N, dim):
    """Dense embedding gradient (one HIP kernel) against ATen's nn.Embedding backward; also bitwise run-to-run."""
    table = gen((N, dim), 26)
    idx = torch.randint(0, N, (R,), generator=torch.Generator().manual_seed(R))
    if N > 5:
        idx[idx == 2] = 3  # one table row never referenced: its gradient must come out as exact zeros
    up = gen((R, dim), 27)
    ref = torch.nn.Embedding(N, dim)
    ref.weight.data.copy_(table)
    (ref(idx).double() * up.double()).sum().backward()
    emb = torch.nn.Embedding(N, dim).cuda()
    emb.weight.data.copy_(table.cuda())
    grads = []
    for _ in range(2):
        emb.weight.grad = None
        rows = hip["ops"].embed_rows(emb, idx.cuda())
        assert torch.equal(cpu(rows), table[idx])
        (rows * up.cuda()).sum().backward()
        grads.append(cpu(emb.weight.grad).clone())
    assert torch.equal(grads[0], grads[1])
    assert rel_err(grads[0], ref.weight.grad) < 1e-6
    if N > 5:
        assert float(grads[0][2].abs().max()) == 0.0


def test_deferred_embedding_gradients_share_one_launch_and_equal_the_immediate_ones(hip):
    """Seven tables gathered with the same indices (a training step's per-image tables) + one with other indices:
    gradients through the end-of-pass grouped kernel are bit-identical to the per-table kernel's."""
    ops = hip["ops"]
    R, N = 3000, 97
    dims = (48, 48, 16, 16, 128, 6, 2, 256, 33)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, N, (R,), generator=g).cuda()
    idx2 = torch.randint(0, N, (R // 2,), generator=g).cuda()
    embs = [torch.nn.Embedding(N, d).cuda() for d in dims]
    ups = [gen((R if i else R // 2, d), 400 + i).cuda() for i, d in enumerate(dims)]
    res = {}
    for defer in (False, True):
        for e in embs:
            e.weight.grad = None
        loss = sum((ops.embed_rows(e, idx if i else idx2, defer_grad=defer) * u).sum() for i, (e, u) in enumerate(zip(embs, ups)))
        loss.backward()
        assert not ops.DEFERRED_EMBEDS.items
        res[defer] = [e.weight.grad.clone() for e in embs]
    for a, b in zip(res[False], res[True]):
        assert torch.equal(a, b)


def test_one_gather_launch_serves_every_table_of_a_step(hip):
    """ops.EMBED_PREFETCH: inside a scope the first embed_rows() gathers every registered table of the same height with ONE
    upnerf_embed_fwd_grouped launch (<= 8 tables each); values, gradients and a second request of a table equal nn.Embedding's."""
    ops = hip["ops"]
    g = torch.Generator().manual_seed(11)
    R, N = 777, 41
    dims = [6, 2, 48, 16, 128, 200, 256, 64, 3, 5]  # ten tables: two launches
    mods = [torch.nn.Embedding(N, d).cuda() for d in dims]
    other = torch.nn.Embedding(N + 1, 7).cuda()  # another height: not in the group
    idx = torch.randint(0, N, (R,), generator=g).cuda()
    weights = [torch.randn(R, d, generator=g).cuda() for d in dims]
    launches = []
    real = ops.lib.upnerf_embed_fwd_grouped

    def counted(*a):
        launches.append(a[4])
        return real(*a)

    ops.lib.upnerf_embed_fwd_grouped = counted
    try:
        with ops.EMBED_PREFETCH.scope(mods + [other, None]):
            rows = [ops.embed_rows(m, idx) for m in mods]
            again = ops.embed_rows(mods[2], idx)
            o = ops.embed_rows(other, idx)
            loss = sum((r * w).sum() for r, w in zip(rows, weights)) + (again * weights[2]).sum() * 0.5 + o.sum()
            loss.backward()
        assert ops.EMBED_PREFETCH.tables is None and not ops.EMBED_PREFETCH.cache
    finally:
        ops.lib.upnerf_embed_fwd_grouped = real
    assert launches == [8, 2]
    for m, r in zip(mods, rows):
        assert torch.equal(r, m.weight.detach()[idx])
    assert torch.equal(again, rows[2]) and again is not rows[2]
    assert torch.equal(o, other.weight.detach()[idx])
    for j, (m, w) in enumerate(zip(mods, weights)):
        ref = torch.zeros_like(m.weight).index_add_(0, idx, w * (1.5 if j == 2 else 1.0))
        assert torch.allclose(m.weight.grad, ref, rtol=1e-5, atol=1e-5), j
    # an index outside the table poisons its row instead of reading out of bounds ...
    bad = idx.clone()
    bad[5] = N
    old = os.environ.get("UPNERF_CHECK_EMBED_IDX")
    try:
        os.environ["UPNERF_CHECK_EMBED_IDX"] = "0"
        with ops.EMBED_PREFETCH.scope(mods[:2]):
            r0 = ops.embed_rows(mods[0], bad)
        assert torch.isnan(r0[5]).all() and not torch.isnan(r0[:5]).any()
        # ... and the host-side range check (the first prefetch of a process; every one with UPNERF_CHECK_EMBED_IDX=1) raises where
        # nn.Embedding / index_select raised a device-side assert (r5 ADVICE)
        os.environ["UPNERF_CHECK_EMBED_IDX"] = "1"
        with ops.EMBED_PREFETCH.scope(mods[:2]):
            with pytest.raises(IndexError):
                ops.embed_rows(mods[0], bad)
    finally:
        if old is None:
            os.environ.pop("UPNERF_CHECK_EMBED_IDX", None)
        else:
            os.environ["UPNERF_CHECK_EMBED_IDX"] = old


def test_a_prefetched_arena_is_served_only_on_the_stream_that_filled_it(hip):
    """r5 ADVICE: the gather arena belongs to the stream of the first embed_rows(); a request on another stream gathers its own rows
    there (index_select on the consuming stream) instead of reading slices that stream was never ordered behind."""
    ops = hip["ops"]
    g = torch.Generator().manual_seed(12)
    N, R = 23, 500
    mods = [torch.nn.Embedding(N, d).cuda() for d in (48, 128)]
    idx = torch.randint(0, N, (R,), generator=g).cuda()
    side = torch.cuda.Stream()
    launches = []
    real = ops.lib.upnerf_embed_fwd_grouped

    def counted(*a):
        launches.append(a[4])
        return real(*a)

    ops.lib.upnerf_embed_fwd_grouped = counted
    try:
        with ops.EMBED_PREFETCH.scope(mods):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                first = ops.embed_rows(mods[1], idx)  # fills the arena ON THE SIDE STREAM
                assert ops.EMBED_PREFETCH.rows(mods[0].weight, idx) is not None  # same stream: served
            assert ops.EMBED_PREFETCH.rows(mods[0].weight, idx) is None  # main stream: not served from the side stream's arena
            second = ops.embed_rows(mods[0], idx)  # ... so this is an index_select on the main stream
            torch.cuda.current_stream().wait_stream(side)
    finally:
        ops.lib.upnerf_embed_fwd_grouped = real
    assert launches == [2]
    assert torch.equal(first, mods[1].weight.detach()[idx]) and torch.equal(second, mods[0].weight.detach()[idx])


# ------------------------------------------------------------------------------------------ generic GEMMs
@pytest.mark.parametrize("M,N,K,relu", [(300, 256, 384, True), (129, 384, 256, False), (64, 1, 256, False),
                                        (500, 3, 128, False), (77, 128, 384, True), (4096, 16, 128, False)])
def test_linear_fwd_bwd(hip, M, N, K, relu):
    x, w, b = gen((M, K), 20), gen((N, K), 21) / K ** 0.5, gen((N,), 22)
    gy = gen((M, N), 23)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y_ref = torch.nn.functional.linear(xr, wr, br)
    y_ref = torch.relu(y_ref) if relu else y_ref
    (y_ref * gy).sum().backward()
    xg, wg, bg = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = hip["ops"].hip_linear(xg, wg, bg, relu)
    (y * gy.cuda()).sum().backward()
    assert rel_err(cpu(y), y_ref.detach()) < TOL_ACT
    assert rel_err(cpu(xg.grad), xr.grad) < TOL_GRAD
    assert rel_err(cpu(wg.grad), wr.grad) < TOL_GRAD
    assert rel_err(cpu(bg.grad), br.grad) < TOL_GRAD


@pytest.mark.parametrize("M,K,N,ld,off", [(300, 128, 48, 336, 283), (4096, 128, 16, 272, 256), (65, 64, 70, 77, 3)])
def test_linear_on_a_strided_kn_view(hip, M, K, N, ld, off):
    """y = x . Wv with Wv[k][n] = base[off + k*ld + n] read in place (column block of a packed matrix, odd strides)."""
    x, base = gen((M, K), 24), gen((off + K * ld + N,), 25)
    y = hip["ops"].linear_kn_view(x.cuda(), base.cuda(), off, ld, N)
    Wv = torch.as_strided(base, (K, N), (ld, 1), off)
    assert rel_err(cpu(y), x.double() @ Wv.double()) < TOL_ACT


@pytest.mark.parametrize("M,N,K", [(1000, 256, 256), (333, 128, 256), (5000, 256, 64), (64, 32, 16), (777, 64, 80),
                                   (40000, 256, 256)])
def test_wgrad_and_bias(hip, M, N, K):
    a, b = gen((M, N), 30), gen((M, K), 31)
    dW = torch.empty(N, K, device="cuda")
    db = torch.empty(N, device="cuda")
    hip["ops"].wgrad_into(M, a.cuda(), N, N, b.cuda(), K, K, dW.data_ptr(), K, db.data_ptr(), torch.device("cuda", 0))
    ref = a.double().t() @ b.double()
    assert rel_err(cpu(dW), ref) < TOL_ACT
    assert rel_err(cpu(db), a.double().sum(0)) < TOL_ACT
    # bitwise reproducible (fixed-order slab reduction, no atomics)
    dW2 = torch.empty(N, K, device="cuda")
    hip["ops"].wgrad_into(M, a.cuda(), N, N, b.cuda(), K, K, dW2.data_ptr(), K, None, torch.device("cuda", 0))
    assert torch.equal(dW, dW2)


def test_grouped_wgrad_matches_the_per_layer_kernel_and_autograd_defers_to_it(hip):
    """upnerf_wgrad_grouped: mixed shapes (blocks cut at 128, ragged N / K / M, strided operands, with and without bias)
    in one launch; and HipLinear's backward hands its small weight gradients to it through the engine callback."""
    import ctypes as C
    from upnerf_amd import _lib
    ops = hip["ops"]
    dev = torch.device("cuda", 0)
    shapes = [(4096, 256, 384, True), (4096, 128, 384, True), (1000, 384, 128, False), (777, 132, 20, True),
              (4096, 256, 256, True), (64, 8, 392, False)]
    groups, keep, outs = [], [], []
    for j, (M, N, K, bias) in enumerate(shapes):
        lda, ldb = N + 4 * (j % 2), K + 8 * (j % 3)  # strided operands: only the first N / K columns are used
        a, b = gen((M, lda), 300 + j).cuda(), gen((M, ldb), 320 + j).cuda()
        dW = torch.full((N, K), float("nan"), device=dev)
        db = torch.full((N,), float("nan"), device=dev) if bias else None
        groups.append(_lib.WgradGroup(A=a.data_ptr(), B=b.data_ptr(), dW=dW.data_ptr(),
                                      db=None if db is None else db.data_ptr(), M=M, N=N, K=K, lda=lda, ldb=ldb, ldo=K))
        keep.append((a, b))
        outs.append((dW, db))
    arr = (_lib.WgradGroup * len(groups))(*groups)
    n = _lib.lib.upnerf_wgrad_grouped_scratch(arr, len(groups), 64)
    assert n > 0
    for rep in range(2):
        ws = torch.empty(n, device=dev)
        assert _lib.lib.upnerf_wgrad_grouped(arr, len(groups), ws.data_ptr(), 64, _lib.stream()) == 0
        if rep == 0:
            first = [(w.clone(), None if b_ is None else b_.clone()) for w, b_ in outs]
    for (M, N, K, bias), (a, b), (dW, db), (w0, b0) in zip(shapes, keep, outs, first):
        ref = a[:, :N].double().cpu().t() @ b[:, :K].double().cpu()
        assert rel_err(cpu(dW), ref) < TOL_ACT, (M, N, K)
        assert torch.equal(dW, w0)  # fixed-order reduction: bitwise reproducible
        if bias:
            assert rel_err(cpu(db), a[:, :N].double().cpu().sum(0)) < TOL_ACT and torch.equal(db, b0)
    assert _lib.lib.upnerf_wgrad_grouped(arr, 0, ws.data_ptr(), 64, None) == -1
    # autograd: a small MLP on hip_linear, gradients with the deferral on and off
    x = gen((512, 384), 340).cuda()
    ws_ = [gen((256, 384), 341).cuda().requires_grad_(True), gen((128, 256), 342).cuda().requires_grad_(True)]
    bs_ = [gen((256,), 343).cuda().requires_grad_(True), None]
    res = {}
    for on in (True, False):
        ops.DEFERRED_WGRADS.enabled = on
        try:
            h = ops.hip_linear(x, ws_[0], bs_[0], True, defer_wgrad=True)
            y = ops.hip_linear(h, ws_[1], bs_[1], defer_wgrad=True)
            res[on] = torch.autograd.grad((y * y).sum(), [ws_[0], bs_[0], ws_[1]])
        finally:
            ops.DEFERRED_WGRADS.enabled = True
    assert not ops.DEFERRED_WGRADS.groups and not ops.DEFERRED_WGRADS.keep
    for g_on, g_off in zip(res[True], res[False]):
        assert torch.isfinite(g_on).all() and rel_err(cpu(g_on), cpu(g_off).double()) < 1e-5


def test_vec_wgrad(hip):
    M, K = 3001, 128
    v, x = gen((M, 4), 32), gen((M, K), 33)
    dw = torch.empty(3, K, device="cuda")
    dbv = torch.empty(3, device="cuda")
    hip["ops"].vec_wgrad_into(M, v.cuda(), 4, 3, x.cuda(), K, K, dw.data_ptr(), dbv.data_ptr(), torch.device("cuda", 0))
    assert rel_err(cpu(dw), v[:, :3].double().t() @ x.double()) < TOL_ACT
    assert rel_err(cpu(dbv), v[:, :3].double().sum(0)) < TOL_ACT


def test_adam_matches_torch_optim(hip):
    n = 10007
    p0 = gen((n,), 40)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=5e-4, eps=1e-8)
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 6):
        g = gen((n,), 40 + step) * (0.0 if step == 3 else 1.0)
        ref.grad = g.clone()
        opt.step()
        hip["ops"].adam_flat_(p, g.cuda(), m, v, step, 5e-4)
        assert rel_err(cpu(p), ref.detach()) < 1e-6


# ------------------------------------------------------------------------------------------ fused field + composite
STAGE_CASES = [("cfg1_small", "coarse"), ("cfg2_phase0", "coarse"), ("cfg2_phase1", "fine"), ("cfg2_phase2", "fine"),
               ("small_nocand", "fine"), ("small_round_half", "fine"), ("small_allmasked", "coarse"),
               ("cfg2_trained_p08", "fine"), ("cfg2_trained_p045", "fine")]  # "trained-like" magnitudes, all bands on


@pytest.fixture
def field_mode(hip, request):
    """Run a test with the field contractions in the given arithmetic ("f16x3" is the default of the product path)."""
    rd = hip["rendering"]
    old = rd.FIELD_MODE
    rd.FIELD_MODE = request.param
    yield request.param
    rd.FIELD_MODE = old


# (the comparison itself, its gates -- the relaxed ones of the "f16" mode and the limits on differing ReLU decisions among them --
# and the inputs of a pass: tests/field_cases.py, shared with tests/test_hip_field_edges.py)
@pytest.mark.parametrize("field_mode", ["f16x3", "f32", "f16"], indirect=True)
@pytest.mark.parametrize("name,typ", STAGE_CASES)
def test_field_pass_stage_by_stage(hip, name, typ, field_mode):
    if field_mode != "f16x3" and Case(name).cfgs()["nerf_coarse"].W != 256:
        pytest.skip("64-wide fields run the fp32 kernels in either mode (and the f16 mode refuses them)")
    check_field_pass(hip, field_cases.load((name, typ)), field_mode, torch.float32, tag=f"{name} {typ}")


def test_frag16_row_norms_bound_every_matrix(hip):
    """upnerf_frag16(..., wnorm): wnorm[j] (forward set) / wnorm[32 + j] (transposed set) = max over the rows of descriptor j of
    the row's 1-norm -- what the register-resident kernels bound |W x|_inf with before a layer's outputs exist."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, trunk_gain=1.6, **kw))
    model = model.cuda()
    pk = model.packer
    P = model.packed().detach()
    _, _, _, wnorm = pk.frag16_hip(P, perm=True)
    torch.cuda.synchronize()
    fd, nf, bd, nb = pk._descs16()
    Pc = P.cpu().double()
    for base, descs, n in ((0, fd, nf), (32, bd, nb)):
        for j in range(n):
            q = descs[j]
            idx = q.src_off + (torch.arange(q.rows)[:, None] * (1 if q.transpose else q.src_ld) +
                               torch.arange(q.cols)[None, :] * (q.src_ld if q.transpose else 1))
            ref = Pc[idx].abs().sum(1).max()
            got = float(wnorm[base + j])
            assert abs(got - float(ref)) <= 1e-5 * float(ref) + 1e-12, (base, j, got, float(ref))


@pytest.mark.parametrize("M,K,nvec", [(1000, 256, 1), (1000, 128, 3), (77, 128, 1), (4099, 256, 3)])
def test_vec_wgrad_frag16_matches_fp64(hip, M, K, nvec):
    """upnerf_vec_wgrad_frag16 (dw[c][k] = sum_m v[m][c] X[m][k], dbv[c] = sum_m v[m][c]) on a fragment-ordered fp16 tensor
    against fp64 on the values the fragments decode to; M not a multiple of the 32-sample tile."""
    lib, rd, ops = hip["lib"], hip["rendering"], hip["ops"]
    dev = "cuda"
    Mp = (M + 31) // 32 * 32
    texp = torch.randint(-3, 4, (Mp // 32,), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    X16 = rd.quant16_frag(gen((Mp, K), 2).to(dev), texp)
    X = rd.dequant16(X16[None], texp[None], frag=True)[0, :M].double()
    ldv = 4 if nvec == 3 else 1
    v = gen((M, ldv), 3).to(dev)
    dw, dbv = torch.full((nvec, K), 7.0, device=dev), torch.full((nvec,), 7.0, device=dev)
    ns = ops.nsplit_for(M)
    ws = torch.empty(ns * 4 * (K + 1), device=dev)
    assert lib.lib.upnerf_vec_wgrad_frag16(M, v.data_ptr(), ldv, nvec, X16.data_ptr(), texp.data_ptr(), K, dw.data_ptr(), dbv.data_ptr(),
                                           ws.data_ptr(), ns, None) == 0
    torch.cuda.synchronize()
    ref = v[:, :nvec].double().t() @ X
    assert rel_err(cpu(dw), cpu(ref)) < 1e-5
    assert rel_err(cpu(dbv), cpu(v[:, :nvec].double().sum(0))) < 1e-5


@pytest.mark.parametrize("R,S", [(7, 40), (5, 33), (3, 128), (4, 257)])
def test_ray_part_finish_sums_the_per_32_sample_partials(hip, R, S):
    """upnerf_ray_part_finish: per-ray sums from the register-resident backward kernel's partials (one row per 32 samples: the
    sums over the rows of its first / second ray, for gz_r1 and gz_g1), rays that straddle and rays that span several rows."""
    lib = hip["lib"]
    dev = "cuda"
    M = R * S
    Mp = (M + 255) // 256 * 256
    x = [torch.zeros(Mp, 128, device=dev), torch.zeros(Mp, 128, device=dev)]
    for t in range(2):
        x[t][:M] = gen((M, 128), 10 + t).to(dev)
    part = torch.full((Mp // 32, 512), float("nan"), device=dev)  # unwritten second-ray blocks must never be read
    m = torch.arange(Mp, device=dev)
    first = (m // 32 * 32) // S  # ray of the first sample of each 32-sample row group
    slot = m // S - first
    for t in range(2):
        for sl in range(2):
            sums = (x[t] * (slot == sl)[:, None]).view(Mp // 32, 32, 128).sum(1)
            has = ((slot == sl).view(Mp // 32, 32).any(1)) | (sl == 0)
            part[has, (2 * t + sl) * 128:(2 * t + sl + 1) * 128] = sums[has]
    rs_g1, rs_r1 = torch.empty(R, 128, device=dev), torch.empty(R, 128, device=dev)
    assert lib.lib.upnerf_ray_part_finish(R, S, part.data_ptr(), rs_g1.data_ptr(), rs_r1.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert rel_err(cpu(rs_r1), cpu(x[0][:M].view(R, S, 128).sum(1))) < 1e-5
    assert rel_err(cpu(rs_g1), cpu(x[1][:M].view(R, S, 128).sum(1))) < 1e-5


def test_wgrad_f16p_on_128_wide_fragments(hip):
    """upnerf_wgrad16 with 128-wide fragment operands (UPNERF_WG_F16_FRAG) on both sides (candidate_encoding.2: gz_g2 x g1) against fp64."""
    lib, rd, ops = hip["lib"], hip["rendering"], hip["ops"]
    dev, M = "cuda", 2999
    Mp = (M + 255) // 256 * 256
    ea = torch.randint(-2, 3, (Mp // 32,), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    eb = torch.randint(-2, 3, (Mp // 32,), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
    A16, B16 = rd.quant16_frag(gen((Mp, 128), 3).to(dev), ea), rd.quant16_frag(gen((Mp, 128), 4).to(dev), eb)
    A = rd.dequant16(A16[None], ea[None], frag=True)[0, :M].double()
    B = rd.dequant16(B16[None], eb[None], frag=True)[0, :M].double()
    expo = torch.tensor([3, 3], device=dev, dtype=torch.int32)
    dW, db = torch.full((128, 128), 7.0, device=dev), torch.full((128,), 7.0, device=dev)
    ns = ops.nsplit_for(M)
    ws = torch.empty(ns * (256 * 256 + 256), device=dev)
    desc = wg_desc(hip, M, (A16, 128, lib.WG_F16_FRAG, ea), 128, (B16, 128, lib.WG_F16_FRAG, eb), 128, expo.data_ptr(), expo.data_ptr() + 4,
                   dW, 128, db, ws, ns)
    assert lib.lib.upnerf_wgrad16(C.byref(desc), None, None) == 0
    torch.cuda.synchronize()
    assert rel_err(cpu(dW), cpu(A.t() @ B)) < 1e-5 and rel_err(cpu(db), cpu(A.sum(0))) < 1e-5


@pytest.mark.parametrize("M,n2", [(3000, 0), (3000, 128), (100, 128)])
def test_wgrad_f16p_chain_on_fragments_with_a_split_result(hip, M, n2):
    """A chained upnerf_wgrad16 with both operands as fp16 fragments (UPNERF_WG_F16_FRAG) and the result split by rows between two
    destinations, finished by upnerf_wgrad_finish, against fp64 on the decoded values."""
    lib, rd, ops = hip["lib"], hip["rendering"], hip["ops"]
    from upnerf_amd._lib import WgradPending
    dev = "cuda"
    Mp = (M + 255) // 256 * 256
    ea = torch.randint(-2, 3, (Mp // 32,), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    eb = torch.randint(-2, 3, (Mp // 32,), generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
    A16, B16 = rd.quant16_frag(gen((Mp, 256), 3).to(dev), ea), rd.quant16_frag(gen((Mp, 256), 4).to(dev), eb)
    A = rd.dequant16(A16[None], ea[None], frag=True)[0, :M].double()
    B = rd.dequant16(B16[None], eb[None], frag=True)[0, :M].double()
    expo = torch.tensor([3, 3], device=dev, dtype=torch.int32)  # tensor-wide exponents: |x| < 1 -> |x * 2^3| < 8
    n1 = n2 if n2 else 256
    dW, db = torch.full((n1, 256), 7.0, device=dev), torch.full((n1,), 7.0, device=dev)
    dW2, db2 = torch.full((256 - n1 if n2 else 1, 300), 7.0, device=dev), torch.full((256,), 7.0, device=dev)
    ns = ops.nsplit_for(M)
    ws = torch.empty(ns * (256 * 256 + 256), device=dev)
    pend = WgradPending()
    desc = wg_desc(hip, M, (A16, 256, lib.WG_F16_FRAG, ea), 256, (B16, 256, lib.WG_F16_FRAG, eb), 256, expo.data_ptr(), expo.data_ptr() + 4,
                   dW, 256, db, ws, ns, n2=n2, dW2=dW2 if n2 else None, ldo2=300, db2=db2 if n2 else None)
    assert lib.lib.upnerf_wgrad16(C.byref(desc), C.byref(pend), None) == 0
    assert lib.lib.upnerf_wgrad_finish(C.byref(pend), None) == 0
    torch.cuda.synchronize()
    ref, refb = A.t() @ B, A.sum(0)
    assert rel_err(cpu(dW), cpu(ref[:n1])) < 1e-5 and rel_err(cpu(db), cpu(refb[:n1])) < 1e-5
    if n2:
        assert rel_err(cpu(dW2[:, :256]), cpu(ref[n1:])) < 1e-5 and rel_err(cpu(db2[:256 - n1]), cpu(refb[n1:])) < 1e-5
        assert float((dW2[:, 256:] - 7.0).abs().max()) == 0.0  # nothing written past the 256 columns of a row


@pytest.mark.parametrize("R,S,mode,use_cand,use_rgb,raygrad", [(300, 64, 3, False, False, False), (41, 70, 3, False, True, True),
                                                                 (37, 70, 1, True, True, False), (1, 40, 1, True, True, True),
                                                                 (2, 32, 0, True, False, False)])
def test_rr_kernels_match_the_tile_kernels_on_the_rarer_paths(hip, R, S, mode, use_cand, use_rgb, raygrad):
    """f16 mode: register-resident kernels against the 64-sample tile kernels of the same arithmetic on paths the goldens do not
    take -- a field without candidate encoding (mode 3: the feature map's rank-1 term is then ALL of d e; round 4 found it
    dropped), no gradient into the rays (the d x0 stages leave the slab sequence), a single ray, S = 32."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk = model.packer
    g = lambda shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    o = (g((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(g((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(g((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = g((R, 16), 73).cuda(), g((R, 48), 74).cuda()
    old = rd.FIELD_MODE, rd.FIELD_RR
    res = {}
    try:
        for tag, rr in (("tile", 0), ("rr", 1)):
            rd.FIELD_MODE, rd.FIELD_RR = "f16", rr
            cfg = rd._PassCfg(pk, mode, use_cand, use_rgb, [1.0] * 10, [1.0] * 4)
            leaves = [t.clone().requires_grad_(rg) for t, rg in zip((o, d, c_rows, a_rows, model.packed().detach()),
                                                                     (raygrad, raygrad, True, True, True))]
            outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
            sum((t * g(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel() and t.requires_grad).backward()
            torch.cuda.synchronize()
            res[tag] = ([cpu(t) for t in outs], [cpu(t.grad) if t.grad is not None else None for t in leaves])
    finally:
        rd.FIELD_MODE, rd.FIELD_RR = old
    l2 = lambda a, b: float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))
    for i, (a, b) in enumerate(zip(res["rr"][0], res["tile"][0])):
        if a.numel():
            assert l2(a, b) < 2e-3, ("out", i, l2(a, b))
    for i, (a, b) in enumerate(zip(res["rr"][1], res["tile"][1])):
        assert (a is None) == (b is None), i
        if a is not None and float(b.abs().max()) > 0:
            assert l2(a, b) < 2e-2, ("grad", i, l2(a, b))
    assert float(res["rr"][1][4].abs().max()) > 0


@pytest.mark.parametrize("R,S,mode,use_cand,use_rgb", [(37, 70, 1, True, True), (11, 33, 0, True, False), (9, 128, 2, False, True),
                                                         (5, 64, 3, False, False)])
def test_rr_inference_pass_matches_the_training_forward(hip, R, S, mode, use_cand, use_rgb):
    """f16 mode, register-resident kernels: the no-grad pass (e / g2 leave as fp16 fragments, nothing else is stored) gives the
    outputs of the training forward (which may keep fp32 rows of e for a single head) to the mode's rounding -- including the
    density-only mode 3, whose feature map needs the final layer although no head consumes e (round 4: it was skipped)."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk = model.packer
    g = lambda shape, seed: torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    o = (g((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(g((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(g((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = g((R, 16), 73).cuda(), g((R, 48), 74).cuda()
    old = rd.FIELD_MODE, rd.FIELD_RR
    res = []
    try:
        rd.FIELD_MODE, rd.FIELD_RR = "f16", 1
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                cfg = rd._PassCfg(pk, mode, use_cand, use_rgb, [1.0] * 10, [1.0] * 4)
                leaves = [t.clone().requires_grad_(grad) for t in (o, d, c_rows, a_rows, model.packed().detach())]
                outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
                torch.cuda.synchronize()
                res.append([cpu(t) for t in outs])
    finally:
        rd.FIELD_MODE, rd.FIELD_RR = old
    for i, (a, b) in enumerate(zip(res[1], res[0])):
        if a.numel():
            assert rel_err(a, b) < 1e-3, (i, rel_err(a, b))


@pytest.mark.parametrize("R,S,mode", [(5, 70, 1), (3, 33, 3), (2, 129, 0)])
def test_compositing_reads_e_as_fp16_fragments(hip, R, S, mode):
    """upnerf_composite_fwd / _bwd with e given as the register-resident field kernels' fp16 operand fragments (e16 / eexp)
    against the same kernels on the fp32 rows those fragments decode to: every output within fp32 summation-order noise."""
    lib, rd = hip["lib"], hip["rendering"]
    from upnerf_amd._lib import CompositeBwdArgs, CompositeFwdArgs
    M, W, W2 = R * S, 256, 128
    Mp = (M + 31) // 32 * 32
    dev = "cuda"
    texp = torch.randint(-3, 4, (Mp // 32,), generator=torch.Generator().manual_seed(5)).to(torch.int32).to(dev)
    e16 = rd.quant16_frag(gen((Mp, W), 1).to(dev), texp)
    e = rd.dequant16(e16[None], texp[None], frag=True)[0, :M].contiguous()
    gexp = torch.randint(-2, 3, (Mp // 32,), generator=torch.Generator().manual_seed(15)).to(torch.int32).to(dev)
    g2_16 = rd.quant16_frag(gen((Mp, W2), 7).to(dev), gexp)
    z = torch.sort(gen((R, S), 2, 0.1, 4.0), dim=-1).values.to(dev)
    sig_s, sig_c, rgb = gen((M,), 3, 0.0, 3.0).to(dev), gen((M,), 4, 0.0, 3.0).to(dev), gen((M, 3), 6, 0.0, 1.0).to(dev)
    g2 = rd.dequant16(g2_16[None], gexp[None], frag=True)[0, :M].contiguous()
    joint = mode <= 1
    p = lambda t: None if t is None else t.data_ptr()

    def run(frag):
        o = {k: torch.zeros(*shp, device=dev) for k, shp in dict(w_all=(M,), w_sj=(M,), w_cj=(M,), w_s=(M,), E_s=(R, W), G_c=(R, W2), sum_sfeat=(R,),
                                                                t_weight=(R,), c_depth=(R,), s_depth=(R,), rgb_map=(R, 3)).items()}
        fa = CompositeFwdArgs(R=R, S=S, W=W, mode=mode, z=p(z), sigma_s=p(sig_s), sigma_c=p(sig_c), rgb=p(rgb), has_rgb=1,
                              e=None if frag else p(e), g2=p(g2) if frag < 2 else None, e16=p(e16) if frag else None,
                              eexp=p(texp) if frag else None, g2_16=p(g2_16) if frag == 2 else None,
                              g2exp=p(gexp) if frag == 2 else None, **{k: p(v) for k, v in o.items()})
        assert lib.lib.upnerf_composite_fwd(C.byref(fa), None) == 0
        gE, gG = gen((R, W), 8).to(dev), gen((R, W2), 9).to(dev)
        gr = {k: gen(shp, 10 + i).to(dev) for i, (k, shp) in enumerate(dict(g_sum_sfeat=(R,), g_t_weight=(R,), g_c_depth=(R,), g_s_depth=(R,),
                                                                            g_rgb_map=(R, 3), g_w_all=(M,), g_w_s=(M,)).items())}
        d = dict(d_sigma_s=torch.zeros(M, device=dev), d_sigma_c=torch.zeros(M, device=dev), d_rgb=torch.zeros(M, 3, device=dev))
        ba = CompositeBwdArgs(R=R, S=S, W=W, mode=mode, has_rgb=1, z=p(z), sigma_s=p(sig_s), sigma_c=p(sig_c), rgb=p(rgb),
                              e=None if frag else p(e), g2=p(g2) if frag < 2 else None, w_all=p(o["w_all"]), w_sj=p(o["w_sj"]), w_cj=p(o["w_cj"]), w_s=p(o["w_s"]),
                              g_E_s=p(gE), g_G_c=p(gG) if joint else None, e16=p(e16) if frag else None, eexp=p(texp) if frag else None,
                              g2_16=p(g2_16) if frag == 2 else None, g2exp=p(gexp) if frag == 2 else None,
                              **{k: p(v) for k, v in gr.items()}, **{k: p(v) for k, v in d.items()})
        assert lib.lib.upnerf_composite_bwd(C.byref(ba), None) == 0
        torch.cuda.synchronize()
        return {**o, **d}

    a = run(0)
    for frag in (1, 2):  # e as fragments; e and g2 as fragments
        b = run(frag)
        for k in a:
            assert rel_err(cpu(b[k]), cpu(a[k])) < 5e-6, (frag, k)
    assert float(a["E_s"].abs().max()) > 0 and (not joint or float(a["G_c"].abs().max()) > 0)


@pytest.mark.parametrize("R,S,mode,use_cand,use_rgb", [(7, 40, 1, True, True), (5, 33, 0, True, False),
                                                         (3, 200, 2, False, True), (9, 32, 3, False, False)])
def test_field_f16x3_matches_fp32_kernels_on_ragged_tiles(hip, R, S, mode, use_cand, use_rgb):
    _ragged_tiles(hip, R, S, mode, use_cand, use_rgb)


@pytest.mark.parametrize("field_mode", ["f16x3", "f16"], indirect=True)
@pytest.mark.parametrize("R,S,mode,use_cand,use_rgb", [(7, 40, 1, True, True), (5, 64, 0, True, False), (3, 256, 2, False, True),
                                                         (6, 33, 1, True, True), (2, 200, 1, True, True)])
def test_tile_partial_sums_match_the_separate_launches(hip, R, S, mode, use_cand, use_rgb, field_mode):
    """upnerf_field_bwd_args.tile_part + upnerf_tile_part_finish (the backward kernel's per-tile partial sums of the 128-wide
    vector heads and of the per-ray sums) against upnerf_vec_wgrad / upnerf_ray_sum on the stored tensors: the same sums in
    another order (1e-5 of the tensor's scale), everything else bitwise; tiles that straddle up to three rays, ragged last tile."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk, L = model.packer, model.packer.L
    o = (gen((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(gen((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = gen((R, 16), 73).cuda(), gen((R, 48), 74).cuda()
    cfg = rd._PassCfg(pk, mode, use_cand, use_rgb, [1.0] * 10, [1.0] * 4)
    res = {}
    old, old_join = rd.TILE_PARTIALS, rd.JOIN_HEADS
    rd.JOIN_HEADS = 0  # (the joined [gz_r1 | gz_g1] weight gradient needs the partial sums: it would differ between the two runs)
    try:
        for tp in (0, 1):
            rd.TILE_PARTIALS = tp
            leaves = [t.clone().requires_grad_(True) for t in (o, d, c_rows, a_rows, model.packed().detach())]
            outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
            sum((t * gen(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel()).backward()
            res[tp] = [cpu(t.grad) if t.grad is not None else None for t in leaves]
    finally:
        rd.TILE_PARTIALS, rd.JOIN_HEADS = old, old_join
    a, b = res[0], res[1]
    W2 = pk.W2
    moved = [(L.wcsig, W2), (L.bcsig, 1), (L.wr2, 3 * W2), (L.br2, 3),                 # the vector heads
             (L.wc1 + pk.W, None), (L.wr1 + pk.W, None)]                                # consumers of the per-ray sums
    dPa, dPb = a[4].clone(), b[4].clone()
    bad = {}
    for off, n in moved[:4]:
        x, y = dPa[off:off + n].double(), dPb[off:off + n].double()
        if x.abs().max() > 0:
            e = float((x - y).abs().max() / x.abs().max())
            if not e < (1e-5 if n > 3 else 2e-4):  # the bias sums are single numbers left over from cancelling terms
                bad[f"dP[{off}:{off + n}]"] = e
        dPa[off:off + n] = 0
        dPb[off:off + n] = 0
    # wc1[:, W:] and wr1[:, W:] (the per-ray inputs' columns) come from the ray sums: strided blocks of the two matrices
    for off, ld, k in ((L.wc1, pk.W + 16, 16), (L.wr1, pk.W + 80, 80)):
        va, vb = dPa[off:off + W2 * ld].view(W2, ld), dPb[off:off + W2 * ld].view(W2, ld)
        x, y = va[:, pk.W:].double(), vb[:, pk.W:].double()
        if x.abs().max() > 0:
            e = float((x - y).abs().max() / x.abs().max())
            if not e < 1e-5:
                bad[f"ray-sum block of {off}"] = e
        va[:, pk.W:] = 0
        vb[:, pk.W:] = 0
    assert torch.equal(dPa, dPb), "parameter gradients outside the re-ordered sums changed"
    for i in (0, 1):
        assert (a[i] is None and b[i] is None) or torch.equal(a[i], b[i])
    for i in (2, 3):  # d c_rows, d a_rows = ray sums . W
        if a[i] is not None and a[i].abs().max() > 0:
            e = float((a[i].double() - b[i].double()).abs().max() / a[i].double().abs().max())
            if not e < 1e-5:
                bad[f"leaf {i}"] = e
    assert not bad, bad


@pytest.mark.parametrize("R", [1, 301, 4096])
def test_ray_aux_with_aligned_misaligned_and_absent_appearance_rows(hip, R):
    """upnerf_ray_aux (the per-ray direction encoding | appearance row | zero padding block of models/nerf.py:96-109's colour
    head input): round 6 copies the 48 appearance floats as twelve 16-byte loads when the rows start on 16 bytes and element by
    element otherwise -- the same bytes either way, and the kernel-space restatement's values."""
    import ctypes as C
    lib, ptr, check, stream = hip["lib"].lib, hip["lib"].ptr, hip["lib"].check, hip["lib"].stream
    d = torch.nn.functional.normalize(gen((R, 3), 5), dim=1)
    a = gen((R, 48), 6)
    wk = [1.0, 0.75, 0.25, 0.0]
    ref = ks.ray_aux(d, a, wk)
    ref0 = ks.ray_aux(d, None, wk)
    dg = d.cuda()
    store = torch.zeros(R * 48 + 8, device="cuda")
    outs = []
    for off in (0, 4, 1, 3):  # floats: 0 and 4 start on 16 bytes, 1 and 3 do not
        rows = store[off:off + R * 48].view(R, 48)
        rows.copy_(a)
        assert (rows.data_ptr() % 16 == 0) == (off % 4 == 0)
        aux = torch.full((R, ks.AUXK), float("nan"), device="cuda")
        check(lib.upnerf_ray_aux(R, ptr(dg), ptr(rows), (C.c_float * 4)(*wk), None, ptr(aux), stream()), "upnerf_ray_aux")
        outs.append(cpu(aux))
    aux = torch.full((R, ks.AUXK), float("nan"), device="cuda")
    check(lib.upnerf_ray_aux(R, ptr(dg), None, (C.c_float * 4)(*wk), None, ptr(aux), stream()), "upnerf_ray_aux")
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert torch.equal(outs[0][:, 27:75], a)  # a copy: bit for bit
    assert float((outs[0] - ref).abs().max()) < 2e-6
    assert float((cpu(aux) - ref0).abs().max()) < 2e-6 and float(cpu(aux)[:, 27:].abs().max()) == 0.0


@pytest.mark.parametrize("R", [1, 17, 37, 65, 129, 1024])
def test_fused_transient_net_matches_torch(hip, R):
    """csrc/transient.hip (the whole TransientNet as one forward and one backward launch + one grouped weight-gradient launch)
    against the same module evaluated by plain torch ops in fp64 on the CPU (models/transient_net.py:27-38): outputs and every
    gradient, a ragged last tile (R % 16 != 0), and against the per-layer HIP path it replaces.  R = 1 .. 129 take the grouped
    weight-gradient launch across its R // 64 split boundaries (no split, one, two) with ragged tiles, through the wrapper's
    slicing of the three heads' rows and the two-block write of wt's gradient; the kernels themselves are held stage by stage in
    tests/test_hip_transient.py."""
    import upnerf_amd.transient_net as tn
    from upnerf_amd import synth
    torch.manual_seed(5)
    NI = 11
    net = tn.TransientNet(NI).cuda()
    net.load_state_dict({k: v.cuda() for k, v in synth.transient_state(NI, seed=4).items()})
    feat = gen((R, 384), 91).cuda()
    ts = (torch.arange(R) * 7 % NI).cuda()
    up = [gen((R, 1), 92).cuda(), gen((R, 3), 93).cuda(), gen((R, 1), 94).cuda()]

    def run(fused, want_feat_grad):
        old = tn.FUSED
        tn.FUSED = fused
        try:
            net.zero_grad(set_to_none=True)
            f = feat.clone().requires_grad_(want_feat_grad)
            out = net(f, ts)
            (out["alpha"] * up[0]).sum().add((out["rgb"] * up[1]).sum()).add((out["beta"] * up[2]).sum()).backward()
            torch.cuda.synchronize()
            return ({k: cpu(v) for k, v in out.items()}, {n: cpu(q.grad) for n, q in net.named_parameters()},
                    cpu(f.grad) if want_feat_grad else None)
        finally:
            tn.FUSED = old

    # fp64 reference with plain torch modules
    import copy
    net64 = copy.deepcopy(net).cpu().double()
    f64 = cpu(feat).double().requires_grad_(True)
    h = net64.feat_encoder(f64)
    e = net64.final_encoder(h)
    t = net64.t_encoder(torch.cat([e, net64.embedding_t(cpu(ts))], -1))
    o64 = {"alpha": net64.alpha_layer(h), "rgb": net64.rgb_layer(t)}
    o64["beta"] = net64.beta_layer(t) * o64["alpha"] + net64.beta_min
    (o64["alpha"] * cpu(up[0]).double()).sum().add((o64["rgb"] * cpu(up[1]).double()).sum()).add(
        (o64["beta"] * cpu(up[2]).double()).sum()).backward()
    g64 = {n: q.grad for n, q in net64.named_parameters()}

    bad = {}

    def chk(tag, x, y, tol):
        x, y = x.double().reshape(-1), y.double().reshape(-1)
        err = float((x - y).abs().max() / max(float(y.abs().max()), 1e-30))
        if not err < tol:
            bad[tag] = err

    for fused in (True, False):
        out, grads, gf = run(fused, True)
        for k in out:
            chk(f"{fused} {k}", out[k], o64[k].detach(), 2e-6)
        for n in grads:
            chk(f"{fused} d {n}", grads[n], g64[n], 2e-5)
        chk(f"{fused} d feat", gf, f64.grad, 2e-5)
    out, grads, gf = run(True, False)  # without a gradient for the features (the training step: they are data)
    assert gf is None
    for n in grads:
        chk(f"nofeat d {n}", grads[n], g64[n], 2e-5)
    assert not bad, bad


@pytest.mark.parametrize("field_mode", ["f16x3", "f16"], indirect=True)
@pytest.mark.parametrize("R,S", [(7, 40), (3, 256)])
def test_joined_head_gradients_match_the_separate_launches(hip, R, S, field_mode):
    """[gz_r1 | gz_g1] stored as one tensor and contracted against e in ONE launch (upnerf_wgrad_desc.n2: rows split
    between the colour and the candidate head) against one launch per head: the same sums under one joint power-of-two scale
    instead of two (differences at the 2^-22 level of the f16x3 split, 1e-2 in the f16 mode), everything else bitwise."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk, L = model.packer, model.packer.L
    o = (gen((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(gen((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = gen((R, 16), 73).cuda(), gen((R, 48), 74).cuda()
    cfg = rd._PassCfg(pk, 1, True, True, [1.0] * 10, [1.0] * 4)
    res = {}
    old = rd.JOIN_HEADS
    try:
        for j in (0, 1):
            rd.JOIN_HEADS = j
            leaves = [t.clone().requires_grad_(True) for t in (o, d, c_rows, a_rows, model.packed().detach())]
            outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
            sum((t * gen(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel()).backward()
            res[j] = [cpu(t.grad) for t in leaves]
    finally:
        rd.JOIN_HEADS = old
    a, b = res[0], res[1]
    if field_mode == "f16":
        # the register-resident kernels also change what is STORED with the joined heads: e and [gz_r1 | gz_g1] leave as fp16
        # operand fragments only (compositing and the weight gradient read those), so nothing is bitwise -- every gradient
        # stays within the mode's rounding of the separate launches
        for i in range(5):
            assert rel_err(b[i], a[i]) < 1e-2, (i, rel_err(b[i], a[i]))
        return
    for i in range(4):
        assert torch.equal(a[i], b[i]), i
    dPa, dPb = a[4].clone(), b[4].clone()
    W, W2 = pk.W, pk.W2
    tol = 2e-6
    for off, ld, nb in ((L.wr1, W + 80, L.br1), (L.wc1, W + 16, L.bc1)):
        va, vb = dPa[off:off + W2 * ld].view(W2, ld), dPb[off:off + W2 * ld].view(W2, ld)
        x, y = va[:, :W].double(), vb[:, :W].double()
        assert float((x - y).abs().max() / x.abs().max()) < tol
        va[:, :W] = 0
        vb[:, :W] = 0
        xb, yb = dPa[nb:nb + W2].double(), dPb[nb:nb + W2].double()
        assert float((xb - yb).abs().max() / xb.abs().max()) < 1e-6  # bias = plain column sums, another order
        dPa[nb:nb + W2] = 0
        dPb[nb:nb + W2] = 0
    assert torch.equal(dPa, dPb)


@pytest.mark.parametrize("field_mode", ["f16x3", "f16"], indirect=True)
def test_chained_slab_reductions_are_bitwise_the_separate_ones(hip, field_mode):
    """upnerf_wgrad16 on a pending record (the slabs of one weight gradient summed by the first workgroups of the next launch) against
    one reduction launch per weight gradient: same slabs, same summation order -- every parameter gradient bit for bit."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk = model.packer
    R, S = 9, 72
    o = (gen((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(gen((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = gen((R, 16), 73).cuda(), gen((R, 48), 74).cuda()
    cfg = rd._PassCfg(pk, 1, True, True, [1.0] * 10, [1.0] * 4)
    res = {}
    old, old_join, old_ride = rd.WGRAD_CHAIN, rd.JOIN_HEADS, rd.VEC_RIDE
    rd.JOIN_HEADS = 0  # (the joined launch exists only in the chained form)
    rd.VEC_RIDE = 0    # (and so does the density head riding on the final layer's launch: another summation order, its own test below)
    try:
        for ch in (0, 1):
            rd.WGRAD_CHAIN = ch
            leaves = [t.clone().requires_grad_(True) for t in (o, d, c_rows, a_rows, model.packed().detach())]
            outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
            sum((t * gen(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel()).backward()
            res[ch] = [cpu(t.grad) for t in leaves]
    finally:
        rd.WGRAD_CHAIN, rd.JOIN_HEADS, rd.VEC_RIDE = old, old_join, old_ride
    for i in range(5):
        assert torch.equal(res[0][i], res[1][i]), i


@pytest.mark.parametrize("field_mode", ["f16x3", "f16"], indirect=True)
def test_density_head_gradient_riding_on_the_final_layer_launch_matches_the_separate_one(hip, field_mode):
    """upnerf_wgrad_desc.v (round 5): the shared density head reads the B operand of the final layer's weight gradient
    (models/nerf.py:89, 93), so its gradient dw_sigma = sum_m dpre_s[m] h[m][:] is summed inside that launch from the rows as
    they pass instead of by upnerf_vec_wgrad on a second read of h.  Same fp32 products in another summation order: 2e-6 of
    the vector's maximum; everything else of the pass bit for bit; and against fp64 on a stand-alone problem with a ragged
    number of rows."""
    from upnerf_amd import ops, synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk = model.packer
    R, S = 11, 70
    o = (gen((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(gen((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = gen((R, 16), 73).cuda(), gen((R, 48), 74).cuda()
    cfg = rd._PassCfg(pk, 1, True, True, [1.0] * 10, [1.0] * 4)
    res = {}
    old = rd.VEC_RIDE
    try:
        for ride in (0, 1):
            rd.VEC_RIDE = ride
            leaves = [t.clone().requires_grad_(True) for t in (o, d, c_rows, a_rows, model.packed().detach())]
            outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
            sum((t * gen(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel()).backward()
            res[ride] = [cpu(t.grad) for t in leaves]
    finally:
        rd.VEC_RIDE = old
    for i in range(4):
        assert torch.equal(res[0][i], res[1][i]), i
    L = pk.L
    dP0, dP1 = res[0][4], res[1][4]
    sig = slice(L.wsig, L.wsig + 256)
    assert float(dP0[sig].abs().max()) > 0
    assert float((dP0[sig] - dP1[sig]).abs().max()) <= 2e-6 * float(dP0[sig].abs().max())
    assert abs(float(dP0[L.bsig] - dP1[L.bsig])) <= 2e-6 * max(abs(float(dP0[L.bsig])), 1e-12)
    rest = torch.ones_like(dP0, dtype=torch.bool)
    rest[sig] = False
    rest[L.bsig] = False
    assert torch.equal(dP0[rest], dP1[rest])
    if field_mode != "f16x3":  # (f16: the head rides on the register-resident kernels' fragments; the pass above is its test)
        return
    # stand-alone, ragged M, against fp64
    M = 64 * 37 + 5
    A, B, v = gen((M, 256), 90).cuda() * 1e-3, torch.relu(gen((M, 256), 91)).cuda(), gen((M,), 92).cuda()
    dW, db, dv, dbv = (torch.empty(n, device="cuda") for n in (256 * 256, 256, 256, 1))
    run = ops.WgradRun(A.device, chained=True)
    expo = ops.scale_exponents(A, B)
    ea, eb = (expo.data_ptr(), expo.data_ptr() + 4) if isinstance(expo, torch.Tensor) else expo
    run.wgrad(M, ops.WgOp(A, 256), 256, ops.WgOp(B, 256), 256, ea, eb, dW=dW.data_ptr(), ldo=256, db=db.data_ptr(), v=v, dv=dv.data_ptr(),
              dbv=dbv.data_ptr())
    run.finish()
    torch.cuda.synchronize()
    ref_v = (v.double()[:, None] * B.double()).sum(0)
    ref_W = A.double().t() @ B.double()
    assert float((dv.double() - ref_v).abs().max() / ref_v.abs().max()) < 2e-6
    assert abs(float(dbv[0]) - float(v.double().sum())) <= 2e-6 * float(v.double().abs().sum())
    assert float((dW.double().view(256, 256) - ref_W).abs().max() / ref_W.abs().max()) < 2e-6
    assert float((db.double() - A.double().sum(0)).abs().max() / A.double().sum(0).abs().max()) < 2e-6


@pytest.mark.parametrize("M,Mf,ns", [(200, 256, 1), (200, 256, 3), (16360, 16384, 256)])
def test_a_mixed_run_on_one_pending_record_is_bitwise_the_unchained_one(hip, M, Mf, ns):
    """Five upnerf_wgrad16 links of different operand kinds and shapes on ONE pending record against the same five descriptors with
    pending = NULL (each summed at once by its own reduction launch): same slabs, same summation order -- every result bit for
    bit -- and each within the fp64 tolerance of its kind (2e-6 of the maximum for fp32 rows and the riding head, 1e-5 for the
    fp16-stored kinds on the values they decode to).
      1. fp32 rows 256 x 64    2. fp32 rows 256 x 256 + riding head    3. fp16 tiles 256 x 256
      4. fp16 fragments 256 x 256, rows [128, 256) to a second destination    5. fp32 rows 128 x 128
    M rows for the row-major links (200: ragged against the 64-row tiles and the 32-row chunks), Mf for the fragments.  Every
    shape is one block, so a launch has `ns` workgroups, and a pending 256 x 64 / 128 x 128 problem wants 64 of them for its
    reduction, a 256 x 256 one 256.  ns = 1, 3: every link after the first finds more pending reduction blocks than it has
    workgroups and takes the FLUSH path (a reduction launch before its own).  ns = 256 (64 rows per split): links 2 to 5 all CARRY
    the previous reduction in their prologue.  Link 1 finds nothing pending; upnerf_wgrad_finish sums link 5."""
    L, ops, rd = hip["lib"], hip["ops"], hip["rendering"]
    lib, dev = L.lib, "cuda"
    f32 = lambda shape, seed, relu=False: (torch.relu(gen(shape, seed)) if relu else gen(shape, seed) * 1e-3).to(dev)
    A1, B1, A2, B2, A5, B5 = (f32((M, 256), 100), f32((M, 64), 101, True), f32((M, 256), 102), f32((M, 256), 103, True),
                              f32((M, 128), 104), f32((M, 128), 105, True))
    v = gen((M,), 106).to(dev)
    e1, e2, e5 = ops.scale_exponents(A1, B1), ops.scale_exponents(A2, B2), ops.scale_exponents(A5, B5)
    e16 = torch.tensor([3, 3], device=dev, dtype=torch.int32)  # tensor-wide exponents of the fp16-stored links: |x| < 1 -> |x * 2^3| < 8
    texp = lambda n, seed: torch.randint(-2, 3, (n,), generator=torch.Generator().manual_seed(seed)).to(torch.int32).to(dev)
    ta, tb, fa, fb = texp((M + 63) // 64, 1), texp((M + 63) // 64, 2), texp(Mf // 32, 3), texp(Mf // 32, 4)
    tile16 = lambda x, t: (x * torch.ldexp(torch.ones((), device=dev), t.float()).repeat_interleave(64)[:M, None]).to(torch.float16)
    A3, B3 = tile16(gen((M, 256), 107).to(dev), ta), tile16(gen((M, 256), 108).to(dev), tb)
    A4, B4 = rd.quant16_frag(gen((Mf, 256), 109).to(dev), fa), rd.quant16_frag(gen((Mf, 256), 110).to(dev), fb)
    at = lambda e, i: e.data_ptr() + 4 * i

    def run(chained):
        o = {k: torch.full(shape, 7.0, device=dev) for k, shape in dict(
            W1=(256, 64), b1=(256,), W2=(256, 256), b2=(256,), dv=(256,), dbv=(1,), W3=(256, 256), b3=(256,), W4=(128, 256), b4=(128,),
            W4b=(128, 256), b4b=(128,), W5=(128, 128), b5=(128,)).items()}
        links = [
            wg_desc(hip, M, (A1, 256), 256, (B1, 64), 64, at(e1, 0), at(e1, 1), o["W1"], 64, o["b1"], None, ns),
            wg_desc(hip, M, (A2, 256), 256, (B2, 256), 256, at(e2, 0), at(e2, 1), o["W2"], 256, o["b2"], None, ns, v=v, dv=o["dv"], dbv=o["dbv"]),
            wg_desc(hip, M, (A3, 256, L.WG_F16_TILE, ta), 256, (B3, 256, L.WG_F16_TILE, tb), 256, at(e16, 0), at(e16, 1), o["W3"], 256,
                    o["b3"], None, ns),
            wg_desc(hip, Mf, (A4, 256, L.WG_F16_FRAG, fa), 256, (B4, 256, L.WG_F16_FRAG, fb), 256, at(e16, 0), at(e16, 1), o["W4"], 256,
                    o["b4"], None, ns, n2=128, dW2=o["W4b"], ldo2=256, db2=o["b4b"]),
            wg_desc(hip, M, (A5, 128), 128, (B5, 128), 128, at(e5, 0), at(e5, 1), o["W5"], 128, o["b5"], None, ns),
        ]  # (slabs: set below, from upnerf_wgrad16_scratch)
        need = max(lib.upnerf_wgrad16_scratch(C.byref(d)) for d in links)
        assert need == ns * (256 * 256 + 256 + 260)  # the 256 x 256 link with its riding head
        ws = [torch.empty(need, device=dev) for _ in range(2)]
        pend = L.WgradPending() if chained else None
        carried = []
        for i, d in enumerate(links):
            d.slabs = ws[i & 1].data_ptr()
            carried.append(chained and pend.nsplit > 0 and pend.rblocks <= ns)
            assert lib.upnerf_wgrad16(C.byref(d), C.byref(pend) if chained else None, None) == 0
        if chained:
            assert carried == [False] + [ns == 256] * 4  # flush path for ns = 1, 3; prologue for ns = 256
            assert lib.upnerf_wgrad_finish(C.byref(pend), None) == 0 and pend.nsplit == 0
        torch.cuda.synchronize()
        return o

    got, alone = run(True), run(False)
    for k in got:
        assert torch.equal(got[k], alone[k]), k
    near = lambda x, ref: float((x.double() - ref).abs().max() / ref.abs().max())
    for W, b, A, B in ((got["W1"], got["b1"], A1, B1), (got["W2"], got["b2"], A2, B2), (got["W5"], got["b5"], A5, B5)):
        assert near(W, A.double().t() @ B.double()) < 2e-6 and near(b, A.double().sum(0)) < 2e-6
    assert near(got["dv"], (v.double()[:, None] * B2.double()).sum(0)) < 2e-6
    assert abs(float(got["dbv"][0]) - float(v.double().sum())) <= 2e-6 * float(v.double().abs().sum())
    A3d, B3d = rd.dequant16(A3[None], ta[None])[0].double(), rd.dequant16(B3[None], tb[None])[0].double()
    assert rel_err(cpu(got["W3"]), cpu(A3d.t() @ B3d)) < 1e-5 and rel_err(cpu(got["b3"]), cpu(A3d.sum(0))) < 1e-5
    A4d = rd.dequant16(A4[None], fa[None], frag=True)[0].double()
    B4d = rd.dequant16(B4[None], fb[None], frag=True)[0].double()
    ref, refb = A4d.t() @ B4d, A4d.sum(0)
    assert rel_err(cpu(got["W4"]), cpu(ref[:128])) < 1e-5 and rel_err(cpu(got["b4"]), cpu(refb[:128])) < 1e-5
    assert rel_err(cpu(got["W4b"]), cpu(ref[128:])) < 1e-5 and rel_err(cpu(got["b4b"]), cpu(refb[128:])) < 1e-5


def test_adam_update_with_gradients_in_place_is_bitwise_the_flat_one(hip):
    """upnerf_adam_gather (every piece reads its gradient where autograd left it) against upnerf_adam on gathered gradients."""
    from upnerf_amd import _lib
    import ctypes as C
    lib, ptr = _lib.lib, _lib.ptr
    sizes = [1, 3, 1024, 1025, 7, 65536 + 5, 256 * 320]
    n = sum(sizes)
    p0, m0, v0 = gen((n,), 31).cuda(), gen((n,), 32).cuda() * 0.01, gen((n,), 33).cuda().abs() * 1e-4
    grads = [gen((k,), 40 + i).cuda() for i, k in enumerate(sizes)]
    flat_g = torch.cat(grads)
    pa, ma, va = p0.clone(), m0.clone(), v0.clone()
    pb, mb, vb = p0.clone(), m0.clone(), v0.clone()
    args = (0.9, 0.999, 1e-8, 1e-3 / (1 - 0.9 ** 3), (1 - 0.999 ** 3) ** 0.5)
    assert lib.upnerf_adam(n, ptr(pa), ptr(flat_g), ptr(ma), ptr(va), *args, None, None) == 0
    descs, off = [], 0
    for g in grads:
        descs.append(_lib.AdamDesc(g.data_ptr(), off, g.numel()))
        off += g.numel()
    arr = (_lib.AdamDesc * len(descs))(*descs)
    assert lib.upnerf_adam_gather(ptr(pb), ptr(mb), ptr(vb), arr, len(descs), *args, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa, p0)


def _ragged_tiles(hip, R, S, mode, use_cand, use_rgb):
    """f16x3 kernels against the fp32 kernels on shapes whose tiles are ragged (M % 64 != 0) and straddle up to three
    rays; large and tiny magnitudes mixed so that the per-tile exponents differ between tiles and stages."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=8, W=256, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    pk = model.packer
    o = (gen((R, 3), 70) * 0.3).cuda()
    d = torch.nn.functional.normalize(gen((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    scale = torch.logspace(-3, 2, R).reshape(R, 1)  # per-ray magnitudes of the side inputs span 5 decades
    c_rows, a_rows = (gen((R, 16), 73) * scale).cuda(), (gen((R, 48), 74) * scale.flip(0)).cuda()
    cfg = rd._PassCfg(pk, mode, use_cand, use_rgb, [1.0] * 10, [1.0] * 4)
    res = {}
    old = rd.FIELD_MODE
    try:
        for fm in ("f32", "f16x3"):
            rd.FIELD_MODE = fm
            leaves = [t.clone().requires_grad_(True) for t in (o, d, c_rows, a_rows, model.packed().detach())]
            outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
            sv = next(t.grad_fn for t in outs if t.grad_fn is not None).saved
            sink = {}
            rd._DEBUG_SINK = sink
            sum((t * gen(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel()).backward()
            rd._DEBUG_SINK = None
            res[fm] = dict(outs=[cpu(t) for t in outs], sv={k: cpu(v) for k, v in sv.items()
                                                              if torch.is_tensor(v) and v.dtype == torch.float32},
                           sink={k: cpu(v) for k, v in sink.items() if v is not None},
                           grads=[cpu(t.grad) if t.grad is not None else None for t in leaves])
    finally:
        rd.FIELD_MODE, rd._DEBUG_SINK = old, None
    a, b = res["f32"], res["f16x3"]
    bad = {}

    def chk(tag, x, y, tol):
        if x is None or x.numel() == 0:
            return
        e = rel_err(y.reshape(-1), x.reshape(-1))
        if not e < tol:
            bad[tag] = float(f"{e:.3g}")

    for k in ("x0", "h", "e", "g1", "g2", "r1", "sigma_s", "sigma_c", "rgb"):
        if k in a["sv"]:
            chk(k, a["sv"][k], b["sv"][k], 2e-6)
    for i, (x, y) in enumerate(zip(a["outs"], b["outs"])):
        chk(f"out{i}", x, y, 2e-6)
    # A pre-activation within rounding of zero can come out on different sides of the ReLU in the two arithmetics;
    # the gradient of that sample then legitimately differs.  Compare the per-sample gradients on all other samples.
    M = R * S
    flipped = torch.zeros(M, dtype=torch.bool)
    for k in ("h", "g1", "g2", "r1"):
        if k in a["sv"]:
            f = ((a["sv"][k] > 0) != (b["sv"][k] > 0)).reshape(-1, M, a["sv"][k].shape[-1]).any(-1).any(0)
            flipped |= f
    assert int(flipped.sum()) <= 2, f"{int(flipped.sum())} samples changed ReLU side"
    keep = (~flipped).float()
    for k in a["sink"]:
        x, y = a["sink"][k], b["sink"][k]
        w = keep.reshape(M, *([1] * (x.dim() - 1))) if x.shape[0] == M else keep.reshape(1, M, 1)
        chk("bwd_" + k, x * w, y * w, 2e-5)
    if not flipped.any():
        for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
            chk(f"grad{i}", x, y, 2e-5)
    assert not bad, bad


def test_frag16_layout_and_exponents(hip):
    """upnerf_frag16: hi + lo reproduces every matrix element to 2^-22 of the matrix maximum, at the documented byte
    offsets, with exponents that put the maximum in [2^13, 2^14)."""
    from upnerf_amd.packing import NerfPacker
    pk = NerfPacker(256, 8, [4], 63, 27, 384, 48, 16)
    L = pk.L
    P = (gen((L.total,), 61) * torch.logspace(-2, 1, L.total)).cuda()
    P16, PT16, wexp, _ = pk.frag16_hip(P)
    wexp = cpu(wexp)
    Pc = cpu(P)

    def unpack(buf, off, n, kp):
        raw = cpu(buf)[off:off + n * kp].view(torch.float16).view(n // 32, kp // 16, 2, 2, 32, 8)
        # [ntile][t][plane][khalf][lane][k%8] -> [plane][ntile*32 + lane][k]
        return raw.permute(2, 0, 4, 1, 3, 5).reshape(2, n, kp).float()

    W, W2 = 256, 128
    checks = [(P16, L.w[0], W, 64, Pc[L.w[0]:L.w[0] + W * 64].view(W, 64), 0),
              (P16, L.w[4], W, 320, Pc[L.w[4]:L.w[4] + W * 320].view(W, 320), 4),
              (P16, L.wr1, W2, 336, Pc[L.wr1:L.wr1 + W2 * 336].view(W2, 336), pk.EXP_R1),
              (PT16, L.t_we, W, W, Pc[L.we:L.we + W * W].view(W, W).t(), pk.EXP_FINAL),
              (PT16, L.t_skipx, 64, W, Pc[L.w[4]:L.w[4] + W * 320].view(W, 320)[:, :64].t(), 4),
              (PT16, L.t_head, W, W, torch.cat([Pc[L.wr1:L.wr1 + W2 * 336].view(W2, 336)[:, :W].t(),
                                               Pc[L.wc1:L.wc1 + W2 * 272].view(W2, 272)[:, :W].t()], 1), pk.EXP_HEAD_T)]
    for buf, off, n, kp, ref, eid in checks:
        hl = unpack(buf, off, n, kp)
        e = int(wexp[eid])
        got = (hl[0] + hl[1]) * 2.0 ** (-e)
        assert (got - ref).abs().max() <= ref.abs().max() * 2.0 ** -21, (off, eid)
        assert hl[0].abs().max() < 2 ** 14.01
    for eid, (off, n, kp) in {0: (L.w[0], W, 64), pk.EXP_FINAL: (L.we, W, W), pk.EXP_C2: (L.wc2, W2, W2)}.items():
        mx = float(Pc[off:off + n * kp].abs().max())
        assert 2 ** 13 <= mx * 2.0 ** int(wexp[eid]) < 2 ** 14


@pytest.mark.parametrize("W,D,cand,feat", [(256, 8, 16, True), (64, 4, 16, True), (256, 8, 0, True), (256, 8, 16, False),
                                           (64, 4, 16, False)])
def test_hip_pack_matches_torch_pack_forward_and_backward(hip, W, D, cand, feat):
    """NerfPacker.pack_hip (upnerf_pack + upnerf_linear, hand-written backward) against the torch restatement pack();
    feat = False: the module without feature layers (encode_feat = False: one pack launch, nothing to fold)."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    kw = dict(D=D, W=W, feat_dim=384 if feat else 0, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=cand)
    m = NeRF("coarse", c2f=None, encode_feat=feat, **kw)
    m.load_state_dict(synth.nerf_state("coarse", seed=4, encode_feat=feat, **kw))
    pk = m.packer
    ref_p = {n: t.detach().clone().requires_grad_(True) for n, t in m.named_parameters()}
    P_ref = pk.pack(ref_p)
    up = gen((pk.L.total,), 33)
    (P_ref * up).sum().backward()
    mg = m.cuda()
    gp = dict(mg.named_parameters())
    P = pk.pack_hip(gp)
    assert rel_err(cpu(P), P_ref.detach()) < 1e-6
    assert float((cpu(P) - P_ref.detach()).abs().max()) < 1e-5 * float(P_ref.detach().abs().max())
    (P * up.cuda()).sum().backward()
    for n in pk.pack_names():
        assert rel_err(cpu(gp[n].grad), ref_p[n].grad) < 2e-6, n
    if cand:  # not part of P: feat_candidate_layer / rgb_candidate_layer (projected per ray by the caller)
        assert gp["feat_candidate_layer.weight" if feat else "rgb_candidate_layer.weight"].grad is None


# ------------------------------------------------------------------------------------------ parameter re-layout
@pytest.mark.parametrize("W,D,skips", [pytest.param(256, 8, [4], id="256-8"), pytest.param(64, 4, [4], id="64-4"),
                                       pytest.param(256, 8, [], id="256-8-noskip"), pytest.param(256, 8, [1], id="256-8-skip1")])
def test_frag_copy_matches_torch_packing(hip, W, D, skips):
    from upnerf_amd.packing import NerfPacker
    pk = NerfPacker(W, D, skips, 63, 27, 384, 48, 16)
    P = gen((pk.L.total,), 60).cuda()
    assert torch.equal(pk.frag_hip(P), pk.frag(P))
    ref = pk.frag_t(pk.pack_t(P))
    got = pk.frag_t_hip(P)
    L = pk.L
    W2 = W // 2
    for off, n in [(L.t_w[l], (64 if l == 0 else W) * W) for l in range(D)] + [(L.t_we, W * W), (L.t_head, W * W),
                                                                              (L.t_wc2, W2 * W2)] + \
            ([(L.t_skipx, 64 * W)] if pk.skip >= 0 else []):
        assert torch.equal(got[off:off + n], ref[off:off + n])


# ------------------------------------------------------------------------------------------ a15 + a17
@pytest.mark.parametrize("m,fine,has_tw", [(0, True, True), (0.37, True, True), (1, True, False), (0.5, False, True),
                                           (0.5, True, False)])
def test_fused_loss_and_depth_prior(hip, m, fine, has_tw):
    from upnerf_amd.losses import UPNeRFLoss
    R, F = 517, 384
    res = {}
    for typ in ("coarse", "fine") if fine else ("coarse",):
        res[f"s_depth_{typ}"] = gen((R,), 70, 0.2, 4.0)
        if m < 1:
            res[f"feat_{typ}"] = gen((R, F), 71)
            if has_tw:
                res[f"t_weight_{typ}"] = gen((R,), 72, 0.0, 1.0)
        if m > 0:
            res[f"s_rgb_{typ}"] = gen((R, 3), 73, 0.0, 1.0)
    if m > 0 and fine:
        res["t_beta"], res["t_alpha"] = gen((R, 1), 74, 0.1, 1.0), gen((R, 1), 75, 0.0, 1.0)
    rgb, feat = gen((R, 3), 76, 0.0, 1.0), gen((R, F), 77)
    inv = 1.0 / gen((R,), 78, 0.05, 8.0)       # some rays hit the 1/far and the near clamps
    rows = gen((R, 2), 79) * 0.3
    wts = gen((8,), 80, 0.5, 1.5)

    def run(dev, direct):
        r = {k: v.clone().to(dev).requires_grad_(not k.startswith("t_weight")) for k, v in res.items()}
        rw = rows.clone().to(dev).requires_grad_(True)
        if dev == "cpu":
            depth = orc.depth_prior(rw, inv, 0.1, 5.0)
            out = orc.upnerf_loss(r, rgb, feat, depth, m, 1e-3, 1.0, fine)
        else:
            lf = UPNeRFLoss(depth_mult=1e-3, alpha_reg=1.0, fine=fine, near=0.1, far=5.0)
            if direct:
                depth = orc.depth_prior(rw.cpu(), inv, 0.1, 5.0).detach().cuda()
                out = lf(r, rgb.cuda(), feat.cuda(), depth, m)
            else:
                out, _ = lf.forward_with_prior(r, rgb.cuda(), feat.cuda(), inv.cuda(), rw, m)
        names = sorted(out)
        tot = sum(out[k] * wts[i].to(dev) for i, k in enumerate(names))
        tot.backward()
        return out, r, rw

    o_ref, r_ref, rw_ref = run("cpu", False)
    for direct in (False, True):
        o, r, rw = run("cuda", direct)
        assert list(o.keys()) == [k for k in ("l_depth_c", "l_feat_c", "l_rgb_c", "l_depth_f", "l_feat_f", "l_rgb_f",
                                              "l_beta", "l_alpha") if k in o_ref]
        for k in o_ref:
            assert abs(float(o[k]) - float(o_ref[k])) <= 2e-6 * max(1e-2, abs(float(o_ref[k]))), k
        for k in r_ref:
            if r_ref[k].grad is not None:
                assert rel_err(cpu(r[k].grad), r_ref[k].grad) < 1e-5, k
        if not direct:
            if rw_ref.grad is None:  # sched == 1: the depth target is not used by any term
                assert rw.grad is None or float(rw.grad.abs().max()) == 0.0
            else:
                assert rel_err(cpu(rw.grad), rw_ref.grad) < 1e-5


@pytest.mark.parametrize("m,fine", [(0, True), (0.5, True), (1, True), (0.5, False)])
def test_loss_total_comes_from_the_loss_launches_and_takes_its_gradient_there(hip, m, fine):
    """UPNeRFLoss.total(): the sum of the phase's terms written by upnerf_loss_fwd itself (term_mask / total), its gradient added
    to the masked terms' upstream gradients inside upnerf_loss_bwd (g_total) -- alone and together with a gradient that reaches
    a term through the dict."""
    from upnerf_amd.losses import UPNeRFLoss
    R, F = 301, 384
    res = {}
    for typ in ("coarse", "fine") if fine else ("coarse",):
        res[f"s_depth_{typ}"] = gen((R,), 70, 0.2, 4.0)
        if m < 1:
            res[f"feat_{typ}"] = gen((R, F), 71)
            res[f"t_weight_{typ}"] = gen((R,), 72, 0.0, 1.0)
        if m > 0:
            res[f"s_rgb_{typ}"] = gen((R, 3), 73, 0.0, 1.0)
    if m > 0 and fine:
        res["t_beta"], res["t_alpha"] = gen((R, 1), 74, 0.1, 1.0), gen((R, 1), 75, 0.0, 1.0)
    rgb, feat = gen((R, 3), 76, 0.0, 1.0), gen((R, F), 77)
    depth = gen((R,), 78, 0.2, 4.5)
    first = "l_depth_c" if m < 1 else "l_rgb_c"

    def run(dev, mixed):
        r = {k: v.clone().to(dev).requires_grad_(not k.startswith("t_weight")) for k, v in res.items()}
        if dev == "cpu":
            out = orc.upnerf_loss(r, rgb, feat, depth, m, 1e-3, 1.0, fine)
            total = sum(out.values())
        else:
            lf = UPNeRFLoss(depth_mult=1e-3, alpha_reg=1.0, fine=fine, near=0.1, far=5.0)
            out = lf(r, rgb.cuda(), feat.cuda(), depth.cuda(), m)
            total = lf.total()
        (total * 0.7 + out[first] * 0.3 if mixed else total).backward()
        return total.detach(), r

    for mixed in (False, True):
        t_ref, r_ref = run("cpu", mixed)
        t, r = run("cuda", mixed)
        assert abs(float(t) - float(t_ref)) <= 2e-6 * max(1e-2, abs(float(t_ref)))
        for k in r_ref:
            if r_ref[k].grad is not None:
                assert rel_err(cpu(r[k].grad), r_ref[k].grad) < 1e-5, (k, mixed)


# ------------------------------------------------------------------------------------------ a18
def test_flat_adam_follows_torch_adam_including_skipped_parameters():
    from upnerf_amd.optim import FlatAdam
    torch.manual_seed(0)
    shapes = [(17, 5), (33,), (8, 8), (1,), (64, 3)]
    ref = [torch.nn.Parameter(gen(s, 90 + i)) for i, s in enumerate(shapes)]
    mine = [torch.nn.Parameter(p.detach().clone().cuda()) for p in ref]
    o_ref = torch.optim.Adam(ref, lr=5e-4, eps=1e-8)
    o_me = FlatAdam(mine, lr=5e-4, eps=1e-8)
    s_ref = torch.optim.lr_scheduler.ExponentialLR(o_ref, gamma=0.9)
    s_me = torch.optim.lr_scheduler.ExponentialLR(o_me, gamma=0.9)
    live_sets = [[0, 1, 2, 3, 4], [0, 1, 4], [0, 1, 4], [0, 1, 2, 3, 4], [2, 3], [0, 1, 2, 3, 4]]
    for step, live in enumerate(live_sets):
        for i in range(len(shapes)):
            g = gen(shapes[i], 200 + 10 * step + i) if i in live else None
            ref[i].grad = None if g is None else g.clone()
            mine[i].grad = None if g is None else g.cuda()
        o_ref.step(); s_ref.step()
        o_me.step(); s_me.step()
        for a, b in zip(mine, ref):
            assert rel_err(cpu(a), b.detach()) < 2e-6
    sd = o_me.state_dict()
    assert int(sd["state"][2]["step"]) == 4 and int(sd["state"][0]["step"]) == 5
    assert rel_err(sd["state"][4]["exp_avg"].cpu(), o_ref.state_dict()["state"][4]["exp_avg"]) < 2e-6


def test_keyed_uniform_draws_follow_the_philox_spec_and_the_global_row(hip):
    """upnerf_uniform_keyed: values = Philox4x32-10(counter (row0 + r, c / 4, step, draw), key seed) >> 8 scaled by 2^-24
    (the numpy restatement: tests/prologue_ref.py, held to the published known answers by tests/test_prologue_ref_cpu.py);
    a batch drawn in two halves with their global row offsets equals the batch drawn at once (rank-count invariance,
    SURVEY.md 8e); the step can come from device memory (graph replay)."""
    import numpy as np
    lib, ptr, stream, check = hip["lib"].lib, hip["lib"].ptr, hip["lib"].stream, hip["lib"].check
    R, n, seed, step, draw = 37, 90, 0x1234567890ABCDEF, 4711, 2
    out = torch.empty(R, n, device="cuda")
    check(lib.upnerf_uniform_keyed(R, n, seed, step, None, 100, 1, draw, ptr(out), stream()), "uniform")
    ref = philox_uniform(seed, step, 100 + np.arange(R), n, draw)
    assert ref.dtype == np.float32 and ref.shape == (R, n)
    assert np.array_equal(cpu(out).numpy(), ref)
    assert 0.0 <= float(out.min()) and float(out.max()) < 1.0 and abs(float(out.mean()) - 0.5) < 0.03
    a, b = torch.empty(20, n, device="cuda"), torch.empty(17, n, device="cuda")
    step_dev = torch.tensor([float(step)], device="cuda")
    check(lib.upnerf_uniform_keyed(20, n, seed, 0, ptr(step_dev), 100, 1, draw, ptr(a), stream()), "uniform")
    check(lib.upnerf_uniform_keyed(17, n, seed, 0, ptr(step_dev), 120, 1, draw, ptr(b), stream()), "uniform")
    assert torch.equal(torch.cat([a, b]), out)
    # shards dealt like DistributedSampler (local ray r of rank k = global ray r * world + k): stride = world
    c0, c1 = torch.empty(19, n, device="cuda"), torch.empty(18, n, device="cuda")
    check(lib.upnerf_uniform_keyed(19, n, seed, 0, ptr(step_dev), 100, 2, draw, ptr(c0), stream()), "uniform")
    check(lib.upnerf_uniform_keyed(18, n, seed, 0, ptr(step_dev), 101, 2, draw, ptr(c1), stream()), "uniform")
    assert torch.equal(c0, out[0::2]) and torch.equal(c1, out[1::2])


def test_two_virtual_ranks_draw_what_one_rank_draws(hip):
    """NeRFSystem passes render_rays the key (seed, step, global row): the sampled depths of a 256-ray batch rendered at once
    equal, bit for bit, those of its two 128-ray halves rendered as ranks 0 and 1 would (rows 0.. and 128..)."""
    from upnerf_amd import synth
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset, default_hparams
    hp = default_hparams(**{"nerf.N_samples": 32, "nerf.N_importance": 32, "train.batch_size": 256, "max_steps": 100, "seed": 11})
    torch.manual_seed(0)
    s = NeRFSystem(hp, SyntheticDataset(5))
    s.setup()
    s.cuda()
    s.global_step = 60
    s.set_progress(0.3)
    batch = {k: v.cuda() for k, v in synth.batch(256, 5, seed=3).items()}

    def depths(b, row0, stride=1):
        s._rng_row0, s._rng_stride = row0, stride
        keep = {}
        with torch.no_grad():
            rays = s.rays_from_batch(b)
            s(rays, b["feats"], b["img_idx"], s.get_schedule_mult(s._host_progress), keep=keep)
        return keep["z_coarse"].clone(), keep["z_fine"].clone()

    zc, zf = depths(batch, 0)
    halves = [depths({k: v[lo:lo + 128] for k, v in batch.items()}, lo) for lo in (0, 128)]
    assert torch.equal(zc, torch.cat([h[0] for h in halves])) and torch.equal(zf, torch.cat([h[1] for h in halves]))
    # the layout the ray sampler actually produces (ray_sampler.py: perm[rank::world]): rank k holds global rays k, k + 2, ...
    for k in (0, 1):
        zk = depths({kk: v[k::2].contiguous() for kk, v in batch.items()}, k, 2)
        assert torch.equal(zk[0], zc[k::2]) and torch.equal(zk[1], zf[k::2])
    # ... and at the rank count of BASELINE.json configs[2]: eight virtual ranks, the sampler's strided layout
    for k in range(8):
        zk = depths({kk: v[k::8].contiguous() for kk, v in batch.items()}, k, 8)
        assert torch.equal(zk[0], zc[k::8]) and torch.equal(zk[1], zf[k::8]), k
    s.global_step = 62  # another step: other numbers
    zc2, _ = depths(batch, 0)
    assert not torch.equal(zc, zc2)


PLAN_CASES = ([(256, 8, R, S, fm) for R, S in ((5, 33), (3, 257)) for fm in ("f16x3", "f32", "f16")]
              + [(64, 4, 5, 33, fm) for fm in ("f16x3", "f32")])  # (64-wide fields: the f16 mode refuses them)


@pytest.mark.parametrize("W,D,R,S,field_mode", PLAN_CASES, indirect=["field_mode"])
def test_field_pass_holds_exactly_what_its_plan_lists(hip, W, D, R, S, field_mode):
    """Forward, backward and plan are one description: every buffer the plan lists is held with the planned shape and dtype on
    storage of at least the planned rows, every form the plan omits is None.  Compared on the allocated tensors."""
    from upnerf_amd import synth
    from upnerf_amd.nerf import NeRF
    rd = hip["rendering"]
    kw = dict(D=D, W=W, feat_dim=384, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    model = NeRF("coarse", c2f=None, **kw)
    model.load_state_dict(synth.nerf_state("coarse", seed=3, **kw))
    model = model.cuda()
    o, d = (gen((R, 3), 70) * 0.3).cuda(), torch.nn.functional.normalize(gen((R, 3), 71), dim=-1).cuda()
    z = (torch.sort(gen((R, S), 72).abs() * 3 + 0.1, dim=-1).values).cuda()
    c_rows, a_rows = gen((R, 16), 73).cuda(), gen((R, 48), 74).cuda()

    def held(plan, got, names):
        pp = hip["pass_plan"]
        for k in names:
            shape, t = plan.buffers[k], got[k]
            if shape is None:
                assert t is None, k
                continue
            assert tuple(t.shape) == shape and t.dtype == getattr(torch, pp.DTYPES.get(k, "float32")), (k, tuple(t.shape), t.dtype)
            # the rows the plan allocates: Mp behind the visible ones of the tensors the kernels write in whole tiles
            numel = int(np.prod((plan.Mp,) + shape[1:] if k in pp.PADDED else shape))
            assert t.untyped_storage().nbytes() >= numel * t.element_size(), (k, shape, plan.Mp)

    for mode, use_cand, use_rgb in ((1, True, True), (0, True, False), (2, False, True), (3, False, False)):
        cfg = rd._PassCfg(model.packer, mode, use_cand, use_rgb, [1.0] * 10, [1.0] * 4)
        leaves = [t.clone().requires_grad_(True) for t in (o, d, c_rows, a_rows, model.packed().detach())]
        outs = rd._FieldPass.apply(leaves[0], leaves[1], z, leaves[2], leaves[3], leaves[4], cfg)
        node = next(t.grad_fn for t in outs if t.grad_fn is not None)
        plan, stages = node.plan, hip["pass_plan"].STAGES
        assert plan == rd._plan(model.packer, R, S, mode, use_cand, use_rgb, False, True) and node.rr == plan.rr
        held(plan, node.saved, stages["aux"] + stages["field"] + ("w_all", "w_sj", "w_cj", "w_s"))
        names = ("E_s", "G_c", "sum_sfeat", "t_weight", "c_depth", "s_depth", "rgb_map", "w_all", "w_s", "rgb_joint_map")
        held(plan, {k: (t if t.numel() else None) for k, t in zip(names, outs)}, names)
        sink = {}
        rd._DEBUG_SINK = sink
        try:
            sum((t * gen(tuple(t.shape), 80 + i).cuda()).sum() for i, t in enumerate(outs) if t.numel()).backward()
        finally:
            rd._DEBUG_SINK = None
        held(plan, node.bwd_buffers, sum((stages[s] for s in ("cbwd", "fbwd", "part", "sums")), ()))
        M = R * S
        rows = dict(gz_h=(D, M, W), gz_e=(M, W), gz_g1=(M, W // 2) if use_cand else None, gz_g2=(M, W // 2) if use_cand else None,
                    gz_r1=(M, W // 2) if use_rgb else None)
        for k, shape in rows.items():  # ... and whatever the form, the sink shows fp32 rows of the visible samples
            assert (sink[k] is None) if shape is None else (tuple(sink[k].shape) == shape and sink[k].dtype == torch.float32), k
        assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in (leaves[0], leaves[1], leaves[4]))
