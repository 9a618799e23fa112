"""The training step's glue kernels -- upnerf_pack in both directions, upnerf_add_pairs (and ops.fanout over it), upnerf_zero,
upnerf_adam_gather, upnerf_set_scalars, upnerf_scale_exponents -- through the C ABI at their edges, against the restatements and
case tables of tests/glue_ref.py (shown sound on the CPU by tests/test_glue_ref_cpu.py).

Every comparison is bit for bit (torch.equal on the data viewed as int32) except two: Adam against fp64 uses the bound
tests/dense_ref.py derives for upnerf_adam (4 e32 + 2^-22 scale; the gather kernel itself is held bitwise to the flat one), and
upnerf_scale_exponents may answer e* + 1 in the band 2^(k-1) < v <= 2^(k-1) (1 + 2^-14) that fp32 log2f cannot resolve
(glue_ref's docstring).  Destinations start as glue_ref.CANARY, a NaN pattern no input holds, with glue_ref.GUARD words of it on
both sides of every used range: a word written outside the described elements is a lost canary.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dense_ref as dr
import glue_ref as gr

pytestmark = pytest.mark.gpu

G = gr.GUARD
CAN = int(gr.canary(1)[0])


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib, ops
    return dict(L=_lib, lib=_lib.lib, ops=ops)


def dev(a):
    """int32 numpy words -> int32 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cpu(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def same(got, want):
    """Bit for bit: device tensor (any 32-bit dtype) against int32 numpy words."""
    return torch.equal(cpu(got).view(torch.int32).reshape(-1), torch.from_numpy(np.ascontiguousarray(want)).reshape(-1))


class Arena:
    """The parameters of a descriptor set inside ONE device buffer, GUARD words in front of, between and behind them."""

    def __init__(self, descs, fills):
        self.off, off = [], G
        for d in descs:
            self.off.append(off)
            off += gr.src_words(d) + G
        self.host = gr.canary(off)
        for o, f in zip(self.off, fills):
            self.host[o:o + f.size] = f
        self.dev = dev(self.host)

    def ptr(self, j):
        return self.dev.data_ptr() + 4 * self.off[j]

    def parts(self, host, descs):
        return [host[o:o + gr.src_words(d)] for o, d in zip(self.off, descs)]


def pack_call(hip, P, descs, arena, unpack, n=None):
    L = hip["L"]
    ds = [L.PackDesc(ptr=arena.ptr(j), rows=d.rows, cols=d.cols, src_ld=d.src_ld, dst_off=d.dst_off, dst_ld=d.dst_ld,
                     accumulate=d.accumulate) for j, d in enumerate(descs)]
    arr = (L.PackDesc * len(ds))(*ds)
    return L.lib.upnerf_pack(P.data_ptr() + 4 * G, arr, len(ds) if n is None else n, unpack, None)


# ========================================================================================================== 1. upnerf_pack, pack
@pytest.mark.parametrize("name", list(gr.PACK_TABLES))
def test_pack_moves_words_and_nothing_else(hip, name):
    """Raw int32 patterns (NaNs with payloads, +-0, denormals, +-inf, 0x80000001: what GraphedTrainingStep._stage_batch sends) land
    on the described elements bit for bit; padding columns, gaps and guards keep the canary; the sources are not written."""
    descs, used = gr.layout(gr.PACK_TABLES[name])
    srcs = [gr.words(gr.src_words(d), 100 + j) for j, d in enumerate(descs)]
    arena = Arena(descs, srcs)
    P0 = gr.canary(used + 2 * G)
    P = dev(P0)
    assert pack_call(hip, P, descs, arena, 0) == 0
    want = gr.pack(P0, descs, srcs, base=G)
    assert same(P, want)
    assert int((cpu(P) != CAN).sum()) == int(gr.starts(descs)[-1])  # (the check above, said in canaries)
    assert same(arena.dev, arena.host)


def test_pack_refuses_49_descriptors_and_writes_nothing(hip):
    descs, used = gr.layout([(1, 1, 1, 1)] * (gr.MAX_PACK_DESC + 1))
    srcs = [gr.words(1, 200 + j) for j in range(len(descs))]
    arena = Arena(descs, srcs)
    for unpack in (0, 1):
        P = dev(gr.canary(used + 2 * G))
        assert pack_call(hip, P, descs, arena, unpack) == -1
        assert pack_call(hip, P, descs, arena, unpack, n=0) == -1
        assert same(P, gr.canary(used + 2 * G)) and same(arena.dev, arena.host)
    P = dev(gr.canary(used + 2 * G))
    assert pack_call(hip, P, descs[:-1], arena, 0) == 0  # 48 of the same are taken
    assert int((cpu(P) != CAN).sum()) == gr.MAX_PACK_DESC


@pytest.mark.parametrize("flags", [[1, 1, 1, 1, 1], [1, 0, 1, 0, 1], [0, 1, 0, 1, 0]])
def test_pack_accumulates_onto_what_the_destination_holds(hip, flags):
    """accumulate = 1 onto a non-zero finite destination is the fp32 P + src that torch computes, flags mixed within one launch
    over disjoint destinations; everything else of P keeps its bits."""
    descs, used = gr.layout(gr.PACK_TABLES["strided"], flags=flags)
    srcs = [gr.finite(gr.src_words(d), 300 + j) for j, d in enumerate(descs)]
    arena = Arena(descs, srcs)
    P0 = np.concatenate([gr.canary(G), gr.finite(used, 310), gr.canary(G)])
    P = dev(P0)
    assert pack_call(hip, P, descs, arena, 0) == 0
    want = torch.from_numpy(P0.copy())
    for d, s in zip(descs, srcs):  # torch's own strided views and fp32 addition
        view = torch.as_strided(want.view(torch.float32), (d.rows, d.cols), (d.dst_ld, 1), G + d.dst_off)
        x = torch.from_numpy(s.copy()).view(torch.float32).as_strided((d.rows, d.cols), (d.src_ld, 1))
        if d.accumulate:
            view += x
        else:
            view[:] = x
    assert same(P, want.numpy())
    assert same(P, gr.pack(P0, descs, srcs, base=G))
    assert not same(P, P0)


# ======================================================================================================== 2. upnerf_pack, unpack
@pytest.mark.parametrize("name", list(gr.PACK_TABLES))
def test_unpack_moves_words_and_leaves_the_padding(hip, name):
    descs, used = gr.layout(gr.PACK_TABLES[name])
    P0 = np.concatenate([gr.canary(G), gr.words(used, 400), gr.canary(G)])
    P = dev(P0)
    arena = Arena(descs, [gr.canary(gr.src_words(d)) for d in descs])
    assert pack_call(hip, P, descs, arena, 1) == 0
    want = gr.unpack(P0, descs, arena.parts(arena.host, descs), base=G)
    got = cpu(arena.dev).numpy()
    for d, g, w in zip(descs, arena.parts(got, descs), want):
        assert np.array_equal(g, w)
        assert int((g != CAN).sum()) == d.rows * d.cols  # src_ld > cols: the padding is untouched
    assert int((got != CAN).sum()) == int(gr.starts(descs)[-1])  # guards between the parameters
    assert same(P, P0)


@pytest.mark.parametrize("name", list(gr.PACK_TABLES))
def test_unpack_of_pack_is_the_identity(hip, name):
    descs, used = gr.layout(gr.PACK_TABLES[name])
    srcs = [gr.words(gr.src_words(d), 500 + j) for j, d in enumerate(descs)]
    a, b = Arena(descs, srcs), Arena(descs, [gr.canary(gr.src_words(d)) for d in descs])
    P = dev(gr.canary(used + 2 * G))
    assert pack_call(hip, P, descs, a, 0) == 0 and pack_call(hip, P, descs, b, 1) == 0
    for d, s, t in zip(descs, srcs, b.parts(cpu(b.dev).numpy(), descs)):
        idx = gr.src_index(d)
        assert np.array_equal(t[idx], s[idx]) and int((t != CAN).sum()) == idx.size


def _counting(monkeypatch, lib, name):
    calls, real = [], getattr(lib, name)

    def counted(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(lib, name, counted)
    return calls


def test_gather_and_scatter_of_the_gradient_exchange(hip, monkeypatch):
    """parallel._gather with 97 tensors (launches of 48, 48 and 1 descriptors) and two empty ones, the views leaving gaps in
    `flat`, against torch._foreach_copy_; then the scatter back."""
    from upnerf_amd import parallel
    sizes = [1 + (37 * i) % 301 for i in range(97)]
    sizes[3], sizes[50], sizes[96] = 256, 1025, 513
    sizes[10:10] = [0]
    sizes[70:70] = [0]
    tensors = [dev(gr.words(n, 600 + i)).view(torch.float32) for i, n in enumerate(sizes)]
    offs, off = [], G
    for i, n in enumerate(sizes):
        off += i % 3  # gaps
        offs.append(off)
        off += n
    flat = dev(gr.canary(off + G)).view(torch.float32)
    ref = flat.clone()
    views = [flat[o:o + n] for o, n in zip(offs, sizes)]
    calls = _counting(monkeypatch, hip["lib"], "upnerf_pack")
    parallel._gather(flat, views, tensors)
    assert [c[2] for c in calls] == [48, 48, 1] and all(c[3] == 0 for c in calls)
    torch._foreach_copy_([ref[o:o + n] for o, n in zip(offs, sizes)], tensors)
    assert torch.equal(cpu(flat).view(torch.int32), cpu(ref).view(torch.int32))
    assert int((cpu(flat).view(torch.int32) != CAN).sum()) == sum(sizes)
    # scatter: new words in flat go back to the tensors
    flat2 = dev(gr.words(flat.numel(), 700)).view(torch.float32)
    views2 = [flat2[o:o + n] for o, n in zip(offs, sizes)]
    outs = [dev(gr.canary(n)).view(torch.float32) for n in sizes]
    del calls[:]
    parallel._gather(flat2, views2, outs, scatter=True)
    assert [c[2] for c in calls] == [48, 48, 1] and all(c[3] == 1 for c in calls)
    want = [dev(gr.canary(n)).view(torch.float32) for n in sizes]
    torch._foreach_copy_(want, views2)
    for o, w in zip(outs, want):
        assert torch.equal(cpu(o).view(torch.int32), cpu(w).view(torch.int32))
    assert same(flat2, gr.words(flat.numel(), 700))


def test_stage_batch_moves_int64_and_int32_tensors_as_words(hip, monkeypatch):
    """GraphedTrainingStep._stage_batch: the batch reaches the static input buffers by ONE upnerf_pack launch, 64-bit indices
    and 32-bit integers as whole words; the padding between the pieces of the flat buffer is not written."""
    from upnerf_amd.graph_step import GraphedTrainingStep
    g = object.__new__(GraphedTrainingStep)
    g.device, g.static, g._static_flat = torch.device("cuda"), {}, {}
    R = 37
    batch = {"img_idx": torch.from_numpy(gr.words(2 * R, 800).copy()).view(torch.int64).cuda(),
             "ray_infos": dev(gr.words(3 * R, 801)).view(R, 3),
             "rgbs": dev(gr.words(3 * R, 802)).view(torch.float32).view(R, 3)}
    static = g._static_batch(batch)
    flat = g._static_flat[R][0]
    flat.view(torch.int32).fill_(CAN)
    calls = _counting(monkeypatch, hip["lib"], "upnerf_pack")
    g._stage_batch(batch, static)
    assert len(calls) == 1 and calls[0][2] == 3
    for k, t in static.items():
        assert t.dtype == batch[k].dtype and t.shape == batch[k].shape
        assert torch.equal(cpu(t).reshape(-1).view(torch.int32), cpu(batch[k]).reshape(-1).view(torch.int32)), k
    assert int((cpu(flat).view(torch.int32) != CAN).sum()) == 2 * R + 3 * R + 3 * R


# ========================================================================================================== 3. upnerf_add_pairs
def add_call(hip, triples):
    L = hip["L"]
    ps = [L.AddPair(a=a, b=b, out=o, n=n) for a, b, o, n in triples]
    return L.lib.upnerf_add_pairs((L.AddPair * len(ps))(*ps), len(ps), None)


@pytest.mark.parametrize("alias", ["none", "a", "b"])
@pytest.mark.parametrize("sizes", [(257,), gr.ADD_SIZES, (1, 255, 256, 257, 70001, 3, 1, 513)], ids=["1", "5", "8"])
def test_add_pairs_is_torchs_sum(hip, sizes, alias):
    """out_j = a_j + b_j with +-inf, NaN, a pair summing to -0 and denormals among the inputs: the bits of torch's a + b on the same
    device (and, where the sum is no NaN, of the CPU's); `out` may alias a or b; a canary stands behind (and before) every out."""
    A = [dev(np.concatenate([gr.canary(G), gr.add_inputs(n, 900 + 2 * j)[0], gr.canary(G)])) for j, n in enumerate(sizes)]
    B = [dev(np.concatenate([gr.canary(G), gr.add_inputs(n, 900 + 2 * j)[1], gr.canary(G)])) for j, n in enumerate(sizes)]
    O = [dev(gr.canary(n + 2 * G)) for n in sizes]
    want = [(a.view(torch.float32)[G:G + n] + b.view(torch.float32)[G:G + n]).view(torch.int32) for a, b, n in zip(A, B, sizes)]
    host = gr.add_pairs(*zip(*[gr.add_inputs(n, 900 + 2 * j) for j, n in enumerate(sizes)]))
    out = {"none": O, "a": A, "b": B}[alias]
    a0, b0 = [cpu(t).clone() for t in A], [cpu(t).clone() for t in B]
    assert add_call(hip, [(a.data_ptr() + 4 * G, b.data_ptr() + 4 * G, o.data_ptr() + 4 * G, n)
                          for a, b, o, n in zip(A, B, out, sizes)]) == 0
    for j, n in enumerate(sizes):
        got = cpu(out[j])
        assert torch.equal(got[G:G + n], cpu(want[j])), (j, n)
        nan = np.isnan(host[j].view(np.float32))
        assert np.array_equal(got[G:G + n].numpy()[~nan], host[j][~nan]) and bool(torch.isnan(got[G:G + n].view(torch.float32))[torch.from_numpy(nan)].all())
        assert bool((got[:G] == CAN).all()) and bool((got[G + n:] == CAN).all())
        if alias != "a":
            assert torch.equal(cpu(A[j]), a0[j])
        if alias != "b":
            assert torch.equal(cpu(B[j]), b0[j])


def test_add_pairs_refuses_nine_pairs_and_writes_nothing(hip):
    a, b = dev(gr.finite(9, 950)), dev(gr.finite(9, 951))
    o = dev(gr.canary(9))
    triples = [(a.data_ptr() + 4 * j, b.data_ptr() + 4 * j, o.data_ptr() + 4 * j, 1) for j in range(9)]
    assert add_call(hip, triples) == -1
    assert same(o, gr.canary(9))
    assert add_call(hip, triples[:8]) == 0
    assert int((cpu(o) != CAN).sum()) == 8


# ================================================================================================================ 4. ops.fanout
def _fan_graph(ops, xs, ws, fan, seen):
    """Consumer A reads x through .t() (its gradient arrives transposed), consumer B through .sum() (its gradient arrives
    expanded) for the first three tensors; the last one gets contiguous gradients."""
    old = ops.ENABLE_FANOUT
    ops.ENABLE_FANOUT = fan
    try:
        xs = [x.detach().clone().requires_grad_(True) for x in xs]
        A, B = ops.fanout(*xs)
        loss = 0
        for j, (a, b, w) in enumerate(zip(A, B, ws)):
            if fan:
                a.register_hook(lambda g, j=j: seen.append((j, g.is_contiguous())))
                b.register_hook(lambda g, j=j: seen.append((j, g.is_contiguous())))
            if j < 3:  # (a contiguous (48, 64) factor: the gradient of a.t() is contiguous, so the gradient of a is its transpose)
                loss = loss + (a.t() * w.t().contiguous()).sum() + b.sum() * (j + 2.0)
            else:
                loss = loss + (a * w).sum() + (b * b * w).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.ENABLE_FANOUT = old
    return [x.grad for x in xs]


def test_fanout_with_non_contiguous_first_gradients(hip, monkeypatch):
    """Four same-shape tensors whose first three pairs of gradients arrive non-contiguous (transposed, expanded): backward makes
    .contiguous() copies of them, and every copy has to live until the one upnerf_add_pairs launch has been enqueued -- a copy
    freed earlier hands its block to a later pair's copy, which overwrites it before the sum reads it.  The gradients are those of
    the same graph without fanout (ops.ENABLE_FANOUT off), bit for bit."""
    ops = hip["ops"]
    xs = [dr.flat((64, 48), 1000 + j).cuda() for j in range(4)]
    ws = [dr.flat((64, 48), 1010 + j).cuda() for j in range(4)]
    seen = []
    want = _fan_graph(ops, xs, ws, False, seen)
    calls = _counting(monkeypatch, ops.lib, "upnerf_add_pairs")
    got = _fan_graph(ops, xs, ws, True, seen)
    assert [c[1] for c in calls] == [4]
    assert sorted(seen) == [(0, False)] * 2 + [(1, False)] * 2 + [(2, False)] * 2 + [(3, True)] * 2  # what arrived at the pairs
    for j, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), j


def test_fanout_with_more_tensors_than_one_launch_takes(hip, monkeypatch):
    ops = hip["ops"]
    n = gr.MAX_ADD_PAIRS + 3
    xs = [dr.flat((5 + j, 31), 1100 + j).cuda() for j in range(n)]
    ws = [dr.flat((5 + j, 31), 1120 + j).cuda() for j in range(n)]

    def run(fan):
        old = ops.ENABLE_FANOUT
        ops.ENABLE_FANOUT = fan
        try:
            ys = [x.detach().clone().requires_grad_(True) for x in xs]
            A, B = ops.fanout(*ys)
            sum((a * w).sum() + (b * b * w).sum() for a, b, w in zip(A, B, ws)).backward()
            torch.cuda.synchronize()
        finally:
            ops.ENABLE_FANOUT = old
        return [y.grad for y in ys]

    want = run(False)
    calls = _counting(monkeypatch, ops.lib, "upnerf_add_pairs")
    got = run(True)
    assert [c[1] for c in calls] == [gr.MAX_ADD_PAIRS, 3]
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_fanout_falls_back_for_other_types_and_mismatched_shapes(hip, monkeypatch):
    """fp64 and fp16 tensors, and a pair whose two gradients differ in shape (one consumer's gradient is a broadcastable (1, n)
    row), are added by torch; the fp32 pair beside them still goes through the launch."""
    ops = hip["ops"]
    x32 = dr.flat((7, 9), 1200).cuda().requires_grad_(True)
    x64 = dr.flat((7, 9), 1201).double().cuda().requires_grad_(True)
    x16 = dr.flat((7, 9), 1202).half().cuda().requires_grad_(True)
    calls = _counting(monkeypatch, ops.lib, "upnerf_add_pairs")
    A, B = ops.fanout(x32, x64, x16)
    sum((a * 3).sum() + (b * b).sum() for a, b in zip(A, B)).backward()
    assert [c[1] for c in calls] == [1]
    for x in (x32, x64, x16):
        assert x.grad.dtype == x.dtype and torch.equal(x.grad, 3 + 2 * x.detach())
    # mismatched shapes, straight through the Function (autograd itself never hands it such a pair)
    ga, gb = dr.flat((4, 6), 1210).cuda(), dr.flat((1, 6), 1211).cuda()
    del calls[:]
    out = ops._Fanout.backward(None, ga, gb)
    assert not calls and torch.equal(out[0], ga + gb)
    out = ops._Fanout.backward(None, ga, None, None, gb)
    assert out[0] is ga and out[1] is gb


# =============================================================================================================== 5. upnerf_zero
@pytest.mark.parametrize("n", gr.ZERO_SIZES)
def test_zero_fills_its_range_and_nothing_else(hip, n):
    """n floats of +0 at a 16-byte-aligned offset inside a larger buffer: the n & 3 tail, n < 4, a launch at the 4096-workgroup
    cap and one past it (a second trip of the grid-stride loop)."""
    lib = hip["lib"]
    buf = torch.full((G + n + G,), CAN, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (4 * G) % 16 == 0
    assert lib.upnerf_zero(buf.data_ptr() + 4 * G, n, None) == 0
    torch.cuda.synchronize()
    assert bool((buf[:G] == CAN).all()) and bool((buf[G + n:] == CAN).all())
    assert int(torch.count_nonzero(buf[G:G + n])) == 0


def test_zero_refuses_a_misaligned_pointer_and_an_empty_range(hip):
    lib = hip["lib"]
    buf = torch.full((2 * G + 64,), CAN, dtype=torch.int32, device="cuda")
    for off in (4, 8, 12):
        assert lib.upnerf_zero(buf.data_ptr() + 4 * G + off, 8, None) == -1
    assert lib.upnerf_zero(buf.data_ptr() + 4 * G, 0, None) == -1
    assert lib.upnerf_zero(buf.data_ptr() + 4 * G, -4, None) == -1
    assert lib.upnerf_zero(None, 4, None) == -1
    assert same(buf, gr.canary(2 * G + 64))


# ======================================================================================================== 6. upnerf_adam_gather
B1, B2, EPS = 0.9, 0.999, 1e-8


def _adam_state(used, seed):
    return dr.flat((used,), seed), dr.flat((used,), seed + 1) * 1e-3, dr.flat((used,), seed + 2).abs() * 1e-5


def _gather_call(hip, state, pieces, ss, bc2, dyn2=None):
    """pieces: (offset, device gradient tensor, element offset of the gradient inside its tensor)."""
    L = hip["L"]
    ds = [L.AdamDesc(g=g.data_ptr() + 4 * go, off=off, n=n) for off, g, go, n in pieces]
    arr = (L.AdamDesc * len(ds))(*ds)
    return L.lib.upnerf_adam_gather(state[0].data_ptr(), state[1].data_ptr(), state[2].data_ptr(), arr, len(ds), B1, B2, EPS, ss, bc2,
                                    None if dyn2 is None else dyn2.data_ptr(), None)


def _flat_call(hip, state, g, ss, bc2, dyn2=None):
    return hip["lib"].upnerf_adam(g.numel(), state[0].data_ptr(), g.data_ptr(), state[1].data_ptr(), state[2].data_ptr(), B1, B2, EPS,
                                  ss, bc2, None if dyn2 is None else dyn2.data_ptr(), None)


@pytest.mark.parametrize("step", [1, 1000])
def test_adam_gather_at_its_edges(hip, step):
    """Pieces of 1, 1023, 1024, 1025 and 4097 elements and the planted table of dense_ref (its overflow rows included), listed out
    of offset order, with gaps between them and gradient pointers that are 4- but not 16-byte aligned: bitwise the flat kernel
    on the gathered gradients, p / m / v in the gaps bit for bit as they were, and the flat kernel inside dense_ref's Adam bound
    against fp64 (4 e32 + 2^-22 scale; where (1 - beta2) g g overflows fp32 the outcome is the fp32 formula's)."""
    tp, tg, tm, tv = dr.adam_table(step)
    sizes = list(gr.ADAM_PIECES) + [tp.numel()]
    offs, used = gr.adam_layout(sizes)
    p, m, v = _adam_state(used, 1300)
    t = slice(offs[-1], offs[-1] + tp.numel())
    p[t], m[t], v[t] = tp, tm, tv
    gs = [dr.flat((n,), 1310 + j) * 1e-2 for j, n in enumerate(sizes[:-1])] + [tg]
    ss, bc2 = dr.adam_bias_scalars(1e-3, B1, B2, step)
    mask, g_flat = torch.zeros(used, dtype=torch.bool), torch.zeros(used)
    for o, g in zip(offs, gs):
        mask[o:o + g.numel()] = True
        g_flat[o:o + g.numel()] = g
    # every gradient one float behind a 16-byte boundary of its own allocation
    g_dev = [torch.cat([torch.zeros(1 + j % 3), g]).cuda() for j, g in enumerate(gs)]
    assert all((gd.data_ptr() + 4 * (1 + j % 3)) % 16 for j, gd in enumerate(g_dev))
    order = [3, 5, 0, 4, 1, 2]
    pieces = [(offs[j], g_dev[j], 1 + j % 3, sizes[j]) for j in order]
    a = [x.clone().cuda() for x in (p, m, v)]
    b = [x.clone().cuda() for x in (p, m, v)]
    assert _gather_call(hip, a, pieces, ss, bc2) == 0
    assert _flat_call(hip, b, g_flat.cuda(), ss, bc2) == 0
    got, flat = [cpu(x) for x in a], [cpu(x) for x in b]
    for x, f, x0 in zip(got, flat, (p, m, v)):
        assert torch.equal(x[mask].view(torch.int32), f[mask].view(torch.int32))
        assert torch.equal(x[~mask].view(torch.int32), x0[~mask].view(torch.int32))
    for gd, g, j in zip(g_dev, gs, range(len(gs))):
        assert torch.equal(cpu(gd)[1 + j % 3:], g)
    r32 = dr.adam_formula(p, g_flat, m, v, B1, B2, EPS, ss, bc2, torch.float32)
    r64 = dr.adam_formula(p, g_flat, m, v, B1, B2, EPS, ss, bc2, torch.float64)
    over = torch.isinf(r32[2])
    assert bool(over.any()) and bool(mask[over].all())
    for x, x32 in zip(flat, r32[:3]):
        assert torch.equal(x[over], x32[over])
    ok = mask & ~over
    for name, x, x32, x64, sc in zip("pmv", flat, r32[:3], r64[:3], r64[3]):
        gate = 4 * (x32.double() - x64).abs() + 2.0 ** -22 * sc
        r = dr.ratio(x[ok], x64[ok], gate[ok])
        print(f"[glue] adam step {step} {name}: ratio {r:.3f}")
        assert r <= 1, (step, name, r)
    # the restatement, piece by piece, in fp32 on the CPU: the same numbers wherever fp32 did not overflow
    ref = gr.adam_gather(p, m, v, [(offs[j], gs[j]) for j in order], B1, B2, EPS, ss, bc2)
    for x, x32 in zip(ref, r32[:3]):
        assert torch.equal(x[~over].view(torch.int32), torch.where(mask, x32, x)[~over].view(torch.int32))


def test_adam_gather_takes_96_pieces_and_refuses_97(hip):
    n = gr.MAX_ADAM_DESC + 1
    sizes = [1 + (5 * j) % 23 for j in range(n)]
    offs, used = gr.adam_layout(sizes)
    p, m, v = _adam_state(used, 1400)
    g = dr.flat((used,), 1410) * 1e-2
    gd = g.cuda()
    ss, bc2 = dr.adam_bias_scalars(1e-3, B1, B2, 7)
    pieces = [(o, gd, o, k) for o, k in zip(offs, sizes)]
    a = [x.clone().cuda() for x in (p, m, v)]
    assert _gather_call(hip, a, pieces, ss, bc2) == -1
    assert _gather_call(hip, a, [], ss, bc2) == -1
    for x, x0 in zip(a, (p, m, v)):
        assert torch.equal(cpu(x), x0)  # refused: nothing written
    assert _gather_call(hip, a, pieces[:-1], ss, bc2) == 0
    b = [x.clone().cuda() for x in (p, m, v)]
    assert _flat_call(hip, b, gd, ss, bc2) == 0
    mask = torch.zeros(used, dtype=torch.bool)
    for o, k in zip(offs[:-1], sizes[:-1]):
        mask[o:o + k] = True
    for x, f, x0 in zip(a, b, (p, m, v)):
        x, f = cpu(x), cpu(f)
        assert torch.equal(x[mask].view(torch.int32), f[mask].view(torch.int32)) and torch.equal(x[~mask], x0[~mask])
        assert not torch.equal(x[mask], x0[mask])


@pytest.mark.parametrize("entry", ["gather", "flat"])
def test_adam_device_scalars_override_the_by_value_pair(hip, entry):
    """dyn2 given together with deliberately different by-value scalars: the result is the by-value call made with dyn2's values."""
    sizes = gr.ADAM_PIECES
    offs, used = gr.adam_layout(sizes)
    p, m, v = _adam_state(used, 1500)
    g = (dr.flat((used,), 1510) * 1e-2).cuda()
    ss, bc2 = dr.adam_bias_scalars(1e-3, B1, B2, 12)
    dyn2 = torch.tensor([ss, bc2], dtype=torch.float32).cuda()
    pieces = [(o, g, o, k) for o, k in zip(offs, sizes)]
    outs = []
    for scalars, d in (((ss, bc2), None), ((5.0, 7.0), dyn2)):
        a = [x.clone().cuda() for x in (p, m, v)]
        rc = _gather_call(hip, a, pieces, *scalars, dyn2=d) if entry == "gather" else _flat_call(hip, a, g, *scalars, dyn2=d)
        assert rc == 0
        outs.append([cpu(x) for x in a])
    for x, y, x0 in zip(outs[0], outs[1], (p, m, v)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and not torch.equal(x, x0)
    wrong = [x.clone().cuda() for x in (p, m, v)]  # the planted by-value pair alone gives something else: the test can tell
    assert (_gather_call(hip, wrong, pieces, 5.0, 7.0) if entry == "gather" else _flat_call(hip, wrong, g, 5.0, 7.0)) == 0
    assert not torch.equal(cpu(wrong[0]), outs[0][0])


# ======================================================================================================== 7. upnerf_set_scalars
def _scalars(hip, dst, words):
    vals = (C.c_float * max(len(words), 1)).from_buffer_copy(np.ascontiguousarray(words).tobytes()) if len(words) else (C.c_float * 1)()
    return hip["lib"].upnerf_set_scalars(dst.data_ptr() + 4 * G, len(words), vals, None)


@pytest.mark.parametrize("n", gr.SCALAR_COUNTS)
def test_set_scalars_carries_bits(hip, n):
    """dst[i] = vals[i], i < n, bit for bit (a NaN payload, -0.0, a denormal, inf among them); dst[n:] keeps its canary."""
    w = np.roll(gr.words(n + 8, 1600 + n), -7 * (n % 3))[:n] if n > 1 else gr.i32([0xFF8ABCDE])
    dst = dev(gr.canary(G + gr.MAX_SCALARS + 32 + G))
    assert _scalars(hip, dst, w) == 0
    want = gr.canary(dst.numel())
    want[G:G + n] = w
    assert same(dst, want)


def test_set_scalars_carries_every_special_word_and_refuses_0_and_97(hip):
    w = gr.i32(gr.SPECIAL_WORDS)
    dst = dev(gr.canary(G + gr.MAX_SCALARS + 32 + G))
    assert _scalars(hip, dst, w) == 0
    want = gr.canary(dst.numel())
    want[G:G + w.size] = w
    assert same(dst, want)
    dst = dev(gr.canary(G + gr.MAX_SCALARS + 32 + G))
    assert _scalars(hip, dst, gr.words(gr.MAX_SCALARS + 1, 1700)) == -1
    assert _scalars(hip, dst, gr.words(0, 1700)) == -1
    assert same(dst, gr.canary(dst.numel()))


# ==================================================================================================== 8. upnerf_scale_exponents
def test_scale_exponents_against_exact_integer_arithmetic(hip):
    """e = 14 - ceil(log2(max(m, 1e-30))) against e* = 14 - k, 2^(k-1) < v <= 2^k in integer arithmetic (glue_ref.exact_exponent), for
    2^p, p in [-100, 127], its fp32 neighbours, 0, a denormal, 1e-30 and its neighbours, FLT_MAX, in launches of 1, 63 and 64
    maxima.  e == e* at every exact power of two and for every v > 2^(k-1) (1 + 2^-14); in the band below that, which fp32 log2f
    (ulp up to 2^-17 for |log2 v| <= 128, a few of them times ln 2 < 2^-15 relative) cannot resolve, e* + 1 is accepted too: the
    scaled maximum is then at most 2^14 (1 + 2^-14) = 16385, still far inside fp16's range (65504).  Entries behind n keep
    their canary; 65 and 0 maxima are refused."""
    lib = hip["lib"]
    mx = gr.exponent_maxima()
    chunks, i = [], 0
    for n in (1, 63, 64) * ((len(mx) + 127) // 128 + 1):
        if i >= len(mx):
            break
        chunks.append(mx[i:i + n])
        i += n
    assert {len(c) for c in chunks} >= set(gr.EXPONENT_COUNTS) and sum(len(c) for c in chunks) == len(mx)
    band = {0: 0, 1: 0}
    for c in chunks:
        src = torch.tensor(c, dtype=torch.float32).cuda()
        out = dev(gr.canary(G + gr.MAX_EXPONENTS + G))
        assert lib.upnerf_scale_exponents(src.data_ptr(), len(c), out.data_ptr() + 4 * G, None) == 0
        got = cpu(out)
        assert bool((got[:G] == CAN).all()) and bool((got[G + len(c):] == CAN).all())
        for x, e in zip(c, got[G:G + len(c)].tolist()):
            want, exact = gr.exact_exponent(x)
            if exact:
                assert e == want, (x, e, want)
            else:
                assert e in (want, want + 1), (x, e, want)
                band[e - want] += 1
    print(f"[glue] scale_exponents inside the band: {band[0]} maxima at e*, {band[1]} at e* + 1")
    src = torch.ones(gr.MAX_EXPONENTS + 1).cuda()
    out = dev(gr.canary(G + gr.MAX_EXPONENTS + 1 + G))
    assert lib.upnerf_scale_exponents(src.data_ptr(), gr.MAX_EXPONENTS + 1, out.data_ptr() + 4 * G, None) == -1
    assert lib.upnerf_scale_exponents(src.data_ptr(), 0, out.data_ptr() + 4 * G, None) == -1
    assert same(out, gr.canary(out.numel()))
