"""tests/glue_ref.py on the CPU: the case tables hit the edges they name, the restatements agree with torch, and the host sides of
the descriptor-driven entry points refuse -- before any launch, so without a GPU -- what their int indices cannot hold."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dense_ref as dr
import glue_ref as gr

EINVAL = -1


# ------------------------------------------------------------------------------------------------------------ the case tables
def test_the_constants_are_the_librarys():
    from upnerf_amd import _lib
    assert (gr.MAX_ADD_PAIRS, gr.MAX_ADAM_DESC, gr.MAX_SCALARS) == (_lib.MAX_ADD_PAIRS, _lib.MAX_ADAM_DESC, _lib.MAX_SCALARS)
    import abi_check
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "upnerf_hip.h")
    assert abi_check.constants(header)["MAX_PACK_DESC"] == gr.MAX_PACK_DESC
    assert gr.CANARY < 2 ** 31 and math.isnan(float(gr.canary(1).view(np.float32)[0]))


def test_pack_tables_hit_their_edges():
    t = gr.PACK_TABLES
    assert [len(t[k]) for k in ("one", "edges256", "strided", "max48")] == [1, 3, 5, gr.MAX_PACK_DESC]
    for name, table in t.items():
        descs, used = gr.layout(table)
        st = gr.starts(descs)
        total = int(st[-1])
        # the last workgroup is ragged -- except for 255 + 256 + 257 = 768, the one launch of whole workgroups
        assert (total % gr.BLOCK != 0) == (name != "edges256"), name
        if len(descs) > 1:  # a descriptor boundary strictly inside a workgroup
            assert any(0 < int(b) % gr.BLOCK for b in st[1:-1]), name
        # disjoint destinations with a gap in front of every descriptor, everything inside [0, used)
        seen = np.zeros(used, dtype=np.int32)
        for d in descs:
            seen[gr.dst_index(d)] += 1
            assert d.src_ld >= d.cols and d.dst_ld >= d.cols
        assert seen.max() == 1 and seen.sum() == total and seen[0] == 0
        for a, b in zip(descs, descs[1:]):
            assert b.dst_off > a.dst_off + (a.rows - 1) * a.dst_ld + a.cols
    st = gr.starts(gr.layout(t["edges256"])[0])
    assert list(st) == [0, 255, 511, 768]
    strided = t["strided"]
    assert any(s > c for _, c, s, _ in strided) and any(dl > c for _, c, _, dl in strided)      # src_ld > cols, dst_ld > cols
    assert any(r * c > gr.BLOCK and c % gr.BLOCK for r, c, _, _ in strided)                     # rows that straddle workgroups
    assert sum(r * c for r, c, _, _ in strided) > 2 * gr.BLOCK                                  # more than one workgroup
    assert sorted(c for _, c, _, _ in t["max48"]) == list(range(1, 49))


def test_inputs_hold_the_special_words_and_never_the_canary():
    w = gr.words(4096, 3)
    u = set(int(x) for x in w.view(np.uint32))
    assert set(gr.SPECIAL_WORDS) <= u and gr.CANARY not in u
    f = np.array(gr.SPECIAL_WORDS, dtype=np.uint32).view(np.float32)
    assert np.isnan(f).sum() >= 5 and np.isinf(f).sum() == 2 and 0x80000001 in gr.SPECIAL_WORDS
    assert sum(1 for x in gr.SPECIAL_WORDS if 0 < (x & 0x7FFFFFFF) < 0x00800000) >= 4            # denormals
    assert sum(1 for x in gr.SPECIAL_WORDS if 0x7F800000 < (x & 0x7FFFFFFF) and not x & 0x00400000) >= 2  # signalling NaNs
    x = gr.finite(1000, 5).view(np.float32)
    assert np.isfinite(x).all() and (np.abs(x[x != 0]) < 2.0 ** -126).any()
    assert gr.CANARY not in set(int(v) for v in gr.finite(1000, 5).view(np.uint32))
    a, b = gr.add_inputs(300, 7)
    s = gr.add_pairs([a], [b])[0].view(np.float32)
    assert np.isnan(s).sum() == 3 and np.isinf(s).sum() == 3
    assert (s.view(np.uint32) == 0x80000000).any()                                               # a pair summing to -0
    assert ((s != 0) & (np.abs(s) < 2.0 ** -126)).sum() >= 3                                     # denormal sums


def test_the_other_tables_hit_their_edges():
    assert set(gr.ADD_SIZES) >= {gr.BLOCK - 1, gr.BLOCK, gr.BLOCK + 1, 1} and max(gr.ADD_SIZES) % gr.BLOCK
    st = np.cumsum(gr.ADD_SIZES)
    assert any(int(b) % gr.BLOCK for b in st[:-1]) and int(st[-1]) % gr.BLOCK
    blocks = lambda n: ((n >> 2) + 255) // 256
    at_cap, big = sorted(gr.ZERO_SIZES)[-2:]
    assert blocks(at_cap) == gr.ZERO_BLOCK_CAP and at_cap & 3                             # every workgroup of the cap, one trip
    assert blocks(big) > gr.ZERO_BLOCK_CAP and big & 3                                    # a second trip of the loop, and the tail
    assert {1, 2, 3} <= set(gr.ZERO_SIZES) and {n & 3 for n in gr.ZERO_SIZES} == {0, 1, 2, 3}  # n < 4, every tail length
    assert {gr.ADAM_BLOCK - 1, gr.ADAM_BLOCK, gr.ADAM_BLOCK + 1, 4 * gr.ADAM_BLOCK + 1, 1} == set(gr.ADAM_PIECES)
    offs, used = gr.adam_layout(gr.ADAM_PIECES)
    assert offs[0] > 0 and all(b > a + n for a, n, b in zip(offs, gr.ADAM_PIECES, offs[1:])) and used > offs[-1] + gr.ADAM_PIECES[-1]
    assert any(o % 4 for o in offs)                                                       # pieces off the 16-byte grid
    assert max(gr.SCALAR_COUNTS) == gr.MAX_SCALARS and {63, 64, 65} <= set(gr.SCALAR_COUNTS)
    assert max(gr.EXPONENT_COUNTS) == gr.MAX_EXPONENTS


# ------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("name", list(gr.PACK_TABLES))
def test_pack_is_a_slice_assignment_and_unpack_undoes_it(name):
    descs, used = gr.layout(gr.PACK_TABLES[name])
    srcs = [gr.words(gr.src_words(d), 10 + j) for j, d in enumerate(descs)]
    zero = np.zeros(used + 2 * gr.GUARD, dtype=np.int32)
    got = gr.pack(zero, descs, srcs, base=gr.GUARD)
    want = torch.zeros(used + 2 * gr.GUARD, dtype=torch.int32)
    for d, s in zip(descs, srcs):
        view = torch.as_strided(want, (d.rows, d.cols), (d.dst_ld, 1), gr.GUARD + d.dst_off)
        view[:] = torch.from_numpy(s.copy()).as_strided((d.rows, d.cols), (d.src_ld, 1))
    assert torch.equal(torch.from_numpy(got), want)
    # unpack o pack is the identity on the described elements and leaves the padding of the parameters alone
    P = gr.pack(gr.canary(used + 2 * gr.GUARD), descs, srcs, base=gr.GUARD)
    assert int((P != gr.canary(1)[0]).sum()) == int(gr.starts(descs)[-1])
    back = gr.unpack(P, descs, [gr.canary(gr.src_words(d)) for d in descs], base=gr.GUARD)
    for d, s, t in zip(descs, srcs, back):
        idx = gr.src_index(d)
        assert np.array_equal(t[idx], s[idx])
        rest = np.ones(t.size, dtype=bool)
        rest[idx] = False
        assert (t[rest] == gr.canary(1)[0]).all()


def test_accumulate_is_torchs_fp32_sum():
    table = gr.PACK_TABLES["strided"]
    descs, used = gr.layout(table, flags=[1, 0, 1, 0, 1])
    srcs = [gr.finite(gr.src_words(d), 20 + j) for j, d in enumerate(descs)]
    P0 = gr.finite(used, 30)
    got = gr.pack(P0, descs, srcs)
    want = torch.from_numpy(P0.copy()).view(torch.float32)
    for d, s in zip(descs, srcs):
        view = torch.as_strided(want, (d.rows, d.cols), (d.dst_ld, 1), d.dst_off)
        x = torch.from_numpy(s.copy()).view(torch.float32).as_strided((d.rows, d.cols), (d.src_ld, 1))
        if d.accumulate:
            view += x
        else:
            view[:] = x
    assert torch.equal(torch.from_numpy(got), want.view(torch.int32))
    assert not np.array_equal(got, P0)


def test_add_pairs_is_torchs_sum():
    for n in gr.ADD_SIZES[:4]:
        a, b = gr.add_inputs(n, 40 + n)
        got = torch.from_numpy(gr.add_pairs([a], [b])[0])
        want = torch.from_numpy(a.copy()).view(torch.float32) + torch.from_numpy(b.copy()).view(torch.float32)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got.view(torch.float32)), nan)
        assert torch.equal(got[~nan], want.view(torch.int32)[~nan])


def test_adam_gather_is_the_flat_formula_on_the_pieces_and_nothing_else():
    sizes = gr.ADAM_PIECES
    offs, used = gr.adam_layout(sizes)
    p, m, v = dr.flat((used,), 1), dr.flat((used,), 2) * 1e-3, dr.flat((used,), 3).abs() * 1e-5
    gs = [dr.flat((n,), 50 + j) * 1e-2 for j, n in enumerate(sizes)]
    ss, bc2 = dr.adam_bias_scalars(1e-3, 0.9, 0.999, 3)
    order = [3, 0, 4, 1, 2]  # out of offset order: the pieces are disjoint, so the order cannot matter
    got = gr.adam_gather(p, m, v, [(offs[j], gs[j]) for j in order], 0.9, 0.999, 1e-8, ss, bc2)
    g_flat, mask = torch.zeros(used), torch.zeros(used, dtype=torch.bool)
    for o, g in zip(offs, gs):
        g_flat[o:o + g.numel()] = g
        mask[o:o + g.numel()] = True
    flat = dr.adam_formula(p, g_flat, m, v, 0.9, 0.999, 1e-8, ss, bc2, torch.float32)[:3]
    for x, f, x0 in zip(got, flat, (p, m, v)):
        assert torch.equal(x[mask], f[mask]) and torch.equal(x[~mask].view(torch.int32), x0[~mask].view(torch.int32))
        assert not torch.equal(x[mask], x0[mask])


def test_exact_exponents():
    mx = gr.exponent_maxima()
    assert len(mx) == 3 * 228 + 6 and all(float(np.float32(x)) == x for x in mx)
    assert 2.0 ** -100 * 1.25 < gr.FLOOR < 2.0 ** -99  # p = -100 and its neighbours are below the clamp (asserted further down)
    for p in range(-99, 128):
        assert gr.exact_exponent(2.0 ** p) == (14 - p, True)
        up, dn = gr._next(2.0 ** p, True), gr._next(2.0 ** p, False)
        assert gr.exact_exponent(up) == (14 - (p + 1), False)        # one ulp above 2^p: in the band of the next binade
        assert gr.exact_exponent(dn) == (14 - p, True)
        assert gr.exact_exponent(2.0 ** p * (1 + 2.0 ** -14)) == (13 - p, False)      # the band's last member
        assert gr.exact_exponent(gr._next(2.0 ** p * (1 + 2.0 ** -14), True)) == (13 - p, True)
    floor = gr.exact_exponent(gr.FLOOR)
    assert floor == (14 + 99, True) and 2.0 ** -100 < gr.FLOOR <= 2.0 ** -99
    for x in (0.0, 1e-40, gr._next(gr.FLOOR, False), -1.0, 2.0 ** -100, gr._next(2.0 ** -100, True), gr._next(2.0 ** -100, False)):
        assert gr.exact_exponent(x) == floor                                           # clamped to 1e-30f
    assert gr.exact_exponent(float(np.finfo(np.float32).max)) == (14 - 128, True)
    # the exact exponent agrees with the fp64 formula the other references use wherever that formula is safe (off the band)
    for x in mx:
        e, exact = gr.exact_exponent(x)
        if exact:
            assert e == dr.host_exponent(torch.tensor([x], dtype=torch.float32)), x


# ------------------------------------------------------------------------------------------------ refusals before any launch
ONE = C.c_void_p(16)  # non-null, never dereferenced: every call below returns on the host


def _lib():
    from upnerf_amd import _lib
    return _lib


def _pack(descs, unpack=0):
    L = _lib()
    arr = (L.PackDesc * len(descs))(*descs)
    return L.lib.upnerf_pack(ONE, arr, len(descs), unpack, None)


def _pd(rows, cols):
    return _lib().PackDesc(ptr=16, rows=rows, cols=cols, src_ld=cols, dst_off=0, dst_ld=cols, accumulate=0)


@pytest.mark.parametrize("unpack", [0, 1])
def test_pack_refuses_what_its_int_indices_cannot_hold(unpack):
    assert _pack([_pd(65536, 32768)], unpack) == EINVAL                      # rows * cols = 2^31 wrapped to INT_MIN
    assert _pack([_pd(1, 2 ** 26)] * 48, unpack) == EINVAL                   # 48 x 2^26 = 3 x 2^30: the prefix sums wrapped
    assert _pack([_pd(1, 2 ** 30), _pd(1, 2 ** 30)], unpack) == EINVAL       # the total is exactly 2^31
    assert _pack([_pd(1, 2 ** 31 - 1)], unpack) == EINVAL                    # rounded up to whole workgroups it passes INT_MAX
    assert _pack([_pd(1, 1)] * 49, unpack) == EINVAL                         # more than UPNERF_MAX_PACK_DESC
    assert _pack([_pd(1, 1), _pd(0, 1)], unpack) == EINVAL


def test_add_pairs_refuses_what_its_int_indices_cannot_hold():
    L = _lib()
    pair = lambda n: L.AddPair(a=16, b=16, out=16, n=n)
    call = lambda ps: L.lib.upnerf_add_pairs((L.AddPair * len(ps))(*ps), len(ps), None)
    assert call([pair(2 ** 28)] * 8) == EINVAL                               # 8 x 2^28 = 2^31
    assert call([pair(2 ** 31 - 1)]) == EINVAL
    assert call([pair(1)] * 9) == EINVAL                                     # more than UPNERF_MAX_ADD_PAIRS
    assert call([pair(1), pair(0)]) == EINVAL


def test_frag_entry_points_refuse_what_their_int_indices_cannot_hold():
    L = _lib()
    big = dict(src_off=0, src_ld=4096, transpose=0, rows=32768, cols=4096, dst_off=0, dst_kp=4096, dst_k0=0)  # 2^27 elements
    small = dict(big, rows=32, cols=16, dst_kp=16, src_ld=16)
    fd = (L.FragDesc * 17)(*[L.FragDesc(**big)] * 17)                        # 17 x 2^27 > 2^31
    assert L.lib.upnerf_frag_copy(ONE, ONE, fd, 17, None) == EINVAL
    fd1 = (L.FragDesc * 1)(L.FragDesc(**dict(big, rows=65536, cols=32768, dst_kp=32768, src_ld=32768)))
    assert L.lib.upnerf_frag_copy(ONE, ONE, fd1, 1, None) == EINVAL          # one descriptor of 2^31
    f16 = lambda n, kw: (L.Frag16Desc * n)(*[L.Frag16Desc(exp_id=0, **kw)] * n)
    args = lambda fwd, nf, bwd, nb: L.lib.upnerf_frag16(ONE, ONE, ONE, fwd, nf, bwd, nb, ONE, ONE, 0, 0, None, None)
    assert args(f16(17, big), 17, f16(1, small), 1) == EINVAL                # the forward set
    assert args(f16(1, small), 1, f16(17, big), 17) == EINVAL                # the transposed set, behind a valid forward set


# ------------------------------------------------------------------------------------------------- parallel._gather's launches
class _Fake:
    """What _gather asks of a tensor, with a made-up size and address: no memory behind it."""
    is_cuda, dtype = True, torch.float32

    def __init__(self, n, addr):
        self.n, self.addr = n, addr

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.addr

    def is_contiguous(self):
        return True


def _run_gather(monkeypatch, sizes, offsets=None, scatter=False):
    """_gather on fake tensors of the given sizes whose views tile `flat` (or start at `offsets`); returns (descriptors per
    upnerf_pack launch with their (cols, dst_off), number of torch copies)."""
    from upnerf_amd import parallel
    L = _lib()
    launches, copies = [], []

    def fake_pack(P, arr, n, unpack, st):
        assert P == 4096 and unpack == (1 if scatter else 0)
        launches.append([(arr[i].cols, arr[i].dst_off) for i in range(n)])
        return 0

    monkeypatch.setattr(L.lib, "upnerf_pack", fake_pack)
    monkeypatch.setattr(L, "stream", lambda: None)
    monkeypatch.setattr(torch, "_foreach_copy_", lambda dst, src: copies.append(len(dst)))
    if offsets is None:
        offsets = [int(x) for x in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
    flat = _Fake(sum(sizes), 4096)
    views = [_Fake(n, 4096 + 4 * o) for n, o in zip(sizes, offsets)]
    tensors = [_Fake(n, 2 ** 40 + 4 * i) for i, n in enumerate(sizes)]
    parallel._gather(flat, views, tensors, scatter=scatter)
    return launches, len(copies)


@pytest.mark.parametrize("scatter", [False, True])
def test_gather_closes_a_launch_at_48_descriptors_or_before_2_31_floats(monkeypatch, scatter):
    from upnerf_amd import parallel
    limit = parallel._PACK_MAX_FLOATS
    assert limit <= 2 ** 31 - 2048 and parallel._PACK_MAX_DESC == gr.MAX_PACK_DESC
    # by count: 97 tensors and two empty ones
    sizes = [1 + (7 * i) % 300 for i in range(97)]
    sizes[5:5] = [0]
    sizes[60:60] = [0]
    launches, copies = _run_gather(monkeypatch, sizes, scatter=scatter)
    assert [len(c) for c in launches] == [48, 48, 1] and copies == 0
    assert [n for c in launches for n, _ in c] == [n for n in sizes if n]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert [o for c in launches for _, o in c] == [int(o) for n, o in zip(sizes, offs) if n]
    # by size: the fourth tensor would bring the launch past the limit
    sizes = [2 ** 30, 2 ** 30 - 4096, 5, 2 ** 29]
    launches, copies = _run_gather(monkeypatch, sizes, scatter=scatter)
    assert [len(c) for c in launches] == [3, 1] and copies == 0
    assert all(sum(n for n, _ in c) < limit for c in launches)
    # every launch stays below the limit for sizes that fill it exactly
    sizes = [limit - 1, 1, limit - 2, 1, 1]
    launches, copies = _run_gather(monkeypatch, sizes, offsets=[0, 8, 16, 24, 32], scatter=scatter)
    assert [[n for n, _ in c] for c in launches] == [[limit - 1], [1, limit - 2], [1, 1]] and copies == 0
    # a single tensor at the limit, or a view that starts beyond what dst_off can hold: the torch path, nothing launched
    for sizes, offsets in (([5, limit, 7], [0, 8, 16]), ([2 ** 30, 2 ** 30, 2 ** 30], None)):
        launches, copies = _run_gather(monkeypatch, sizes, offsets=offsets, scatter=scatter)
        assert launches == [] and copies == 1


def test_pack_chunks():
    from upnerf_amd.parallel import _PACK_MAX_FLOATS as limit, _pack_chunks
    assert _pack_chunks([]) == [] and _pack_chunks([3]) == [(0, 1)]
    assert _pack_chunks([1] * 48) == [(0, 48)] and _pack_chunks([1] * 49) == [(0, 48), (48, 49)]
    assert _pack_chunks([1] * 97) == [(0, 48), (48, 96), (96, 97)]
    assert _pack_chunks([limit - 2, 1]) == [(0, 2)] and _pack_chunks([limit - 1, 1]) == [(0, 1), (1, 2)]
    for sizes in ([2 ** 29] * 9, [limit - 1] * 3, [2 ** 26] * 48):
        for lo, hi in _pack_chunks(sizes):
            assert 0 < hi - lo <= 48 and sum(sizes[lo:hi]) < limit
