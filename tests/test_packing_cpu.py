"""CPU checks of the host logic around the kernels: the packed parameter layout, the folded colour layer and the
composite-then-project algebra reproduce the oracle (and therefore the reference) when evaluated by the torch
restatement of the kernels' arithmetic in tests/kernel_space.py.  No GPU involved."""
import numpy as np
import pytest
import torch

import kernel_space as ks
from golden_util import Case, orc, rel_err
from upnerf_amd.nerf import NeRF
from upnerf_amd.rendering import band_weights

NAMES = ["cfg1_small", "cfg1_small_fine", "cfg2_phase1", "small_tto", "small_nocand", "small_allmasked"]


def build_model(c, typ, st):
    m = NeRF(typ, c2f=c.c2f, encode_feat=c.encode_feat, **c.nerf_kw())
    sd = {k: v.detach().clone() for k, v in st[f"nerf_{typ}"].items()}
    sd["progress"] = torch.tensor(c.progress)
    m.load_state_dict(sd)
    if c.encode_candidate is False:
        m.encode_candidate = False
    return m


@pytest.mark.parametrize("name", NAMES)
def test_packed_kernel_space_matches_oracle(name):
    c = Case(name)
    st = c.state(requires_grad=False)
    keep = {}
    b, hp = c.batch(), c.hparams()
    real = orc.schedule_mult
    orc.schedule_mult = lambda p, s: c.sched
    try:
        with torch.no_grad():
            _, res = orc.training_forward(st, c.cfgs(), b, hp, c.progress, u_list=c.u_list, keep=keep)
    finally:
        orc.schedule_mult = real
    idx = b["img_idx"]
    pose = orc.compose_pair(orc.se3_exp(st["se3_refine"][idx]), b["c2w"]) if c.pose_opt else b["c2w"]
    o, d = orc.get_rays(b["directions"], pose)
    for typ, zkey in (("coarse", "z_coarse"), ("fine", "z_fine")):
        if typ == "fine" and not c.fine:
            continue
        model = build_model(c, typ, st)
        pk = model.packer
        with torch.no_grad():
            P = model.packed()
            assert P.numel() == pk.L.total
            use_cand = bool(c.sched < 1 and model.encode_candidate)
            use_rgb = bool(c.sched > 0)
            mode = (1 if use_rgb else 0) if use_cand else (3 if c.sched < 1 else 2)
            a_rows = st[f"embedding_{typ}_a"][idx]
            c_rows = st[f"embedding_{typ}_c"][idx]
            aux = ks.ray_aux(d, a_rows, band_weights(4, c.progress, c.c2f))
            z = keep[zkey]
            f = ks.field(P, pk, o, d, z, c_rows, aux, band_weights(10, c.progress, c.c2f), use_cand, use_rgb)
            out = ks.composite(f, z, mode, use_rgb, pk.W)
            wf, bf = model.feat_share_layer.weight, model.feat_share_layer.bias
            if c.sched < 1:
                feat = out["E_s"] @ wf.t() + out["sum_sfeat"][:, None] * bf
                if use_cand:
                    feat = feat + out["G_c"] @ model.feat_candidate_layer.weight.t() \
                        + out["t_weight"][:, None] * model.feat_candidate_layer.bias
                    assert rel_err(out["w_all"], res[f"c_weights_{typ}"]) < 2e-5
                    assert rel_err(out["c_depth"], res[f"c_depth_{typ}"]) < 2e-5
                    assert rel_err(out["t_weight"], res[f"t_weight_{typ}"]) < 2e-5
                assert rel_err(feat, res[f"feat_{typ}"]) < 2e-5
            if c.sched > 0:
                assert rel_err(out["rgb_map"], res[f"s_rgb_{typ}"]) < 2e-5
                assert rel_err(out["w_s"], res[f"s_weights_{typ}"]) < 2e-5
            assert rel_err(out["s_depth"], res[f"s_depth_{typ}"]) < 2e-5
            # transposed copies are exact transposes of the forward pieces
            PT = pk.pack_t(P)
            L, W, W2 = pk.L, pk.W, pk.W2
            assert torch.equal(ks.mat(PT, L.t_we, W, W), ks.mat(P, L.we, W, W).t())
            assert torch.equal(ks.mat(PT, L.t_w[0], 64, W), ks.mat(P, L.w[0], W, 64).t())
            assert torch.equal(ks.mat(PT, L.t_head, W, W)[:, W2:], ks.mat(P, L.wc1, W2, W + 16)[:, :W].t())


@pytest.mark.parametrize("name", ["nofeat_phase0", "nofeat_phase1", "nofeat_w256_phase1"])
def test_rgb_joint_map_reproduces_the_oracle_c_rgb(name):
    """encode_feat = False: kernel_space.composite's rgb_joint_map (sum_i w_sj rgb_i, the shared half of c_rgb) plus the candidate
    half projected per ray (W_rc G_c + b_rc t_weight) is the oracle's c_rgb."""
    c = Case(name)
    assert not c.encode_feat and c.sched < 1
    st = c.state(requires_grad=False)
    keep = {}
    b, hp = c.batch(), c.hparams()
    real = orc.schedule_mult
    orc.schedule_mult = lambda p, s: c.sched
    try:
        with torch.no_grad():
            _, res = orc.training_forward(st, c.cfgs(), b, hp, c.progress, u_list=c.u_list, keep=keep)
    finally:
        orc.schedule_mult = real
    idx = b["img_idx"]
    pose = orc.compose_pair(orc.se3_exp(st["se3_refine"][idx]), b["c2w"]) if c.pose_opt else b["c2w"]
    o, d = orc.get_rays(b["directions"], pose)
    for typ, zkey in (("coarse", "z_coarse"), ("fine", "z_fine")):
        if typ == "fine" and not c.fine:
            continue
        model = build_model(c, typ, st)
        pk = model.packer
        with torch.no_grad():
            P = model.packed()
            aux = ks.ray_aux(d, st[f"embedding_{typ}_a"][idx], band_weights(4, c.progress, c.c2f))
            z = keep[zkey]
            f = ks.field(P, pk, o, d, z, st[f"embedding_{typ}_c"][idx], aux, band_weights(10, c.progress, c.c2f), True, True)
            out = ks.composite(f, z, 1, True, pk.W)
            rc = model.rgb_candidate_layer
            c_rgb = out["rgb_joint_map"] + out["G_c"] @ rc.weight.t() + out["t_weight"][:, None] * rc.bias
            assert rel_err(c_rgb, res[f"c_rgb_{typ}"]) < 2e-5, typ
            assert float(out["rgb_joint_map"].abs().max()) > 0


def test_pack_is_differentiable_to_reference_named_parameters():
    c = Case("cfg1_small_fine")
    model = build_model(c, "coarse", c.state(requires_grad=False))
    P = model.packed()
    (P * torch.linspace(0, 1, P.numel())).sum().backward()
    for n, p in model.named_parameters():
        if n in ("progress", "feat_candidate_layer.weight", "feat_candidate_layer.bias"):
            continue  # not part of the packed buffer (projected per ray on the host side)
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


def test_state_dict_keys_and_shapes_match_the_reference_modules():
    """Checkpoint interchange: the modules expose exactly the reference's state_dict keys and shapes
    (fixture recorded from the real models/nerf.py and models/transient_net.py by tools/make_goldens.py)."""
    import json
    import os
    from golden_util import GOLDEN
    from upnerf_amd.nerf import NeRF
    from upnerf_amd.transient_net import TransientNet
    fx = json.load(open(os.path.join(GOLDEN, "state_keys.json")))
    for tag, item in fx.items():
        m = TransientNet(**item["kwargs"]) if tag.startswith("transient") else NeRF("coarse", c2f=(0.1, 0.5), **item["kwargs"])
        mine = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert mine == item["state"], (tag, set(mine) ^ set(item["state"]))


def test_pack_without_the_feature_layer_places_the_colour_matrix_as_it_stands():
    """encode_feat = False (nerf.py:52-56): rgb_share_layer.0 reads [xyz_encoding_final | PE(dir) | appearance] itself, so the
    layout's "folded" colour matrix is W_r1[:, :W] and its side columns W_r1[:, W:], unchanged; its bias is b_r1."""
    import torch
    from upnerf_amd._lib import AUXK
    from upnerf_amd.nerf import NeRF
    m = NeRF("coarse", D=4, W=64, encode_feat=False, feat_dim=0, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=16)
    p = dict(m.named_parameters())
    assert "feat_share_layer.weight" not in p and "rgb_candidate_layer.weight" in p
    assert "feat_share_layer.weight" not in m.packer.pack_names()
    P = m.packer.pack(p).detach()
    L, W, W2 = m.packer.L, 64, 32
    wr1 = P[L.wr1:L.wr1 + W2 * (W + AUXK)].view(W2, W + AUXK)
    w = p["rgb_share_layer.0.weight"].detach()
    assert w.shape == (W2, W + 27 + 48)
    assert torch.equal(wr1[:, :W + 75], w) and float(wr1[:, W + 75:].abs().max()) == 0.0
    assert torch.equal(P[L.br1:L.br1 + W2], p["rgb_share_layer.0.bias"].detach())
    # gradients flow straight back
    (m.packer.pack(p) * torch.arange(L.total, dtype=torch.float32)).sum().backward()
    g = p["rgb_share_layer.0.weight"].grad
    assert torch.equal(g[3, :5], torch.arange(L.wr1 + 3 * (W + AUXK), L.wr1 + 3 * (W + AUXK) + 5, dtype=torch.float32))


@pytest.mark.parametrize("W,D,skips", [(256, 8, [4]), (256, 8, []), (256, 8, [1]), (64, 4, []), (256, 1, []), (64, 1, [])])
def test_layout_struct_is_layout_offsets_field_by_field(W, D, skips):
    """The struct the kernels take holds pass_plan.layout_offsets' integers (which the weight-gradient schedule reads), layers
    beyond D zero."""
    from upnerf_amd import _lib, pass_plan
    from upnerf_amd.packing import NerfPacker
    pk = NerfPacker(W, D, skips, 63, 27, 384, 48, 16)
    want = pass_plan.layout_offsets(W, D, skips[0] if skips else -1)
    assert pk.offsets == want and {f for f, _ in _lib.Layout._fields_} == set(want._fields)
    for f, v in want._asdict().items():
        got = getattr(pk.L, f)
        assert (list(got) == list(v) + [0] * (_lib.MAX_D - D)) if isinstance(v, tuple) else got == v, f


# ---------------------------------------------------------------------------------------------------------------------------------
# the block tables of pass_plan (param_blocks / t_blocks) and everything NerfPacker derives from them, on the host
LAYOUTS = [(256, 8, [4]), (256, 8, []), (256, 8, [1]), (64, 4, []), (256, 1, []), (64, 1, [])]
PACKERS = [(W, D, skips, cand, feat) for W, D, skips in LAYOUTS for cand in (16, 0) for feat in (True, False)]
WR1 = "rgb_share_layer.0.weight"


def make_packer(W, D, skips, cand, feat):
    from upnerf_amd.packing import NerfPacker
    return NerfPacker(W, D, skips, 63, 27, 384 if feat else 0, 48, cand, encode_feat=feat)


def seeded_params(pk):
    from upnerf_amd import synth
    kw = dict(D=pk.D, W=pk.W, skips=(pk.skip,), feat_dim=pk.feat_dim, xyz_L=10, dir_L=4, appearance_dim=48, candidate_dim=pk.C)
    return {k: v for k, v in synth.nerf_state("coarse", seed=4, encode_feat=pk.encode_feat, **kw).items() if k != "progress"}


def decoded(pk, shapes, scratch_off=None):
    """The pack descriptors against made-up, far-apart base addresses: [(descriptor, parameter name, first source element)],
    every source range checked to lie inside its parameter."""
    base = {n: (i + 1) << 40 for i, n in enumerate(sorted(shapes))}
    out = []
    for q in pk._pack_descs(base.__getitem__, scratch_off):
        name = sorted(shapes)[(q.ptr >> 40) - 1]
        first, shape = (q.ptr - base[name]) // 4, shapes[name]
        width = shape[-1]
        assert (q.ptr - base[name]) % 4 == 0 and q.src_ld == width and q.accumulate == 0, name
        assert first + q.cols <= width and q.rows * width <= int(np.prod(shape)) and q.cols <= q.dst_ld, name
        out.append((q, name, first))
    return out


def grid(off, rows, cols, ld):
    return (off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]).reshape(-1)


def forward_writes(pk, p):
    """(how often the forward descriptors write each element of [P | scratch], the buffer they produce from p)."""
    n = pk.L.total + (pk.W2 * pk.feat_dim if pk.encode_feat else 0)
    count, buf = np.zeros(n, np.int32), np.zeros(n, np.float32)
    for q, name, first in decoded(pk, {k: tuple(v.shape) for k, v in p.items()}, pk.L.total if pk.encode_feat else None):
        dst = grid(q.dst_off, q.rows, q.cols, q.dst_ld)  # (an index past the end raises)
        np.add.at(count, dst, 1)
        buf[dst] = p[name].detach().numpy().reshape(-1)[grid(first, q.rows, q.cols, q.src_ld)]  # the ten-line copy loop
    return count, buf


def expected_writes(pk):
    """One write for every used element of every block the table states, with the stated exceptions; the scratch copy once."""
    from upnerf_amd import pass_plan as pp
    expect = np.zeros(pk.L.total + (pk.W2 * pk.feat_dim if pk.encode_feat else 0), np.int32)
    for b in pp.param_blocks(pk.W, pk.D, pk.skip):
        if b.field in ("wc1", "bc1", "wc2", "bc2", "wcsig", "bcsig") and not pk.has_cand:
            continue  # no candidate head: its blocks stay zero
        for part in b.parts:
            if pk.encode_feat and (b.field == "br1" or (b.field == "wr1" and part.name == "e")):
                continue  # written by the fold
            expect[grid(pp.block_offset(pk.L, b) + part.col0, b.used_rows, part.cols, b.ld)] += 1
    expect[pk.L.total:] = 1
    return expect


@pytest.mark.parametrize("W,D,skips", LAYOUTS)
def test_blocks_tile_the_buffers_in_struct_order(W, D, skips):
    from upnerf_amd import _lib, pass_plan as pp
    skip = skips[0] if skips else -1
    L = pp.layout_offsets(W, D, skip)
    fields = [f for f, _ in _lib.Layout._fields_]
    order = lambda names: [(f, l) for f in names for l in (range(D) if isinstance(getattr(L, f), tuple) else [None])]
    for blocks, total, names in ((pp.param_blocks(W, D, skip), L.total, fields[3:fields.index("total")]),
                                 (pp.t_blocks(W, D, skip), L.t_total, fields[fields.index("total") + 1:-1])):
        assert [(b.field, b.layer) for b in blocks] == order(names)
        end = 0
        for b in blocks:
            o, size = pp.block_offset(L, b), pp.block_size(b)
            assert o % 4 == 0 and o == end and b.rows * b.ld <= size < b.rows * b.ld + 4, (b.field, b.layer)
            end = o + size
        assert end == total
    for b in pp.param_blocks(W, D, skip):  # the parts lie side by side inside the pitch, `cols` counts what they use
        ends = [p.col0 + p.cols for p in b.parts]
        assert all(p.col0 >= e for p, e in zip(b.parts[1:], ends)) and ends[-1] <= b.ld and b.cols == sum(p.cols for p in b.parts)
        assert 0 < b.used_rows <= b.rows and (b.exp is not None) == b.matrix


@pytest.mark.parametrize("W,D,skips,cand,feat", PACKERS)
def test_forward_pack_descriptors_write_each_element_once_and_agree_with_pack(W, D, skips, cand, feat):
    pk = make_packer(W, D, skips, cand, feat)
    p = seeded_params(pk)
    count, buf = forward_writes(pk, p)
    expect = expected_writes(pk)
    bad = np.flatnonzero(count != expect)
    assert bad.size == 0, (bad[:8], count[bad[:8]], expect[bad[:8]])
    # the padding, restated without the table: column 63 of the encoding's columns, the side columns behind [PE(dir) | appearance],
    # the floats behind the 1-wide biases, the fourth row / float of the colour head
    L, W2 = pk.L, W // 2
    pad = [grid(L.w[0] + 63, W, 1, 64), grid(L.wr1 + W + 75, W2, 5, W + 80), np.arange(L.bsig + 1, L.bsig + 4),
           np.arange(L.bcsig + 1, L.bcsig + 4), np.arange(L.wr2 + 3 * W2, L.wr2 + 4 * W2), np.array([L.br2 + 3])]
    if pk.skip > 0:
        pad.append(grid(L.w[pk.skip] + 63, W, 1, 64 + W))
    assert all(int(count[i].max()) == 0 for i in pad)
    assert int(count.sum()) == int(expect.sum()) > 0 and (not feat or int(count[L.total:].min()) == 1)
    # executing the descriptors gives pack()'s bytes wherever they write
    P = pk.pack(p).detach().numpy()
    once = np.flatnonzero(count[:L.total] == 1)
    assert np.array_equal(buf[once].view(np.int32), P[once].view(np.int32))
    if feat:
        assert np.array_equal(buf[L.total:].reshape(W2, -1), p[WR1].numpy()[:, :pk.feat_dim])
    unwritten = np.flatnonzero(expect[:L.total] == 0)  # padding and absent heads are zero in pack() too; the rest is the fold's
    fold = np.concatenate([grid(L.wr1, W2, W, W + 80), np.arange(L.br1, L.br1 + W2)]) if feat else np.zeros(0, np.int64)
    assert not P[np.setdiff1d(unwritten, fold)].any()


@pytest.mark.parametrize("W,D,skips,cand,feat", PACKERS)
def test_backward_pack_descriptors_write_each_gradient_element_once(W, D, skips, cand, feat):
    pk = make_packer(W, D, skips, cand, feat)
    shapes = {k: tuple(v.shape) for k, v in seeded_params(pk).items() if k in pk.pack_names()}
    assert sorted(shapes) == sorted(pk.pack_names())
    count = {n: np.zeros(int(np.prod(s)), np.int32) for n, s in shapes.items()}
    for q, name, first in decoded(pk, shapes):
        np.add.at(count[name], grid(first, q.rows, q.cols, q.src_ld), 1)
        assert 0 <= q.dst_off and q.dst_off + (q.rows - 1) * q.dst_ld + q.cols <= pk.L.total
    for n, s in shapes.items():
        expect = np.ones(s, np.int32)
        if feat and n == WR1:
            expect[:, :pk.feat_dim] = 0  # filled by the fold's backward
        if feat and n.startswith("feat_share_layer"):
            expect[:] = 0
        assert np.array_equal(count[n].reshape(s), expect), n


def fragment_descs(pk):
    f32, nf, t32, nt = pk._descs()
    f16, nf16, t16, nt16 = pk._descs16()
    names = [f for f, _ in type(f32[0])._fields_]
    tup = lambda q: tuple(getattr(q, f) for f in names)
    assert (nf, nt) == (nf16, nt16) == (len(f32), len(t32)) and [tup(q) for q in f16] == [tup(q) for q in f32]
    assert [tup(q) for q in t16] == [tup(q) for q in t32]
    return [tup(q) for q in f32], [tup(q) for q in t32], [q.exp_id for q in f16], [q.exp_id for q in t16]


@pytest.mark.parametrize("W,D,skips", LAYOUTS)
def test_fragment_descriptors_cover_the_matrix_blocks_and_the_transposed_set(W, D, skips):
    from upnerf_amd import pass_plan as pp
    pk = make_packer(W, D, skips, 16, True)
    L, off = pk.L, lambda b: pp.block_offset(pk.L, b)
    fwd, bwd, _, _ = fragment_descs(pk)
    mats = [b for b in pp.param_blocks(W, D, pk.skip) if b.matrix]
    assert [b.field for b in mats] == ["w"] * D + ["we", "wc1", "wc2", "wr1"]  # (the kernels index the row norms in this order)
    assert fwd == [(off(b), b.ld, 0, b.rows, b.ld, off(b), b.ld, 0) for b in mats]
    tb = pp.t_blocks(W, D, pk.skip)
    want = [(off(f.src) + f.col0, f.src.ld, 1, f.cols, f.src.rows, off(t), t.ld, f.dst_col0) for t in tb for f in t.feeds]
    assert sorted(bwd) == sorted(want) and len(set(bwd)) == len(bwd)
    count = np.zeros(L.t_total, np.int32)
    for src_off, src_ld, tr, rows, cols, dst_off, kp, k0 in bwd:
        np.add.at(count, grid(dst_off + k0, rows, cols, kp), 1)
        src = next(b for b in mats if off(b) <= src_off < off(b) + b.rows * b.ld)  # rows of the copy: columns of one source block
        assert tr == 1 and src_ld == src.ld and cols == src.rows and (src_off - off(src)) + rows <= src.ld
    for t in tb:
        fed = t.field != "t_skipx" or pk.skip > 0
        assert (count[off(t):off(t) + t.rows * t.ld] == int(fed)).all(), t.field
    # a layer's own copy holds its last part, the skip block the encoding's columns, the shared head block the two first layers
    by = {(t.field, t.layer): [(f.src.field, f.src.layer, f.col0, f.cols, f.dst_col0) for f in t.feeds] for t in tb}
    for l in range(D):
        assert by["t_w", l] == [("w", l, 64 if l == pk.skip else 0, 64 if l == 0 else W, 0)]
    assert by["t_skipx", None] == ([("w", pk.skip, 0, 64, 0)] if pk.skip > 0 else [])
    assert by["t_head", None] == [("wr1", None, 0, W, 0), ("wc1", None, 0, W, W // 2)]
    assert by["t_we", None] == [("we", None, 0, W, 0)] and by["t_wc2", None] == [("wc2", None, 0, W // 2, 0)]


@pytest.mark.parametrize("W,D,skips", LAYOUTS)
def test_exponent_ids_name_one_matrix_each(W, D, skips):
    """Descriptors into one transposed block share an id; different matrices have different ids, apart from a matrix and its own
    transposed copy (a block of PT fed by that matrix alone); every id fits the [16] exponent table."""
    from upnerf_amd import pass_plan as pp
    pk = make_packer(W, D, skips, 16, True)
    off = lambda b: pp.block_offset(pk.L, b)
    fwd, bwd, fid, tid = fragment_descs(pk)
    mats = [b for b in pp.param_blocks(W, D, pk.skip) if b.matrix]
    tb = pp.t_blocks(W, D, pk.skip)
    source = lambda o: next((b.field, b.layer) for b in mats if off(b) <= o < off(b) + b.rows * b.ld)
    target = lambda o: next((t.field, t.layer) for t in tb if off(t) <= o < off(t) + t.rows * t.ld)
    feeders = {}
    for q in bwd:
        feeders.setdefault(target(q[5]), set()).add(source(q[0]))
    family = {}  # id -> the matrices that carry it
    for q, e in zip(fwd, fid):
        family.setdefault(e, set()).add(source(q[0]))
    per_target = {}
    for q, e in zip(bwd, tid):
        t = target(q[5])
        per_target.setdefault(t, set()).add(e)
        family.setdefault(e, set()).add(next(iter(feeders[t])) if len(feeders[t]) == 1 else t)
    assert all(len(ids) == 1 for ids in per_target.values()), per_target
    assert all(len(ms) == 1 for ms in family.values()), family
    assert all(0 <= e < 16 for e in fid + tid) and len(set(fid)) == len(fid)
    assert (pk.EXP_FINAL, pk.EXP_C1, pk.EXP_C2, pk.EXP_R1, pk.EXP_HEAD_T) == (8, 9, 10, 11, 12) and fid[:D] == list(range(D))
