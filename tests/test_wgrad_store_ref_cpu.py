"""The bounds of tests/wgrad_store_ref.py, proven on the CPU: an emulation of the stored-operand kernels' arithmetic stays inside
them on every input family (they are not tighter than the design), each listed slip leaves them -- by more than a factor of 10 on
the flat family, which the reference alone guarantees (asserted) -- and the fragment index map, stated from the header, is the one
rendering.quant16_frag / dequant16 implement.  The arithmetic the kernels had before (exponent difference clamped at -24, f24's
residual decoded as v * s + o with s = f / 32 rounded to fp16) is shown OUTSIDE the bounds on the far-tile family: that is the
finding the kernel change of this module's pull request answers."""
import pytest
import torch

import dense_ref as dr
import wgrad_store_ref as ws

W = 32   # two fragment k-blocks; the bounds are per element, the width adds nothing
M_OF = {"tile": 200, "frag": 77, "f24": 200, "planes": 192}   # ragged last tile where the kind allows one; >= 3 tiles


def pair(kind, fam, M, seed, b_fam=None, side="A", **kw):
    """(A, B, ea, eb): A of the family, B of b_fam (default: the same family; flat beside zeros and beside a far tile, whose
    products would otherwise be 2^-2far); side = "B": the other way round."""
    other = b_fam or ("flat" if fam in ("zero", "zerotile", "far") else fam)
    (A, fa), (B, fb) = ws.family(kind, fam, M, W, seed, **kw), ws.family(kind, other, M, W, seed + 50)
    if side == "B":
        A, fa, B, fb = B, fb, A, fa
    ea = fa if fa is not None else ws.tensor_exponent(A)
    eb = fb if fb is not None else ws.tensor_exponent(B)
    return A, B, ea, eb


def inside(A, B, ea, eb, **kw):
    ref = ws.reference(A, B, ea, eb)
    got = ws.emulate(A, B, ea, eb, **kw)
    return dr.ratio(got["dW"], ref["dW"], ref["gate"]), dr.ratio(got["db"], ref["db"], ref["gate_db"])


# ------------------------------------------------------------------------------------------------ encoders, decoders, the map
def test_fragment_map_is_the_one_of_quant16_frag_and_dequant16():
    from upnerf_amd import rendering as rd
    for Mp, Wf in ((64, 128), (96, 256)):
        rows = dr.flat((Mp, Wf), 5)
        texp = torch.randint(-3, 4, (Mp // 32,), generator=dr._gen(6)).to(torch.int32)
        theirs = rd.quant16_frag(rows, texp)                     # fragment order, fp16
        st = ws.encode("frag", rows, texp)
        mine = ws.device_image(st)["p"]
        assert torch.equal(theirs.reshape(-1).view(torch.int16), mine)
        back = rd.dequant16(theirs[None], texp[None], frag=True)[0].double()
        assert torch.equal(back, ws.decode(st))
        assert torch.equal(ws.from_frag(mine, Mp, Wf), st.hi.view(torch.int16))
    idx = ws.frag_index(32, 16)   # the header's formula, spot values: (row 5, feature 13) = lane 32 + 5, j = 4 + 1
    assert int(idx[5, 13]) == (32 + 5) * 8 + 5 and int(idx[0, 0]) == 0 and int(idx[31, 3]) == 31 * 8 + 3 and int(idx[0, 4]) == 32 * 8


@pytest.mark.parametrize("kind", ws.KINDS)
def test_decoders_state_the_header_and_encoders_invert_them(kind):
    M = M_OF[kind]
    st, _ = ws.family(kind, "tiles10", M, W, 3)
    x = ws.decode(st)
    m, c = M - 1, 7
    e = int(st.exp[m // ws.TILE[kind]])
    lo = {"tile": 0.0, "frag": 0.0, "f24": (int(st.lo[m, c]) - 128) / 32.0 if kind == "f24" else 0.0,
          "planes": float(st.lo[m, c]) if kind == "planes" else 0.0}[kind]
    assert float(x[m, c]) == (float(st.hi[m, c]) + lo) * 2.0 ** -e
    again = ws.encode(kind, x, st.exp)   # the decoded value is stored as the same bits
    assert torch.equal(ws.decode(again), x)   # (planes: a residual of exactly half an ulp may move to the neighbouring hi)
    assert kind == "planes" or (torch.equal(again.hi, st.hi) and (st.lo is None or torch.equal(again.lo, st.lo)))
    src = dr.flat((M, W), 3).double() * ws.pow2(14 - st.row_exp())[:, None]
    tol = {"tile": 2.0 ** -11, "frag": 2.0 ** -11, "f24": 2.0 ** -19, "planes": 2.0 ** -21}[kind]  # of the tile's peak 2^14
    assert float(((x - src).abs() * ws.pow2(st.row_exp())[:, None]).max()) <= tol * 2.0 ** 14
    img = ws.device_image(st, ld=W + 8)
    t = ws.TILE[kind]
    assert img["Mp"] % t == 0 and img["exp"].numel() == img["Mp"] // t
    if kind != "frag":
        assert bool((img["p"][M:] == ws.NAN16).all()) and bool((img["p"][:, W:] == ws.NAN16).all())


def test_families_are_what_they_claim():
    for kind in ws.KINDS:
        M = M_OF[kind]
        st, f = ws.family(kind, "flat", M, W, 1)
        x = ws.decode(st).abs()
        assert f is None and float(x.min()) >= 0.5 - 2.0 ** -11 and float(x.max()) <= 1.0 and len(set(st.exp.tolist())) == 1
        st, _ = ws.family(kind, "tiles10", M, W, 1)
        assert int(st.exp.max()) - int(st.exp.min()) == 10
        st, _ = ws.family(kind, "zerotile", M, W, 1)
        t = ws.TILE[kind]
        tz = st.exp.numel() // 2
        assert float(ws.decode(st)[tz * t:(tz + 1) * t].abs().max()) == 0.0 and float(ws.decode(st).abs().max()) > 0
        assert float(ws.decode(ws.family(kind, "zero", M, W, 1)[0]).abs().max()) == 0.0
        st, f = ws.family(kind, "peak", M, W, 1)
        assert f == 14 and float(st.hi.float().max()) == ws.H_MAX and float(st.hi.float().min()) == -ws.H_MAX
        assert float(st.hi.float().abs().min()) == ws.H_MIN
        for far in ws.FAR:
            st, _ = ws.family(kind, "far", M, W, 1, far=far, small_col=5)
            assert ws.tensor_exponent(st) == 14 and int(st.exp[-1]) - 14 == far
            assert float(st.hi[-1].float().abs().min()) >= 2.0 ** 12      # the far tile's planes are as large as any
            assert float(st.hi[0, 5].float().abs()) <= 2.0 ** -12          # and column 5 is small everywhere else
    st, _ = ws.family("f24", "resid", 200, W, 1)
    assert set(st.lo.unique().tolist()) == {0, 128, 255} and float(st.hi.float().abs().max()) <= 0.125
    st, _ = ws.family("planes", "resid", 192, W, 1)
    assert bool((torch.sign(st.lo.float()) == -torch.sign(st.hi.float())).all())
    assert bool((st.lo.double().abs() * 2 == ws.ulp16(st.hi)).all())


# -------------------------------------------------------------------------------------- the emulation is inside every bound
def cases(kind):
    M = M_OF[kind]
    out = [("flat", {}), ("tiles10", {}), ("zerotile", {}), ("zero", {}), ("peak", {})]
    if kind in ws.TWO_PLANES:
        out.append(("resid", {}))
    for far in ws.FAR:
        out += [("far", dict(far=far)), ("far", dict(far=far, small_col=5)), ("far", dict(far=far, far_tile=0, small_col=5, side="B")),
                ("far", dict(far=far, b_fam="far"))]
    return M, out


@pytest.mark.parametrize("kind", ws.KINDS)
def test_emulation_is_inside_the_bounds_on_every_family(kind):
    M, fams = cases(kind)
    for i, (fam, kw) in enumerate(fams):
        for Mx in (M, 1, 33 if kind != "planes" else 64):
            A, B, ea, eb = pair(kind, fam, Mx, 100 + i, **kw)
            r, rb = inside(A, B, ea, eb)
            assert r <= 1 and rb <= 1, (kind, fam, kw, Mx, r, rb)
            if fam == "zero":
                got = ws.emulate(A, B, ea, eb)
                assert float(got["dW"].abs().max()) == 0.0 and float(got["db"].abs().max()) == 0.0
                assert float(ws.reference(A, B, ea, eb)["gate"].max()) == 0.0
            if kind in ("tile", "frag", "f24") and fam in ("flat", "tiles10", "far"):  # fp32 B beside the stored A (the encoding x0)
                Bf = dr.flat((Mx, 16), 300 + i)
                ebf = dr.host_exponent(Bf)
                r, rb = inside(A, Bf, ea, ebf)
                assert r <= 1 and rb <= 1, (kind, fam, kw, Mx, "fp32 B", r)


@pytest.mark.parametrize("kind", ws.KINDS)
def test_the_clamped_rescale_is_outside_the_bound_on_far_tiles(kind):
    """The finding: with the exponent difference clamped at -24 a tile 2^-25 (2^-40) below the tensor's maximum enters 2 (2^16)
    times too large.  Behind a large S that hides; in the column that is small everywhere it is far outside the floor."""
    M = M_OF[kind]
    for far in (10, 23, 24):
        A, B, ea, eb = pair(kind, "far", M, 7, far=far, small_col=5)
        if kind != "f24" or far == 10:  # (f24's old byte decode lost s = f / 32 below 2^-19 already)
            assert max(inside(A, B, ea, eb, legacy=True)) <= 1, (kind, far)
    for far in (25, 40):
        for side in "AB":
            A, B, ea, eb = pair(kind, "far", M, 7, far=far, small_col=5, side=side)
            r, _ = inside(A, B, ea, eb, legacy=True)
            assert r > 10, (kind, far, side, r)
            assert max(inside(A, B, ea, eb)) <= 1


def test_the_old_byte_decode_is_outside_the_bound_below_2_to_the_minus_19():
    A, B, ea, eb = pair("f24", "far", 200, 7, far=19, small_col=5)   # s = 2^-24: the last exponent difference it survives
    assert max(inside(A, B, ea, eb, legacy=True)) <= 1
    for far, least in ((20, 1), (23, 1), (24, 1)):   # s rounds to zero: every residual of the tile decodes as -4 f
        A, B, ea, eb = pair("f24", "far", 200, 7, far=far, small_col=5)
        assert inside(A, B, ea, eb, legacy=True)[0] > least and max(inside(A, B, ea, eb)) <= 1
    A, B, ea, eb = pair("f24", "zero", 65, 9)   # ea = 113: s = 2^10 and o = -2^17 overflow fp16, inf - inf
    assert not inside(A, B, ea, eb, legacy=True)[0] <= 1


# ------------------------------------------------------------------------------------------- each listed slip lands outside
MUT_KINDS = {"last_row": ws.KINDS, "neighbour_exp": ws.KINDS, "drop_lo": ws.TWO_PLANES, "byte127": ("f24",), "lane_half": ("frag",),
             "col_block": ws.KINDS}


@pytest.mark.parametrize("mut", ws.MUTATIONS)
def test_every_listed_slip_is_more_than_ten_gates_away(mut):
    for kind in MUT_KINDS[mut]:
        M = {"tile": 65, "frag": 33, "f24": 65, "planes": 64 if mut == "drop_lo" else 128}[kind]   # a ragged row in a tile of its own
        # the flat family, except where it cannot show the slip: equal exponents hide a neighbour's, and under full-size hi
        # planes one unit of a residual byte (2^-19 of the peak) is below the accumulation term -- the byte-carried family shows it
        fam = {"neighbour_exp": "tiles10", "byte127": "resid"}.get(mut, "flat")
        A, B, ea, eb = pair(kind, fam, M, 11, b_fam="flat")
        ref = ws.reference(A, B, ea, eb)
        if fam == "flat":  # the condition on the inputs: a lost term is >= 1/4, the gate below 1/40 everywhere
            assert float(ref["gate"].max()) < 1.0 / 40 and float(ref["gate_db"].max()) < 0.5 / 10
            assert float(ref["A"].abs().min()) >= 0.499 and float(ref["B"].abs().min()) >= 0.499
        assert max(inside(A, B, ea, eb)) <= 1
        got = ws.emulate(A, B, ea, eb, mut=mut)
        r = dr.ratio(got["dW"], ref["dW"], ref["gate"])
        assert r > 10, (mut, kind, r)
        if mut in ("last_row", "byte127"):
            assert dr.ratio(got["db"], ref["db"], ref["gate_db"]) > 10, (mut, kind)
        if kind in ("tile", "frag", "f24") and mut in ("last_row", "col_block"):  # fp32 B: 2^-11 S by design, M small enough
            Ms = 33
            As, Bf = A.rows(Ms), dr.flat((Ms, 16), 12)
            eas, ebf = ws.tensor_exponent(As), dr.host_exponent(Bf)
            ref = ws.reference(As, Bf, eas, ebf)
            assert float(ref["gate"].max()) < 1.0 / 40
            assert dr.ratio(ws.emulate(As, Bf, eas, ebf, mut=mut)["dW"], ref["dW"], ref["gate"]) > 10, (mut, kind, "fp32 B")


def test_vec_gate_sees_a_lost_row():
    st, _ = ws.family("frag", "flat", 77, W, 21)
    v = dr.flat((77, 3), 22)
    ref = ws.vec_reference(v, st, 77)
    x = ws.decode(st)
    got = (v.double().t() @ x).float()
    assert dr.ratio(got, ref["dw"], ref["gate"]) <= 1 and float(ref["gate"].max()) < 1.0 / 40
    lost = (v[:-1].double().t() @ x[:-1]).float()
    assert dr.ratio(lost, ref["dw"], ref["gate"]) > 10
