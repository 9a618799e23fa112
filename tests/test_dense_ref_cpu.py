"""The gates of tests/dense_ref.py, proven on the CPU: an emulation of each kernel's own arithmetic stays inside its gate on every
input family (the gate is not tighter than the design), and the same emulation with one term dropped or one ragged column zeroed
leaves it on the flat family (the gate is not vacuous).  Every element takes part in every comparison (dense_ref.ratio)."""
import math

import pytest
import torch

import dense_ref as dr

M, N, K = 200, 68, 60  # ragged against every block shape, several 32-row chunks


@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, fam in enumerate(dr.FAMILIES):
        A, B = dr.family(fam, M, N, K, 100 + 2 * i)
        out[fam] = (A, B, dr.host_exponent(A), dr.host_exponent(B), dr.wgrad_ref(A, B))
    return out


def test_families_are_what_they_claim():
    A, B = dr.family("flat", M, N, K, 1)
    assert float(A.abs().min()) >= 0.5 and float(A.abs().max()) <= 1.0 and bool((A < 0).any()) and bool((A > 0).any())
    A, _ = dr.family("cols", M, N, K, 1)
    sc = (A * 2.0 ** dr.host_exponent(A)).abs()
    sub = (sc.max(0)[0] < 2.0 ** -14) & (sc.min(0)[0] >= 2.0 ** -25)
    assert int(sub.sum()) == N // 2 and float(sc[:, 0].max()) >= 2.0 ** 13
    assert float(dr.family("zeroA", M, N, K, 1)[0].abs().max()) == 0.0 and dr.host_exponent(torch.zeros(3)) == 14 + 99
    for p, tag in ((-3, "m3"), (0, "0"), (5, "5")):
        assert float(dr.family("pow2_" + tag, M, N, K, 1)[0].abs().max()) == 2.0 ** p
        mx = float(dr.family("below_" + tag, M, N, K, 1)[0].abs().max())
        assert mx == dr.below(2.0 ** p) and mx < 2.0 ** p
        assert dr.host_exponent(torch.tensor([2.0 ** p])) == 14 - p == dr.host_exponent(torch.tensor([mx]))
    A, B = dr.family("tiny60", M, N, K, 1)
    assert dr.host_exponent(A) + dr.host_exponent(B) > 126
    assert float((A.double().t() @ B.double()).abs().min()) > 0  # (and every |entry| is far above fp32's smallest normal)
    A, B = dr.family("rows12", M, N, K, 1)
    assert float(A.abs().max()) > 2048 and int((A.abs().max(1)[0] > 2).sum()) == 3


@pytest.mark.parametrize("planes", [0, 1, 2])
def test_f16_emulation_is_inside_its_gate_on_every_family(cases, planes):
    for fam, (A, B, ea, eb, ref) in cases.items():
        got = dr.emulate_f16(A, B, ea, eb, planes)
        r = dr.ratio(got, ref["dW"], dr.gate_f16(ref, M, ea, eb, planes))
        assert r <= 1, (fam, planes, r)
        if fam == "zeroA":
            assert float(got.abs().max()) == 0.0
        if fam == "tiny60":
            assert bool(torch.isfinite(got).all()) and float(got.abs().min()) > 0


@pytest.mark.parametrize("planes", [0, 1, 2])
def test_f16_gate_sees_one_lost_term_and_one_lost_column(cases, planes):
    A, B, ea, eb, ref = cases["flat"]
    gate = dr.gate_f16(ref, M, ea, eb, planes)
    if planes != 1:
        # one lost term moves its element by >= 1/4 = S / (4 M); the three-term gate at M <= 512 is below S * 4e-5
        assert float((gate / ref["S"]).max()) < 1.0 / (40 * M)
        assert dr.ratio(dr.emulate_f16(A, B, ea, eb, planes, drop=(M - 1, N - 1, K - 1)), ref["dW"], gate) > 1
        assert dr.ratio(dr.emulate_f16(A, B, ea, eb, planes, drop=(0, 3, 5)), ref["dW"], gate) > 1
    # (planes = 1 carries 2^-10 of S by design: at M = 200 one term of 1/4 .. 1 among S ~ 110 is inside it; a lost column is not)
    assert dr.ratio(dr.emulate_f16(A, B, ea, eb, planes, zero_col=K - 1), ref["dW"], gate) > 1
    small = slice(0, 8)  # and at M = 8 the rounded-operand gate sees a single term too
    refs = dr.wgrad_ref(A[small], B[small])
    gs = dr.gate_f16(refs, 8, ea, eb, planes)
    assert dr.ratio(dr.emulate_f16(A[small], B[small], ea, eb, planes), refs["dW"], gs) <= 1
    assert dr.ratio(dr.emulate_f16(A[small], B[small], ea, eb, planes, drop=(7, 1, 2)), refs["dW"], gs) > 1


def test_fp32_emulation_is_inside_its_gate_and_a_lost_term_is_not(cases):
    for fam in dr.FAMILIES:
        A, B, _, _, ref = cases[fam]
        r = dr.ratio(dr.emulate_fp32(A, B), ref["dW"], dr.gate_fp32(M, ref["S"]))
        assert r <= 1, (fam, r)
        db = A.double().sum(0).float()
        assert dr.ratio(db, ref["db"], dr.gate_fp32(M, ref["sa"])) <= 1, fam
    A, B, _, _, ref = cases["flat"]
    assert dr.ratio(dr.emulate_fp32(A, B, drop=(M - 1, N - 1, K - 1)), ref["dW"], dr.gate_fp32(M, ref["S"])) > 1
    assert float((dr.gate_fp32(512, torch.tensor(1.0)))) < 1.0 / (40 * 512)  # M = 512: a lost term (S / 4M) is > 10 gates


def test_ratio_counts_every_element_and_fails_on_nan():
    ref = torch.ones(3, 4, dtype=torch.float64)
    assert dr.ratio(ref.float(), ref, 0.0) == 0.0
    bad = ref.clone().float()
    bad[2, 3] += 1e-3
    assert dr.ratio(bad, ref, 1e-4) > 1 and dr.ratio(bad, ref, 0.0) == math.inf
    bad[0, 0] = float("nan")
    assert math.isnan(dr.ratio(bad, ref, 1.0)) and not dr.ratio(bad, ref, 1.0) <= 1


def test_linear_gate_sees_a_dropped_k_element():
    x, w = dr.flat((65, 72), 5), dr.flat((5, 72), 6)
    bias = dr.flat((5,), 7)
    pre, S = dr.linear_ref(x, w, bias)
    got = (x.double() @ w.double().t() + bias.double()).float()
    assert dr.ratio(got, pre, dr.gate_fp32(73, S)) <= 1
    lost = (x[:, :71].double() @ w[:, :71].double().t() + bias.double()).float()  # the last element of the ragged chunk
    assert dr.ratio(lost, pre, dr.gate_fp32(73, S)) > 1


def test_adam_formula_matches_torch_adam_including_the_overflow():
    p, g, m, v = dr.adam_table(3)
    lr, b1, b2, eps, step = 1e-3, 0.9, 0.999, 1e-8, 2
    ss, bc2 = dr.adam_bias_scalars(lr, b1, b2, step)
    p32, m32, v32, _ = dr.adam_formula(p, g, m, v, b1, b2, eps, ss, bc2, torch.float32)
    _, _, v64, _ = dr.adam_formula(p, g, m, v, b1, b2, eps, ss, bc2, torch.float64)
    tp, tm, tv = dr.torch_adam(p, g, m, v, lr, b1, b2, eps, step)
    inf = torch.isinf(tv)
    assert bool(inf.any()) and bool((torch.isinf(v32) == inf).all())
    assert torch.equal(p32[inf], tp[inf]) and torch.equal(tp[inf], p[inf])  # update 0
    # (finite elements: torch forms 1 - beta2 in double and rounds it, the kernel's comment subtracts in fp32 -- 5e-5 apart in the
    # weight of g^2 -- so torch is the reference of the overflow's OUTCOME only; the values are held to the kernel's own formula)
    assert bool(torch.isinf(v64[inf]).logical_not().all())  # fp64 does not overflow there: the gate cannot speak about them


def test_frag16_byte_offsets_are_a_bijection_per_block():
    for perm in (0, 1):
        seen = {dr.frag16_byte(r, k, 48, pl, perm) for r in range(64) for k in range(48) for pl in (0, 1)}
        assert len(seen) == 64 * 48 * 2 and min(seen) == 0 and max(seen) == 64 * 48 * 4 - 2
    assert dr.frag16_exponent(0.0) == 0 and dr.frag16_exponent(1.0) == 13 and dr.frag16_exponent(dr.below(1.0)) == 14
