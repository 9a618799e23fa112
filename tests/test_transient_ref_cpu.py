"""CPU proof of the gates of tests/transient_ref.py (module docstring there): an fp32 emulation of every stage of
csrc/transient.hip (torch float32 on the CPU) stays inside its gate at every R and on every input family that
tests/test_hip_transient.py runs, and each planted defect lands outside the gate of the stage it corrupts:
    one 16-wide k-group dropped / fed from the neighbouring group's weights     in each of the six forward and six backward layers
    the ReLU mask of row R - 1 taken from row R - 2                             in gz_t and gz_h[3..0]  (R >= 2: at R = 1 there is
                                                                                no row R - 2 and the defect does not exist)
    the rank-1 alpha term left out of gz_h[3];  dz_beta without the alpha factor;  g_temb columns shifted by 64.
All of them are pushed outside with O(1) inputs (normal features and upstreams, the synth weights): a lost k-group moves an
element by about 4 |x| |w| ~ 1e-1 against gates of 1e-5, a wrong mask row replaces about half of a row's elements by a value of
the gradient's own size or by 0 against a gate of 0, and alpha is about 1/2 on the synth family, so dz_beta is off by its own size.
"""
import math

import pytest
import torch

import transient_ref as tr


@pytest.fixture(scope="module")
def fams():
    return {name: tr.family(name) for name in tr.FAMILIES}


def _case(fams, name, R, off=0):
    P, feat, temb, up = fams[name]
    return P, tr.rows(feat, off, R), tr.rows(temb, off, R), tuple(tr.rows(u, off, R) for u in up)


def test_heads_family_is_where_it_says(fams):
    P, feat, temb, _ = fams["heads"]
    f = tr.heads_family_facts(P, feat, temb)
    assert f["spre_margin"] > 1e-3 and f["above"] > 0 and f["below"] > 0, f
    assert f["spre_lo"] < -29 and f["spre_hi"] > 39, f
    assert min(f["alpha_one"], f["alpha_small"], f["rgb_one"], f["rgb_small"]) > 0, f
    assert min(f["first8"].values()) > 0, f  # every R >= 15 holds all of them; R = 1 visits offsets 0 .. 7
    # the dead family: a whole plane of h is zero already in fp64
    P, feat, temb, _ = fams["dead"]
    assert float(tr.forward64(P, feat, temb)["h"][2].abs().max()) == 0.0


@pytest.mark.parametrize("name", tr.FAMILIES)
@pytest.mark.parametrize("R", tr.RS)
def test_fp32_emulation_is_inside_every_gate(fams, name, R):
    for off in tr.offsets(name, R):
        P, feat, temb, up = _case(fams, name, R, off)
        fwd = tr.emulate_fwd(P, feat, temb)
        res = tr.forward_checks(P, feat, temb, fwd)
        for ups in (up, (up[0], None, up[2]), (None, up[1], None)):
            res.update({f"{k} {[u is not None for u in ups]}": v for k, v in
                        tr.backward_checks(P, fwd, ups, tr.emulate_bwd(P, fwd, ups)).items()})
        bad = {k: v for k, v in res.items() if not v <= 1}
        assert not bad, (name, R, off, bad)
        if name == "dead":
            b = tr.emulate_bwd(P, fwd, up)
            assert all(float(b["gz_h"][l].abs().max()) == 0.0 for l in (2, 1, 0)) and float(b["g_feat"].abs().max()) == 0.0


def _ratios(P, feat, temb, up, defect):
    """Ratios of an emulated run with one defect; the backward runs on the defective forward's stored outputs, as the kernel's
    would, so a forward defect must show in its own stage and nowhere else."""
    fwd = tr.emulate_fwd(P, feat, temb, defect=defect)
    res = tr.forward_checks(P, feat, temb, fwd)
    res.update(tr.backward_checks(P, fwd, up, tr.emulate_bwd(P, fwd, up, defect=defect)))
    return res


PLANTED = ([(k, s) for k in ("drop_kgroup", "swap_kgroup") for s in tr.FWD_LAYERS + tr.BWD_LAYERS]
           + [("mask_prev_row", s) for s in tr.MASKED]
           + [("no_rank1", "gz_h3"), ("dz_beta_no_alpha", "dz_heads"), ("temb_shift64", "g_temb")])


@pytest.mark.parametrize("defect", PLANTED, ids=lambda d: f"{d[0]}-{d[1]}")
@pytest.mark.parametrize("R", [17, 33])
def test_planted_defect_is_outside_its_gate(fams, defect, R):
    P, feat, temb, up = _case(fams, "synth", R)
    res = _ratios(P, feat, temb, up, defect)
    stage = defect[1]
    hit = res.pop(stage)
    if stage == "gz_e":  # (one product, two destinations: a k-group of gz_t . W_t lost shows in both)
        assert not res.pop("g_temb") <= 1
    assert not hit <= 1 and (math.isinf(hit) or hit > 10), (defect, R, hit)
    # stage-local: every OTHER stage reads the defective stage's stored output and stays inside its own gate
    bad = {k: v for k, v in res.items() if not v <= 1}
    assert not bad, (defect, R, bad)


def test_mask_defect_needs_a_second_row(fams):
    """At R = 1 `row R - 2` does not exist: the emulation has no defect to plant and stays inside."""
    P, feat, temb, up = _case(fams, "synth", 1)
    res = _ratios(P, feat, temb, up, ("mask_prev_row", "gz_h3"))
    assert all(v <= 1 for v in res.values()), res


def test_a_nan_and_a_nonzero_where_zero_is_due_fail(fams):
    P, feat, temb, up = _case(fams, "dead", 17)
    fwd = tr.emulate_fwd(P, feat, temb)
    b = tr.emulate_bwd(P, fwd, up)
    b["gz_h"][1, 3, 7] = 1e-30  # h[1] > 0 there or not: upstream of the dead layer the limit is 0
    assert math.isinf(tr.backward_checks(P, fwd, up, b)["gz_h1"])
    fwd["e"][5, 9] = float("nan")
    assert math.isnan(tr.forward_checks(P, feat, temb, fwd)["e"])
    fwd = tr.emulate_fwd(P, feat, temb)
    fwd["h"][2, 0, 0] = -1e-30  # a ReLU output below 0
    assert math.isinf(tr.forward_checks(P, feat, temb, fwd)["h2"])
