"""csrc/transient.hip (upnerf_transient_fwd / upnerf_transient_bwd) through the C ABI, stage by stage against fp64, at
R in {1, 15, 16, 17, 33, 129} (one ragged tile, exactly one tile, one row into the second, three tiles, nine workgroups: the
weight warm-up's second slice).  tests/test_hip_kernels.py reaches the kernels only through the autograd wrapper and gates
normalised by a tensor's maximum, and never looks at h, e, t, spre, dz_heads, gz_t, gz_e, gz_h or g_temb.

References, gates and input families are those of tests/transient_ref.py (derivations in its module docstring; proved on an
fp32 emulation and on planted defects by tests/test_transient_ref_cpu.py): every stage's fp64 reference starts from the kernel's
own stored output of the stage before it, dense stages are held to L u S per element, element-wise stages to 4 e32 + 2^-22 scale
(alpha and rgb plus a quarter of their dot product's L u S), a backward mask is exact and asks for exact zeros.  Every gate is
computed on the CPU from the inputs of its stage, no element is left out, a NaN fails, a limit of 0 asks for exactly 0.

Every output buffer has 16 rows of a sentinel in front of it and behind it, which have to be untouched afterwards.  The four
[R][256] planes of h and of gz_h are ONE allocation by the ABI (plane l starts at h + l R 256), so nothing can stand between
them: a store past the end of plane l lands in the first rows of plane l + 1, which are compared like every other row.

Null pointers: each of d_alpha, d_rgb, d_beta null on its own is bitwise the call with an all-zero upstream, and every output
that does not depend on the missing input is bitwise the full call's; g_temb null, and the training step's case (d_rgb and g_feat
null), leave every other output bitwise unchanged.  A null required pointer or R = 0 is UPNERF_EINVAL and writes nothing.  Two
runs of the same call are bitwise equal.

Worst measured ratio error / gate on an MI355X (gate: <= 1), over all families and R:
    forward    h[0..3] 0.016   e 0.015   t 0.019   spre 0.007   alpha 0.06   rgb 0.05   beta 0.29
    backward   dz_heads 0.41 (0.59 with a null upstream)   gz_t 0.67   gz_e 0.035   g_temb 0.044   gz_h[3..0] 0.017   g_feat 0.02
The 256- and 384-term sums sit far inside L u S, a worst-case bound whose L the matrix cores' 4-deep steps and the random signs
never come near; gz_t is a sum of FOUR products (L = 4), where the bound is nearly attainable; beta and dz_heads are a handful of
fp32 operations held to 4 e32 + 4 ulp.
"""
import ctypes as C
import math

import pytest
import torch

import transient_ref as tr

pytestmark = pytest.mark.gpu

SENT = -7.25
GUARD = 16
EINVAL = -1  # UPNERF_EINVAL (include/upnerf_hip.h)
WORST = {}
FWD_OUT = dict(h=(4, 256), e=(1, 256), t=(1, 128), alpha=(1, 1), rgb=(1, 3), beta=(1, 1), spre=(1, 1))       # planes, columns
BWD_OUT = dict(dz_heads=(1, 8), gz_t=(1, 128), gz_e=(1, 256), gz_h=(4, 256), g_temb=(1, 128), g_feat=(1, 384))


@pytest.fixture(scope="module")
def hip():
    from upnerf_amd import _lib
    return dict(L=_lib, lib=_lib.lib)


@pytest.fixture(scope="module")
def fams():
    out = {}
    for name in tr.FAMILIES:
        P, feat, temb, up = tr.family(name)
        out[name] = dict(P=P, feat=feat, temb=temb, up=up, Pd={k: P[k].cuda() for k in tr.NAMES})
    return out


def note(part, r):
    """Keeps the worst ratio of a part and prints it (pytest -s shows the figures before the assertion)."""
    WORST[part] = r if math.isnan(r) else max(WORST.get(part, 0.0), r)
    print(f"[transient] {part}: ratio {r:.3f} (worst so far {WORST[part]:.3f})")
    return r


class Buf:
    """[planes * R][cols] floats between two guards of 16 sentinel rows."""

    def __init__(self, R, planes, cols):
        self.R, self.planes, self.cols = R, planes, cols
        self.t = torch.full((2 * GUARD + planes * R, cols), SENT, device="cuda")
        self.ptr = self.t.data_ptr() + 4 * GUARD * cols

    def read(self):
        """The body on the CPU ([R] for one column, [4][R][cols] for four planes); asserts the guards."""
        c = self.t.detach().cpu()
        assert bool((c[:GUARD] == SENT).all()) and bool((c[-GUARD:] == SENT).all()), "sentinel rows overwritten"
        b = c[GUARD:-GUARD]
        b = b.reshape(self.planes, self.R, self.cols) if self.planes > 1 else b
        return b[:, 0].contiguous() if self.cols == 1 else b.contiguous()

    def untouched(self):
        return bool((self.t == SENT).all())


def run_fwd(hip, fam, off, R):
    L = hip["L"]
    feat, temb = tr.rows(fam["feat"], off, R).cuda(), tr.rows(fam["temb"], off, R).cuda()
    bufs = {k: Buf(R, *pc) for k, pc in FWD_OUT.items()}
    a = L.TransientArgs(R=R, beta_min=tr.BETA_MIN, feat=feat.data_ptr(), t_emb=temb.data_ptr(),
                        **{k: fam["Pd"][k].data_ptr() for k in tr.NAMES}, **{k: b.ptr for k, b in bufs.items()})
    assert hip["lib"].upnerf_transient_fwd(C.byref(a), None) == 0
    torch.cuda.synchronize()
    return a, bufs, {k: b.read() for k, b in bufs.items()}, (feat, temb)


def run_bwd(hip, a, R, up, temb=True, feat=True):
    """up: three CPU tensors or None.  Returns the outputs on the CPU (None for an output that was not asked for)."""
    L = hip["L"]
    upd = [None if u is None else u.contiguous().cuda() for u in up]
    bufs = {k: Buf(R, *pc) for k, pc in BWD_OUT.items()}
    want = dict(g_temb=temb, g_feat=feat)
    g = L.TransientGrads(d_alpha=None if upd[0] is None else upd[0].data_ptr(), d_rgb=None if upd[1] is None else upd[1].data_ptr(),
                         d_beta=None if upd[2] is None else upd[2].data_ptr(),
                         **{k: (b.ptr if want.get(k, True) else None) for k, b in bufs.items()})
    assert hip["lib"].upnerf_transient_bwd(C.byref(a), C.byref(g), None) == 0
    torch.cuda.synchronize()
    out = {}
    for k, b in bufs.items():
        if want.get(k, True):
            out[k] = b.read()
        else:
            assert b.untouched(), k
            out[k] = None
    return out


def same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def all_same_bits(a, b, but=()):
    return [k for k in a if k not in but and a[k] is not None and b[k] is not None and not same_bits(a[k], b[k])]


def gated(tag, res, what):
    for k, r in res.items():
        note(f"{tag} {k}", r)
    bad = {k: r for k, r in res.items() if not r <= 1}
    assert not bad, (what, bad)


# =========================================================================================== 1. every stage against fp64
def test_input_families_are_where_they_say(fams):
    f = fams["heads"]
    facts = tr.heads_family_facts(f["P"], f["feat"], f["temb"])
    assert facts["spre_margin"] > 1e-3 and facts["above"] > 0 and facts["below"] > 0, facts
    assert facts["spre_lo"] < -29 and facts["spre_hi"] > 39 and min(facts["first8"].values()) > 0, facts
    assert min(facts["alpha_one"], facts["alpha_small"], facts["rgb_one"], facts["rgb_small"]) > 0, facts


@pytest.mark.parametrize("name", tr.FAMILIES)
@pytest.mark.parametrize("R", tr.RS)
def test_every_stage_against_fp64(hip, fams, name, R):
    fam = fams[name]
    for off in tr.offsets(name, R):
        up = tuple(tr.rows(u, off, R) for u in fam["up"])
        a, bufs, fwd, keep = run_fwd(hip, fam, off, R)  # (bufs, keep: the device memory `a` points to)
        assert not all_same_bits(fwd, run_fwd(hip, fam, off, R)[2]), "forward not reproducible"
        gated("fwd", tr.forward_checks(fam["P"], tr.rows(fam["feat"], off, R), tr.rows(fam["temb"], off, R), fwd), (name, R, off))
        bwd = run_bwd(hip, a, R, up)
        assert not all_same_bits(bwd, run_bwd(hip, a, R, up)), "backward not reproducible"
        gated("bwd", tr.backward_checks(fam["P"], fwd, up, bwd), (name, R, off))
        if name == "heads":  # saturated rows: exactly 1.0f gives a gradient of exactly 0 (the gate above is 0 there; said again)
            one = fwd["alpha"] == 1.0
            assert float(bwd["dz_heads"][one][:, 0].abs().max() if one.any() else 0.0) == 0.0
            assert float(bwd["dz_heads"][:, 2:5][fwd["rgb"] == 1.0].abs().sum()) == 0.0
            assert float(bwd["dz_heads"][:, 5:].abs().max()) == 0.0
        if name == "dead":
            assert float(fwd["h"][2].abs().max()) == 0.0
            assert all(float(bwd["gz_h"][l].abs().max()) == 0.0 for l in (2, 1, 0)) and float(bwd["g_feat"].abs().max()) == 0.0


# ===================================================================================================== 2. null pointers
@pytest.mark.parametrize("R", tr.RS)
def test_null_pointers(hip, fams, R):
    fam = fams["synth"]
    up = tuple(tr.rows(u, 0, R) for u in fam["up"])
    a, bufs, fwd, keep = run_fwd(hip, fam, 0, R)  # (bufs, keep: the device memory `a` points to)
    full = run_bwd(hip, a, R, up)
    # (missing upstream, the outputs that do not depend on it, and the columns of dz_heads that do not)
    cases = ((0, ("gz_t", "gz_e", "g_temb"), slice(1, 8)), (1, (), slice(0, 2)), (2, (), slice(2, 8)))
    for j, indep, cols in cases:
        ups = tuple(None if i == j else u for i, u in enumerate(up))
        zer = tuple(torch.zeros_like(u) if i == j else u for i, u in enumerate(up))
        null, zero = run_bwd(hip, a, R, ups), run_bwd(hip, a, R, zer)
        assert not all_same_bits(null, zero), (R, j, "a null upstream is not an all-zero upstream")
        assert same_bits(null["dz_heads"][:, cols], full["dz_heads"][:, cols]), (R, j)
        for k in indep:
            assert same_bits(null[k], full[k]), (R, j, k)
        gated("null", tr.backward_checks(fam["P"], fwd, ups, null), (R, j))
    # g_temb null: everything else unchanged
    assert not all_same_bits(run_bwd(hip, a, R, up, temb=False), full), R
    assert not all_same_bits(run_bwd(hip, a, R, up, feat=False), full), R
    assert not all_same_bits(run_bwd(hip, a, R, up, temb=False, feat=False), full), R
    # the training step's call: no d_rgb, no g_feat
    ups = (up[0], None, up[2])
    train, ref = run_bwd(hip, a, R, ups, feat=False), run_bwd(hip, a, R, ups)
    assert not all_same_bits(train, ref), R
    gated("null", tr.backward_checks(fam["P"], fwd, ups, train), (R, "training step"))
    # all three null: every gradient is exactly zero
    none = run_bwd(hip, a, R, (None, None, None))
    assert all(float(v.abs().max()) == 0.0 for v in none.values()), R


# ============================================================================================================ 3. refusals
def test_refusals_write_nothing(hip, fams):
    L, lib = hip["L"], hip["lib"]
    fam, R = fams["synth"], 17
    a, bufs, fwd, keep = run_fwd(hip, fam, 0, R)  # (bufs, keep: the device memory `a` points to)
    up = [u[:R].contiguous().cuda() for u in fam["up"]]
    fb = {k: Buf(R, *pc) for k, pc in FWD_OUT.items()}
    bb = {k: Buf(R, *pc) for k, pc in BWD_OUT.items()}

    def args(**over):
        kw = dict(R=R, beta_min=tr.BETA_MIN, feat=keep[0].data_ptr(), t_emb=keep[1].data_ptr(),
                  **{k: fam["Pd"][k].data_ptr() for k in tr.NAMES}, **{k: b.ptr for k, b in fb.items()})
        kw.update(over)
        return L.TransientArgs(**kw)

    def grads(**over):
        kw = dict(d_alpha=up[0].data_ptr(), d_rgb=up[1].data_ptr(), d_beta=up[2].data_ptr(), **{k: b.ptr for k, b in bb.items()})
        kw.update(over)
        return L.TransientGrads(**kw)

    g = grads()
    required = ("feat", "t_emb") + tr.NAMES + tuple(FWD_OUT)
    for bad in [dict(R=0), dict(R=-3)] + [{k: None} for k in required]:
        x = args(**bad)
        assert lib.upnerf_transient_fwd(C.byref(x), None) == EINVAL, bad
        assert lib.upnerf_transient_bwd(C.byref(x), C.byref(g), None) == EINVAL, bad
    assert lib.upnerf_transient_fwd(None, None) == EINVAL and lib.upnerf_transient_bwd(None, C.byref(g), None) == EINVAL
    assert lib.upnerf_transient_bwd(C.byref(a), None, None) == EINVAL
    for k in ("dz_heads", "gz_t", "gz_e", "gz_h"):
        x = grads(**{k: None})
        assert lib.upnerf_transient_bwd(C.byref(a), C.byref(x), None) == EINVAL, k
    torch.cuda.synchronize()
    assert all(b.untouched() for b in fb.values()) and all(b.untouched() for b in bb.values()), "a refused call wrote something"
