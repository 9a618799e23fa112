"""The kernels in front of the first field pass -- stratified coarse depths (upnerf_sample_coarse, upnerf_sample_coarse_keyed),
keyed uniforms (upnerf_uniform_keyed), the colour head's per-ray side input (upnerf_ray_aux) and the train-split ray gather
(upnerf_gather_rays) -- against the CPU references of tests/prologue_ref.py at the shapes and values tests/test_hip_kernels.py
and tests/test_sampler.py never reach: S = 1, 2, 3, R S around the 256-thread block, near == far, a far plane 2^20 above near in
disparity mode, u = 0 and 1 - 2^-24, Philox tails n % 4 != 0 with rows beyond 2^16 and the step 2^24 - 1 from device memory,
axis-aligned / zero / un-normalised directions under four band-weight vectors given by value and through device memory, feature
maps of 1, 2 and 9 pixels a side with C off the 64-lane stride and coordinates on, and one fp32 ulp beside, every pixel centre.

Gate of every floating-point output (test_hip_perray.gate_ratio, unchanged), per element, computed on the CPU:

    |kernel - fp64|  <=  4 * e32 + 2^-22 * |fp64 value|,      e32 = |fp32 restatement - fp64 restatement| on the same inputs;

a limit of 0 (bands weighted 0, the five padding floats, absent appearance rows, features on the last row / column, the sines of
a zero direction) asks for exactly 0.  The coarse depths and the gather claim the reference's operation order and are held to bit
equality with the fp32 restatement as well; the uniforms are integers scaled by 2^-24 and held to bit equality alone.  No element
is left out; tests/test_prologue_ref_cpu.py asserts on the CPU what this relies on (margins, exact planted values, monotone rows).
Every output is followed by a NaN (img_idx: -7) guard band that has to stay intact.

Worst measured ratio kernel error / gate on an MI355X (gate: <= 1):
    coarse depths, u from a buffer          0.19  (R = 6, S = 64 and R = 37, S = 65 in disparity mode; S = 1: 0.00; bit-equal throughout)
    coarse depths, u generated (keyed)      0.19  (R = 6, S = 64 in disparity mode; by value and through step_dev alike)
    direction encoding / aux rows           0.50  (R = 127, wk = (1, 0.75, 0.25, 0); wk = (0, 0, 0, 1): 0.44; wk = 0 and R = 1: 0.00)
    gathered features                       0.25  (h = 2 and h = 9 at every C: the kernel IS the fp32 restatement, so its error is
                                                   e32 and the ratio at most 1/4; h = 1: 0.00, every feature exactly 0)
The whole file runs in 3.5 s there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import prologue_ref as pr
from test_hip_kernels import hip  # noqa: F401  (fixture)
from test_hip_perray import gate_ratio

pytestmark = pytest.mark.gpu

EINVAL = -1  # UPNERF_EINVAL (include/upnerf_hip.h)
NAN = float("nan")


def cpu(t):
    return t.detach().cpu()


def guarded(n, guard, dtype=torch.float32):
    """A flat device buffer of n + guard elements, all NaN (int64: -7)."""
    return torch.full((n + guard,), NAN if dtype.is_floating_point else -7, device="cuda", dtype=dtype)


def intact(buf, n):
    g = cpu(buf)[n:]
    return bool(torch.isnan(g).all()) if g.dtype.is_floating_point else bool((g == -7).all())


# ====================================================================================== 1. coarse depths
def check_depths(got, R, S, disp, perturb, keyed, nf):
    """Gate, bit equality with the fp32 restatement, order and range; returns the gate ratio."""
    z32, z64, lo32 = pr.coarse_refs(R, S, disp, perturb, keyed)
    ratio = gate_ratio(got, z64, z32)
    assert ratio <= 1, (R, S, disp, perturb, ratio)
    assert np.array_equal(got.numpy(), z32.numpy())  # same operation order, no contraction
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    assert bool((got >= nf[:, :1]).all()) and bool((got <= nf[:, 1:]).all())
    assert bool((got[R - len(pr.COARSE_PLANTED)] == 2.0).all())  # near == far
    return ratio


@pytest.mark.parametrize("disp", [0, 1])
@pytest.mark.parametrize("R,S", pr.COARSE_SHAPES)
def test_coarse_depths_from_a_buffer_of_draws(hip, R, S, disp):
    L = hip["lib"]
    nf, steps, u = pr.coarse_case(R, S)
    nfd, sd, ud = nf.cuda(), steps.cuda(), u.cuda()
    worst = 0.0
    for perturb in pr.PERTURBS:
        z = guarded(R * S, S)
        L.check(L.lib.upnerf_sample_coarse(R, S, L.ptr(nfd), L.ptr(sd), L.ptr(ud) if perturb > 0 else None, perturb, disp, L.ptr(z),
                                           L.stream()), "sample_coarse")
        assert intact(z, R * S)
        got = cpu(z)[:R * S].view(R, S)
        worst = max(worst, check_depths(got, R, S, disp, perturb, False, nf))
        if perturb > 0:
            assert torch.equal(got[0], pr.coarse_refs(R, S, disp, perturb)[2][0])  # u = 0: the lower bin edge, exactly
        elif not disp:
            assert torch.equal(got[:, 0], nf[:, 0]) and (S == 1 or torch.equal(got[:, -1], nf[:, 1]))
    print(f"coarse R={R} S={S} disp={disp}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("disp", [0, 1])
@pytest.mark.parametrize("R,S", pr.COARSE_SHAPES)
def test_coarse_depths_with_generated_draws_against_the_cpu_philox(hip, R, S, disp):
    """The keyed entry against coarse_depths(u = philox_uniform(...)) from the CPU, not against its sibling kernel; the step by
    value and through step_dev (2^24 - 1, the largest odd step fp32 holds) give the same bits."""
    L = hip["lib"]
    nf, steps, _ = pr.coarse_case(R, S)
    nfd, sd = nf.cuda(), steps.cuda()
    k = pr.KEYED
    step_dev = torch.tensor([float(k["step"])], device="cuda")
    assert int(step_dev.item()) == k["step"]
    worst = 0.0
    for perturb in (0.5, 1.0):
        outs = []
        for rng in (L.Rng(seed=k["seed"], step=k["step"], row0=k["row0"], row_stride=k["row_stride"], step_dev=None),
                    L.Rng(seed=k["seed"], step=0, row0=k["row0"], row_stride=k["row_stride"], step_dev=step_dev.data_ptr())):
            z = guarded(R * S, S)
            L.check(L.lib.upnerf_sample_coarse_keyed(R, S, L.ptr(nfd), L.ptr(sd), C.byref(rng), perturb, disp, L.ptr(z), L.stream()),
                    "sample_coarse_keyed")
            assert intact(z, R * S)
            outs.append(cpu(z)[:R * S].view(R, S))
        assert np.array_equal(outs[0].numpy(), outs[1].numpy())
        worst = max(worst, check_depths(outs[0], R, S, disp, perturb, True, nf))
    print(f"keyed coarse R={R} S={S} disp={disp}: worst ratio {worst:.3f}")


def test_coarse_entries_refuse_what_they_cannot_run(hip):
    L = hip["lib"]
    R, S = 4, 8
    nf, sd, ud = torch.tensor([[0.5, 2.0]] * R).cuda(), torch.linspace(0, 1, S).cuda(), torch.rand(R, S).cuda()
    z = guarded(R * S, 0)
    p, st = L.ptr, L.stream
    plain = lambda r, s, u, perturb: L.lib.upnerf_sample_coarse(r, s, p(nf), p(sd), u, perturb, 0, p(z), st())
    assert plain(0, S, p(ud), 1.0) == EINVAL and plain(R, 0, p(ud), 1.0) == EINVAL
    assert plain(R, S, None, 0.5) == EINVAL  # perturb > 0 without u
    ok = dict(seed=7, step=3, row0=0, row_stride=1, step_dev=None)

    def keyed(r, s, perturb, **kw):
        rng = L.Rng(**{**ok, **kw})
        return L.lib.upnerf_sample_coarse_keyed(r, s, p(nf), p(sd), C.byref(rng), perturb, 0, p(z), st())

    assert keyed(0, S, 1.0) == EINVAL and keyed(R, 0, 1.0) == EINVAL
    assert keyed(R, S, 0.0) == EINVAL  # the keyed entry is the jittered one
    assert keyed(R, S, 1.0, row_stride=0) == EINVAL and keyed(R, S, 1.0, step=-1) == EINVAL and keyed(R, S, 1.0, row0=-1) == EINVAL
    assert L.lib.upnerf_sample_coarse_keyed(R, S, p(nf), p(sd), None, 1.0, 0, p(z), st()) == EINVAL
    torch.cuda.synchronize()
    assert intact(z, 0)  # nothing was launched
    assert keyed(R, S, 1.0) == 0 and plain(R, S, p(ud), 1.0) == 0  # (the same arguments, made valid, run)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(z).all())


# ====================================================================================== 2. keyed uniforms
@pytest.mark.parametrize("R", pr.UNIFORM_R)
def test_keyed_uniforms_on_tails_high_rows_and_later_draws(hip, R):
    L = hip["lib"]
    k = pr.UNIFORM_KEY
    rows = k["row0"] + k["row_stride"] * np.arange(R)
    step_devs = {s: torch.tensor([float(s)], device="cuda") for s in (k["step"], pr.KEYED["step"])}
    for n in pr.UNIFORM_N:
        for draw in pr.UNIFORM_DRAWS:
            for step, sdev in step_devs.items():
                ref = pr.philox_uniform(k["seed"], step, rows, n, draw)
                outs = []
                for host_step, dev in ((step, None), (0, sdev)):
                    out = guarded(R * n, n)
                    L.check(L.lib.upnerf_uniform_keyed(R, n, k["seed"], host_step, L.ptr(dev), k["row0"], k["row_stride"], draw, L.ptr(out),
                                                       L.stream()), "uniform_keyed")
                    assert intact(out, R * n), (n, draw)
                    outs.append(cpu(out)[:R * n].view(R, n).numpy())
                assert np.array_equal(outs[0], ref), (n, draw, step)
                assert np.array_equal(outs[1], ref), (n, draw, step)
                assert outs[0].min() >= 0.0 and outs[0].max() < 1.0
    out = guarded(8, 0)
    bad = lambda **kw: L.lib.upnerf_uniform_keyed(*[{**dict(R=2, n=4, seed=1, step=0, dev=None, row0=0, stride=1, draw=0), **kw}[a]
                                                    for a in ("R", "n", "seed", "step", "dev", "row0", "stride", "draw")], L.ptr(out), L.stream())
    assert [bad(R=0), bad(n=0), bad(step=-1), bad(row0=-1), bad(stride=0), bad(draw=-1)] == [EINVAL] * 6
    torch.cuda.synchronize()
    assert intact(out, 0)


# ====================================================================================== 3. direction encoding / aux rows
@pytest.mark.parametrize("wk", pr.AUX_WK)
@pytest.mark.parametrize("R", pr.AUX_R)
def test_aux_rows_under_every_band_weight_vector_by_value_and_from_device_memory(hip, R, wk):
    L = hip["lib"]
    d, a = pr.aux_case(R)
    dg = d.cuda()
    store = torch.zeros(R * 48 + 8, device="cuda")
    wk_dev = torch.tensor(wk, device="cuda")
    other = tuple(3.0 - w for w in wk)  # a host array the device values have to win over

    def run(rows, host, dev):
        aux = guarded(R * pr.AUXK, pr.AUXK)
        L.check(L.lib.upnerf_ray_aux(R, L.ptr(dg), L.ptr(rows), (C.c_float * 4)(*host), L.ptr(dev), L.ptr(aux), L.stream()), "upnerf_ray_aux")
        assert intact(aux, R * pr.AUXK)
        return cpu(aux)[:R * pr.AUXK].view(R, pr.AUXK)

    worst = 0.0
    for off in (0, 1, None):  # appearance rows on 16 bytes, off them, absent
        rows = None
        if off is not None:
            rows = store[off:off + R * 48].view(R, 48)
            rows.copy_(a)
            assert (rows.data_ptr() % 16 == 0) == (off == 0)
        a_ref = a if off is not None else None
        r32, r64 = pr.ray_aux(d, a_ref, wk, torch.float32), pr.ray_aux(d, a_ref, wk, torch.float64)
        got = run(rows, wk, None)
        ratio = gate_ratio(got, r64, r32)
        assert ratio <= 1, (R, wk, off, ratio)
        worst = max(worst, ratio)
        assert torch.equal(got[:, :3], d) and torch.equal(got[:, 27:75], a if off is not None else torch.zeros(R, 48))
        assert torch.equal(run(rows, other, wk_dev), got)  # the device values win, and give the same bits
    print(f"ray_aux R={R} wk={wk}: worst ratio {worst:.3f}")


# ====================================================================================== 4. ray gather
def launch_gather(L, dev, idx, h, Cc, feats=True, inv=True):
    """upnerf_gather_rays into outputs with a guard band behind each; returns {key: (buffer, elements)}."""
    R = idx.numel()
    sizes = {"ray_infos": R * 2, "directions": R * 3, "img_idx": R, "c2w": R * 12, "rgbs": R * 3}
    if feats:
        sizes["feats"] = R * Cc
    if inv:
        sizes["inv_depths"] = R
    out = {k: guarded(n, 64, torch.int64 if k == "img_idx" else torch.float32) for k, n in sizes.items()}
    p = lambda k: L.ptr(out[k]) if k in out else None
    idx_d = idx.cuda()
    a = L.GatherRaysArgs(R=R, h=h, C=Cc, idx=L.ptr(idx_d), all_ray_infos=L.ptr(dev["all_ray_infos"]),
                         all_directions=L.ptr(dev["all_directions"]), all_rgbs=L.ptr(dev["all_rgbs"]),
                         all_pxl_coords=L.ptr(dev["all_pxl_coords"]), all_inv_depths=L.ptr(dev["all_inv_depths"]),
                         feat_maps=L.ptr(dev["feat_maps"]), poses=L.ptr(dev["poses"]), ray_infos=p("ray_infos"), directions=p("directions"),
                         img_idx=p("img_idx"), c2w=p("c2w"), rgbs=p("rgbs"), feats=p("feats"), inv_depths=p("inv_depths"))
    L.check(L.lib.upnerf_gather_rays(C.byref(a), L.stream()), "upnerf_gather_rays")
    torch.cuda.synchronize()
    return {k: (out[k], sizes[k]) for k in out}


@pytest.mark.parametrize("h", pr.GATHER_H)
@pytest.mark.parametrize("Cc", pr.GATHER_C)
def test_gather_on_every_pixel_centre_and_channel_tail(hip, Cc, h):
    L = hip["lib"]
    bufs, _ = pr.gather_case(Cc, h)
    dev = {k: v.cuda() for k, v in bufs.items()}
    worst = 0.0
    for R in pr.GATHER_R:
        idx = pr.gather_idx(R)
        ref, f32, f64 = pr.gather_refs(Cc, h, R)
        out = launch_gather(L, dev, idx, h, Cc)
        assert tuple(out) == pr.GATHER_KEYS
        for k, (buf, n) in out.items():
            assert intact(buf, n), k
            assert torch.equal(cpu(buf)[:n].view(ref[k].shape), ref[k]), (k, R)  # the oracle, bit for bit
        ratio = gate_ratio(cpu(out["feats"][0])[:R * Cc].view(R, Cc), f64, f32)  # and the independent fp64 bilinear value
        assert ratio <= 1, (Cc, h, R, ratio)
        worst = max(worst, ratio)
    print(f"gather C={Cc} h={h}: worst ratio {worst:.3f}")


def test_gather_without_feature_maps_or_inverse_depths(hip):
    """Absent feats / inv_depths outputs leave the other outputs as they are, through the entry point (guard bands) and through
    GpuRaySampler, whose batch then lacks the keys."""
    from upnerf_amd.ray_sampler import GpuRaySampler
    L = hip["lib"]
    Cc, h, R = 65, 9, 261
    bufs, _ = pr.gather_case(Cc, h)
    dev = {k: v.cuda() for k, v in bufs.items()}
    idx = pr.gather_idx(R)
    ref = pr.gather_refs(Cc, h, R)[0]
    for feats, inv in ((False, False), (True, False), (False, True)):
        out = launch_gather(L, dev, idx, h if feats else 0, Cc if feats else 0, feats=feats, inv=inv)
        assert set(out) == set(pr.GATHER_KEYS) - ({"feats"} if not feats else set()) - ({"inv_depths"} if not inv else set())
        for k, (buf, n) in out.items():
            assert intact(buf, n) and torch.equal(cpu(buf)[:n].view(ref[k].shape), ref[k]), (k, feats, inv)
    mk = lambda **kw: GpuRaySampler(bufs["all_ray_infos"], bufs["all_directions"], bufs["all_rgbs"], bufs["poses"], **kw)
    for kw, keys in ((dict(), pr.GATHER_KEYS[:5]),
                     (dict(all_pxl_coords=bufs["all_pxl_coords"], feat_maps=bufs["feat_maps"]), pr.GATHER_KEYS[:6]),
                     (dict(all_inv_depths=bufs["all_inv_depths"]), pr.GATHER_KEYS[:5]),  # (the reference reads them beside the features)
                     (dict(all_pxl_coords=bufs["all_pxl_coords"], feat_maps=bufs["feat_maps"], all_inv_depths=bufs["all_inv_depths"]),
                      pr.GATHER_KEYS)):
        got = mk(**kw).sample(idx.cuda())
        assert tuple(got) == tuple(keys)
        for k in keys:
            assert torch.equal(cpu(got[k]), ref[k]), (k, sorted(kw))


def test_sampler_refuses_an_index_outside_the_split_before_any_launch(hip):
    from upnerf_amd.ray_sampler import GpuRaySampler
    L = hip["lib"]
    bufs, _ = pr.gather_case(1, 2)
    smp = GpuRaySampler(bufs["all_ray_infos"], bufs["all_directions"], bufs["all_rgbs"], bufs["poses"],
                        all_pxl_coords=bufs["all_pxl_coords"], feat_maps=bufs["feat_maps"], all_inv_depths=bufs["all_inv_depths"])
    N = len(smp)
    calls = L.CALLS[0]
    for bad in ([N], [-1], [0, 5, N, 3], [2 ** 31], [0, -2 ** 40]):
        with pytest.raises(IndexError):
            smp.sample(torch.tensor(bad, dtype=torch.int64, device="cuda"))
    assert L.CALLS[0] == calls  # no C-ABI call was made
    got = smp.sample(torch.tensor([0, N - 1], dtype=torch.int64))  # the ends of the split are inside
    assert L.CALLS[0] == calls + 1 and torch.equal(cpu(got["rgbs"]), bufs["all_rgbs"][[0, N - 1]])
    # the entry point's own refusals leave the outputs untouched
    dev = {k: v.cuda() for k, v in bufs.items()}
    z = guarded(64, 0)
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    base = dict(R=2, h=2, C=1, idx=L.ptr(idx), all_ray_infos=L.ptr(dev["all_ray_infos"]), all_directions=L.ptr(dev["all_directions"]),
                all_rgbs=L.ptr(dev["all_rgbs"]), all_pxl_coords=L.ptr(dev["all_pxl_coords"]), all_inv_depths=L.ptr(dev["all_inv_depths"]),
                feat_maps=L.ptr(dev["feat_maps"]), poses=L.ptr(dev["poses"]), ray_infos=L.ptr(z), directions=L.ptr(z),
                img_idx=L.ptr(z), c2w=L.ptr(z), rgbs=L.ptr(z), feats=L.ptr(z), inv_depths=L.ptr(z))
    for kw in (dict(R=0), dict(h=0), dict(C=0), dict(feat_maps=None), dict(all_pxl_coords=None), dict(all_inv_depths=None), dict(idx=None)):
        a = L.GatherRaysArgs(**{**base, **kw})
        assert L.lib.upnerf_gather_rays(C.byref(a), L.stream()) == EINVAL, kw
    torch.cuda.synchronize()
    assert intact(z, 0)
