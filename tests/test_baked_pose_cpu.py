"""The baked marcher's ray gradient without a GPU (csrc/baked.hip: upnerf_baked_ray_bwd; upnerf_amd/baked_pose.py).

The closed form of tests/baked_pose_ref.py is held to torch.autograd (fp64, on a forward restated here in torch with the visited
samples and their cells frozen) and to central differences of baked_tune_ref.render64; each planted omission must break its gate;
and the kernel's own __host__ __device__ body, run by the stand-alone program tests/host/baked_ray_host.hip (plain, and with
AddressSanitizer and UBSan on the host side where there is no GPU), is held to the gates element by element -- sparse equal to
dense and the march with the bits equal to the march without them, bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import baked_pose_ref as pr
import baked_ref as br
import baked_sh_ref as sh
import baked_tune_ref as tr
import walk_cases as wc
from walk_checks import BACKGROUND, host_build, run_clean

SANITIZE = not torch.cuda.is_available()  # sanitizer runs belong on a machine without a GPU
SETTINGS = {"bg0-all": (0.0, 0.0, True), "bg1-stop-rgb": (1.0, 1e-3, False)}  # (those of tests/test_hip_baked_tune.py)


def numbers(name, degree):
    """The numbers the reference differentiates: rgbs, or (k, sigma) of the stored records."""
    if degree == 0:
        return sh.GRIDS[name]()[0]
    return sh.unpack(sh.sh_grid(name, degree)[0], degree)


def rays_all(name):
    return np.concatenate([br.make_rays(), tr.extra_rays(sh.GRIDS[name]()[0])])


# ---- 1: the closed form against autograd ------------------------------------------------------------------------------------------

def torch_basis(u, degree):
    x, y, z = u
    B = [torch.full_like(x, sh.Y0), -sh.Y1 * y, sh.Y1 * z, -sh.Y1 * x, sh.Y2 * x * y, -sh.Y2 * y * z, sh.Y3 * (2 * z * z - x * x - y * y),
         -sh.Y2 * x * z, sh.Y4 * (x * x - y * y)]
    return torch.stack(B[:sh.NB[degree]])


def frozen_functional(points, degree, row, step, background, stop, gr, gd, go):
    """sum g . outputs of one ray as a torch fp64 function of its row [8]: the forward of baked_ref / baked_sh_ref with every
    sample's cell taken from the numbers (not differentiated) and the loop over the samples inside the box ended by `stop`."""
    lo, hi = (torch.tensor(b) for b in br.bounds64(br.BOUNDS))
    o, d, near, far = row[:3], row[3:6], row[6], row[7]
    length = torch.sqrt((d * d).sum())
    if degree == 0:
        grid = torch.tensor(np.asarray(points, np.float64))
    else:
        k, sigma = (torch.tensor(np.asarray(z, np.float64)) for z in points)
        grid = torch.cat([k @ torch_basis(d / length, degree), sigma[..., None]], -1)
    C = torch.tensor(grid.shape[2::-1], dtype=torch.float64) - 1
    K = br.n_samples(float(near.detach()), float(far.detach()), step)
    rgb, depth, op, T = torch.zeros(3, dtype=torch.float64), 0.0, 0.0, 1.0
    for kk in range(K):
        t = near + (kk + 0.5) * step
        g = (o + t * d - lo) * C / (hi - lo)
        if bool(((g < 0) | (g > C)).any()):
            continue
        i = torch.minimum(torch.floor(g.detach()), C - 1).long()
        f = g - i
        c = lambda dz, dy, dx: grid[i[2] + dz, i[1] + dy, i[0] + dx]
        x00, x10 = c(0, 0, 0) + f[0] * (c(0, 0, 1) - c(0, 0, 0)), c(0, 1, 0) + f[0] * (c(0, 1, 1) - c(0, 1, 0))
        x01, x11 = c(1, 0, 0) + f[0] * (c(1, 0, 1) - c(1, 0, 0)), c(1, 1, 0) + f[0] * (c(1, 1, 1) - c(1, 1, 0))
        y0, y1 = x00 + f[1] * (x10 - x00), x01 + f[1] * (x11 - x01)
        v = y0 + f[2] * (y1 - y0)
        col = torch.clamp(v[:3], 0.0, 1.0) if degree else v[:3]
        alpha = -torch.expm1(-step * length * v[3])
        w = T * alpha
        rgb, depth, op, T = rgb + w * col, depth + w * t, op + w, T * (1 - alpha)
        if stop > 0 and float(T.detach()) < stop:
            break
    rgb, depth = rgb + (1 - op) * background, depth + (1 - op) * far
    return (torch.tensor(gr) * rgb).sum() + gd * depth + go * op


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("degree", [0, 2])
def test_the_closed_form_is_autograds_gradient_of_the_frozen_forward(degree, setting):
    bg, stop, rest = SETTINGS[setting]
    name = "blob"
    P = numbers(name, degree)
    rays = rays_all(name)
    rays = rays[[0, 1, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14, 64 + 67]]  # the named hits, seven random rays, the ray inside a cell face
    step = sh.steps(sh.GRIDS[name]()[0])["cell"]
    g_rgb, g_depth, g_op = (g.astype(np.float64) for g in tr.upstream(len(rays), zero_rows=()))
    if not rest:
        g_depth, g_op = np.zeros_like(g_depth), np.zeros_like(g_op)
    ref = pr.ray_grad(P, degree, br.BOUNDS, rays, step, bg, stop, g_rgb, g_depth, g_op, gates=False)["grad"]
    worst, clamped = 0.0, 0
    for r, row in enumerate(rays.astype(np.float64)):
        x = torch.tensor(row, requires_grad=True)
        frozen_functional(P, degree, x, float(np.float32(step)), bg, float(np.float32(stop)), g_rgb[r], g_depth[r], g_op[r]).backward()
        got = x.grad.numpy()
        scale = np.abs(ref[r]).max()
        assert scale > 0
        worst = max(worst, float(np.abs(got - ref[r]).max() / scale))
    print(f"degree {degree} {setting}: worst |closed form - autograd| / largest entry {worst:.2e}")
    assert worst <= 1e-9


# ---- 2: central differences -------------------------------------------------------------------------------------------------------

H = 2.0 ** -12  # the difference step: the rays are multiples of H / 2, so ray +- H and ray +- H / 2 are fp32 numbers


def smooth_rays(rgbs, step, want=6):
    """Rays on the lattice of H / 2 whose samples in or next to the box stay more than the step's reach away from every grid plane
    (the box's faces among them), and whose K does not change with near or far +- H."""
    lo, hi = br.bounds64(br.BOUNDS)
    C = np.array(rgbs.shape[2::-1], np.float64) - 1
    inv = C / (hi - lo)
    out = []
    for row in br.make_rays(seed=17, R=200)[8:].astype(np.float64):
        row = np.round(row / (H / 2)) * (H / 2)
        near, far = row[6], row[7]
        if len({br.n_samples(near + a, far + b, step) for a in (-H, 0, H) for b in (-H, 0, H)}) != 1:
            continue
        t = near + (np.arange(br.n_samples(near, far, step)) + 0.5) * step
        g = (row[:3] + t[:, None] * row[3:6] - lo) * inv
        close = ((g > -1) & (g < C + 1)).all(1)
        reach = 1.01 * H * inv * max(1.0, np.abs(t).max(), np.abs(row[3:6]).max())
        if close.any() and (np.abs(g[close] - np.round(g[close])) > reach).all():
            out.append(row)
        if len(out) == want:
            break
    assert len(out) == want
    return np.asarray(out)


@pytest.mark.parametrize("degree", [0, 2])
def test_the_closed_form_is_the_central_difference_of_the_fp64_render(degree):
    """D(h) = (L(x + h) - L(x - h)) / 2h of L = sum g . render64 at h = H and H / 2: the truncation error of D(H / 2) is a third of
    |D(H) - D(H / 2)| to leading order, and fp64 rounds L to a few 1e-16 of its terms: the closed form must be within
    |D(H) - D(H / 2)| + 1e-12 / H of D(H / 2)."""
    A = tr.tuning_problem(degree)[0]  # (degree 2: gentle coefficients, few clamped blends -- a clamp is a kink a difference cannot see)
    rgbs = br.blob_grid()[0]
    step = float(np.float32(br.cell_size(rgbs)))
    rays = smooth_rays(rgbs, step)
    g_rgb, g_depth, g_op = (g.astype(np.float64) for g in tr.upstream(len(rays), zero_rows=()))
    ref = pr.ray_grad(A, degree, br.BOUNDS, rays, step, 0.25, 0.0, g_rgb, g_depth, g_op, gates=False)["grad"]
    L = lambda x: tr.functional(A, degree, br.BOUNDS, x, step, 0.25, 0.0, g_rgb, g_depth, g_op)
    worst = 0.0
    for r in range(len(rays)):
        one = lambda x: tr.functional(A, degree, br.BOUNDS, x[None], step, 0.25, 0.0, g_rgb[r:r + 1], g_depth[r:r + 1], g_op[r:r + 1])
        for i in range(8):
            e = np.zeros(8)
            e[i] = 1.0
            D1 = (one(rays[r] + H * e) - one(rays[r] - H * e)) / (2 * H)
            D2 = (one(rays[r] + H / 2 * e) - one(rays[r] - H / 2 * e)) / H
            bound = abs(D1 - D2) + 1e-12 / H
            worst = max(worst, abs(ref[r, i] - D2) / bound)
            assert abs(ref[r, i] - D2) <= bound, (r, i, ref[r, i], D1, D2)
    assert np.abs(ref).max() > 1e-2 and L(rays) != 0
    print(f"degree {degree}: worst |closed form - D(H / 2)| / bound {worst:.3f}")


# ---- 3: the gate sees each planted omission ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("omit", pr.OMISSIONS)
def test_each_planted_omission_exceeds_the_gate_on_some_ray(omit):
    name, degree = "blob", 2
    P = numbers(name, degree)
    rays = rays_all(name)
    step = sh.steps(sh.GRIDS[name]()[0])["cell"]
    g_rgb, g_depth, g_op = tr.upstream(len(rays))
    ref = pr.ray_grad(P, degree, br.BOUNDS, rays, step, 0.0, 0.0, g_rgb, g_depth, g_op)
    bad = pr.ray_grad(P, degree, br.BOUNDS, rays, step, 0.0, 0.0, g_rgb, g_depth, g_op, gates=False, omit=(omit,))["grad"]
    over = np.abs(bad - ref["grad"]) > ref["gate"]
    print(f"without the {omit} term: {int(over.any(1).sum())} of {len(rays)} rays leave their gate")
    assert over.any(1).sum() >= 5


# ---- 4: the kernel's body on the host -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if host_build.hipcc() is None:
        pytest.skip("hipcc is not installed")
    out = str(tmp_path_factory.mktemp("ray_host"))
    return {san: host_build.build(out, sanitize=san, names=("baked_ray_host",))["baked_ray_host"] for san in ((False, True) if SANITIZE else (False,))}


def run_host(exe, directory, name, rays, up, step, stop):
    """baked_ray_host on a scene of walk_cases: grad [12, R, 8] as uint32 (c = (degree * 2 + layout) * 2 + use_bits)."""
    S = wc.scene(name)
    d = str(directory)
    lo, hi = (np.asarray(b, np.float32) for b in wc.BOUNDS)
    R = len(rays)
    np.asarray(list(S["cells"]) + [R, len(S["bricks"])], np.int32).tofile(os.path.join(d, "dims.bin"))
    np.concatenate([lo, hi, [step, BACKGROUND, stop]]).astype(np.float32).tofile(os.path.join(d, "params.bin"))
    for degree in (0, 1, 2):
        np.ascontiguousarray(S["points"][degree]).tofile(os.path.join(d, f"points{degree}.bin"))
        np.ascontiguousarray(S["pool"][degree]).tofile(os.path.join(d, f"pool{degree}.bin"))
    S["slots"].astype(np.int32).tofile(os.path.join(d, "slots.bin"))
    S["words"].astype(np.uint32).tofile(os.path.join(d, "words.bin"))
    np.ascontiguousarray(rays, np.float32).tofile(os.path.join(d, "rays.bin"))
    np.ascontiguousarray(up, np.float32).tofile(os.path.join(d, "up.bin"))
    run_clean(exe, d)
    return np.fromfile(os.path.join(d, "grad.bin"), np.uint32).reshape(12, R, 8)


def host_case(name, step_name, setting):
    """(rays, upstream [R, 5], step, stop, the rays the gate is asked of): the rays of the kernel tests and the families of
    walk_cases (drawn away from the box's faces; a ray with a sample within its dg of one is left out of the comparison with
    fp64, as tests/test_walks_host_cpu.py leaves it out: the slopes do not vanish there as the blend does)."""
    S = wc.scene(name)
    step = wc.steps(name)[step_name]
    stop, rest = SETTINGS[setting][1:]
    fam = wc.rays_of(4, 5, S["cells"], step, ref=True, big=False)[0]
    rays = np.concatenate([rays_all(name), fam])
    g = tr.upstream(len(rays))
    up = np.concatenate([g[0], (g[1] if rest else 0 * g[1])[:, None], (g[2] if rest else 0 * g[2])[:, None]], 1).astype(np.float32)
    return rays, up, step, stop, ~wc.borderline(S["cells"], rays, step)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("step_name", ["cell", "tenth"])
@pytest.mark.parametrize("name", list(sh.GRIDS))
def test_the_host_body_is_within_the_gates_and_layouts_and_bits_agree_bit_for_bit(programs, tmp_path, name, step_name, setting):
    rays, up, step, stop, asked = host_case(name, step_name, setting)
    got = run_host(programs[False], tmp_path, name, rays, up, step, stop)
    assert asked.mean() >= 0.95
    for degree in (0, 1, 2):
        c = degree * 4
        assert np.array_equal(got[c], got[c + 1]) and np.array_equal(got[c + 2], got[c + 3])  # with the bits = without them
        assert np.array_equal(got[c], got[c + 2])  # sparse = dense
        P = wc.scene(name)["rgbs"] if degree == 0 else sh.unpack(wc.scene(name)["points"][degree], degree)
        ref = pr.ray_grad(P, degree, wc.BOUNDS, rays, step, BACKGROUND, stop, up[:, :3], up[:, 3], up[:, 4])
        if stop > 0:
            assert ref["stop_margin"] > 0
        val = got[c].view(np.float32).astype(np.float64)
        assert np.isfinite(val).all()
        err, gate = np.abs(val - ref["grad"])[asked], ref["gate"][asked]
        worst = float((err / np.maximum(gate, 1e-300))[gate > 0].max(initial=0.0))
        print(f"{name} {step_name} {setting} degree {degree}: {int((ref['gate'][asked] > 0).any(1).sum())} rays with a gradient, worst err / gate {worst:.3f}")
        assert (val[asked][gate == 0] == 0).all()
        assert (err <= gate).all(), (degree, np.argwhere(err > gate)[:5], worst)
        zero = ~np.isfinite(rays).all(1) | ~(rays[:, 7] > rays[:, 6]) | ~up.any(1)
        assert zero.sum() >= 5 and not got[c][zero].any()  # misses and rows without an upstream gradient: eight zeros (+0)


@pytest.mark.skipif(not SANITIZE, reason="sanitizer runs belong on a machine without a GPU")
def test_the_host_body_is_clean_under_the_sanitizers(programs, tmp_path):
    for name in sh.GRIDS:
        rays, up, step, stop, _ = host_case(name, "tenth", "bg1-stop-rgb")
        plain = run_host(programs[False], tmp_path, name, rays, up, step, stop)
        assert np.array_equal(run_host(programs[True], tmp_path, name, rays, up, step, stop), plain)


# ---- the entry point's refusals (on the host, before any launch) --------------------------------------------------------------------

def test_the_entry_point_refuses_before_launch():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(64)  # (non-null, aligned, never dereferenced: each case is refused on the host)
    f3 = lambda v: (ctypes.c_float * 3)(*v)

    def args(**kw):
        a = _lib.BakedRayBwdArgs(Cx=8, Cy=8, Cz=8, R=4, lo=f3((0, 0, 0)), hi=f3((1, 1, 1)), step=0.1, background=0.0, stop=0.0, degree=0,
                                 points=one, slots=None, words=one, rays=one, g_rgb=one, g_depth=None, g_opacity=None, g_rays=one)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cases = [dict(g_rgb=None), dict(g_rays=None), dict(g_rays=ctypes.c_void_p(68)), dict(degree=3), dict(degree=-1), dict(R=0), dict(step=0.0),
             dict(stop=1.0), dict(points=None), dict(words=None), dict(rays=None), dict(rays=ctypes.c_void_p(72)), dict(Cx=0),
             dict(hi=f3((0, 1, 1))), dict(background=float("nan")), dict(degree=2, points=ctypes.c_void_p(96))]
    for case in cases:
        assert _lib.lib.upnerf_baked_ray_bwd(ctypes.byref(args(**case)), None) == -1, case
    assert _lib.lib.upnerf_baked_ray_bwd(None, None) == -1
