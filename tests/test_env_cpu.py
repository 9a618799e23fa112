"""The environment map without a GPU (csrc/env.hip; upnerf_amd/baked_env.py).

The restatement tests/env_ref.py is held to its own claims -- continuity across the 12 edges and 8 corners of the cube, a constant
map returned exactly, its d-gradient equal to central differences of itself, seam ownership by the lowest face, the share of
directions it leaves out of a slope comparison -- and the kernels' own __host__ __device__ bodies, run by the stand-alone program
tests/host/env_host.hip (plain, and with AddressSanitizer and UBSan on the host side where there is no GPU), are held to its gates
on every direction family at E = 1, 2 and 5."""
import ctypes
import os

import numpy as np
import pytest
import torch

import env_ref as er
from walk_checks import host_build, run_clean

SANITIZE = not torch.cuda.is_available()  # sanitizer runs belong on a machine without a GPU
SIZES = (1, 2, 5)
BOXES = {"cube": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "1:3:7": ((-0.5, -1.0, 0.25), (0.5, 2.0, 7.25))}


# ---- 1: the restatement's own claims --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", SIZES)
def test_the_lookup_is_continuous_across_every_edge_and_corner(E):
    """A direction on a face edge or a cube corner, pushed a hair into each of the faces that meet there, gives colours that
    differ by no more than the map's largest slope times the push; and ON the edge, whichever face the tie rule picks, the value is
    the shared node line's (the copies are equal)."""
    env = er.random_map(E, seed=E)
    s = [1.0, -1.0]
    pts = [np.array([sx, sy, t]) for sx in s for sy in s for t in (-0.83, 0.0, 0.41)]  # the 4 edges along z, then x and y by rolling
    edges = [np.roll(p, k) for p in pts for k in range(3)]
    corners = [np.array([sx, sy, sz]) for sx in s for sy in s for sz in s]
    assert len(edges) == 12 * 3 and len(corners) == 8
    h = 1e-9
    slope = 4.0 * E * np.abs(np.diff(env[..., :3].astype(np.float64), axis=1)).max(initial=0) + 4.0 * E * np.abs(np.diff(env[..., :3].astype(np.float64), axis=2)).max(initial=0)
    for p in edges + corners:
        big = np.abs(p) == 1.0
        base = er.lookup(env, p[None])["rgb"][0]
        faces = set()
        for k in np.nonzero(big)[0]:  # shrink every tied axis but k: face k wins
            q = p.copy()
            q[big] *= 1 - h
            q[k] = p[k]
            L = er.lookup(env, q[None])
            faces.add(int(L["face"][0]))
            assert np.abs(L["rgb"][0] - base).max() <= slope * h * 4 + 1e-15, (p, k)
        assert len(faces) == big.sum()


@pytest.mark.parametrize("E", SIZES)
def test_a_constant_map_returns_the_constant_exactly(E):
    fam = er.families(E)
    for c in (0.0, 1.0, 0.3):
        env = np.zeros((6, E + 1, E + 1, 4), np.float32)
        env[..., :3] = np.float32(c)
        for name, dirs in fam.items():
            L = er.lookup(env, er.scaled(dirs))
            want = np.broadcast_to(np.where(L["dead"][:, None], 0.0, float(np.float32(c))), L["rgb"].shape)
            assert np.array_equal(L["rgb"], want), (c, name)
            assert not L["su"].any() and not L["sv"].any()


@pytest.mark.parametrize("E", SIZES)
def test_the_gradient_is_the_central_difference_of_the_value(E):
    """Away from node lines and ties the composite is a smooth function of d; D(h) at h and h / 2, the closed form within
    |D(h) - D(h / 2)| + 1e-12 / h of D(h / 2) (the truncation error and fp64's rounding of the value)."""
    env = er.smooth_map(E, seed=E + 1)
    rng = np.random.default_rng(5)
    d = rng.normal(size=(400, 3))
    L = er.lookup(env, d)
    h = 2.0 ** -16
    room = 4 * h * E * (1 + np.abs(d).max(1) / L["am"])  # how far g moves under d +- h e, generously
    frac = lambda g: np.abs(g - np.round(g))
    srt = np.sort(np.abs(d), 1)
    keep = (frac(L["gu"]) > room) & (frac(L["gv"]) > room) & (srt[:, 2] - srt[:, 1] > 2 * h)
    d = d[keep][:40]
    assert len(d) == 40
    n = len(d)
    rays = np.concatenate([np.zeros((n, 3)), d, np.zeros((n, 2))], 1)
    opacity, g = rng.uniform(0, 0.9, n), rng.normal(size=(n, 3))
    f = lambda r: (er.composite(env, r, opacity, np.zeros((n, 3)))["rgb"] * g).sum(1)
    ref = er.composite_bwd(env, rays, opacity, g)
    worst = 0.0
    for i in range(8):
        e = np.zeros(8)
        e[i] = 1.0
        D1, D2 = (f(rays + h * e) - f(rays - h * e)) / (2 * h), (f(rays + h / 2 * e) - f(rays - h / 2 * e)) / h
        bound = np.abs(D1 - D2) + 1e-12 / h
        err = np.abs(ref["g_rays"][:, i] - D2)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (i, np.argmax(err / bound))
    assert np.abs(ref["g_rays"][:, 3:6]).max() > 1e-2 and not ref["g_rays"][:, [0, 1, 2, 6, 7]].any()
    # the opacity's gradient: the composite is linear in it
    assert np.allclose(ref["g_opacity"], -(er.lookup(env, d)["rgb"] * g).sum(1), rtol=0, atol=1e-15)
    print(f"E {E}: worst |closed form - D(h / 2)| / bound {worst:.3f}")


@pytest.mark.parametrize("E", SIZES)
def test_seam_ownership_is_the_lowest_face(E):
    own = er.owners(E)
    N = E + 1
    face = np.arange(6 * N * N) // (N * N)
    d = er.node_dirs(E).reshape(-1, 3)
    assert (own <= np.arange(len(own))).all() and (face[own] <= face).all()
    assert np.array_equal(own[own], own)  # an owner owns itself
    assert np.array_equal(d[own], d)  # the same direction, bit for bit
    edge = er.edge_mask(E).reshape(-1)
    assert (own[~edge] == np.arange(len(own))[~edge]).all()  # interior nodes are their own
    # every direction occurs on one owner only, and the copies per direction are 1 (interior), 2 (edge) or 3 (corner)
    copies = np.bincount(own, minlength=len(own))
    assert set(copies[copies > 0]) <= {1, 2, 3} and (copies == 3).sum() == 8
    assert len(np.unique(d, axis=0)) == (copies > 0).sum() == 6 * E * E + 2


@pytest.mark.parametrize("E", SIZES)
def test_the_restatement_leaves_out_few_directions_of_the_generic_families(E):
    """For g_rays a test may leave out the directions within their own dg of a node line or a tie: at most 2 % of a family."""
    env = er.random_map(E, seed=E)
    for name, dirs in er.families(E).items():
        if er.value_only(name, E):
            continue
        rays, opacity, _, g = er.problem(E, name, dirs)
        ref = er.composite_bwd(env, rays, opacity, g)
        left = ref["near_line"] & ~ref["dead"]
        print(f"E {E} {name}: {int(left.sum())} of {len(rays)} left out")
        assert left.mean() <= er.LEFT_OUT_CAP, (name, left.mean())


# ---- 2: the kernels' bodies on the host ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if host_build.hipcc() is None:
        pytest.skip("hipcc is not installed")
    out = str(tmp_path_factory.mktemp("env_host"))
    return {san: host_build.build(out, sanitize=san, names=("env_host",))["env_host"] for san in ((False, True) if SANITIZE else (False,))}


def run_host(exe, directory, env, box, far, rays, opacity, rgb_in, g_out):
    d = str(directory)
    E, R = env.shape[1] - 1, len(rays)
    np.asarray([E, R], np.int32).tofile(os.path.join(d, "dims.bin"))
    np.concatenate([box[0], box[1], [far]]).astype(np.float32).tofile(os.path.join(d, "box.bin"))
    np.ascontiguousarray(env, np.float32).tofile(os.path.join(d, "env.bin"))
    np.ascontiguousarray(rays, np.float32).tofile(os.path.join(d, "rays.bin"))
    np.concatenate([opacity[:, None], rgb_in, g_out], 1).astype(np.float32).tofile(os.path.join(d, "rest.bin"))
    run_clean(exe, d)
    load = lambda f, t: np.fromfile(os.path.join(d, f), t)
    return dict(rgb=load("rgb.bin", np.float32).reshape(R, 3), grad=load("grad.bin", np.float32).reshape(R, 9),
                nodes=load("nodes.bin", np.float32).reshape(-1, 8), owner=load("owner.bin", np.int64))


def check_against_gates(E, name, rays, opacity, rgb_in, g_out, rgb, g_opacity, g_rays, env, what):
    """The comparisons every implementation (host body, kernel) is held to on one family; returns the worst err / gate ratios."""
    ref = er.composite(env, rays, opacity, rgb_in)
    err = np.abs(rgb.astype(np.float64) - ref["rgb"])
    assert np.isfinite(rgb).all() and (err <= ref["gate"]).all(), (what, E, name, "rgb", np.argwhere(err > ref["gate"])[:4].tolist())
    worst = {"rgb": float((err / np.maximum(ref["gate"], 1e-300)).max())}
    dead = ref["look"]["dead"]
    assert np.array_equal(rgb[dead], rgb_in[dead])  # a dead direction adds exactly nothing
    if g_opacity is None:
        return worst
    b = er.composite_bwd(env, rays, opacity, g_out)
    err = np.abs(g_opacity.astype(np.float64) - b["g_opacity"])
    assert (err <= b["gate_opacity"]).all(), (what, E, name, "g_opacity", np.argwhere(err > b["gate_opacity"])[:4].tolist())
    worst["g_opacity"] = float((err / np.maximum(b["gate_opacity"], 1e-300)).max())
    assert not g_rays[dead].any() and not g_opacity[dead].any()
    assert not g_rays[:, [0, 1, 2, 6, 7]].any()
    if not er.value_only(name, E):
        keep = ~b["near_line"]
        assert (~keep & ~dead).mean() <= er.LEFT_OUT_CAP
        with np.errstate(invalid="ignore"):
            err = np.abs(g_rays.astype(np.float64) - b["g_rays"])[keep]
        gate = b["gate_rays"][keep]
        assert np.isfinite(g_rays[keep]).all() and (err <= gate).all(), (what, E, name, "g_rays", np.argwhere(err > gate)[:4].tolist())
        worst["g_rays"] = float((err / np.maximum(gate, 1e-300)).max())
    return worst


@pytest.mark.parametrize("E", SIZES)
def test_the_host_bodies_are_within_the_gates_on_every_family(programs, tmp_path, E):
    env = er.random_map(E, seed=E)
    box = BOXES["1:3:7"]
    nodes, owner = None, None
    for name, dirs in er.families(E).items():
        rays, opacity, rgb_in, g_out = er.problem(E, name, dirs)
        got = run_host(programs[False], tmp_path, env, box, 9.0, rays, opacity, rgb_in, g_out)
        worst = check_against_gates(E, name, rays, opacity, rgb_in, g_out, got["rgb"], got["grad"][:, 0], got["grad"][:, 1:], env, "host")
        print(f"E {E} {name}: {len(rays)} directions, worst err / gate " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        nodes, owner = got["nodes"], got["owner"]
    assert np.array_equal(owner, er.owners(E))
    for bname, b in BOXES.items():
        nodes = run_host(programs[False], tmp_path, env, b, 9.0, rays, opacity, rgb_in, g_out)["nodes"]
        ref = er.node_rays(E, b, 9.0)
        assert np.array_equal(nodes[:, :6].astype(np.float64), ref["rays"][:, :6]) and (nodes[:, 7] == 9.0).all()
        err = np.abs(nodes[:, 6].astype(np.float64) - ref["rays"][:, 6])
        assert (err <= ref["gate_near"]).all() and (nodes[:, 6] > 0).all()
        assert np.array_equal(nodes[er.owners(E)], nodes)  # copies of a shared node carry identical rows
        print(f"E {E} box {bname}: near worst err / gate {float((err / ref['gate_near']).max()):.3f}")


@pytest.mark.skipif(not SANITIZE, reason="sanitizer runs belong on a machine without a GPU")
def test_the_host_bodies_are_clean_under_the_sanitizers(programs, tmp_path):
    for E in SIZES:
        env = er.random_map(E, seed=E)
        rays, opacity, rgb_in, g_out = (np.concatenate(x) for x in zip(*(er.problem(E, n, d) for n, d in er.families(E).items())))
        plain = run_host(programs[False], tmp_path, env, BOXES["1:3:7"], 9.0, rays, opacity, rgb_in, g_out)
        san = run_host(programs[True], tmp_path, env, BOXES["1:3:7"], 9.0, rays, opacity, rgb_in, g_out)
        for k in plain:
            assert np.array_equal(plain[k].view(np.uint8), san[k].view(np.uint8)), (E, k)


# ---- the entry points' refusals (on the host, before any launch) -----------------------------------------------------------------------

def test_the_entry_points_refuse_before_launch():
    from upnerf_amd import _lib
    one, odd, off4 = ctypes.c_void_p(64), ctypes.c_void_p(66), ctypes.c_void_p(68)
    f3 = lambda v: (ctypes.c_float * 3)(*v)

    def cases(make, fn, bad):
        for case in bad:
            a = make()
            for k, v in case.items():
                setattr(a, k, v)
            assert fn(ctypes.byref(a), None) == -1, case
        assert fn(None, None) == -1

    lib = _lib.lib
    cases(lambda: _lib.EnvRaysArgs(E=2, count=4, n0=0, lo=f3((0, 0, 0)), hi=f3((1, 1, 1)), far=2.0, rays=one), lib.upnerf_env_rays,
          [dict(E=0), dict(E=_lib.ENV_MAX_E + 1), dict(rays=None), dict(rays=off4), dict(count=0), dict(n0=-1), dict(n0=51), dict(count=55),
           dict(hi=f3((0, 1, 1))), dict(lo=f3((float("nan"), 0, 0))), dict(hi=f3((float("inf"), 1, 1))), dict(far=0.0), dict(far=-1.0),
           dict(far=float("inf")), dict(far=float("nan"))])
    cases(lambda: _lib.EnvSeamArgs(E=2, env=one), lib.upnerf_env_seam, [dict(E=0), dict(env=None), dict(env=off4)])
    cases(lambda: _lib.EnvCompositeArgs(E=2, R=4, env=one, rays=one, opacity=one, rgb_in=one, rgb_out=one), lib.upnerf_env_composite,
          [dict(E=0), dict(R=-1), dict(env=None), dict(env=off4), dict(rays=None), dict(rays=off4), dict(opacity=None), dict(opacity=odd),
           dict(rgb_in=None), dict(rgb_out=None), dict(rgb_out=odd)])
    cases(lambda: _lib.EnvCompositeBwdArgs(E=2, R=4, env=one, rays=one, opacity=one, g_out=one, g_opacity=one, g_rays=one),
          lib.upnerf_env_composite_bwd,
          [dict(E=0), dict(R=-1), dict(env=None), dict(rays=off4), dict(opacity=None), dict(g_out=None), dict(g_out=odd), dict(g_opacity=None),
           dict(g_rays=None), dict(g_rays=off4)])
