"""The baked scene with spherical-harmonic colour without a GPU: the basis and the projection of the fp64 restatement
(tests/baked_sh_ref.py) and of upnerf_amd.baked against closed forms, the host-side refusals of the three new entry points and
of the Python surface, the arrays of a saved scene, and the conditions on the fixtures that tests/test_hip_baked_sh.py
renders (that they clamp on both sides, and that the direction matters far beyond the gates)."""
import ctypes

import numpy as np
import pytest

import baked_ref as br
import baked_sh_ref as sh


@pytest.mark.parametrize("degree", [1, 2])
def test_the_basis_is_orthonormal_on_the_sphere(degree):
    # Gauss-Legendre in z times the rectangle rule in the longitude: exact for the products of two degree-2 harmonics
    z, wz = np.polynomial.legendre.leggauss(16)
    phi = (np.arange(32) + 0.5) * (2 * np.pi / 32)
    Z, P = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1 - Z * Z)
    dirs = np.stack([r * np.cos(P), r * np.sin(P), Z], -1).reshape(-1, 3)
    w = (wz[:, None] * np.full(32, 2 * np.pi / 32)).reshape(-1)
    from upnerf_amd import baked
    for B in (sh.basis(dirs, degree), baked.sh_basis(dirs, degree)):
        gram = (B * w[:, None]).T @ B
        assert np.abs(gram - np.eye(sh.NB[degree])).max() < 1e-13
    assert np.abs(sh.basis(dirs * 3.0, degree) - sh.basis(dirs, degree)).max() < 1e-15  # (a direction, not a vector)
    assert np.abs(baked.sphere_directions(48) - sh.sphere_directions(48)).max() == 0
    assert np.abs(np.linalg.norm(baked.sphere_directions(48), axis=1) - 1).max() < 1e-15


@pytest.mark.parametrize("degree", [1, 2])
def test_project_recovers_known_coefficients_at_the_default_directions(degree):
    from upnerf_amd import baked
    nb = sh.NB[degree]
    dirs = sh.sphere_directions(48)
    coef = np.random.RandomState(3).randn(5, 4, 3, 3, nb)
    rgb_dirs = np.einsum("kj,...cj->k...c", sh.basis(dirs, degree), coef)
    got, cond = sh.project(rgb_dirs, dirs, degree)
    assert got.shape == coef.shape and np.abs(got - coef).max() < 1e-13
    assert (cond >= np.abs(got) - 1e-13).all()
    W = baked.sh_weights(dirs, degree)  # the weights the kernel is handed: the same pseudo-inverse, rounded once
    assert W.dtype == np.float32 and W.shape == (nb, 48)
    assert np.abs(W - np.linalg.pinv(sh.basis(dirs, degree))).max() <= 2.0 ** -24 * np.abs(W).max()
    # a colour that does not depend on the direction: k[c][0] = colour / Y0, zeros elsewhere
    colour = np.array([0.2, 0.5, 0.9])
    flat, _ = sh.project(np.broadcast_to(colour, (48, 2, 3)), dirs, degree)
    assert np.abs(flat[..., 0] - colour / sh.Y0).max() < 1e-13 and np.abs(flat[..., 1:]).max() < 1e-13


def test_directions_that_do_not_determine_the_expansion_are_refused():
    from upnerf_amd import baked
    dirs = sh.sphere_directions(48)
    with pytest.raises(ValueError):
        baked.sh_weights(dirs[:3], 1)  # K < nb
    with pytest.raises(ValueError):
        baked.sh_weights(dirs[:8], 2)
    ang = np.linspace(0, 2 * np.pi, 24, endpoint=False)
    coplanar = np.stack([np.cos(ang), np.sin(ang), np.zeros(24)], 1)
    with pytest.raises(ValueError):
        baked.sh_weights(coplanar, 2)
    with pytest.raises(ValueError):
        baked.sh_weights(coplanar, 1)  # (z never varies)
    bad = dirs.copy()
    bad[5] = 0
    with pytest.raises(ValueError):
        baked.sh_weights(bad, 1)
    bad[5] = (np.nan, 0, 1)
    with pytest.raises(ValueError):
        baked.sh_weights(bad, 1)
    for degree in (0, 3, None):
        with pytest.raises(ValueError):
            baked.sh_weights(dirs, degree)
    assert baked.sh_weights(dirs[:9], 2).shape == (9, 9) and baked.sh_weights(dirs[:4], 1).shape == (4, 4)
    with pytest.raises(ValueError):
        baked.sphere_directions(0)


def test_pack_and_unpack_are_the_stated_record():
    rng = np.random.RandomState(2)
    for degree in (1, 2):
        nb = sh.NB[degree]
        coef = rng.randn(4, 3, 5, 3, nb).astype(np.float32)
        sigma = rng.uniform(-0.5, 3.0, (4, 3, 5)).astype(np.float32)
        sigma.reshape(-1)[[1, 9]] = [np.nan, np.inf]
        coef[2, 1, 3, 1, 2] = np.inf      # a coefficient that is not finite drops its point
        coef[3, 2, 4, 0, 0] = 1e6         # saturates
        coef[3, 2, 3, 2, nb - 1] = -7e4
        sigma[3, 2, 4] = sigma[3, 2, 3] = sigma[2, 1, 3] = 2.0
        rec, keep = sh.pack(coef, sigma, 1.0, degree)
        assert rec.shape == (4, 3, 5, sh.RECORD[degree]) and rec.dtype == np.uint8
        want = br.prune(sigma, None, 1.0)[..., 3] > 0
        want[2, 1, 3] = False
        assert np.array_equal(keep, want) and 0.2 < keep.mean() < 0.8
        assert not rec[~keep].any()  # a dropped point is an all-zero record
        k, s = sh.unpack(rec, degree)
        assert np.array_equal(s, np.where(keep, sigma, 0).astype(np.float64))
        assert k[3, 2, 4, 0, 0] == 65504.0 and k[3, 2, 3, 2, nb - 1] == -65504.0
        ok = keep & (np.abs(coef).max((-1, -2)) < 6e4)
        assert np.abs(k[ok] - coef[ok]).max() <= 2.0 ** -11 * np.abs(coef[ok]).max()
        pad = np.ones(sh.RECORD[degree], bool)
        pad[:6 * nb] = False
        pad[sh.SIGMA_BYTE[degree]:sh.SIGMA_BYTE[degree] + 4] = False
        assert pad.sum() == (4 if degree == 1 else 6) and not rec[..., pad].any()  # every other byte is zero


# ---- host checks ---------------------------------------------------------------------------------------------------------------------

def _render_args(**kw):
    from upnerf_amd import _lib
    one = ctypes.c_void_p(64)  # (non-null, aligned, never dereferenced: every case below is refused on the host)
    a = _lib.BakedShRenderArgs(Cx=8, Cy=9, Cz=10, R=5, lo=(ctypes.c_float * 3)(-1, -1, -1), hi=(ctypes.c_float * 3)(1, 1, 1), step=0.1,
                               background=0.0, stop=0.0, degree=2, records=one, words=one, rays=one, rgb=one, depth=one, opacity=one)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("case", [
    dict(degree=0), dict(degree=3), dict(degree=-1),
    dict(records=ctypes.c_void_p(32)), dict(records=ctypes.c_void_p(16), degree=1), dict(records=None),  # aligned to the record size
    dict(R=0), dict(Cx=0), dict(Cz=-1), dict(Cx=70000, Cy=70000), dict(step=0.0), dict(step=float("nan")), dict(step=float("inf")),
    dict(background=float("nan")), dict(stop=-0.1), dict(stop=1.0), dict(stop=float("nan")),
    dict(words=None), dict(rays=None), dict(rgb=None), dict(depth=None), dict(opacity=None), dict(rays=ctypes.c_void_p(20)),
    dict(hi=(ctypes.c_float * 3)(1, -1, 1)), dict(lo=(ctypes.c_float * 3)(float("nan"), -1, -1)),
])
def test_baked_sh_render_refuses_before_launch(case):
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_baked_sh_render(ctypes.byref(_render_args(**case)), None) == -1
    assert _lib.lib.upnerf_baked_sh_render(None, None) == -1


def test_sh_accumulate_and_sh_pack_refuse_before_launch():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(64)
    w = lambda *v: (ctypes.c_float * 9)(*v)
    ok = dict(n=10, nb=4, first=1, w=w(1, 2, 3, 4), rgb=one, acc=one)
    for bad in (dict(n=0), dict(nb=0), dict(nb=3), dict(nb=16), dict(rgb=None), dict(acc=None), dict(w=w(1, float("nan"), 3, 4)),
                dict(nb=9, w=w(1, 2, 3, 4, 5, 6, 7, 8, float("inf")))):
        assert _lib.lib.upnerf_sh_accumulate(ctypes.byref(_lib.ShAccumulateArgs(**{**ok, **bad})), None) == -1, bad
    assert _lib.lib.upnerf_sh_accumulate(None, None) == -1
    ok = dict(n=10, level=0.5, degree=2, sigma=one, acc=one, records=one, kept=None)
    for bad in (dict(n=0), dict(degree=0), dict(degree=3), dict(sigma=None), dict(acc=None), dict(records=None),
                dict(records=ctypes.c_void_p(32)), dict(records=ctypes.c_void_p(16), degree=1), dict(level=float("nan"))):
        assert _lib.lib.upnerf_baked_sh_pack(ctypes.byref(_lib.BakedShPackArgs(**{**ok, **bad})), None) == -1, bad
    assert _lib.lib.upnerf_baked_sh_pack(None, None) == -1


def test_the_python_surface_refuses_on_the_host():
    import torch
    from upnerf_amd import baked
    dirs = sh.sphere_directions(8)
    with pytest.raises(RuntimeError):  # no CPU path
        baked.BakedScene.from_records(torch.zeros(3, 3, 3, 32, dtype=torch.uint8), br.BOUNDS, 0.0, 1)
    with pytest.raises(RuntimeError):
        baked.BakedScene.from_direction_grids(torch.zeros(3, 3, 3), torch.zeros(8, 3, 3, 3, 3), dirs, br.BOUNDS, 0.0, 1)
    for degree in (0, 3):
        with pytest.raises(ValueError):
            baked.BakedScene.from_records(torch.zeros(3, 3, 3, 32, dtype=torch.uint8), br.BOUNDS, 0.0, degree)
    # build refuses view_dir beside sh_degree > 0, dirs at degree 0, an unknown degree and too few directions before it looks at the system
    for kw in (dict(sh_degree=1, view_dir=(0, 0, 1)), dict(dirs=dirs), dict(sh_degree=3), dict(sh_degree=2, dirs=dirs)):
        with pytest.raises(ValueError):
            baked.BakedScene.build(None, br.BOUNDS, (4, 4, 4), 1.0, img_id=0, **kw)


def test_save_and_load_round_trip_the_arrays(tmp_path):
    from upnerf_amd import baked
    for degree in (1, 2):
        records, level = sh.sh_grid("blob", degree)
        path = str(tmp_path / f"scene{degree}.npz")
        baked.save_arrays(path, records, br.BOUNDS, level, sh_degree=degree)
        with np.load(path) as f:
            assert set(f.files) == {"records", "degree", "bounds", "level"}
        back, bounds, lv, deg = baked.load_arrays(path)
        assert back.dtype == np.uint8 and np.array_equal(back, records) and deg == degree and lv == level
        assert bounds == (tuple(float(x) for x in br.BOUNDS[0]), tuple(float(x) for x in br.BOUNDS[1]))
        with pytest.raises(ValueError):
            baked.save_arrays(path, records, br.BOUNDS, level, sh_degree=3 - degree)  # the other degree's record size
        with pytest.raises(ValueError):
            baked.save_arrays(path, records.astype(np.float32), br.BOUNDS, level, sh_degree=degree)
    rgbs, level = br.blob_grid()
    old = str(tmp_path / "old.npz")
    baked.save_arrays(old, rgbs, br.BOUNDS, level)  # a degree-0 file: the arrays it always had, and it still loads
    with np.load(old) as f:
        assert set(f.files) == {"rgbs", "bounds", "level"}
    back = baked.load_arrays(old)
    assert len(back) == 3 and np.array_equal(back[0].view(np.int32), rgbs.view(np.int32))
    mixed = str(tmp_path / "mixed.npz")
    np.savez(mixed, records=records, degree=np.int64(2), bounds=np.zeros((2, 3)), level=np.float64(0), rgbs=rgbs)
    with pytest.raises(ValueError):
        baked.load_arrays(mixed)  # neither of the two exact key sets
    np.savez(mixed, records=records, degree=np.int64(1), bounds=np.asarray(br.BOUNDS, np.float64), level=np.float64(0))
    with pytest.raises(ValueError):
        baked.load_arrays(mixed)  # 64-byte records under degree 1


# ---- the fixtures of the GPU test ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", list(sh.GRIDS))
def test_the_fixtures_clamp_on_both_sides_and_depend_on_the_direction(name, degree):
    records, _ = sh.sh_grid(name, degree)
    rgbs, _ = sh.GRIDS[name]()
    k, sigma = sh.unpack(records, degree)
    assert np.array_equal(sigma, rgbs[..., 3].astype(np.float64))  # the density, kept points and bits of baked_ref's grid
    assert not records[sigma == 0].any() and np.abs(k).max() < 16
    rays = br.make_rays()
    dt = sh.steps(records)["cell"]
    ref = sh.render(records, degree, br.BOUNDS, rays, dt, 0.0)
    below, above, neither = ref["clamp"].sum(0) / ref["clamp"].sum()
    print(f"{name} degree {degree}: of {ref['clamp'].sum()} blended colour values {below:.3f} clamp at 0, {above:.3f} at 1, {neither:.3f} at neither")
    assert below >= 0.05 and above >= 0.05 and neither >= 0.5
    # the two axis-parallel rays where they meet the density (they pass between the two corner bricks of the second grid and show
    # the background there whatever the direction), and on either grid the most opaque ray
    picked = [r for r in (0, 7) if ref["n"][r] > 0] + [int(np.argmax(ref["opacity"]))]
    assert name != "blob" or picked[:2] == [0, 7]
    other = sh.render(records, degree, br.BOUNDS, rays[picked], dt, 0.0, view_sign=-1.0)
    for i, r in enumerate(picked):
        ratio = np.abs(other["rgb"][i] - ref["rgb"][r]) / ref["gate_rgb"][r]
        print(f"  ray {r}: rgb {ref['rgb'][r]} against {other['rgb'][i]} for the opposite direction: {ratio.max():.0f} gates")
        assert ref["n"][r] > 0 and ratio.max() > 100
