"""Surface normals (upnerf_amd/normals.py), the parts that need no GPU: the fp64 restatement the GPU tests
compare against is itself checked against central differences, its ReLU margins against the 2 % the GPU gate assumes, the
compositing and colour rules on hand-made cases, and the host-side guards."""
import ctypes
import os

import numpy as np
import pytest
import torch

import normals_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_gradient_agrees_with_central_differences():
    """autograd of the restatement against (sigma(x + h e) - sigma(x - h e)) / 2h in fp64, h = 1e-6, on 32 seeded points.
    Gate: the truncation error of the difference, h^2 / 6 |sigma'''| with |sigma'''| <= (2^9 pi)^3 max|grad| / (2^9 pi) at
    worst, plus its rounding error eps64 sigma / h -- relative to max |grad|: 1e-12 * 2.6e6 / 6 + 2.2e-16 / 1e-6 < 1e-6.
    A point is left out when a ReLU decision differs between x - h e and x + h e on some axis: the kink between them breaks the
    difference, not the gradient (the pre-activations move by up to 2^9 pi h relative to their scale: a few per 32 points)."""
    W, D, skip = 64, 8, 4
    sd, pts = nr.make_field(W, D, skip, nr.SEEDS[(W, D, skip)]), nr.make_points(5, 32)
    wk = nr.band_weights("ones")
    sigma, grad, margin, _ = nr.density(sd, pts, wk, D, skip)
    h = 1e-6
    fd = np.zeros_like(grad)
    x = pts.double()
    keep = np.ones(32, bool)
    for n in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[n] = h
        (sp, onp), (sm, onm) = nr.density_only(sd, x + e, wk, D, skip), nr.density_only(sd, x - e, wk, D, skip)
        fd[:, n] = ((sp - sm) / (2 * h)).numpy()
        keep &= (onp == onm).all(1).numpy()
    print(f"{keep.sum()} of 32 points without a kink inside the stencil")
    assert keep.sum() >= 24
    err = np.abs(fd - grad)[keep].max() / np.sqrt((grad ** 2).sum(1)).max()
    print(f"central differences vs autograd: {err:.3e}")
    assert err < 1e-6


@pytest.mark.parametrize("shape", nr.SHAPES, ids=str)
@pytest.mark.parametrize("band", nr.BANDS)
def test_committed_seeds_leave_out_at_most_two_percent(shape, band):
    """The precondition of the GPU gate, on the reference alone: at most 2 % of a case's points have a ReLU margin below 1e-5,
    and the density is neither saturated nor dead."""
    W, D, skip = shape
    sd, pts = nr.make_field(W, D, skip, nr.SEEDS[shape]), nr.make_points(nr.SEEDS[shape])
    sigma, grad, margin, pre = nr.density(sd, pts, nr.band_weights(band), D, skip)
    out = int((margin < nr.MARGIN_MIN).sum())
    print(f"{shape} {band}: {out} of {len(margin)} below the margin; sigma {sigma.min():.3g} .. {sigma.max():.3g}")
    assert out <= 0.02 * len(margin)
    assert margin[0] >= nr.MARGIN_MIN  # the one-point case M = 1 is point 0: it must be among the measured ones
    assert pts.abs().max() <= 1 and float(pts[0, 1]) == 0.0
    assert pre.max() < 20 and np.median(sigma) > 1e-2 and sigma.max() > 1.2 * sigma.min()
    assert (np.abs(grad).sum(1) > 0).all()
    if band == "zeros":  # only the identity block carries gradient: no 2^k pi factor anywhere
        assert np.sqrt((grad ** 2).sum(1)).max() < 10


@pytest.mark.parametrize("band", nr.BANDS)
def test_dense_256x8_field_states_its_left_out_share(band):
    """The dense (256, 8, 4) field of the GPU test: 2048 data-dependent units leave 12 - 14 % of the points below the margin
    (32 - 35 of 257), which is why the 2 % case of that shape keeps 24 live units per layer; point 0 is above it."""
    W, D, skip = 256, 8, 4
    sd, pts = nr.make_field(W, D, skip, nr.SEEDS[(W, D, skip)], dense=True), nr.make_points(nr.SEEDS[(W, D, skip)])
    sigma, grad, margin, pre = nr.density(sd, pts, nr.band_weights(band), D, skip)
    out = int((margin < nr.MARGIN_MIN).sum())
    print(f"dense (256, 8, 4) {band}: {out} of {len(margin)} below the margin")
    assert 0.02 * len(margin) < out <= 0.15 * len(margin) and margin[0] >= nr.MARGIN_MIN
    assert pre.max() < 20 and np.median(sigma) > 1e-2


def test_live_units_sit_in_every_column_block():
    cols = nr.live_columns(256, nr.LIVE[(256, 8, 4)])
    assert len(cols) == 24 and sorted(set((cols // 32).tolist())) == list(range(8))
    sd = nr.make_field(256, 8, 4, 11)
    assert all(int((sd[f"xyz_encoding_{l + 1}.0.bias"] > -999).sum()) == 24 for l in range(8))


def test_head_bias_case_takes_the_linear_branch():
    (W, D, skip), bias = nr.HEAD_BIAS_CASE
    sd, pts = nr.make_field(W, D, skip, nr.SEEDS[(W, D, skip)], head_bias=bias), nr.make_points(nr.SEEDS[(W, D, skip)])
    sigma, grad, margin, pre = nr.density(sd, pts, nr.band_weights("ones"), D, skip)
    assert pre.min() > 20 and int((margin < nr.MARGIN_MIN).sum()) <= 0.02 * len(margin) and margin[0] >= nr.MARGIN_MIN


def test_entry_points_refuse_bad_arguments_before_launch():
    from upnerf_amd import _lib
    one = ctypes.c_void_p(16)
    L = _lib.Layout()
    L.W, L.D, L.skip = 256, 8, 4
    ok = dict(M=5, points=one, P=one, PT=one, sigma=one, grad=one)
    call = lambda L, **kw: _lib.lib.upnerf_density_grad(ctypes.byref(L), ctypes.byref(_lib.DensityGradArgs(**{**ok, **kw})), None)
    assert call(L, M=0) == -1 and call(L, points=None) == -1 and call(L, PT=None) == -1 and call(L, grad=None) == -1
    L.W = 128
    assert call(L) == -2
    L.W, L.D = 64, 9
    assert call(L) == -2
    L.D, L.skip = 4, 4
    assert call(L) == -1
    assert _lib.lib.upnerf_density_grad(None, None, None) == -1
    nc = lambda **kw: _lib.lib.upnerf_normal_composite(
        ctypes.byref(_lib.NormalCompositeArgs(**{**dict(R=3, S=4, grad=one, w=one, normal=one), **kw})), None)
    assert nc(R=0) == -1 and nc(S=0) == -1 and nc(w=None) == -1 and nc(R=1 << 20, S=1 << 12) == -1
    vz = lambda **kw: _lib.lib.upnerf_viz_normals(ctypes.byref(_lib.VizNormalsArgs(**{**dict(H=2, W=2, n=one, rgb=one), **kw})), None)
    assert vz(H=0) == -1 and vz(n=None) == -1 and vz(rgb=None) == -1


def test_composite_rule_on_hand_made_cases():
    g = np.zeros((4, 3, 3), np.float32)
    w = np.zeros((4, 3), np.float32)
    g[0] = [[1, 0, 0], [0, 2, 0], [0, 0, 3]]                      # ray 0: all weights zero -> (0, 0, 0)
    g[1], w[1] = [[0, 0, 0], [0, 0, -5], [0, 0, 0]], [0.5, 0.25, 0.1]   # ray 1: zero gradients count as zero -> +z
    g[2], w[2] = [[3, 4, 0], [0, 1, 0], [1, 0, 0]], [1.0, 1e-9, 1e-9]   # ray 2: one dominant sample -> -(0.6, 0.8, 0)
    g[3], w[3] = [[np.nan, 1, 0], [np.inf, 0, 0], [0, 0, 0]], [1, 1, 1]  # ray 3: nothing usable -> (0, 0, 0), not NaN
    out, tol = nr.composite_ref(g.reshape(-1, 3), w)
    assert np.array_equal(out[0], [0, 0, 0]) and np.array_equal(out[3], [0, 0, 0]) and not np.isnan(out).any()
    assert np.allclose(out[1], [0, 0, 1], atol=1e-15)
    assert np.allclose(out[2], [-0.6, -0.8, 0], atol=1e-8)
    assert np.allclose(np.sqrt((out[[1, 2]] ** 2).sum(1)), 1.0, atol=1e-15) and tol[0] == 0 and tol[1] < 1e-5


def test_colour_rule_on_hand_made_cases():
    n = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [0, 0, 1], [np.nan, 0.5, -0.5], [-0.0, 0.0, 0.0]], np.float32)
    got = nr.viz_ref(n)
    assert got.tolist() == [[128, 128, 128], [255, 127, 127], [127, 0, 127], [127, 127, 255], [0, 191, 63], [128, 128, 128]]
    rot = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float32)  # x -> -y, y -> x
    assert nr.viz_ref(n[1:4], rot).tolist() == [[127, 0, 127], [0, 127, 127], [127, 127, 255]]
    assert nr.viz_ref(n[:1], rot).tolist() == [[128, 128, 128]]  # a zero normal stays grey under any rotation


def test_cpu_devices_are_refused_with_the_usual_errors():
    from upnerf_amd import normals as nm
    from upnerf_amd import novel_view as nv
    from upnerf_amd.rendering import render_rays
    from upnerf_amd.visualization import normal_image, plan_validation_images
    with pytest.raises(RuntimeError, match="GPU only"):
        render_rays({}, {}, torch.zeros(4, 8), None, 1, normals=True)
    with pytest.raises(RuntimeError):
        nm.normal_composite(torch.zeros(4, 3), torch.zeros(2, 2))
    with pytest.raises(RuntimeError):
        normal_image(torch.zeros(4, 3), (2, 2))
    W, D, skip = 64, 2, None
    model = nr.build_module(W, D, skip, nr.make_field(W, D, skip, 11))
    with pytest.raises(RuntimeError):
        nm.field_density_gradient(model, torch.zeros(4, 3))
    system = type("S", (), {"models": {"nerf_fine": model}})()
    with pytest.raises(RuntimeError, match="GPU only"):
        nm.density_gradient(system, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        nm.density_gradient(system, torch.zeros(4, 3), field="transient")
    with pytest.raises(ValueError):
        nm.density_gradient(system, torch.zeros(4, 3), field="coarse")

    class Sys(torch.nn.Module):
        hparams = {"val.chunk_size": 64}
        fine, _host_progress = True, 1.0

        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(2, 2)

        def get_schedule_mult(self, p):
            return 1

    path = nv.CameraPath.from_poses(torch.eye(4)[:3].repeat(2, 1, 1), (0.1, 2.0), 2, (0, 0), (4, 4),
                                    torch.tensor([[4.0, 0, 2], [0, 4.0, 2], [0, 0, 1]]))
    with pytest.raises(RuntimeError, match="GPU only"):
        nv.render_path(Sys(), path, outputs=("rgb", "normal"))
    with pytest.raises(ValueError):
        nv.render_path(Sys(), path, outputs=("normals",))  # not a name
    plan = plan_validation_images(["rgb_fine", "normal_fine", "normal_coarse"], {"rgb_fine": (16, 3), "normal_fine": (16, 3)}, "fine",
                                  False, False)
    assert plan == [("rgb_GT", "rgb", "rgbs"), ("rgb_fine", "rgb", "rgb_fine"), ("normal_fine", "normal", "normal_fine")]


def test_refine_normals_keeps_vertices_and_faces(monkeypatch):
    from upnerf_amd import geometry
    from upnerf_amd import normals as nm
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    n = torch.nn.functional.normalize(torch.tensor([[1.0, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]]), dim=1)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    col = torch.rand(4, 3)
    mesh = geometry.Mesh(v, n, f, col)
    grad = torch.tensor([[0.0, 0, -2], [3, 4, 0], [0, 0, 0], [float("nan"), 1, 0]])
    seen = {}

    def fake(system, points, field="fine"):
        seen.update(points=points, field=field)
        return torch.ones(4), grad
    monkeypatch.setattr(nm, "density_gradient", fake)
    out = geometry.refine_normals(None, mesh, field="coarse")
    assert out.vertices is mesh.vertices and out.faces is mesh.faces and out.colours is mesh.colours
    assert seen["points"] is mesh.vertices and seen["field"] == "coarse"
    assert torch.equal(mesh.normals, n)  # the input mesh is untouched
    want = torch.stack([torch.tensor([0.0, 0, 1]), torch.tensor([-0.6, -0.8, 0]), n[2], n[3]])  # zero / NaN keep the grid normal
    assert torch.allclose(out.normals, want, atol=1e-7) and torch.equal(out.normals[2:], n[2:])


def test_tools_know_the_new_flags():
    import importlib.util
    for tool, flag, attr in (("render_path", "--normals", "normals"), ("extract_mesh", "--analytic-normals", "analytic_normals")):
        spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, "tools", tool + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        acts = {a.dest: a for a in mod.parser()._actions}
        assert attr in acts and flag in acts[attr].option_strings and acts[attr].default is False
