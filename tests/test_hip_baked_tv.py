"""The total variation of a baked scene's point arrays on the GPU (csrc/baked_reg.hip: upnerf_baked_tv; upnerf_amd/baked_reg.py;
DESIGN.md 2.37).

Reference: tests/baked_tv_ref.py -- fp64 numpy; its docstring derives the per-element gate from a count of the roundings in the
stated operation order (four for the sum and the product with w on a dense grid, seven over the copies of a pool).  No element is
left out: an element the definition does not touch must keep its bits.  Nothing here is atomic, so two runs are held to equality.
The five grids are baked_tv_ref.GRIDS; F = 1, 4, 12, 27 are the point arrays of the three degrees; eps = 1e-8 and 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import baked_cases as cases
import baked_ref as br
import baked_sparse_ref as sr
import baked_tv_ref as tvr
from baked_cases import dev

pytestmark = pytest.mark.gpu

_CACHE = {}
FS = [1, 4, 12, 27]
EPS = [1e-8, 1.0]


def grid(name):
    """(sigma [Nz, Ny, Nx], cells bool, the OccupancyGrid of the cells) of a grid."""
    if ("grid", name) not in _CACHE:
        from upnerf_amd.occupancy import OccupancyGrid
        rgbs = tvr.GRIDS[name]()[0]
        cells = br.occupied_cells(rgbs)
        _CACHE["grid", name] = (rgbs[..., 3].copy(), cells, OccupancyGrid.from_cells(dev(cells), br.BOUNDS))
    return _CACHE["grid", name]


def layout(name):
    """(PoolParams of the grid's occupied bricks, bricks as numpy)."""
    if ("layout", name) not in _CACHE:
        from upnerf_amd import baked
        from upnerf_amd import baked_sparse_tune as st
        _, cells, occ = grid(name)
        slots, bricks, n = baked.brick_table(occ.words, occ.dims)
        assert n >= 1
        _CACHE["layout", name] = (st.PoolParams(slots, bricks, occ, br.BOUNDS, 0, rgbs=torch.zeros(n, 9, 9, 9, 4, device="cuda")),
                                  bricks.cpu().numpy())
    return _CACHE["layout", name]


def reference(name, F, eps, roundings=4):
    key = ("ref", name, F, eps, roundings)
    if key not in _CACHE:
        sigma, cells, _ = grid(name)
        _CACHE[key] = tvr.tv(tvr.point_data(name, F), sigma, cells, tvr.weights(F), eps, roundings=roundings)
    return _CACHE[key]


def held(got, want, gate, touched, before=None, what=""):
    """Every element within its gate; an element the definition does not touch keeps its bits.  Returns the worst err / gate."""
    g = got.astype(np.float64)
    assert np.isfinite(g).all(), what
    err = np.abs(g - want)
    assert (err <= gate).all(), (what, np.argwhere(err > gate)[:5], float(err.max()))
    before = np.zeros_like(got) if before is None else before
    assert np.array_equal(got[~touched].view(np.uint32), before[~touched].view(np.uint32)), what
    return float((err / np.maximum(gate, 1e-300))[gate > 0].max(initial=0.0))


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("name", list(tvr.GRIDS))
def test_dense_value_and_gradient_are_within_the_gate_on_every_element(name, F, eps):
    from upnerf_amd import baked_reg
    sigma, cells, occ = grid(name)
    ref = reference(name, F, eps)
    data, w = dev(tvr.point_data(name, F)), tvr.weights(F)
    value, grad = baked_reg.tv(data, dev(sigma), occ, w, eps)
    torch.cuda.synchronize()
    assert value.dim() == 0 and value.is_cuda and tuple(grad.shape) == tuple(data.shape)
    got = grad.cpu().numpy()
    worst = held(got, ref["grad"], ref["gate"], ref["touched"], what=(name, F, eps))
    verr = abs(float(value) - ref["value"])
    print(f"{name} F {F} eps {eps}: {int(ref['touched'].sum())} elements touched, worst err / gate {worst:.3f}; value {float(value):.6e}, "
          f"err / gate {verr / max(ref['value_gate'], 1e-300):.3f}")
    assert verr <= ref["value_gate"]
    assert ref["touched"].sum() >= F and ref["value"] > 0
    value2, grad2 = baked_reg.tv(data, dev(sigma), occ, w, eps)  # a second run: the same bits
    assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32)) and torch.equal(value2.view(torch.int32), value.view(torch.int32))


@pytest.mark.parametrize("name", ["blob", "big", "face"])
def test_gradient_is_added_and_a_zero_weight_leaves_the_bits(name):
    from upnerf_amd import baked_reg
    F, eps = 4, 1e-8
    sigma, cells, occ = grid(name)
    data = tvr.point_data(name, F)
    out0 = (np.random.RandomState(5).randn(*data.shape) * 3).astype(np.float32)
    out0[..., 0] = -0.0  # (bits that an added +0 would change)
    w = tvr.weights(F)
    ref = tvr.tv(data, sigma, cells, w, eps, grad0=out0)
    out = dev(out0)
    value, back = baked_reg.tv_backward(dev(data), dev(sigma), occ, w, eps, out=out)
    assert back is out
    held(out.cpu().numpy(), out0.astype(np.float64) + ref["grad"], ref["gate"], ref["touched"], before=out0, what=name)
    w0 = w.copy()
    w0[1] = 0.0
    out = dev(out0)
    baked_reg.tv_backward(dev(data), dev(sigma), occ, w0, eps, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got[..., 1].view(np.uint32), out0[..., 1].view(np.uint32))
    assert not np.array_equal(got[..., 2], out0[..., 2])
    # rgbs[..., 3] as the sigma pointer: an element stride of four
    rgbs = dev(np.concatenate([data[..., :3], sigma[..., None]], -1))
    strided = baked_reg.tv(dev(data), rgbs[..., 3], occ, w, eps)[1]
    assert torch.equal(strided, baked_reg.tv(dev(data), dev(sigma), occ, w, eps)[1])


@pytest.mark.parametrize("F", [1, 4, 27])
@pytest.mark.parametrize("name", list(tvr.GRIDS))
def test_pool_copies_receive_their_own_bricks_cells_and_the_face_sum_gives_the_dense_gradient(name, F):
    from upnerf_amd import baked_reg
    eps = 1e-8
    sigma, cells, occ = grid(name)
    params, bricks = layout(name)
    data, w = tvr.point_data(name, F), tvr.weights(F)
    pool_data, pool_sigma = sr.gather(data, bricks), sr.gather(sigma[..., None], bricks)[..., 0]
    per_copy = tvr.tv_pool(pool_data, pool_sigma, bricks, cells, w, eps)
    value, raw = baked_reg.tv(dev(pool_data), dev(pool_sigma), occ, w, eps, layout=params, face_sum=False)
    worst = held(raw.cpu().numpy(), per_copy["grad"], per_copy["gate"], per_copy["touched"], what=(name, F, "copies"))
    assert abs(float(value) - per_copy["value"]) <= per_copy["value_gate"]
    dense = reference(name, F, eps, roundings=7)
    g = lambda a: sr.gather(a, bricks)
    _, summed = baked_reg.tv(dev(pool_data), dev(pool_sigma), occ, w, eps, layout=params)
    got = summed.cpu().numpy()
    worst2 = held(got, g(dense["grad"]), g(dense["gate"]), g(dense["touched"]), what=(name, F, "summed"))
    print(f"{name} F {F}: {len(bricks)} bricks; worst err / gate per copy {worst:.3f}, after the face sum {worst2:.3f}")
    # the copies of a shared point hold identical bytes: every copy is its owner's
    Nz, Ny, Nx = sigma.shape
    again = sr.gather(sr.scatter(got, bricks, (Nx, Ny, Nz)), bricks)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    _, twice = baked_reg.tv(dev(pool_data), dev(pool_sigma), occ, w, eps, layout=params)
    assert torch.equal(twice.view(torch.int32), summed.view(torch.int32))


def test_refusals():
    from upnerf_amd import _lib
    from upnerf_amd._lib import lib, ptr
    sigma, cells, occ = grid("blob")
    params, bricks = layout("blob")
    Cx, Cy, Cz = occ.dims
    data, grad = torch.zeros(Cz + 1, Cy + 1, Cx + 1, 4, device="cuda"), torch.zeros(Cz + 1, Cy + 1, Cx + 1, 4, device="cuda")
    s = dev(sigma)

    def call(**kw):
        w = kw.pop("w", [1.0] * 4)
        a = dict(Cx=Cx, Cy=Cy, Cz=Cz, n_bricks=0, F=4, sigma_stride=1, eps=1e-8, words=ptr(occ.words), slots=None, bricks=None,
                 data=ptr(data), sigma=ptr(s), grad=ptr(grad), partial=None)
        a.update(kw)
        args = _lib.BakedTvArgs(w=(C.c_float * 28)(*(list(w) + [0.0] * (28 - len(w)))), **a)
        return lib.upnerf_baked_tv(C.byref(args), None)

    assert call() == 0
    torch.cuda.synchronize()
    assert lib.upnerf_baked_tv(None, None) == -1
    for field in ("words", "data", "sigma", "grad"):
        assert call(**{field: None}) == -1, field
    for bad in (dict(Cx=0), dict(Cx=1 << 16, Cy=1 << 16, Cz=2), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")),
                dict(w=[1.0, float("nan"), 1.0, 1.0]), dict(w=[1.0, 1.0, float("inf"), 1.0]), dict(F=0), dict(F=29), dict(sigma_stride=0),
                dict(n_bricks=-1), dict(n_bricks=5), dict(slots=ptr(params.slots)), dict(bricks=ptr(params.bricks)),
                dict(n_bricks=len(bricks)), dict(n_bricks=len(bricks), slots=ptr(params.slots))):
        assert call(**bad) == -1, bad
    assert lib.upnerf_baked_tv_blocks(0, 1, 1, 0) == -1 and lib.upnerf_baked_tv_blocks(Cx, Cy, Cz, 0) == 2 * 2 * 2
    assert lib.upnerf_baked_tv_blocks(Cx, Cy, Cz, len(bricks)) == len(bricks)
    assert float(grad.abs().max()) == 0.0  # a refused call launches nothing (the accepted one ran on zero data: zero gradient)
    from upnerf_amd import baked_reg
    with pytest.raises(ValueError):
        baked_reg.tv(data, s, occ, [1.0] * 3, 1e-8)
    with pytest.raises(ValueError):
        baked_reg.tv(data[:-1], s, occ, [1.0] * 4, 1e-8)


def missing_rays(R=16):
    """Rays that all point away from the box: the marcher's backward pass adds nothing."""
    rays = np.zeros((R, 8), np.float32)
    rays[:, :3] = [3.0, 3.0, 3.0]
    rays[:, 3:6] = [1.0, 0.2, 0.3]
    rays[:, 7] = 2.0
    return rays


def scene_of(degree, sparse):
    import baked_upsample_ref as ur
    dense = cases.build(*ur.parents("big", degree), degree)  # (built anew at every call)
    return dense.sparsify() if sparse else dense


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("degree", [0, 2])
def test_a_tuner_on_missing_rays_lowers_the_tv_bit_for_bit_and_launches_nothing_when_off(degree, sparse):
    from upnerf_amd.ops import TIMER
    rays = dev(missing_rays())
    target = torch.zeros(rays.shape[0], 3, device="cuda")

    def run(**tv):
        scene = scene_of(degree, sparse)
        tuner = (scene.tune_pool if sparse else scene.tune)(0.01, **tv)
        values = []
        for _ in range(5):
            tuner.step(rays, target, 0.05)
            values.append(tuner.last_tv)
        return tuner, values

    on = dict(tv_sigma=1.0, tv_colour=0.5)
    tuner, values = run(**on)
    assert all(v.dim() == 0 and v.is_cuda for v in values)
    values = [float(v) for v in values]
    print(f"degree {degree} {'pool' if sparse else 'dense'}: tv {values[0]:.6e} -> {values[-1]:.6e}")
    assert values[-1] < values[0] and np.isfinite(values).all()
    again, _ = run(**on)
    assert torch.equal(again.p.view(torch.int32), tuner.p.view(torch.int32))  # two runs: bit-identical masters
    start = (scene_of(degree, sparse).tune_pool if sparse else scene_of(degree, sparse).tune)(0.01)
    assert not torch.equal(start.p, tuner.p)
    if sparse:  # the copies of a shared point stay identical through the steps
        Nx, Ny, Nz = tuner.resolution
        bricks = tuner.bricks.cpu().numpy()
        for m in tuner.masters:
            got = m.reshape(len(bricks), 9, 9, 9, -1).cpu().numpy()
            assert np.array_equal(sr.gather(sr.scatter(got, bricks, (Nx, Ny, Nz)), bricks).view(np.uint32), got.view(np.uint32))
    TIMER.reset()
    TIMER.enabled = True
    try:
        off, none = run()
        names_off = set(TIMER.records)
        TIMER.reset()
        run(**on)
        names_on = set(TIMER.records)
    finally:
        TIMER.enabled = False
        TIMER.reset()
    assert "baked_tv" not in names_off and "baked_tv" in names_on and none == [None] * 5 and off.last_tv is None
    assert torch.equal(off.p, start.p)  # rays that miss and no penalty: no gradient at all, Adam moves nothing
