"""The total variation restatement tests/baked_tv_ref.py, checked against itself on the CPU: its gradient is the
derivative of its value, the closed form of a constant grid, and who contributes and who receives."""
import numpy as np
import pytest

import baked_ref as br
import baked_tv_ref as tvr


def case(name, F):
    rgbs = tvr.GRIDS[name]()[0]
    return tvr.point_data(name, F), rgbs[..., 3], br.occupied_cells(rgbs), tvr.weights(F)


def _local_value(d, cells, w, eps, z, y, x, f):
    """w[f] times the tv of float f summed over the (up to) eight cells that have point (z, y, x) as ANY corner -- every cell whose
    tv can depend on the point, found without the gather's list of four -- in fp64 on numbers that are NOT rounded to fp32 first,
    and the sum of the terms' magnitudes."""
    Cz, Cy, Cx = cells.shape
    total = mag = 0.0
    for cz in (z - 1, z):
        for cy in (y - 1, y):
            for cx in (x - 1, x):
                if 0 <= cz < Cz and 0 <= cy < Cy and 0 <= cx < Cx and cells[cz, cy, cx]:
                    a = d[cz, cy, cx, f]
                    dx, dy, dz = d[cz, cy, cx + 1, f] - a, d[cz, cy + 1, cx, f] - a, d[cz + 1, cy, cx, f] - a
                    t = float(w[f]) * np.sqrt(eps + dx * dx + dy * dy + dz * dz)
                    total += t
                    mag += abs(t)
    return total, mag


@pytest.mark.parametrize("eps", [1e-8, 1.0])
@pytest.mark.parametrize("name,F", [("blob", 4), ("big", 4), ("cell", 1), ("face", 12), ("exact", 4)])
def test_gradient_is_the_central_difference_of_the_value(name, F, eps):
    """The restated gradient against central differences of the value, element by element.  The bound has two parts, neither
    fitted: the truncation error of D(h), taken as |D(h) - D(h / 2)| (it falls by four per halving: the difference is three
    quarters of it, and D(h / 2) carries the last quarter, so D(h / 2) is held to the whole difference); and the fp64 roundoff of
    the two values -- the sum is over the at most eight cells round the point, each term a dozen roundings (three differences,
    three squares, three additions, the root, the product with w) and the sum seven more: 19 u64 of the terms' magnitudes per
    value, two values over 2 h: 19 * 2^-53 * V / h."""
    data, sigma, cells, w = case(name, F)
    ref = tvr.tv(data, sigma, cells, w, eps)
    d64, e = data.astype(np.float64), float(np.float32(eps))
    rng = np.random.RandomState(3)
    live = np.argwhere(ref["touched"])
    assert len(live) >= 4
    worst = 0.0
    for z, y, x, f in live[rng.choice(len(live), min(60, len(live)), replace=False)]:
        D, V = [], 0.0
        for h in (2e-4, 1e-4):
            up, dn = d64.copy(), d64.copy()
            up[z, y, x, f] += h
            dn[z, y, x, f] -= h
            (vu, mu), (vd, md) = _local_value(up, cells, w, e, z, y, x, f), _local_value(dn, cells, w, e, z, y, x, f)
            D.append((vu - vd) / (2 * h))
            V = max(V, mu, md)
        bound = abs(D[0] - D[1]) + 19 * 2.0 ** -53 * V / 1e-4
        err = abs(D[1] - ref["grad"][z, y, x, f])
        worst = max(worst, err / bound)
        assert err <= bound, (name, F, eps, z, y, x, f, err, bound, ref["grad"][z, y, x, f])
    # the local value is the whole value's dependence on the point: the same difference from the value over every cell
    z, y, x, f = live[0]
    up = d64.copy()
    up[z, y, x, f] += 0.25
    whole = _value64(up, cells, w, eps) - _value64(d64, cells, w, eps)
    local = _local_value(up, cells, w, e, z, y, x, f)[0] - _local_value(d64, cells, w, e, z, y, x, f)[0]
    assert abs(whole - local) <= 1e-12 * abs(ref["value"])  # (fp64 roundoff of a sum over every cell)
    assert abs(_value64(d64, cells, w, eps) - ref["value"]) <= 1e-12 * abs(ref["value"])
    print(f"{name} F {F} eps {eps}: worst err / bound {worst:.3f}")


def _value64(d, cells, w, eps):
    """The value of fp64 data that is NOT rounded to fp32 first, over every cell."""
    a = d[:-1, :-1, :-1]
    dx, dy, dz = d[:-1, :-1, 1:] - a, d[:-1, 1:, :-1] - a, d[1:, :-1, :-1] - a
    t = np.sqrt(float(np.float32(eps)) + dx * dx + dy * dy + dz * dz)
    return float((w.astype(np.float64) * t * cells[..., None]).sum())


def test_occupied_cells_are_counted_from_the_words():
    import baked_sparse_ref as sr
    import torch
    from upnerf_amd.occupancy import OccupancyGrid
    for name in tvr.GRIDS:
        cells = br.occupied_cells(tvr.GRIDS[name]()[0])
        words = torch.from_numpy(sr.words(cells).view(np.int32).copy())
        occ = OccupancyGrid(words, br.BOUNDS, cells.shape[::-1])
        assert occ.n_occupied() == int(cells.sum())
    full = np.ones((3, 5, 7), bool)  # 105 cells: the last word is ragged, and stray bits beyond the cells do not count
    words = sr.words(full).copy()
    words[3] |= np.uint32(0xFFFFFE00)
    assert OccupancyGrid(torch.from_numpy(words.view(np.int32).copy()), br.BOUNDS, (7, 5, 3)).n_occupied() == 105


@pytest.mark.parametrize("eps", [1e-8, 1.0])
@pytest.mark.parametrize("name", list(tvr.GRIDS))
def test_constant_grid_has_the_closed_form(name, eps):
    rgbs = tvr.GRIDS[name]()[0]
    cells, w = br.occupied_cells(rgbs), tvr.weights(4)
    data = np.broadcast_to(np.array([0.3, -2.0, 7.5, 0.0], np.float32), rgbs.shape).copy()
    ref = tvr.tv(data, rgbs[..., 3], cells, w, eps)
    want = int(cells.sum()) * np.sqrt(float(np.float32(eps))) * float(w.astype(np.float64).sum())
    assert abs(ref["value"] - want) <= 1e-12 * want
    assert not ref["grad"].any()
    assert cells.sum() >= 1


@pytest.mark.parametrize("name", ["blob", "big", "face"])
def test_dead_points_and_clear_cells(name):
    F = 4
    data, sigma, cells, w = case(name, F)
    ref = tvr.tv(data, sigma, cells, w, 1e-8)
    assert not ref["grad"][sigma == 0].any() and not ref["gate"][sigma == 0].any() and not ref["touched"][sigma == 0].any()
    # the data of a point that touches no occupied cell does not matter: neither to the value nor to any gradient
    corner = np.zeros(tuple(n + 1 for n in cells.shape), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                corner[dz:dz + cells.shape[0], dy:dy + cells.shape[1], dx:dx + cells.shape[2]] |= cells
    assert (~corner).any()
    other = data.copy()
    other[~corner] += 100.0
    ref2 = tvr.tv(other, sigma, cells, w, 1e-8)
    assert ref2["value"] == ref["value"] and np.array_equal(ref2["grad"], ref["grad"])
    # a zero weight: that float receives nothing and adds nothing
    w0 = w.copy()
    w0[2] = 0
    ref3 = tvr.tv(data, sigma, cells, w0, 1e-8)
    assert not ref3["grad"][..., 2].any() and not ref3["touched"][..., 2].any()
    assert np.array_equal(ref3["grad"][..., :2], ref["grad"][..., :2])
    # with no cell occupied there is nothing at all
    none = tvr.tv(data, sigma, np.zeros_like(cells), w, 1e-8)
    assert none["value"] == 0 and not none["grad"].any()


@pytest.mark.parametrize("name", ["big", "face", "blob"])
def test_the_copies_of_a_pool_sum_to_the_dense_gradient(name):
    import baked_sparse_ref as sr
    F = 4
    data, sigma, cells, w = case(name, F)
    slots, bricks = sr.table(sr.brick_bits(cells))
    dense = tvr.tv(data, sigma, cells, w, 1e-8)
    pool = tvr.tv_pool(sr.gather(data, bricks), sr.gather(sigma[..., None], bricks)[..., 0], bricks, cells, w, 1e-8)
    summed = np.zeros_like(dense["grad"])
    Nz, Ny, Nx = sigma.shape
    Bx, By, Bz = sr.brick_dims(cells.shape[::-1])
    for s, b in enumerate(bricks):
        bx, by, bz = b % Bx, (b // Bx) % By, b // (Bx * By)
        nz, ny, nx = min(9, Nz - 8 * bz), min(9, Ny - 8 * by), min(9, Nx - 8 * bx)
        summed[8 * bz:8 * bz + nz, 8 * by:8 * by + ny, 8 * bx:8 * bx + nx] += pool["grad"][s, :nz, :ny, :nx]
        assert not pool["grad"][s, nz:].any() and not pool["grad"][s, :, ny:].any() and not pool["grad"][s, :, :, nx:].any()
    assert np.abs(summed - dense["grad"]).max() <= 1e-12 * np.abs(dense["grad"]).max()
    assert abs(pool["value"] - dense["value"]) <= 1e-12 * dense["value"]
