"""The arithmetic of baked.Layout -- what the marcher needs beside a point array, dense grid or brick pool -- on CPU tensors
(upnerf_amd/baked.py): shapes, bytes, the empty pool, the pointer pair, and the two parameter classes' refusals.
A Layout does no device work; everything that launches still refuses host memory."""
import pytest
import torch

import baked_ref as br

DEGREES = [0, 1, 2]
POINT_BYTES = {0: 16, 1: 32, 2: 64}
SIGMA_AT = {0: 12, 1: 24, 2: 56}


def occupancy(cells):
    from upnerf_amd import _lib
    from upnerf_amd.occupancy import OccupancyGrid
    words = torch.zeros(int(_lib.lib.upnerf_occ_words(*cells)), dtype=torch.int32)
    return OccupancyGrid(words, br.BOUNDS, cells)


def dense_layout(degree):
    """3 x 4 x 5 points (x, y, z)."""
    from upnerf_amd.baked import Layout
    return Layout(occupancy((2, 3, 4)), br.BOUNDS, degree)


def pool_layout(degree, occupied=(1, 10)):
    """9 x 10 x 17 cells: 2 x 2 x 3 bricks, of which `occupied` (linear indices, ascending) are in the pool."""
    from upnerf_amd.baked import Layout
    slots = torch.full((3, 2, 2), -1, dtype=torch.int32)
    bricks = torch.tensor(occupied, dtype=torch.int32)
    slots.view(-1)[bricks.long()] = torch.arange(len(occupied), dtype=torch.int32)
    return Layout(occupancy((9, 10, 17)), br.BOUNDS, degree, slots, bricks)


@pytest.mark.parametrize("degree", DEGREES)
def test_shapes_and_bytes_of_a_grid_and_of_a_pool(degree):
    nb = (degree + 1) ** 2
    for layout, sparse, shape, res in ((dense_layout(degree), False, (5, 4, 3), (3, 4, 5)), (pool_layout(degree), True, (2, 9, 9, 9), (10, 11, 18))):
        assert layout.sparse is sparse and layout.shape == shape and layout.resolution == res and layout.degree == degree
        assert layout.nb == nb and layout.point_bytes == POINT_BYTES[degree] and layout.sigma_at == SIGMA_AT[degree]
        assert layout.param_shapes == ((shape + (4,),) if degree == 0 else (shape + (3, nb), shape))
        zeros = layout.zeros("cpu")
        assert tuple(tuple(z.shape) for z in zeros) == layout.param_shapes
        assert all(z.dtype == torch.float32 and not z.any() for z in zeros)
        empty = layout.empty_pool(degree, "cpu")
        assert empty.dtype == (torch.float32 if degree == 0 else torch.uint8)
        assert tuple(empty.shape) == (0, 9, 9, 9, 4 if degree == 0 else POINT_BYTES[degree])
        points = torch.zeros(shape + (POINT_BYTES[degree],), dtype=torch.uint8)
        assert layout.marched(points) is points  # with a point to read, the marcher is given the points themselves
    assert dense_layout(degree).slots is None and dense_layout(degree).bricks is None


@pytest.mark.parametrize("degree", DEGREES)
def test_a_pool_with_no_brick_still_has_an_address_for_the_marcher(degree):
    from upnerf_amd.baked import Layout
    layout = pool_layout(degree, occupied=())
    E = POINT_BYTES[degree]
    assert layout.shape == (0, 9, 9, 9)
    spare = layout.marched(Layout.empty_pool(degree, "cpu"))
    assert spare.numel() * spare.element_size() >= E and spare.data_ptr() != 0 and spare.data_ptr() % E == 0
    assert layout.marched(Layout.empty_pool(degree, "cpu")) is spare  # the scene keeps its one spare point
    with pytest.raises(RuntimeError):  # the pair itself is of device addresses: there is no CPU path
        layout.pointers(Layout.empty_pool(degree, "cpu"))


def test_a_layout_is_immutable_and_a_table_is_whole():
    from upnerf_amd.baked import BakedScene, Layout
    layout = pool_layout(0)
    with pytest.raises(AttributeError):
        layout.degree = 2
    with pytest.raises(ValueError):
        Layout(occupancy((9, 10, 17)), br.BOUNDS, 0, slots=layout.slots)
    assert hasattr(BakedScene, "layout") and isinstance(BakedScene.points, property)


@pytest.mark.parametrize("degree", DEGREES)
def test_parameter_classes_refuse_a_wrong_shape_or_dtype_before_the_device(degree):
    """Both check shapes before require_cuda, so CPU tensors reach the refusal; tensors that fit get as far as 'no CPU path'."""
    from upnerf_amd.baked_sparse_tune import PoolParams
    from upnerf_amd.baked_tune import SceneParams
    nb = (degree + 1) ** 2
    dense, pool = dense_layout(degree), pool_layout(degree)
    makers = ((lambda **kw: SceneParams(dense.occupancy, br.BOUNDS, degree, **kw), dense, "scene"),
              (lambda **kw: PoolParams(pool.slots, pool.bricks, pool.occupancy, br.BOUNDS, degree, **kw), pool, "pool"))
    for make, layout, noun in makers:
        shape = layout.shape
        text = f"a degree-{degree} {noun} of {shape} points has fp32 rgbs [.., 4] (degree 0) or coef [.., 3, nb] and sigma [..]"
        good = dict(rgbs=torch.zeros(shape + (4,))) if degree == 0 else dict(coef=torch.zeros(shape + (3, nb)), sigma=torch.zeros(shape))
        bad = [{}, {k: v.double() for k, v in good.items()}, {k: v[1:] for k, v in good.items()}]
        if degree:
            bad += [dict(good, sigma=None), dict(good, coef=torch.zeros(shape + (3, nb + 1))), dict(rgbs=torch.zeros(shape + (4,)))]
        else:
            bad += [dict(rgbs=torch.zeros(shape + (3,))), dict(coef=torch.zeros(shape + (3, 4)), sigma=torch.zeros(shape))]
        for kw in bad:
            with pytest.raises(ValueError) as e:
                make(**kw)
            assert str(e.value) == text
        with pytest.raises(RuntimeError):
            make(**good)
