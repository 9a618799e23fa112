"""Host side of the occupancy grid (csrc/occupancy.hip, upnerf_amd/occupancy.py): refusals
before any launch, the wrappers' guards -- and the fp64 reference of the GPU test (tests/occupancy_ref.py) checked against
itself on cases one can do by hand, with the grazing share of that test's random inputs.  No GPU."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import occupancy_ref as ref
from upnerf_amd import _lib
from upnerf_amd import occupancy as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
ONE = ctypes.c_void_p(16)  # non-null, never dereferenced: every case below is refused on the host


def test_sizing_calls():
    L = _lib.lib
    assert L.upnerf_occ_words(12, 10, 9) == (1080 + 31) // 32 + 1  # 2 x 2 x 2 bricks: one word
    assert L.upnerf_occ_words(256, 256, 256) == 2 ** 24 // 32 + 2 ** 15 // 32
    assert L.upnerf_occ_words(69, 8, 8) == 138 + 1
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (2048, 2048, 2048)):
        assert L.upnerf_occ_words(*bad) == EINVAL and L.upnerf_occ_build_scratch(*bad) == EINVAL, bad
    assert L.upnerf_occ_build_scratch(12, 10, 9) >= 2 * 1080
    assert L.upnerf_occ_compact_scratch(0) == EINVAL and L.upnerf_occ_compact_scratch(1000) >= 4000


def build_args(**kw):
    a = _lib.OccBuildArgs(Cx=4, Cy=4, Cz=4, dilate=1, level=0.5, grid=ONE, cells=None, words=ONE, scratch=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def spans_args(**kw):
    a = _lib.OccSpansArgs(Cx=4, Cy=4, Cz=4, R=8, lo=(ctypes.c_float * 3)(0, 0, 0), hi=(ctypes.c_float * 3)(1, 1, 1), words=ONE,
                          rays=ONE, t0=ONE, t1=ONE, hit=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def compact_args(**kw):
    a = _lib.OccCompactArgs(R=8, n_tables=1, hit=ONE, t0=ONE, t1=ONE, rays=ONE, rays_c=ONE, index=ONE, count=ONE, scratch=ONE)
    a.tables[0] = _lib.PathTable(table=ONE, dim=16, n_rows=8, out=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def scatter_args(**kw):
    a = _lib.OccScatterArgs(R=8, n_hit=3, background=1.0, index=ONE, rays=ONE, rgb_c=ONE, depth_c=ONE, rgb=ONE, depth=ONE)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


REFUSALS = [
    ("upnerf_occ_build", build_args, [dict(Cx=0), dict(Cy=0), dict(Cz=0), dict(dilate=-1), dict(grid=None), dict(cells=ONE),
                                      dict(words=None), dict(scratch=None), dict(level=float("nan"))]),
    ("upnerf_occ_spans", spans_args, [dict(R=0), dict(R=-3), dict(Cx=0), dict(Cz=0), dict(words=None), dict(rays=None), dict(t0=None),
                                      dict(t1=None), dict(hit=None), dict(hi=(ctypes.c_float * 3)(1, 0, 1)),
                                      dict(lo=(ctypes.c_float * 3)(float("nan"), 0, 0))]),
    ("upnerf_occ_compact", compact_args, [dict(R=0), dict(n_tables=_lib.PATH_MAX_TABLES + 1), dict(n_tables=-1), dict(hit=None),
                                          dict(t0=None), dict(t1=None), dict(rays=None), dict(rays_c=None), dict(index=None),
                                          dict(count=None), dict(scratch=None), dict(scratch=ctypes.c_void_p(20))]),
    ("upnerf_occ_scatter", scatter_args, [dict(R=0), dict(n_hit=-1), dict(n_hit=9), dict(rgb=None), dict(index=None),
                                          dict(rgb_c=None), dict(depth_c=None), dict(rays=None)]),
]


@pytest.mark.parametrize("name,make,case", [(n, m, c) for n, m, cases in REFUSALS for c in cases])
def test_argument_errors_are_refused_before_launch(name, make, case):
    fn = getattr(_lib.lib, name)
    assert fn(ctypes.byref(make(**case)), None) == EINVAL  # (a None stream: nothing may be launched)
    assert fn(None, None) == EINVAL


def test_a_table_the_kernel_cannot_copy_is_refused():
    for dim in (0, _lib.PATH_MAX_DIM + 1):
        a = compact_args()
        a.tables[0].dim = dim
        assert _lib.lib.upnerf_occ_compact(ctypes.byref(a), None) == EINVAL
    a = compact_args()
    a.tables[0].out = None
    assert _lib.lib.upnerf_occ_compact(ctypes.byref(a), None) == EINVAL


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    b = ref.BOUNDS
    with pytest.raises(RuntimeError, match="device memory only"):
        oc.OccupancyGrid.from_density(torch.zeros(3, 3, 3), b, 0.5)
    with pytest.raises(RuntimeError, match="device memory only"):
        oc.OccupancyGrid.from_cells(torch.zeros(3, 3, 3, dtype=torch.bool), b)
    occ = object()  # (never reached)
    rays = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="device memory only"):
        oc.ray_spans(occ, rays)
    with pytest.raises(RuntimeError, match="device memory only"):
        oc.compact_rays(occ, rays)
    with pytest.raises(RuntimeError, match="device memory only"):
        oc.compact_hits(rays, torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="device memory only"):
        oc.scatter_results(torch.zeros(0, dtype=torch.int32), rays, None)
    # `level` has no default, as in extract_surface
    for fn in (oc.OccupancyGrid.from_density, oc.OccupancyGrid.build):
        assert inspect.signature(fn).parameters["level"].default is inspect.Parameter.empty
    with pytest.raises(ValueError):
        oc._bounds(((0, 0, 0), (1, 0, 1)))
    with pytest.raises(ValueError):
        oc._bounds(((0, 0), (1, 1)))


def test_render_path_and_the_tools_know_the_grid():
    import importlib.util
    from upnerf_amd import novel_view
    p = inspect.signature(novel_view.render_path).parameters["occupancy"]
    assert p.default is None and isinstance(novel_view.LAST_STATS, dict)
    spec = importlib.util.spec_from_file_location("render_path_tool", os.path.join(ROOT, "tools", "render_path.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--config", "c.yaml", "--ckpt", "x.ckpt", "--images", "0", "1", "--frames", "4", "--out", "o"]
    a = tool.parser().parse_args(base)
    assert a.occupancy is None
    a = tool.parser().parse_args(base + ["--occupancy", "64", "48", "32", "--level", "7.5"])
    assert a.occupancy == [64, 48, 32] and a.level == 7.5 and a.dilate == 1 and a.bounds is None
    with pytest.raises(SystemExit):  # a grid needs its level: there is no default
        tool.check_args(tool.parser().parse_args(base + ["--occupancy", "64", "48", "32"]))


# ---- the reference against itself ---------------------------------------------------------------------------------------------

UNIT = ((0.0, 0.0, 0.0), (4.0, 4.0, 4.0))  # 4 x 4 x 4 cells of edge 1


def one_cell(x=1, y=2, z=3):
    c = np.zeros((4, 4, 4), bool)
    c[z, y, x] = True
    return c


def ray(o, d, near=0.0, far=100.0):
    return np.array([list(o) + list(d) + [near, far]], np.float64)


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_reference_single_cell_hit_centrally_along_each_axis(axis, sign):
    cells = one_cell()  # the box [1, 2] x [2, 3] x [3, 4]
    centre = np.array([1.5, 2.5, 3.5])
    d = np.zeros(3)
    d[axis] = sign
    o = centre - 10.0 * d  # 10 from the centre: the faces are at 9.5 and 10.5
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray(o, d))
    assert hit[0] and t0[0] == 9.5 and t1[0] == 10.5
    # t is in units of d
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray(o, 2 * d))
    assert hit[0] and t0[0] == 4.75 and t1[0] == 5.25
    # beside the cell by one cell on another axis: a miss, whatever the zero components are
    o2 = o.copy()
    o2[(axis + 1) % 3] += 1.0
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray(o2, d))
    assert not hit[0] and t0[0] == t1[0] == 100.0
    assert not ref.grazing(cells, UNIT, ray(o, d))[0]


def test_reference_inside_away_and_clipped():
    cells = one_cell()
    centre = [1.5, 2.5, 3.5]
    # starting inside the cell: t0 = near
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray(centre, (1, 0, 0), near=0.125))
    assert hit[0] and t0[0] == 0.125 and t1[0] == 0.5
    # pointing away from it
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray((3.5, 2.5, 3.5), (1, 0, 0)))
    assert not hit[0]
    # the cell lies behind far, or before near: the clipped span is empty
    assert not ref.spans_ref(cells, UNIT, ray((-5.0, 2.5, 3.5), (1, 0, 0), near=0.0, far=6.0))[2][0]
    assert not ref.spans_ref(cells, UNIT, ray((-5.0, 2.5, 3.5), (1, 0, 0), near=7.0, far=9.0))[2][0]
    # far inside the cell: t1 = far
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray((-5.0, 2.5, 3.5), (1, 0, 0), near=0.0, far=6.25))
    assert hit[0] and t0[0] == 6.0 and t1[0] == 6.25
    # two cells: first entry, last exit, the gap between them included
    cells[3, 2, 3] = True
    t0, t1, hit = ref.spans_ref(cells, UNIT, ray((-5.0, 2.5, 3.5), (1, 0, 0)))
    assert hit[0] and t0[0] == 6.0 and t1[0] == 9.0
    # a diagonal ray through the cell's centre: entry and exit half a cell diagonal from it
    d = np.ones(3) / np.sqrt(3.0)
    t0, t1, hit = ref.spans_ref(one_cell(), UNIT, ray(np.array(centre) - 5 * d, d))
    assert hit[0] and abs(t0[0] - (5 - np.sqrt(0.75))) < 1e-12 and abs(t1[0] - (5 + np.sqrt(0.75))) < 1e-12
    # a ray along a face of the cell is grazing; an empty grid has no hits
    assert ref.grazing(one_cell(), UNIT, ray((-5.0, 2.0, 3.5), (1, 0, 0)))[0]
    assert not ref.spans_ref(np.zeros((4, 4, 4), bool), UNIT, ray(centre, (1, 0, 0)))[2][0]


@pytest.mark.parametrize("dims,share,seed", ref.SPAN_CASES)
def test_random_inputs_of_the_gpu_test_are_rarely_grazing_and_have_both_classes(dims, share, seed):
    cells, rays = ref.random_cells(dims, share, seed), ref.random_rays(ref.BOUNDS, seed)
    assert rays.shape == (ref.N_RAYS, 8) and np.abs(rays[:, 3:6]).min() >= 0.05
    assert np.abs(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1) - 1).max() < 1e-6
    lo, hi = ref.bounds64(ref.BOUNDS)
    inside = ((rays[:, :3] >= lo) & (rays[:, :3] <= hi)).all(1)
    assert inside[ref.N_RAYS // 2:].all() and not inside[:ref.N_RAYS // 2].any()
    g = ref.grazing(cells, ref.BOUNDS, rays)
    hit = ref.spans_ref(cells, ref.BOUNDS, rays)[2]
    print(f"{dims} at {share}: grazing {g.mean():.4f}, hits {hit[~g].mean():.3f}")
    assert g.mean() <= 0.03
    assert 0.15 <= hit[~g].mean() <= 0.85
