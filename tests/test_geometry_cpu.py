"""Host side of the mesh extraction (upnerf_amd/geometry.py): the tables the kernels are handed, PLY files, camera bounds and
the `level` argument.  No GPU."""
import importlib.util
import inspect
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def corner(c):
    return np.array([c & 1, (c >> 1) & 1, c >> 2])


def test_the_six_tetrahedra_have_volume_one_sixth_and_tile_the_cube():
    from upnerf_amd.geometry import TETS
    assert len(TETS) == 6 and len(set(tuple(sorted(t)) for t in TETS)) == 6
    for t in TETS:
        v = [corner(c) for c in t]
        det = int(round(np.linalg.det(np.stack([v[1] - v[0], v[2] - v[0], v[3] - v[0]]).astype(float))))
        assert Fraction(det, 6) == Fraction(1, 6), (t, det)  # signed: all six are positively oriented
    # every point of a lattice that no face passes through lies strictly inside exactly one tetrahedron
    n = 7
    pts = (np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.array([0.31, 0.47, 0.13])) / n
    hits = np.zeros(len(pts), int)
    for t in TETS:
        v = np.stack([corner(c) for c in t]).astype(float)
        bary = np.linalg.solve(np.concatenate([v.T, np.ones((1, 4))]), np.concatenate([pts.T, np.ones((1, len(pts)))]))
        assert np.abs(bary).min() > 1e-9
        hits += (bary > 0).all(0)
    assert (hits == 1).all()


def cell_edges(TETS, TET_EDGES):
    return sorted({tuple(sorted((t[i], t[j]))) for t in TETS for i, j in TET_EDGES})


def test_face_diagonals_agree_with_the_neighbouring_cells():
    """The diagonal the split draws on the face x = 1 (y = 1, z = 1) of a cell is the one its neighbour draws on its face x = 0."""
    from upnerf_amd.geometry import TETS, TET_EDGES
    edges = cell_edges(TETS, TET_EDGES)
    for axis in range(3):
        bit = 1 << axis
        on = lambda side: {(a, b) for a, b in edges if bin(a ^ b).count("1") == 2 and (a ^ b) & bit == 0 and bool(a & bit) == side}
        near, far = on(False), on(True)
        assert len(near) == len(far) == 1
        assert {(a | bit, b | bit) for a, b in near} == far


def test_every_cell_edge_has_one_owner_and_slot():
    from upnerf_amd.geometry import EDGES, TETS, TET_EDGES, edge_owner
    edges = cell_edges(TETS, TET_EDGES)
    assert len(edges) == 19 and len(EDGES) == 7 and len(set(EDGES)) == 7
    seen = {}
    for a, b in edges:
        own, slot = edge_owner(a, b)
        assert edge_owner(b, a) == (own, slot)
        ends = {tuple(own), tuple(np.array(own) + np.array(EDGES[slot]))}
        assert ends == {tuple(corner(a)), tuple(corner(b))}  # the owner's slot IS this edge
        assert (own, slot) not in seen, (a, b, seen.get((own, slot)))
        seen[(own, slot)] = (a, b)
    assert len(seen) == 19
    with pytest.raises(ValueError):
        edge_owner(1, 2)  # the other diagonal of the z = 0 face is not an edge of the split
    with pytest.raises(ValueError):
        edge_owner(3, 3)


def test_triangle_table_joins_differently_classified_corners_and_faces_outwards():
    from upnerf_amd.geometry import TET_EDGES, TRI_TABLE
    assert len(TRI_TABLE) == 16 and len(TET_EDGES) == 6 and len(set(map(frozenset, TET_EDGES))) == 6
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)  # a positively oriented tetrahedron
    for case, tris in enumerate(TRI_TABLE):
        ins = [(case >> i) & 1 for i in range(4)]
        crossed = {e for e, (i, j) in enumerate(TET_EDGES) if ins[i] != ins[j]}
        assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(ins)]
        used = set()
        for tri in tris:
            assert len(set(tri)) == 3
            for e in tri:
                i, j = TET_EDGES[e]
                assert ins[i] != ins[j], (case, tri)
            used |= set(tri)
            mid = [(X[TET_EDGES[e][0]] + X[TET_EDGES[e][1]]) / 2 for e in tri]
            normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
            out = X[[i for i in range(4) if not ins[i]]].mean(0) - X[[i for i in range(4) if ins[i]]].mean(0)
            assert normal @ out > 0, (case, tri)  # towards the outside vertices: lower density
        assert used == crossed
        if len(tris) == 2:  # the two triangles share one diagonal of the quad, in opposite directions
            d = lambda t: {(t[k], t[(k + 1) % 3]) for k in range(3)}
            assert len({(b, a) for a, b in d(tris[0])} & d(tris[1])) == 1


def small_mesh():
    from upnerf_amd.geometry import Mesh
    g = torch.Generator().manual_seed(1)
    v = torch.randn(5, 3, generator=g)
    n = torch.nn.functional.normalize(torch.randn(5, 3, generator=g), dim=1)
    f = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 0, 1]], dtype=torch.int32)
    c = torch.tensor([[0.0, 0.5, 1.0], [1.5, -0.2, 0.25], [0.999, 0.001, 0.5], [float("nan"), 0.1, 0.2], [1.0, 1.0, 0.0]])
    return Mesh(v, n, f, c)


def test_ply_header_is_exact_and_the_file_round_trips(tmp_path):
    from upnerf_amd.geometry import Mesh, read_ply
    m = small_mesh()
    p = str(tmp_path / "m.ply")
    m.write_ply(p)
    raw = open(p, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
              "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nelement face 3\nproperty list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header.encode("ascii"))
    assert len(raw) == len(header) + 5 * 27 + 3 * 13
    back = read_ply(p)
    assert torch.equal(back.vertices, m.vertices) and torch.equal(back.normals, m.normals) and torch.equal(back.faces, m.faces)
    assert back.faces.dtype == torch.int32 and back.colours.dtype == torch.uint8
    assert back.colours.tolist() == [[0, 127, 255], [255, 0, 63], [254, 0, 127], [0, 25, 51], [255, 255, 0]]
    # written again from what was read: the same bytes (uint8 colours are taken as they are)
    q = str(tmp_path / "again.ply")
    back.write_ply(q)
    assert open(q, "rb").read() == raw
    # no colours: grey
    Mesh(m.vertices, m.normals, m.faces).write_ply(q)
    assert read_ply(q).colours.unique().tolist() == [128]
    with pytest.raises(ValueError):
        open(q, "wb").write(raw.replace(b"property float nx\n", b""))
        read_ply(q)
    with pytest.raises(ValueError):
        open(q, "wb").write(raw[:-1])
        read_ply(q)


def test_empty_meshes_round_trip(tmp_path):
    from upnerf_amd.geometry import Mesh, read_ply
    p = str(tmp_path / "empty.ply")
    Mesh(torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)).write_ply(p)
    assert open(p, "rb").read().endswith(b"end_header\n")
    back = read_ply(p)
    assert tuple(back.vertices.shape) == (0, 3) and tuple(back.faces.shape) == (0, 3) and tuple(back.colours.shape) == (0, 3)
    # vertices without faces
    Mesh(torch.ones(2, 3), torch.zeros(2, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(2, 3)).write_ply(p)
    back = read_ply(p)
    assert tuple(back.vertices.shape) == (2, 3) and tuple(back.faces.shape) == (0, 3)


class _Sys:
    def __init__(self, fars=None):
        self.hparams = {"nerf.far": 2.0}
        self.train_dataset = type("D", (), {})()
        if fars is not None:
            self.train_dataset.fars = fars


def test_bounds_from_cameras_on_a_hand_made_pose_set():
    from upnerf_amd.geometry import bounds_from_cameras
    eye = [[1.0, 0, 0], [0, 1, 0], [0, 0, 1]]
    # camera 0 at (1, 2, 3) with the identity rotation looks down -z; camera 1 at (-1, 0, 0) turned so that it looks down +x
    # (its z axis is -x: R[:, 2] = (-1, 0, 0))
    turn = [[0.0, 0, -1], [0, 1, 0], [1, 0, 0]]
    poses = torch.tensor([[r + [t] for r, t in zip(eye, (1.0, 2.0, 3.0))], [r + [t] for r, t in zip(turn, (-1.0, 0.0, 0.0))]])
    lo, hi = bounds_from_cameras(_Sys(), 0.5, poses=poses)  # far = 2 from the hyper-parameters
    # points: (1, 2, 3), (-1, 0, 0), (1, 2, 1), (1, 0, 0)
    assert lo == (-1.5, -0.5, -0.5) and hi == (1.5, 2.5, 3.5)
    lo, hi = bounds_from_cameras(_Sys(fars=[1.0, 4.0]), 0.0, poses=poses)  # per-image far planes of the dataset
    # points: (1, 2, 3), (-1, 0, 0), (1, 2, 2), (3, 0, 0)
    assert lo == (-1.0, 0.0, 0.0) and hi == (3.0, 2.0, 3.0)
    with pytest.raises(ValueError):
        bounds_from_cameras(_Sys(), 0.0, poses=poses * float("nan"))


def test_level_is_required_and_cpu_tensors_are_refused(tmp_path):
    from upnerf_amd import geometry
    p = inspect.signature(geometry.extract_surface).parameters["level"]
    assert p.default is inspect.Parameter.empty
    with pytest.raises(TypeError):
        geometry.extract_surface(torch.zeros(2, 2, 2), ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(RuntimeError):
        geometry.extract_surface(torch.zeros(2, 2, 2), ((0, 0, 0), (1, 1, 1)), 0.5)  # no CPU path
    spec = importlib.util.spec_from_file_location("extract_mesh_tool", os.path.join(ROOT, "tools", "extract_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    base = ["--ckpt", "x.ckpt", "--out", str(tmp_path / "o.ply"), "--bounds", "0", "0", "0", "1", "1", "1"]
    with pytest.raises(SystemExit):
        tool.parser().parse_args(base)
    a = tool.parser().parse_args(base + ["--level", "7.5"])
    assert a.level == 7.5 and a.resolution == [256] and a.from_cameras is None
    with pytest.raises(SystemExit):  # one box, not two
        tool.parser().parse_args(base + ["--level", "1", "--from-cameras", "0.5"])


def test_sizing_call_refuses_what_does_not_fit_int32_without_a_gpu():
    from upnerf_amd import _lib
    assert _lib.lib.upnerf_mtet_scratch(1024, 1024, 512) == -1  # 7 x 2^29 edges
    assert _lib.lib.upnerf_mtet_scratch(1, 8, 8) == -1 and _lib.lib.upnerf_mtet_scratch(8, 8, 0) == -1
    n = 9 * 8 * 7
    assert _lib.lib.upnerf_mtet_scratch(9, 8, 7) >= 10 * n
    assert _lib.lib.upnerf_mtet_scratch(512, 512, 512) > 0
    # the tables are checked on the host as well: a tetrahedron with an edge that is not of the split is refused
    import ctypes
    from upnerf_amd import geometry
    one = ctypes.c_void_p(16)
    tab = geometry._tables()
    a = _lib.MtetArgs(Nx=4, Ny=4, Nz=4, level=0.5, grid=one, tab=tab)
    tab.tets[0][1] = 2  # (0, 2, 3, 7) is fine; now break it: corners 1 and 2 in one tetrahedron
    tab.tets[0][2] = 1
    a.tab = tab
    assert _lib.lib.upnerf_mtet_count(ctypes.byref(a), one, one, None) == -1
    assert _lib.lib.upnerf_mtet_count(None, one, one, None) == -1
