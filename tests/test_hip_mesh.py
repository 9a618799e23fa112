"""Marching tetrahedra on the GPU (csrc/mesh.hip, upnerf_amd.geometry.extract_surface) against a fp64 numpy restatement that
derives its own tables (nothing is imported from the module under test but the function).

Gates.  Topology: both sides classify the SAME fp32 samples with the same comparison (finite and >= level), so the vertex count
and the faces are equal, `torch.equal`.  Positions: the kernel forms t = (level - v0) / (v1 - v0) in fp32 -- two subtractions of
exact inputs and a division, three roundings of 2^-24 = 6e-8 relative -- then p0 + t (p1 - p0), one multiplication and one
addition more: five roundings at most, 3e-7 of (the largest coordinate + the longest cell edge); the gate is 1e-6 of that, about
3x the bound.  (The kernel spends fewer: it forms the grid coordinates and the last two operations in fp64 and rounds once.)
Normals: both sides difference the same fp32 samples; the kernel's fp32 differences, interpolation and normalisation are a
dozen roundings on components of a unit vector, and the fields below keep every interpolated gradient well away from zero
(asserted), so 1e-4 absolute per component is the issue's gate with two orders of margin.  Volumes: sums of ~1e3 products of
fp32-rounded positions, 1e-5 relative."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# ---- fp64 restatement, with tables of its own -------------------------------------------------------------------------------

SLOTS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]  # edge slot -> offset of the far end
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]                               # tet edge -> its two tet vertices


def kuhn_tets():
    """One tetrahedron per order of the axes, corner 0 to corner 7; odd orders swap two vertices: all positively oriented."""
    tets = []
    for p in itertools.permutations((0, 1, 2)):
        a, b = 1 << p[0], (1 << p[0]) | (1 << p[1])
        odd = sum(p[i] > p[j] for i in range(3) for j in range(i + 1, 3)) % 2
        tets.append((0, b, a, 7) if odd else (0, a, b, 7))
    return tets


def tri_cases():
    """case -> triangles (tet edges), wound so that the normal points from the inside to the outside vertices of the positively
    oriented reference tetrahedron.  One odd vertex: its edges ascending; two and two: the quad (ac, ad, bd, bc) cut along ac-bd."""
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], float)
    eid = lambda a, b: PAIRS.index((min(a, b), max(a, b)))
    mid = lambda e: (X[PAIRS[e][0]] + X[PAIRS[e][1]]) / 2
    table = []
    for case in range(16):
        ins = [i for i in range(4) if (case >> i) & 1]
        out = [i for i in range(4) if not (case >> i) & 1]
        tris = []
        if len(ins) in (1, 3):
            a = (ins if len(ins) == 1 else out)[0]
            tris = [tuple(sorted(eid(a, b) for b in range(4) if b != a))]
        elif len(ins) == 2:
            (a, b), (c, d) = ins, out
            q = [eid(a, c), eid(a, d), eid(b, d), eid(b, c)]
            tris = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
        fixed = []
        for t in tris:
            n = np.cross(mid(t[1]) - mid(t[0]), mid(t[2]) - mid(t[0]))
            fixed.append(t if n @ (X[out].mean(0) - X[ins].mean(0)) > 0 else (t[0], t[2], t[1]))
        table.append(fixed)
    return table


def axis_coords(lo, hi, n):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + np.arange(n, dtype=np.float64) * ((hi - lo) / (n - 1))


def gradient(G, bounds):
    """fp64 central differences of the fp32 samples over the spacing, one-sided at the border: [Nz, Ny, Nx, 3] (x, y, z)."""
    g = np.zeros(G.shape + (3,))
    V = G.astype(np.float64)
    for k, ax in enumerate((2, 1, 0)):
        n = G.shape[ax]
        h = (float(np.float32(bounds[1][k])) - float(np.float32(bounds[0][k]))) / (n - 1)
        Vm = np.moveaxis(V, ax, 0)
        d = np.empty_like(Vm)
        d[1:-1] = (Vm[2:] - Vm[:-2]) / (2 * h)
        d[0] = (Vm[1] - Vm[0]) / h
        d[-1] = (Vm[-1] - Vm[-2]) / h
        g[..., k] = np.moveaxis(d, 0, ax)
    return g


def mtet_ref(G, bounds, level):
    """(vertices [V, 3], raw normals -grad [V, 3] (not normalised), faces [F, 3]) in fp64 / int64, in the module's stated order:
    vertices by (grid point, edge slot), faces by (cell, tetrahedron, triangle)."""
    G = np.asarray(G, np.float32)
    Nz, Ny, Nx = G.shape
    level = np.float32(level)
    with np.errstate(invalid="ignore"):
        ins = np.isfinite(G) & (G >= level)
    V64 = G.astype(np.float64)
    N = G.size
    flag = np.zeros((Nz, Ny, Nx, 7), bool)
    for s, (dx, dy, dz) in enumerate(SLOTS):
        a = ins[:Nz - dz, :Ny - dy, :Nx - dx]
        b = ins[dz:, dy:, dx:]
        flag[:Nz - dz, :Ny - dy, :Nx - dx, s] = a != b
    flat = flag.reshape(-1)
    vid = np.cumsum(flat) - 1  # vertex index of (point, slot) where flagged
    where = np.nonzero(flat)[0]
    pt, slot = where // 7, where % 7
    z0, y0, x0 = pt // (Nx * Ny), (pt // Nx) % Ny, pt % Nx
    off = np.array(SLOTS)[slot]
    x1, y1, z1 = x0 + off[:, 0], y0 + off[:, 1], z0 + off[:, 2]
    v0, v1 = V64[z0, y0, x0], V64[z1, y1, x1]
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(np.isfinite(v0) & np.isfinite(v1), (float(level) - v0) / (v1 - v0), 0.5)
    cx, cy, cz = (axis_coords(bounds[0][k], bounds[1][k], n) for k, n in enumerate((Nx, Ny, Nz)))
    p0 = np.stack([cx[x0], cy[y0], cz[z0]], 1)
    p1 = np.stack([cx[x1], cy[y1], cz[z1]], 1)
    verts = p0 + t[:, None] * (p1 - p0)
    with np.errstate(invalid="ignore"):
        g = gradient(G, bounds)
        g0, g1 = g[z0, y0, x0], g[z1, y1, x1]
        normals = -(g0 + t[:, None] * (g1 - g0))
    # faces
    tets, cases = kuhn_tets(), tri_cases()
    cz_, cy_, cx_ = np.meshgrid(np.arange(Nz - 1), np.arange(Ny - 1), np.arange(Nx - 1), indexing="ij")
    corner_in = np.stack([ins[(c >> 2):Nz - 1 + (c >> 2), ((c >> 1) & 1):Ny - 1 + ((c >> 1) & 1), (c & 1):Nx - 1 + (c & 1)]
                          for c in range(8)], -1).reshape(-1, 8)
    mixed = np.nonzero(corner_in.any(1) & ~corner_in.all(1))[0]
    ox, oy, oz = cx_.reshape(-1)[mixed], cy_.reshape(-1)[mixed], cz_.reshape(-1)[mixed]
    cin = corner_in[mixed]
    cell_lin = (oz * Ny + oy) * Nx + ox  # the cell's origin as a grid point: the same order as its own linear index
    recs = []
    for ti, tet in enumerate(tets):
        case = sum(cin[:, tet[i]].astype(int) << i for i in range(4))
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if not len(sel):
                continue
            for k, tri in enumerate(cases[cs]):
                idx = []
                for e in tri:
                    ca, cb = tet[PAIRS[e][0]], tet[PAIRS[e][1]]
                    lo_c, d = ca & cb, ca ^ cb
                    assert lo_c in (ca, cb)
                    s = SLOTS.index((d & 1, (d >> 1) & 1, d >> 2))
                    own = ((oz[sel] + (lo_c >> 2)) * Ny + oy[sel] + ((lo_c >> 1) & 1)) * Nx + ox[sel] + (lo_c & 1)
                    assert flat[own * 7 + s].all()
                    idx.append(vid[own * 7 + s])
                recs.append(np.stack([cell_lin[sel], np.full(len(sel), ti), np.full(len(sel), k)] + idx, 1))
    if recs:
        recs = np.concatenate(recs)
        recs = recs[np.lexsort((recs[:, 2], recs[:, 1], recs[:, 0]))]
        faces = recs[:, 3:]
    else:
        faces = np.zeros((0, 3), np.int64)
    return verts, normals, faces


# ---- grids: 9 x 8 x 7 points, another spacing on every axis -----------------------------------------------------------------

RES = (9, 8, 7)                                   # Nx, Ny, Nz
BOUNDS = ((-1.0, -0.8, -0.9), (1.0, 0.88, 0.72))  # spacing 0.25, 0.24, 0.27


def points(res=RES, bounds=BOUNDS):
    cx, cy, cz = (axis_coords(bounds[0][k], bounds[1][k], n) for k, n in enumerate(res))
    Z, Y, X = np.meshgrid(cz, cy, cx, indexing="ij")
    return X, Y, Z


def sphere(c=(0.02, 0.05, -0.08)):
    X, Y, Z = points()
    return (-np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(np.float32)


SPHERE_LEVEL = -0.55
TORUS_R, TORUS_LEVEL = 0.56, -0.0530  # level = -r^2 of the tube, r = 0.23


def torus():
    X, Y, Z = points()
    return (-((np.sqrt((X - 0.01) ** 2 + (Y - 0.03) ** 2) - TORUS_R) ** 2 + (Z + 0.09) ** 2)).astype(np.float32)


def two_spheres():
    X, Y, Z = points()
    a = 0.30 - np.sqrt((X + 0.5) ** 2 + (Y + 0.3) ** 2 + (Z + 0.4) ** 2)
    b = 0.32 - np.sqrt((X - 0.45) ** 2 + (Y - 0.35) ** 2 + (Z - 0.2) ** 2)
    return np.maximum(a, b).astype(np.float32)


def with_nonfinite():
    G = sphere().copy()
    ins = G >= np.float32(SPHERE_LEVEL)
    # one inside sample with an outside +x neighbour becomes NaN, one outside sample with an inside -y neighbour becomes +inf
    z, y, x = [int(v[0]) for v in np.nonzero(ins[:, :, :-1] & ~ins[:, :, 1:])]
    G[z, y, x] = np.nan
    z2, y2, x2 = [int(v[-1]) for v in np.nonzero(ins[:, :-1, :] & ~ins[:, 1:, :])]
    assert (z2, y2 + 1, x2) != (z, y, x)
    G[z2, y2 + 1, x2] = np.inf
    return G


def plane(sign):
    X, _, _ = points()
    return (sign * X).astype(np.float32)


PLANE_LEVEL = float(np.float32(axis_coords(BOUNDS[0][0], BOUNDS[1][0], RES[0])[4]))  # a grid coordinate (0.0 is one)

CASES = {
    "sphere": (sphere, SPHERE_LEVEL),
    "torus": (torus, TORUS_LEVEL),
    "two_spheres": (two_spheres, 0.0),
    "empty": (sphere, 1.0),           # nothing reaches the level
    "all_inside": (sphere, -10.0),    # everything does
    "plane_t1": (lambda: plane(1.0), PLANE_LEVEL),    # v = x: the inside end of a crossed edge IS the level, t = 1
    "plane_t0": (lambda: plane(-1.0), -PLANE_LEVEL),  # v = -x: the owner of a crossed edge is, t = 0
    "nonfinite": (with_nonfinite, SPHERE_LEVEL),
}
_REF = {}


def reference(name):
    if name not in _REF:
        make, level = CASES[name]
        G = make()
        _REF[name] = (G, level) + mtet_ref(G, BOUNDS, level)
    return _REF[name]


def run(G, bounds, level):
    from upnerf_amd.geometry import extract_surface
    return extract_surface(torch.from_numpy(np.ascontiguousarray(G)).cuda(), bounds, level)


def position_gate(bounds, res):
    edge = np.sqrt(sum(((h - l) / (n - 1)) ** 2 for l, h, n in zip(bounds[0], bounds[1], res)))
    return 1e-6 * (max(abs(v) for b in bounds for v in b) + edge)


def check_against(mesh, verts, faces, bounds, res, tag):
    assert mesh.vertices.dtype == torch.float32 and mesh.normals.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert tuple(mesh.vertices.shape) == (len(verts), 3) == tuple(mesh.normals.shape), (tag, mesh.vertices.shape, len(verts))
    assert tuple(mesh.faces.shape) == (len(faces), 3), (tag, mesh.faces.shape, len(faces))
    assert torch.equal(mesh.faces.cpu(), torch.from_numpy(faces.astype(np.int32))), tag
    if len(verts):
        err = np.abs(mesh.vertices.cpu().numpy().astype(np.float64) - verts).max()
        gate = position_gate(bounds, res)
        print(f"{tag}: V {len(verts)} F {len(faces)} max position error {err:.2e} (gate {gate:.2e})")
        assert err <= gate, (tag, err, gate)


@pytest.mark.parametrize("name", list(CASES))
def test_mesh_equals_the_restatement(name):
    G, level, verts, _, faces = reference(name)
    mesh = run(G, BOUNDS, level)
    check_against(mesh, verts, faces, BOUNDS, RES, name)
    if name in ("empty", "all_inside"):
        assert len(verts) == 0 and len(faces) == 0
    else:
        assert len(faces) > 0
        used = torch.unique(mesh.faces.long())
        assert int(used.min()) == 0 and int(used.max()) == len(verts) - 1 and len(used) == len(verts)  # welded: no spare vertex
        n = mesh.normals
        lens = n.norm(dim=1)
        assert bool(((lens - 1).abs() < 1e-5).logical_or(lens == 0).all())
    if name == "two_spheres":  # two components: faces of one never index vertices of the other
        f = faces
        parent = np.arange(len(verts))
        for _ in range(64):
            m = np.minimum.reduce([parent[f[:, 0]], parent[f[:, 1]], parent[f[:, 2]]])
            for k in range(3):
                np.minimum.at(parent, f[:, k], m)
        assert len(np.unique(parent)) == 2
    if name == "plane_t1":
        assert np.allclose(verts[:, 0], PLANE_LEVEL, atol=0) and bool((mesh.vertices[:, 0] == PLANE_LEVEL).all())
    if name == "plane_t0":
        assert bool((mesh.vertices[:, 0] == PLANE_LEVEL).all())
        assert bool((mesh.normals.cpu() == torch.tensor([1.0, 0.0, 0.0])).all())  # -grad(-x)
    if name == "nonfinite":
        assert torch.isfinite(mesh.vertices).all() and torch.isfinite(mesh.normals).all()
        assert (len(verts), len(faces)) != (len(reference("sphere")[2]), len(reference("sphere")[4]))


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_match_on_every_vertex(name):
    G, level, verts, raw, faces = reference(name)
    lens = np.linalg.norm(raw, axis=1)
    assert lens.min() > 0.05 * lens.max(), (lens.min(), lens.max())  # no vertex with a near-zero gradient: none is left out
    mesh = run(G, BOUNDS, level)
    err = np.abs(mesh.normals.cpu().numpy().astype(np.float64) - raw / lens[:, None]).max()
    print(f"{name}: {len(verts)} normals, max component error {err:.2e}, |grad| in [{lens.min():.3f}, {lens.max():.3f}]")
    assert mesh.normals.shape[0] == len(verts) and err <= 1e-4, err


def signed_volume(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_closed_meshes_are_manifold_oriented_and_of_the_right_genus(name, euler):
    G, level, verts, raw, faces = reference(name)
    ins = G >= np.float32(level)
    assert not (ins[0].any() or ins[-1].any() or ins[:, 0].any() or ins[:, -1].any() or ins[:, :, 0].any() or ins[:, :, -1].any())
    mesh = run(G, BOUNDS, level)
    f = mesh.faces.cpu().numpy().astype(np.int64)
    v = mesh.vertices.cpu().numpy().astype(np.float64)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    assert len(np.unique(directed, axis=0)) == len(directed)                       # no directed edge twice
    assert set(map(tuple, directed)) == set(map(tuple, directed[:, ::-1]))         # each met by its opposite
    und = np.unique(np.sort(directed, 1), axis=0, return_counts=True)
    assert (und[1] == 2).all()                                                     # two faces per undirected edge
    V, E, F = len(v), len(und[0]), len(f)
    assert V - E + F == euler, (V, E, F)
    vol, vol_ref = signed_volume(v, f), signed_volume(verts, faces)
    print(f"{name}: V {V} E {E} F {F}; signed volume {vol:.8f} (restatement {vol_ref:.8f})")
    assert vol > 0 and abs(vol - vol_ref) <= 1e-5 * abs(vol_ref)
    if name == "sphere":
        geo = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        n = mesh.normals.cpu().numpy().astype(np.float64)
        dots = np.einsum("ij,ij->i", geo, n[f].mean(1))
        assert (dots > 0).all(), int((dots <= 0).sum())


def test_two_runs_give_the_same_bits():
    G, level = reference("torus")[:2]
    a, b = run(G, BOUNDS, level), run(G, BOUNDS, level)
    assert torch.equal(a.faces, b.faces)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    assert torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))


# ---- the scan: 1024 elements per workgroup, one element per grid point -----------------------------------------------------
# One level up to 1024 points, two up to 1024^2, three beyond; 1048578 = 174763 x 3 x 2 is the smallest number above 1024^2
# that is a product of three factors >= 2.  (41 x 5 x 5 and 9 x 8 x 7 are no multiples of the 256-thread workgroup either.)
SCAN_GRIDS = [(16, 8, 8), (41, 5, 5), (128, 128, 64), (174763, 3, 2)]


def wavy(res):
    """Crossings all along the grid (so every block of the scan contributes), but few enough for a quick restatement."""
    Nx, Ny, Nz = res
    k, j, i = np.meshgrid(np.arange(Nz), np.arange(Ny), np.arange(Nx), indexing="ij")
    period = 7.3 if Nx * Ny * Nz < 4096 else 61.7
    return (np.cos(2 * np.pi * i / period) + 0.35 * np.cos(1.3 * j + 0.4) + 0.3 * np.cos(0.9 * k + 0.2 * j)).astype(np.float32)


@pytest.mark.parametrize("res", SCAN_GRIDS, ids=lambda r: "x".join(map(str, r)))
def test_every_level_of_the_scan(res):
    n = res[0] * res[1] * res[2]
    assert n in (1024, 1025, 1024 ** 2, 1024 ** 2 + 2)
    bounds = ((0.0, -1.0, 0.5), (0.37 * (res[0] - 1), -1.0 + 0.21 * (res[1] - 1), 0.5 + 0.29 * (res[2] - 1)))
    G = wavy(res)
    level = 1.25 if n > 4096 else 0.4
    verts, _, faces = mtet_ref(G, bounds, level)
    assert len(faces) > 0
    # crossings from one end of the longest axis to the other: the blocks of every level of the scan carry an offset
    k = int(np.argmax(res))
    span = bounds[1][k] - bounds[0][k]
    assert verts[:, k].min() < bounds[0][k] + 0.1 * span and verts[:, k].max() > bounds[1][k] - 0.1 * span
    assert len(np.unique(faces)) == len(verts)
    mesh = run(G, bounds, level)
    check_against(mesh, verts, faces, bounds, res, "x".join(map(str, res)))


# ---- capacities ------------------------------------------------------------------------------------------------------------

def test_emit_refuses_a_capacity_one_short_and_writes_nothing():
    from upnerf_amd import _lib, geometry
    G, level, verts, _, faces = reference("sphere")
    V, F = len(verts), len(faces)
    grid = torch.from_numpy(G).cuda()
    Nz, Ny, Nx = G.shape
    nbytes = _lib.lib.upnerf_mtet_scratch(Nx, Ny, Nz)
    assert nbytes > 0
    scratch = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    totals = torch.zeros(2, device="cuda", dtype=torch.int32)
    a = _lib.MtetArgs(Nx=Nx, Ny=Ny, Nz=Nz, level=level, lo=(C.c_float * 3)(*BOUNDS[0]), hi=(C.c_float * 3)(*BOUNDS[1]),
                      grid=grid.data_ptr(), tab=geometry._tables())
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.lib.upnerf_mtet_count(C.byref(a), scratch.data_ptr(), totals.data_ptr(), st) == 0
    assert totals.tolist() == [V, F]
    vb = torch.full((V, 3), -7.0, device="cuda")
    nb = torch.full((V, 3), -7.0, device="cuda")
    fb = torch.full((F, 3), -7, device="cuda", dtype=torch.int32)
    a.n_vertices, a.n_faces = V, F
    a.vertices, a.normals, a.faces = vb.data_ptr(), nb.data_ptr(), fb.data_ptr()
    for cap_v, cap_f in ((V - 1, F), (V, F - 1)):
        a.cap_vertices, a.cap_faces = cap_v, cap_f
        assert _lib.lib.upnerf_mtet_emit(C.byref(a), scratch.data_ptr(), st) == -1
        torch.cuda.synchronize()
        assert bool((vb == -7).all()) and bool((nb == -7).all()) and bool((fb == -7).all())
    a.cap_vertices, a.cap_faces = V, F
    assert _lib.lib.upnerf_mtet_emit(C.byref(a), scratch.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(fb.cpu(), torch.from_numpy(faces.astype(np.int32))) and not bool((vb == -7).any())


def test_sizes_beyond_int32_are_refused_by_the_sizing_call():
    from upnerf_amd import _lib
    from upnerf_amd.geometry import extract_surface
    assert 7 * 12400 * 12400 * 2 > 2 ** 31 - 1 > 12 * 12399 * 12399   # the edges do not fit, the triangles would
    assert _lib.lib.upnerf_mtet_scratch(12400, 12400, 2) == -1   # UPNERF_EINVAL, nothing launched (a host function)
    assert 12 * 600 ** 3 > 2 ** 31 - 1 > 7 * 601 ** 3            # the triangles do not fit, the edges would
    assert _lib.lib.upnerf_mtet_scratch(601, 601, 601) == -1
    assert _lib.lib.upnerf_mtet_scratch(563, 563, 563) > 0       # both fit
    with pytest.raises(RuntimeError):
        extract_surface(torch.zeros(2, 2, 2).cuda()[:1], BOUNDS, 0.5)  # an axis with one point
