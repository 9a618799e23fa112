"""Camera-path novel views on the GPU (csrc/path.hip, upnerf_amd/novel_view.py, the `embed_rows` keyword of render_rays).

Gates.  Poses: the kernel evaluates in fp64 and rounds once, the restatement below is fp64 numpy; rotation entries are at most 1
in magnitude, so one fp32 rounding is 6e-8 and device sin / acos are within a few fp64 ulp of numpy's: 1e-6 absolute.  Rays:
a unit vector out of a handful of fp32 operations at 6e-8 each: 1e-6 absolute, norm within 2e-7 of 1.  Everything else is bit
for bit (`torch.equal`)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = [0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 2.999, 3.0]
H, W, FX, FY, CX, CY = 5, 7, 9.25, 8.5, 3.3, 1.7
ID0, ID1 = 1, 4


# ---- fp64 restatement of upnerf_path_poses ------------------------------------------------------------------------------

def rot_of(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_of(m):
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    d = [m[0, 0], m[1, 1], m[2, 2]]
    if tr >= max(d):
        q = [1 + tr, m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]]
    elif d[0] >= d[1] and d[0] >= d[2]:
        q = [m[2, 1] - m[1, 2], 1 + d[0] - d[1] - d[2], m[0, 1] + m[1, 0], m[0, 2] + m[2, 0]]
    elif d[1] >= d[2]:
        q = [m[0, 2] - m[2, 0], m[0, 1] + m[1, 0], 1 - d[0] + d[1] - d[2], m[1, 2] + m[2, 1]]
    else:
        q = [m[1, 0] - m[0, 1], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], 1 - d[0] - d[1] + d[2]]
    q = np.array(q, dtype=np.float64)
    return q / np.sqrt((q * q).sum())


def pose_ref(key_c2w, key_nf, u, mode):
    """fp64 pose [3, 4] and (near, far) at path parameter u of the fp32 keys."""
    kc, kn = key_c2w.astype(np.float64), key_nf.astype(np.float64)
    K = kc.shape[0]
    u = min(max(float(np.float32(u)), 0.0), K - 1.0)
    k = min(int(np.floor(u)), K - 2)
    s = u - k
    if s == 0.0 or s == 1.0:
        kk = k if s == 0.0 else k + 1
        return kc[kk], kn[kk]
    q0, q1 = quat_of(kc[k, :, :3]), quat_of(kc[k + 1, :, :3])
    dot = float(q0 @ q1)
    if dot < 0:
        q1, dot = -q1, -dot
    if dot > 1 - 1e-9:
        q = (1 - s) * q0 + s * q1
        q = q / np.sqrt((q * q).sum())
    else:
        th = np.arccos(dot)
        q = np.sin((1 - s) * th) / np.sin(th) * q0 + np.sin(s * th) / np.sin(th) * q1
    p0, p1, p2, p3 = kc[max(k - 1, 0), :, 3], kc[k, :, 3], kc[k + 1, :, 3], kc[min(k + 2, K - 1), :, 3]
    if mode == "catmull":
        t = 0.5 * (2 * p1 + (p2 - p0) * s + (2 * p0 - 5 * p1 + 4 * p2 - p3) * s ** 2 + (3 * p1 - p0 - 3 * p2 + p3) * s ** 3)
    else:
        t = (1 - s) * p1 + s * p2
    return np.concatenate([rot_of(q), t[:, None]], 1), (1 - s) * kn[k] + s * kn[k + 1]


@pytest.fixture(scope="module")
def keys():
    """K = 4 keyframes: pair (0, 1) has a negative quaternion dot (shortest-arc flip), pair (2, 3) is one pose twice (nlerp)."""
    rng = np.random.RandomState(7)
    qa = np.array([0.3, 0.9, 0.2, 0.1])
    qb = np.array([0.9, -0.4, 0.1, 0.1])
    qc = rng.randn(4)
    R = [rot_of(q / np.linalg.norm(q)) for q in (qa, qb, qc, qc)]
    t = rng.uniform(-1.5, 1.5, (4, 3))
    t[3] = t[2]
    c2w = np.stack([np.concatenate([r, p[:, None]], 1) for r, p in zip(R, t)]).astype(np.float32)
    nf = np.stack([rng.uniform(0.1, 0.3, 4), rng.uniform(4.0, 6.0, 4)], 1).astype(np.float32)
    nf[3] = nf[2]
    assert float(quat_of(c2w[0, :, :3].astype(np.float64)) @ quat_of(c2w[1, :, :3].astype(np.float64))) < -0.01
    return c2w, nf


@pytest.fixture(scope="module")
def frames(keys):
    """F = 3 interpolated poses (device) for the ray and row tests."""
    from upnerf_amd.novel_view import path_poses
    c2w, nf = path_poses(torch.from_numpy(keys[0]).cuda(), torch.from_numpy(keys[1]).cuda(), torch.tensor([0.25, 1.5, 2.999]).cuda(),
                         "catmull")
    return c2w, nf


@pytest.mark.parametrize("mode", ["linear", "catmull"])
def test_poses_match_the_fp64_restatement(keys, mode):
    from upnerf_amd.novel_view import path_poses
    kc, kn = keys
    dc, dn = torch.from_numpy(kc).cuda(), torch.from_numpy(kn).cuda()
    c2w, nf = path_poses(dc, dn, torch.tensor(U, dtype=torch.float32).cuda(), mode)
    assert tuple(c2w.shape) == (len(U), 3, 4) and tuple(nf.shape) == (len(U), 2)
    assert torch.isfinite(c2w).all() and torch.isfinite(nf).all()
    for f, u in enumerate(U):
        if u == int(u):  # on a keyframe: its floats, bit for bit
            assert torch.equal(c2w[f], dc[int(u)]) and torch.equal(nf[f], dn[int(u)]), u
            continue
        ref_c, ref_n = pose_ref(kc, kn, u, mode)
        got_c, got_n = c2w[f].cpu().numpy().astype(np.float64), nf[f].cpu().numpy().astype(np.float64)
        err_r = np.abs(got_c[:, :3] - ref_c[:, :3]).max()
        err_t = (np.abs(got_c[:, 3] - ref_c[:, 3]) / np.maximum(1, np.abs(ref_c[:, 3]))).max()
        err_n = (np.abs(got_n - ref_n) / np.maximum(1, np.abs(ref_n))).max()
        orth = np.abs(got_c[:, :3].T @ got_c[:, :3] - np.eye(3)).max()
        print(f"mode={mode} u={u}: rot {err_r:.2e} trans {err_t:.2e} near/far {err_n:.2e} RtR-I {orth:.2e}")
        assert err_r <= 1e-6 and err_t <= 1e-6 and err_n <= 1e-6 and orth <= 1e-6, (u, err_r, err_t, err_n, orth)
    # continuity into a keyframe (the copy at u = 2 against the interpolation just before it), and clamping outside [0, K-1]
    c2, n2 = path_poses(dc, dn, torch.tensor([2 - 1e-4, 2.0, -0.5, 7.0, float("nan")]).cuda(), mode)
    jump = max(float((c2[0] - c2[1]).abs().max()), float((n2[0] - n2[1]).abs().max()))
    print(f"mode={mode}: |pose(2 - 1e-4) - pose(2)| = {jump:.2e}")
    assert jump <= 1e-3
    assert torch.equal(c2[2], dc[0]) and torch.equal(c2[3], dc[3]) and torch.equal(c2[4], dc[0])


def rays_ref(c2w, nf, row0, R):
    """fp64 (o, d, near far) of rows [row0, row0 + R) from the fp32 frame poses."""
    c, n = c2w.cpu().numpy().astype(np.float64), nf.cpu().numpy().astype(np.float64)
    g = np.arange(row0, row0 + R)
    f, p = g // (H * W), g % (H * W)
    y, x = p // W, p % W
    fx, fy, cx, cy = (float(np.float32(v)) for v in (FX, FY, CX, CY))
    dirs = np.stack([(x - cx) / fx, -(y - cy) / fy, -np.ones(R)], 1)
    d = np.einsum("rj,rij->ri", dirs, c[f][:, :, :3])
    return c[f][:, :, 3], d / np.linalg.norm(d, axis=1, keepdims=True), n[f], f


def test_rays_match_fp64_and_do_not_depend_on_the_chunk(frames):
    from upnerf_amd.novel_view import path_rays
    c2w, nf = frames
    row0, R = 30, 50  # starts mid-row and mid-frame, crosses frame boundaries
    rays, _ = path_rays(c2w, nf, (W, H), (FX, FY, CX, CY), row0, R)
    assert tuple(rays.shape) == (R, 8)
    o, d, n, f = rays_ref(c2w, nf, row0, R)
    assert set(f.tolist()) == {0, 1, 2} and row0 % W != 0  # both frame boundaries inside the range
    fi = torch.from_numpy(f).cuda()
    assert torch.equal(rays[:, 0:3], c2w[fi][:, :, 3])
    assert torch.equal(rays[:, 6:8], nf[fi])
    got = rays[:, 3:6].cpu().numpy().astype(np.float64)
    err, nrm = np.abs(got - d).max(), np.abs(np.linalg.norm(got, axis=1) - 1).max()
    print(f"directions: max abs err {err:.2e}, max | |d| - 1 | {nrm:.2e}")
    assert err <= 1e-6 and nrm <= 2e-7
    whole, _ = path_rays(c2w, nf, (W, H), (FX, FY, CX, CY), 0, 3 * H * W)
    assert torch.equal(whole[row0:row0 + R], rays)
    # a ray buffer that is not 16-byte aligned takes the scalar stores: the same bits
    big = torch.zeros(R * 8 + 1, device="cuda")
    odd, _ = path_rays(c2w, nf, (W, H), (FX, FY, CX, CY), row0, R, rays=big[1:].view(R, 8))
    assert odd.data_ptr() % 16 != 0 and torch.equal(odd, rays) and float(big[0]) == 0
    # intrinsics as a 3 x 3 matrix
    Km = torch.tensor([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    assert torch.equal(path_rays(c2w, nf, (W, H), Km, row0, R)[0], rays)


def test_blended_rows_return_table_rows_bit_for_bit(frames):
    from upnerf_amd.novel_view import path_rays
    c2w, nf = frames
    g = torch.Generator().manual_seed(3)
    tabs = [torch.randn(6, dim, generator=g).cuda() for dim in (48, 16, 6)]  # dim 6: the path without 16-byte accesses
    i0 = torch.tensor([1, 4, 2], dtype=torch.int32).cuda()
    i1 = torch.tensor([3, 0, 5], dtype=torch.int32).cuda()
    t = torch.tensor([0.0, 1.0, 0.5]).cuda()
    n = H * W
    _, rows = path_rays(c2w, nf, (W, H), (FX, FY, CX, CY), 0, 3 * n, tables=[(T, None) for T in tabs], i0=i0, i1=i1, t=t)
    for T, out in zip(tabs, rows):
        assert tuple(out.shape) == (3 * n, T.shape[1])
        assert torch.equal(out[:n], T[1].expand(n, -1))
        assert torch.equal(out[n:2 * n], T[0].expand(n, -1))
        assert torch.equal(out[2 * n:], (0.5 * T[2] + 0.5 * T[5]).expand(n, -1))
    # a chunk that starts mid-frame, into preallocated buffers with spare rows
    bufs = [torch.full((60, T.shape[1]), 7.0, device="cuda") for T in tabs]
    _, part = path_rays(c2w, nf, (W, H), (FX, FY, CX, CY), 30, 50, tables=list(zip(tabs, bufs)), i0=i0, i1=i1, t=t)
    for out, full, buf in zip(part, rows, bufs):
        assert torch.equal(out, full[30:80]) and bool((buf[50:] == 7.0).all())
    # an index outside the table is clamped into it
    bad0 = torch.tensor([-3, 99, 2], dtype=torch.int32).cuda()
    _, rows = path_rays(c2w, nf, (W, H), (FX, FY, CX, CY), 0, 3 * n, tables=[(tabs[0], None)], i0=bad0, i1=bad0,
                        t=torch.zeros(3).cuda())
    assert torch.equal(rows[0][0], tabs[0][0]) and torch.equal(rows[0][n], tabs[0][5]) and torch.equal(rows[0][2 * n], tabs[0][2])


# ---- through the fields -------------------------------------------------------------------------------------------------

def make_system(progress):
    from upnerf_amd.nerf_system import NeRFSystem, SyntheticDataset, default_hparams
    hp = default_hparams(**{"nerf.N_samples": 32, "nerf.N_importance": 32, "max_steps": 1000})
    torch.manual_seed(11)
    s = NeRFSystem(hp, SyntheticDataset(6))
    s.setup()
    with torch.no_grad():
        for emb in s.embeddings.values():
            emb.weight.copy_(torch.randn(emb.weight.shape))
    s.cuda()
    s.set_progress(progress)
    return s


@pytest.fixture(scope="module")
def systems():
    return {p: make_system(p) for p in (0.8, 0.3, 0.05)}  # sched_mult 1, 0.5 (candidate head on), 0


def render(system, rays, **kw):
    from upnerf_amd.rendering import render_rays
    hp = system.hparams
    with torch.no_grad():
        return render_rays(system.models, system.embeddings, rays, sched_mult=system.get_schedule_mult(system._host_progress),
                           N_samples=hp["nerf.N_samples"], N_importance=hp["nerf.N_importance"], use_disp=hp["nerf.use_disp"],
                           perturb=0, encode_feat=True, **kw)


@pytest.mark.parametrize("progress", [0.8, 0.3])
def test_embed_rows_keyword_equals_the_gather(systems, frames, progress):
    from upnerf_amd.novel_view import path_rays
    s = systems[progress]
    sm = s.get_schedule_mult(s._host_progress)
    assert sm == 1 if progress == 0.8 else abs(sm - 0.5) < 1e-6
    rays, _ = path_rays(frames[0], frames[1], (W, H), (FX, FY, CX, CY), 30, 48)
    idx = torch.randint(0, 6, (48,), generator=torch.Generator().manual_seed(5)).cuda()
    ref = render(s, rays, img_idx=idx)
    keys = [k for k in s.embeddings if k.endswith("_a") or sm < 1]
    assert len(keys) == (2 if sm == 1 else 4)
    got = render(s, rays, img_idx=None, embed_rows={k: s.embeddings[k].weight.detach()[idx] for k in keys})
    assert set(got) == set(ref) and "s_rgb_fine" in ref
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    if sm < 1:
        assert "c_weights_fine" in ref
    with pytest.raises(ValueError):
        render(s, rays, img_idx=None, embed_rows={keys[0]: s.embeddings[keys[0]].weight.detach()[idx]} if len(keys) > 1 else {})
    with pytest.raises(ValueError):
        render(s, rays, img_idx=None, embed_rows={k: s.embeddings[k].weight.detach()[idx][:, :-1] for k in keys})


def two_key_path(n_frames=3, wh=(8, 6)):
    from upnerf_amd.novel_view import CameraPath
    c = np.cos(0.3), np.sin(0.3)
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.05], [0, 0, 1, 0.2]],
                        [[c[0], 0, c[1], -0.2], [0, 1, 0, 0.1], [-c[1], 0, c[0], 0.0]]])
    K = torch.tensor([[7.5, 0, 3.6], [0, 7.0, 2.8], [0, 0, 1]])
    return CameraPath.from_poses(c2w, [(0.1, 5.0), (0.2, 4.5)], n_frames, appearance=(ID0, ID1), img_wh=wh, K=K)


def frame_rays(path, f):
    from upnerf_amd.novel_view import path_poses, path_rays
    c2w, nf = path_poses(path.key_c2w.cuda(), path.key_near_far.cuda(), path.u.cuda(), path.mode)
    n = path.img_wh[0] * path.img_wh[1]
    return path_rays(c2w, nf, path.img_wh, path.K, f * n, n)[0]


@pytest.mark.parametrize("progress", [0.8, 0.3])
def test_render_path_frames_are_renders_with_blended_rows(systems, progress):
    from upnerf_amd.novel_view import render_path
    s, path = systems[progress], two_key_path()
    n = 48
    out = render_path(s, path, outputs=("rgb_float",))
    maps = out["rgb_float"]
    assert tuple(maps.shape) == (3, n, 3) and torch.isfinite(maps).all()
    # (a) the end frames sit on the keyframes with t = 0 and t = 1: plain renders with the image's own rows
    for f, img in ((0, ID0), (2, ID1)):
        ref = render(s, frame_rays(path, f), img_idx=torch.full((n,), img, dtype=torch.int64).cuda())["s_rgb_fine"]
        assert torch.equal(maps[f], ref), f
    # (b) the middle frame: the same render through a copy of the system whose row ID0 IS the blended vector
    assert float(path.t[1]) == 0.5
    twin = copy.deepcopy(s)
    with torch.no_grad():
        for emb in twin.embeddings.values():
            emb.weight[ID0] = 0.5 * emb.weight[ID0] + 0.5 * emb.weight[ID1]
    ref = render(twin, frame_rays(path, 1), img_idx=torch.full((n,), ID0, dtype=torch.int64).cuda())["s_rgb_fine"]
    assert torch.equal(maps[1], ref)
    plain = render(s, frame_rays(path, 1), img_idx=torch.full((n,), ID0, dtype=torch.int64).cuda())["s_rgb_fine"]
    assert not torch.equal(maps[1], plain)  # the blend is visible
    # (c) and it is a different picture from both ends
    assert not torch.equal(maps[1], maps[0]) and not torch.equal(maps[1], maps[2])


def test_render_path_outputs_chunks_depth_range_and_sink(systems):
    from upnerf_amd import visualization as viz
    from upnerf_amd.novel_view import render_path
    s, path = systems[0.8], two_key_path()
    calls = []
    keys = ("rgb_float", "rgb", "depth")
    a = render_path(s, path, chunk=17, outputs=keys, sink=lambda tag, f, images: calls.append((tag, f, sorted(images))))
    b = render_path(s, path, chunk=10_000, outputs=keys)
    assert set(a) == set(b) == set(keys)
    for k in keys:  # (d)
        assert torch.equal(a[k], b[k]), k
    assert a["rgb"].dtype == torch.uint8 and tuple(a["rgb"].shape) == (3, 6, 8, 3) and tuple(a["depth"].shape) == (3, 6, 8, 3)
    for f in range(3):  # (e)
        assert torch.equal(a["rgb"][f], viz.rgb_image(a["rgb_float"][f], (8, 6)))
    # (f) one depth range for the whole sequence, frame 0's: the same bytes as rendering with that range given
    d0 = render(s, frame_rays(path, 0), img_idx=torch.full((48,), ID0, dtype=torch.int64).cuda())["s_depth_fine"]
    mi, ma = (float(x) for x in viz.min_max_of(d0).cpu())
    assert ma > mi
    c = render_path(s, path, outputs=("depth",), depth_range=(mi, ma))
    assert torch.equal(c["depth"], a["depth"])
    assert torch.equal(a["depth"][0], viz.depth_image(d0, (8, 6)))
    d1 = render(s, frame_rays(path, 1), img_idx=None, embed_rows={
        k: (0.5 * e.weight[ID0] + 0.5 * e.weight[ID1]).detach().expand(48, -1).contiguous() for k, e in s.embeddings.items()
        if k.endswith("_a")})["s_depth_fine"]
    assert torch.equal(a["depth"][1], viz.depth_image(d1, (8, 6), min_max=(mi, ma)))  # ... not frame 1's own range
    # (g) the sink saw every frame once, in order
    assert calls == [("path", f, ["depth", "rgb"]) for f in range(3)]
    with pytest.raises(ValueError):
        render_path(s, path, outputs=("rgb", "normals"))


def test_render_path_refuses_a_phase_without_static_colour(systems):
    from upnerf_amd.novel_view import render_path
    s = systems[0.05]
    assert s.get_schedule_mult(s._host_progress) == 0
    with pytest.raises(ValueError, match="sched_mult == 0"):
        render_path(s, two_key_path())


def test_render_path_memory_is_the_chunk_not_the_sequence(systems):
    """The per-chunk buffers have `chunk` rows whatever the number of frames, and a longer sequence costs its outputs only.
    (The bound 'below one [F H W][48] buffer per table' cannot be asked of max_memory_allocated at this size: one 16-ray chunk
    of the fields alone holds 16 x 64 samples x 256 floats = 1 MiB of activations against 4 x 36 KiB of such buffers; so the
    workspace shapes are asserted, and the growth of the peak with F.)"""
    from upnerf_amd import novel_view
    s = systems[0.3]  # four tables
    peaks = {}
    for F in (1, 4):
        path = two_key_path(n_frames=F)
        novel_view.render_path(s, path, chunk=16, outputs=("rgb",))  # warm-up: cached tables, workspaces
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = novel_view.render_path(s, path, chunk=16, outputs=("rgb",))
        torch.cuda.synchronize()
        peaks[F] = torch.cuda.max_memory_allocated() - base
        assert novel_view.LAST_WORKSPACE == {"rays": (16, 8), "coarse_a": (16, 48), "fine_a": (16, 48), "coarse_c": (16, 16),
                                             "fine_c": (16, 16)}
        del out
    # three more frames: their uint8 output (3 x 48 x 3 B) and pose rows, each allocation rounded up to 512 B by the allocator
    print(f"peak over the baseline: F=1 {peaks[1]} B, F=4 {peaks[4]} B")
    assert peaks[4] - peaks[1] <= 8 * 512
    assert peaks[4] - peaks[1] < 4 * (3 * 48 * 48 * 4)  # far below [extra rows][48] fp32 per table


def test_through_images_uses_the_refined_poses_and_writes_frames(systems, tmp_path):
    from upnerf_amd.novel_view import CameraPath, render_path
    from upnerf_amd.pose_align import refined_poses
    from upnerf_amd.visualization import ImageWriter
    s = copy.deepcopy(systems[0.8])
    g = torch.Generator().manual_seed(9)
    ds = s.train_dataset
    ang = torch.rand(6, generator=g) * 0.4
    ds.poses = torch.zeros(6, 3, 4)
    ds.poses[:, 0, 0] = ds.poses[:, 2, 2] = torch.cos(ang)
    ds.poses[:, 0, 2], ds.poses[:, 2, 0], ds.poses[:, 1, 1] = torch.sin(ang), -torch.sin(ang), 1.0
    ds.poses[:, :, 3] = torch.rand(6, 3, generator=g) * 0.2
    ds.nears, ds.fars = [0.1 + 0.01 * i for i in range(6)], [5.0 - 0.1 * i for i in range(6)]
    ds.Ks = [np.array([[6.0 + i, 0, 2.0], [0, 6.5 + i, 1.5], [0, 0, 1]]) for i in range(6)]
    ds.all_imgs_wh = torch.tensor([[4 + i, 3 + i] for i in range(6)])
    with torch.no_grad():
        s.se3_refine.weight.copy_(torch.randn(6, 6, generator=g) * 1e-2)
    path = CameraPath.through_images(s, [3, 0, 5], n_frames=4, mode="linear", loop=True)
    ref = refined_poses(s.se3_refine.weight.detach(), ds.poses).cpu()
    assert torch.equal(path.key_c2w, ref[[3, 0, 5, 3]])
    assert path.img_wh == (7, 6) and float(path.K[0, 0]) == 9.0 and path.mode == "linear"
    assert torch.equal(path.key_near_far[1], torch.tensor([0.1, 5.0])) and torch.equal(path.key_near_far[3], path.key_near_far[0])
    assert path.u.tolist() == [0.0, 1.0, 2.0, 3.0] and path.i0.tolist() == [3, 0, 5, 3] and path.t.tolist() == [0.0] * 4
    writer = ImageWriter(str(tmp_path / "frames"))
    out = render_path(s, path, outputs=("rgb",), sink=writer)
    assert tuple(out["rgb"].shape) == (4, 6, 7, 3) and len(writer.written) == 4
    assert torch.equal(out["rgb"][0], out["rgb"][3])  # the loop closes on the first image, pose and appearance
    from PIL import Image
    back = np.asarray(Image.open(writer.path("path", 2, "rgb")))
    assert np.array_equal(back, out["rgb"][2].cpu().numpy())


def test_a_training_view_is_the_same_picture_by_three_routes(systems, monkeypatch):
    """Image i seen from its own refined pose under its own appearance: frame 0 of a path through it (render_path), the colour
    map fuse_views renders of it, and render_static on the path_rays of that pose are the same rays, rows and kernels -- bit for
    bit, with chunks of 20 rows over 48-pixel frames (they straddle the frame boundary; the last one is partial)."""
    from upnerf_amd import geometry
    from upnerf_amd import static_scene as ss
    from upnerf_amd.novel_view import CameraPath, path_rays, render_path
    s = copy.deepcopy(systems[0.8])
    assert s.get_schedule_mult(s._host_progress) == 1
    g = torch.Generator().manual_seed(21)
    ds = s.train_dataset
    ang = torch.linspace(-0.4, 0.4, 6)
    ds.poses = torch.zeros(6, 3, 4)
    ds.poses[:, 0, 0] = ds.poses[:, 2, 2] = torch.cos(ang)
    ds.poses[:, 0, 2], ds.poses[:, 2, 0], ds.poses[:, 1, 1] = torch.sin(ang), -torch.sin(ang), 1.0
    ds.poses[:, :, 3] = torch.rand(6, 3, generator=g) * 0.2
    ds.nears, ds.fars = [0.1 + 0.01 * k for k in range(6)], [5.0 - 0.1 * k for k in range(6)]
    ds.Ks = [np.array([[7.5 + k, 0, 3.6], [0, 7.0 + k, 2.8], [0, 0, 1]]) for k in range(6)]
    ds.all_imgs_wh = torch.tensor([[8, 6]] * 6)
    with torch.no_grad():
        s.se3_refine.weight.copy_(torch.randn(6, 6, generator=g) * 1e-2)
    i, j, n = 4, 1, 48
    path = CameraPath.through_images(s, [i, j], n_frames=2)
    by_path = render_path(s, path, chunk=20, outputs=("rgb_float",))["rgb_float"][0]
    assert tuple(by_path.shape) == (n, 3) and torch.isfinite(by_path).all() and float(by_path.std()) > 0
    fused = []
    integrate = geometry.TsdfVolume.integrate
    monkeypatch.setattr(geometry.TsdfVolume, "integrate", lambda self, depth, *a, rgb=None, **kw: (fused.extend(rgb), integrate(self, depth, *a, rgb=rgb, **kw))[1])
    geometry.fuse_views(s, ((-1.0, -1.0, -3.0), (1.0, 1.0, 0.5)), (8, 8, 8), img_ids=[i], chunk=20)
    assert len(fused) == 1
    pose = ss.refined_training_poses(s, [i]).cuda().contiguous()
    nf = torch.tensor([ss.near_far(s, i)], dtype=torch.float32).cuda()
    rays, _ = path_rays(pose, nf, (8, 6), ds.Ks[i], 0, n)
    with torch.no_grad():
        own = ss.render_static(s, rays, ss.appearance_rows(s, ss.static_keys(s, 1), i, n), 1)["s_rgb_fine"]
    assert torch.equal(by_path, fused[0]) and torch.equal(by_path, own)
    other = render_path(s, CameraPath.through_images(s, [j, i], n_frames=2), chunk=20, outputs=("rgb_float",))["rgb_float"][0]
    assert not torch.equal(by_path, other)  # (the comparison tells two images apart)
