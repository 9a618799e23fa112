"""The adversarial grids and ray families of tests/walk_cases.py through the real entry points on the GPU: upnerf_baked_render,
upnerf_baked_sh_render (degrees 1 and 2), upnerf_baked_sparse_render and upnerf_occ_spans.  The claims and their gates are those
of tests/test_walks_host_cpu.py (the same functions judge both): the fp64 restatements' own derived gates with the borderline
rule and its 2 % cap on the grids with density on their faces; everything else bit for bit -- the scene's bits against all bits
set, sparse against dense (on the rays of the fp64 comparison as well), a second run, and the background at `far` on a miss:
a ray with a number that is none, far <= near, and a ray of finite numbers none of whose samples is inside the box.  Host and device may contract fmas differently,
so nothing is asserted between them: the largest difference per output is printed for the record."""
import numpy as np
import pytest
import torch

import walk_cases as wc
from walk_checks import BACKGROUND, CONFIGS, N_REF, N_SPAN, REF_CONFIGS, check_spans, compare_fp64, host_build, run_march

pytestmark = pytest.mark.gpu

GRIDS = ["faces", "ragged", "corners"]
N_GPU = 200  # rays per family and configuration; the two rays of `caps` with more samples than the cap are among them
_CACHE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scenes(name, degree):
    """(the dense scene, the same scene with every bit set, its sparse form), built once."""
    key = (name, degree)
    if key not in _CACHE:
        from upnerf_amd.baked import BakedScene
        from upnerf_amd.occupancy import OccupancyGrid
        S = wc.scene(name)
        make = (lambda: BakedScene.from_grids(dev(S["rgbs"][..., 3]), dev(S["rgbs"][..., :3]), wc.BOUNDS, S["level"])) if degree == 0 else \
            (lambda: BakedScene.from_records(dev(S["points"][degree]), wc.BOUNDS, S["level"], degree))
        scene, full = make(), make()
        assert (scene.occupancy.words.cpu().numpy().view(np.uint32) == S["words"]).all()
        full.occupancy = OccupancyGrid.from_cells(torch.ones_like(scene.occupancy.cells()), wc.BOUNDS)
        _CACHE[key] = (scene, full, scene.sparsify())
    return _CACHE[key]


def same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("rgb", "depth", "opacity"))  # (as bits: a far that is a NaN)


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("name", GRIDS)
def test_skipping_layout_and_runs_agree_bit_for_bit_and_a_miss_is_the_background(name, degree):
    scene, full, sparse = scenes(name, degree)
    S = wc.scene(name)
    for step_name, stop in CONFIGS:
        step = wc.steps(name)[step_name]
        rays, fam = wc.rays_of(N_GPU, 6, S["cells"], step)
        r = dev(rays)
        out = scene.render(r, step, background=BACKGROUND, stop=stop)
        assert same(full.render(r, step, background=BACKGROUND, stop=stop), out), (step_name, stop, "all bits set")
        assert same(sparse.render(r, step, background=BACKGROUND, stop=stop), out), (step_name, stop, "sparse")
        assert same(scene.render(r, step, background=BACKGROUND, stop=stop), out), (step_name, stop, "a second run")
        miss = ~np.isfinite(rays).all(1) | ~(rays[:, 7] > rays[:, 6])
        assert miss.sum() >= 20
        rgb, depth, op = (out[k].cpu().numpy() for k in ("rgb", "depth", "opacity"))
        assert (rgb[miss] == np.float32(BACKGROUND)).all() and (op[miss] == 0).all()
        assert np.array_equal(depth[miss].view(np.uint32), rays[miss, 7].view(np.uint32))
        assert int((op > 0).sum()) >= 50  # the comparison looked at rays that met the volume


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if host_build.hipcc() is None:
        return None
    return host_build.build(str(tmp_path_factory.mktemp("walk_host")), names=("baked_host",))["baked_host"]


@pytest.mark.parametrize("name", GRIDS)
def test_the_entry_points_are_within_the_fp64_restatements_gates(name, host_program, tmp_path):
    S = wc.scene(name)
    for step_name, stop in REF_CONFIGS:
        step = wc.steps(name)[step_name]
        rays, fam = wc.rays_of(N_REF[S["edge"]], 3, S["cells"], step, ref=S["edge"], big=False)
        far_off = ~wc.borderline(S["cells"], rays, step)  # (no sample within its dg of a face: fp32 and fp64 agree on the side)
        host = run_march(host_program, tmp_path, name, rays, step, stop)["march"].view(np.float32) if host_program else None
        for degree in (0, 1, 2):
            scene, _, sparse = scenes(name, degree)
            out = scene.render(dev(rays), step, background=BACKGROUND, stop=stop)
            got = torch.cat([out["rgb"], out["depth"][:, None], out["opacity"][:, None]], 1).cpu().numpy()
            assert same(sparse.render(dev(rays), step, background=BACKGROUND, stop=stop), out), (step_name, degree, "sparse")
            worst, left, n, ref, _ = compare_fp64(name, degree, rays, fam, step, stop, got)
            # a ray of finite numbers none of whose samples falls inside the box (it passes beside the box, lies in the plane of
            # the hi face and beyond, or ends before the box): the background at far, exactly
            miss = np.isfinite(rays).all(1) & (rays[:, 7] > rays[:, 6]) & (ref["inside"] == 0) & far_off
            assert miss.sum() >= 10, (step_name, int(miss.sum()))
            assert (got[miss, :3] == np.float32(BACKGROUND)).all() and (got[miss, 4] == 0).all()
            assert np.array_equal(got[miss, 3].view(np.uint32), rays[miss, 7].view(np.uint32))
            line = f"{name} {step_name} stop {stop} degree {degree}: worst err / gate {worst:.3f}, left out {left:.4f}, {n} rays hit"
            if host is not None:
                with np.errstate(invalid="ignore"):
                    diff = np.nan_to_num(np.abs(got.astype(np.float64) - host[degree * 4 + 1]), nan=0.0, posinf=0.0)
                line += f"; host - device: rgb {diff[:, :3].max():.2e} depth {diff[:, 3].max():.2e} opacity {diff[:, 4].max():.2e}"
            print(line)


@pytest.mark.parametrize("name", GRIDS)
def test_the_span_kernel_gives_brute_forces_spans(name):
    from upnerf_amd.occupancy import OccupancyGrid, ray_spans
    S = wc.scene(name)
    rays, fam = wc.rays_of(N_SPAN, 4, S["cells"], wc.steps(name)["cell"], big=False)
    occ = OccupancyGrid.from_cells(dev(S["bits"]), wc.BOUNDS)
    t0, t1, hit = (x.cpu().numpy() for x in ray_spans(occ, dev(rays)))
    assert check_spans(name, rays, fam, t0, t1, hit) >= 50
    again = ray_spans(occ, dev(rays))
    assert np.array_equal(again[0].cpu().numpy().view(np.uint32), t0.view(np.uint32)) and np.array_equal(again[2].cpu().numpy(), hit)
