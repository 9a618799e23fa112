"""The shared host layer of the scene tools (upnerf_amd/static_scene.py) and NeRF.host_progress_value, without a GPU: dataset
accessors, intrinsics, boxes, and the arguments render_static hands to render_rays."""
import numpy as np
import pytest
import torch

from upnerf_amd import static_scene as ss


def _system(**ds_members):
    ds = type("D", (), ds_members)()
    return type("S", (), {"train_dataset": ds, "hparams": {"nerf.near": 0.1, "nerf.far": 5.0}})()


def test_per_image_reads_dict_keyed_and_list_indexed_datasets():
    keyed = type("D", (), {"img_ids_train": [40, 7, 19], "nears": {7: 0.25, 19: 0.5, 40: 0.75}, "fars": [3.0, 4.0, 5.0]})()
    assert ss.per_image(keyed, "nears", 0) == 0.75 and ss.per_image(keyed, "nears", 1) == 0.25  # through img_ids_train
    assert ss.per_image(keyed, "fars", 2) == 5.0  # a list is indexed by the training index even where the ids exist
    plain = type("D", (), {"nears": [0.1, 0.2]})()
    assert ss.per_image(plain, "nears", 1) == 0.2
    assert ss.per_image(plain, "Ks", 0) is None


def test_near_far_prefers_the_datasets_values_and_falls_back_per_plane():
    assert ss.near_far(_system(), 3) == (0.1, 5.0)
    s = _system(nears=[0.2, 0.3], fars=[2.0, np.float32(2.5)])
    assert ss.near_far(s, 1) == (0.3, 2.5) and all(type(v) is float for v in ss.near_far(s, 1))
    assert ss.near_far(_system(fars=[2.0, 4.0]), 1) == (0.1, 4.0)
    assert ss.plane(_system(fars=[2.0, 4.0]), "far", 0) == 2.0
    only_far = type("S", (), {"train_dataset": type("D", (), {})(), "hparams": {"nerf.far": 2.0}})()
    assert ss.plane(only_far, "far", 0) == 2.0  # (bounds_from_cameras asks for nothing else)


def test_intrinsics_of_a_tensor_an_array_and_a_tuple_are_the_same_floats():
    fx, fy, cx, cy = np.float32(14.3), np.float32(13.7), np.float32(7.45), np.float32(5.55)  # not fp32-exact in decimal
    K32 = torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float32)
    K64 = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)
    want = (float(fx), float(fy), float(cx), float(cy))
    for K in (K32, K64, (fx, fy, cx, cy), want, K32.requires_grad_()):
        got = ss.intrinsics(K)
        assert got == want and all(type(v) is float for v in got)
    with pytest.raises(ValueError):
        ss.intrinsics((1.0, 2.0, 3.0))


def test_box_in_both_modes():
    good = ((0, 0, 0), (1, 2, 3))
    for strict in (False, True):
        assert ss.box(good, strict=strict) == ((0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
        with pytest.raises(ValueError):
            ss.box(((0, 0), (1, 1)), strict=strict)  # two axes
    flat = ((0, 0, 0), (1, 0, 1))  # no extent along y
    assert ss.box(flat) == ((0.0, 0.0, 0.0), (1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        ss.box(flat, strict=True)
    assert list(ss.c_float3((1.0, 2.5, -3.0))) == [1.0, 2.5, -3.0]


def test_host_progress_value_is_what_the_parameter_holds():
    from upnerf_amd.nerf import NeRF
    m = NeRF("fine", D=2, W=64, skips=[], dir_L=4, c2f=(0.1, 0.5))
    m.set_progress(0.3)
    v = m.host_progress_value()
    m.flush_progress()
    assert type(v) is float and v == float(m.progress.data) == float(np.float32(0.3)) != 0.3
    m.load_state_dict(m.state_dict())  # as after a checkpoint: no mirror
    m.progress.data.fill_(0.7)  # the reference's way of writing it
    assert m.host_progress is None and m.host_progress_value() == float(m.progress.data) == float(np.float32(0.7))


def test_guards_and_field_selection():
    with pytest.raises(RuntimeError, match="device memory only"):
        ss.require_cuda("f", torch.zeros(2))
    with pytest.raises(RuntimeError, match="device memory only"):
        ss.require_cuda("f", torch.device("cpu"))
    with pytest.raises(RuntimeError):
        ss.require_cuda("f", None)
    ss.require_cuda("f", torch.device("cuda", 0))  # (a device is a name: nothing is initialised)
    system = type("S", (), {"models": {"nerf_fine": torch.nn.Linear(2, 2)}})()
    with pytest.raises(RuntimeError, match="density_grid runs on the GPU only"):
        ss.field_of(system, "fine", "density_grid")
    with pytest.raises(ValueError, match="no coarse field"):
        ss.field_of(system, "coarse", "density_grid")
    with pytest.raises(ValueError, match="'fine' or 'coarse'"):
        ss.field_of(system, "transient", "density_grid")


class _Tables(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embeddings = torch.nn.ModuleDict({k: torch.nn.Embedding(4, d) for k, d in
                                               (("coarse_a", 3), ("fine_a", 3), ("coarse_c", 2), ("fine_c", 2))})
        self.models, self.train_dataset = {}, type("D", (), {"white_back": True})()
        self.hparams = {"nerf.N_samples": 32, "nerf.N_importance": 16, "nerf.use_disp": False, "nerf.feat_dim": 0}


@pytest.mark.parametrize("sched_mult, phase, keys", [(0.3, 1, ["coarse_a", "fine_a", "coarse_c", "fine_c"]), (1, 2, ["coarse_a", "fine_a"])])
def test_render_static_hands_render_rays_the_phase_of_the_schedule(monkeypatch, sched_mult, phase, keys):
    from upnerf_amd import rendering
    s = _Tables()
    assert ss.static_keys(s, sched_mult) == keys
    rows = ss.appearance_rows(s, keys, 2, 5)
    assert list(rows) == keys and all(torch.equal(r, s.embeddings[k].weight[2].expand(5, -1)) and r.is_contiguous() for k, r in rows.items())
    with pytest.raises(ValueError, match="img_id"):
        ss.appearance_rows(s, keys, 4, 5)
    seen = {}
    monkeypatch.setattr(rendering, "render_rays", lambda **kw: seen.update(kw) or {"marker": 1})
    rays = torch.zeros(5, 8)
    assert ss.render_static(s, rays, rows, sched_mult) == {"marker": 1}
    assert seen["sched_phase"] == phase and seen["sched_mult"] == sched_mult and seen["rays"] is rays and seen["embed_rows"] is rows
    assert seen["img_idx"] is None and seen["perturb"] == 0 and seen["validation"] is True and seen["normals"] is False
    assert (seen["N_samples"], seen["N_importance"], seen["white_back"], seen["encode_feat"]) == (32, 16, True, False)
    ss.render_static(s, rays, rows, sched_mult, normals=True)
    assert seen["normals"] is True
