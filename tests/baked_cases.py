"""What the GPU tests of the baked scenes (tests/test_hip_baked*.py) share: the way to the device, the scenes of the reference
grids built once, the 132 rays and the synthetic system.  A plain module: every test file imports what it uses."""
import numpy as np
import torch

import baked_ref as br
import baked_tune_ref as tr

_SCENES = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(points, level, degree=0):
    """The dense BakedScene of rgbs [Nz, Ny, Nx, 4] (degree 0) or records (degree 1 | 2) in baked_ref.BOUNDS; from_grids prunes
    again what the reference pruned: the same grid."""
    from upnerf_amd.baked import BakedScene
    if degree == 0:
        return BakedScene.from_grids(dev(points[..., 3]), dev(points[..., :3]), br.BOUNDS, level)
    return BakedScene.from_records(dev(points), br.BOUNDS, level, degree)


def scene_of(key, make, sparse=False):
    """The scene make() of `key` (the caller's module among it), or its sparsify(): each built once and never changed."""
    if (key, sparse) not in _SCENES:
        _SCENES[key, sparse] = scene_of(key, make).sparsify() if sparse else make()
    return _SCENES[key, sparse]


def rays_all(rgbs):
    """[132, 8]: baked_ref's 67 rays (a full wave and a ragged one, misses and non-finite rows among them), then baked_tune_ref's
    64 identical rays and the one inside a cell face of the grid."""
    return np.concatenate([br.make_rays(), tr.extra_rays(rgbs)])


def make_system():
    """The synthetic system of the scene-tool tests: trained-like fields, posed cameras (the body of each module's fixture)."""
    from test_hip_tsdf import make_system
    return make_system()
