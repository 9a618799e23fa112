"""The fused field kernels (csrc/field.hip, field16.hip, field16rr.hip) against the fp64 restatement of the pass
(tests/field_cases.py, tests/kernel_space.py) where test_hip_kernels.py::test_field_pass_stage_by_stage does not reach: partial
last tiles, tiles that straddle two and three rays, 32-sample partial sums at an S that is no multiple of 32, a fractional band
weight under zero bands, per-tile exponents that differ inside a launch, zero tiles inside a live launch, mode 3 with the colour
head, feature-less fields.  Same comparisons, gates and mask limits as the stage test (the "f16" mode keeps its stated relaxed
ones); tests/test_field_cases_cpu.py shows on the CPU that the fp32 restatement meets half of each gate on these inputs, so a miss
here is the kernels'."""
import pytest
import torch

import field_cases as fc
from golden_util import Case
from test_hip_kernels import STAGE_CASES, field_mode, hip  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

MODES = ["f16x3", "f32", "f16"]


@pytest.mark.parametrize("field_mode", MODES, indirect=True)
@pytest.mark.parametrize("key", fc.SYNTH_256, ids=fc.label)
def test_field_pass_on_ragged_tiles_against_fp64(hip, key, field_mode):
    fc.check_field_pass(hip, fc.load(key), field_mode, torch.float64, tag=fc.label(key))


@pytest.mark.parametrize("key", fc.SYNTH_64, ids=fc.label)
def test_64_wide_field_pass_on_ragged_tiles_against_fp64(hip, key):
    assert hip["rendering"].FIELD_MODE == "f16x3"
    fc.check_field_pass(hip, fc.load(key), "f16x3", torch.float64, tag=fc.label(key))


@pytest.mark.parametrize("field_mode", MODES, indirect=True)
def test_smallest_pass_against_fp64(hip, field_mode):
    """One sample of one ray: the fp32 kernels in the f32 and f16x3 modes (S < 32); the f16 mode refuses it before any launch."""
    key = fc.SYNTH_SMALLEST
    if field_mode == "f16":
        rd, s = hip["rendering"], fc.load(key)
        with pytest.raises(ValueError, match="at least 32 samples"):
            rd._plan(s["model"].packer, key.R, key.S, key.mode, key.use_cand, key.use_rgb, train=True)
        return
    fc.check_field_pass(hip, fc.load(key), field_mode, torch.float64, tag=fc.label(key))


@pytest.mark.parametrize("field_mode", MODES, indirect=True)
@pytest.mark.parametrize("name,typ", fc.NOFEAT)
def test_featureless_field_pass_against_fp64(hip, name, typ, field_mode):
    if field_mode != "f16x3" and Case(name).W != 256:
        pytest.skip("64-wide fields run the fp32 kernels in either mode (and the f16 mode refuses them)")
    s = fc.load((name, typ))
    assert s["rgb_joint"] and s["mode"] == 1
    fc.check_field_pass(hip, s, field_mode, torch.float64, tag=f"{name} {typ}")


@pytest.mark.parametrize("field_mode", ["f16x3", "f32"], indirect=True)
@pytest.mark.parametrize("name,typ", STAGE_CASES)
def test_golden_stage_cases_hold_against_fp64_too(hip, name, typ, field_mode):
    if field_mode != "f16x3" and Case(name).W != 256:
        pytest.skip("64-wide fields run the fp32 kernels in either mode")
    fc.check_field_pass(hip, fc.load((name, typ)), field_mode, torch.float64, tag=f"{name} {typ}")
