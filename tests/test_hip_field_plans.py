"""The plans of rendering._FieldPass outside the full training pass, on the ragged shapes of tests/test_hip_field_edges.py and
against the same fp64 restatement (tests/field_cases.py) under the same gates: the forward-only plan (train=False: the kernels
get NULL for everything only a backward pass reads, and the register-resident "f16" kernels hand compositing fp16 fragments of e
and g2), the density-only pass (mode 2, neither head, no per-ray rows), and the backward pass with frozen leaves (no weight
gradients, need_dxyz = 0, NULL targets in the partial-sum finish) or with outputs the loss does not read (NULL upstream gradients
in the field backward kernels).  tests/test_field_cases_cpu.py shows on the CPU that the fp32 restatement meets half of each gate
on every pair run here, so a miss here is the kernels'.

Measured on an MI355X (worst figure over all cases / its gate).  f16x3 and f32: forward-only x0 9.8e-8 / 2e-6, aux 4.7e-8 / 2e-6,
activations and outputs 1.6e-6 / 1e-5, bit-equal to the training forward on every case; partial backward 1.1e-5 / 1e-4 (the
density head under colour_loss_only on 7 x 40), differing ReLU decisions 8.1e-6 / 1e-4 of a layer and 1 / 256 of a row.  f16:
forward-only x0 1.1e-8 / 1e-3, activations and outputs 9.0e-4 / 1e-2; the training plan keeps fp32 rows of e (and g2) where the
forward-only plan hands compositing fragments on 5 x 33 (mode 0), 2 x 257 and 9 x 32 (mode 3), training forward there
5.5e-4 / 1e-2, bit-equal everywhere else; partial backward, relative L2 4.4e-2 / 6e-2 (d_o under feature_loss_only on 9 x 32),
ReLU decisions 2.4e-4 / 1e-3 and 2 / 256 of a row.  A leaf or parameter block the upstreams do not reach came back an exact
zero, and no frozen field launched a weight gradient, in every mode."""
import pytest
import torch

import field_cases as fc
from test_hip_kernels import field_mode, hip  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

MODES = fc.MODES  # ["f16x3", "f32", "f16"]: every 256-wide case in each; fc.SYNTH_64 (the fp32 kernels either way) in f16x3 only
_id = lambda v: v if isinstance(v, str) else fc.label(v)


@pytest.mark.parametrize("key,field_mode", fc.FORWARD_RUNS, indirect=["field_mode"], ids=_id)
def test_forward_only_pass_against_fp64_and_the_training_forward(hip, key, field_mode):
    fc.check_forward_only(hip, fc.load(key), field_mode, torch.float64, tag=fc.label(key))


@pytest.mark.parametrize("key,field_mode", fc.DENSITY_RUNS, indirect=["field_mode"], ids=_id)
def test_density_only_pass_against_fp64(hip, key, field_mode):
    s = fc.load(key)
    assert s["c_rows"] is None and s["a_rows"] is None
    fc.check_forward_only(hip, s, field_mode, torch.float64, tag=fc.label(key))


@pytest.mark.parametrize("key,variant,field_mode", fc.BACKWARD_RUNS, indirect=["field_mode"], ids=_id)
def test_partial_backward_against_fp64(hip, key, variant, field_mode):
    fc.check_partial_backward(hip, fc.load(key), variant, field_mode, torch.float64, tag=fc.label(key))


@pytest.mark.parametrize("field_mode", ["f16"], indirect=True)
def test_f16_mode_refuses_the_smallest_pass_under_either_plan(hip, field_mode):
    """One sample of one ray: the f16 mode refuses it before any launch, with or without a gradient."""
    key = fc.SYNTH_SMALLEST
    assert "f16" not in fc.modes_of(key)
    rd, s = hip["rendering"], fc.load(key)
    for train in (False, True):
        with pytest.raises(ValueError, match="at least 32 samples"):
            rd._plan(s["model"].packer, key.R, key.S, key.mode, key.use_cand, key.use_rgb, train=train)
    with torch.no_grad(), pytest.raises(ValueError, match="at least 32 samples"):
        fc._apply(rd, s, fc._gpu_inputs(s, ()))
