"""The parity gates themselves (tests/golden_util.py): what the per-ray gate sees that the batch-wide one does not.  No GPU."""
import numpy as np

from golden_util import ray_rel_err, rel_err


def _batch(seed=0):
    rng = np.random.default_rng(seed)
    ref = rng.uniform(-1.0, 1.0, (9, 64))
    ref[4] *= 1e-4  # a ray whose values are 1e-4 of the batch maximum (behind an opaque surface, nearly transparent)
    return ref


def test_per_ray_gate_sees_an_error_on_a_small_ray():
    ref = _batch()
    got = ref.copy()
    got[4, 17] += 1e-3 * np.abs(ref[4]).max()  # 1e-3 relative to that ray, 1e-7 relative to the batch
    assert rel_err(got, ref) < 1e-6
    assert ray_rel_err(got, ref) > 1e-4
    # the floor: an error of the same absolute size on a ray whose reference is exactly zero is measured against 1e-3 of the batch
    zero = ref.copy()
    zero[4] = 0.0
    assert 1e-5 < ray_rel_err(zero + (np.arange(9) == 4)[:, None] * 1e-7, zero) < 1e-3


def test_per_ray_gate_passes_fp32_rounding():
    ref = _batch(1)
    got = ref.astype(np.float32).astype(np.float64)
    assert 0 < ray_rel_err(got, ref) < 1e-7
    assert ray_rel_err(got.reshape(9, 8, 8), ref.reshape(9, 8, 8)) == ray_rel_err(got, ref)  # any trailing shape is one ray
    assert np.isnan(ray_rel_err(np.where(ref > 0.9, np.nan, got), ref))  # a NaN never passes a `<` gate
