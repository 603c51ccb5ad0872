"""tests/raster_units_ref.py on the CPU: every scene meets the conditions and its regime, the one-pixel runs of the fp64 oracle
sum to its full run, the units are positive wherever a value is not zero, and the fp32 oracle stays inside UNITS_LITERAL on
every image value and every gradient entry, nothing left out (the record that the plain fp32 statement of the algorithm alone
meets the condition the kernels are held to, at half their bound).  The measured tables are in the docstring of
tests/test_raster_units_gpu.py."""
import numpy as np
import pytest

import raster_units_ref as ru


@pytest.mark.parametrize("name", ru.SCENES)
def test_scene_meets_the_conditions_and_its_regime(name):
    sc = ru.scene(name)
    ru.assert_conditions(sc)
    print(f"[raster-units] {name}: {len(sc.g['means3D'])} Gaussians, {sc.redraws} redrawn; {sc.regime(sc)}")
    again = ru._BUILDERS[name]()                     # a pure function of the seed
    for k in sc.g:
        assert np.array_equal(sc.g[k], again.g[k]), k


@pytest.mark.parametrize("name", ru.SCENES)
def test_units_are_positive_and_the_one_pixel_runs_sum_up(name, oracle64):
    sc = ru.scene(name)
    ref = ru.reference(oracle64, sc)                 # (asserts the sum of the one-pixel runs)
    ru.assert_units_positive(ref.image, ref.units["image"], "image")
    for k in ru.GRADS:
        ru.assert_units_positive(ref.grads[k], ref.units[k], k)
        dead = ref.radii <= 0
        assert (ref.units[k][dead] == 0).all(), k
    assert (ref.units["dL_dmeans2D"][:, 2] == 0).all()
    assert (ref.absgrad >= np.abs(ref.grads["dL_dmeans2D"][:, :2])).all()
    w = ru.walk64(sc.cam, sc.g)
    blended = w.contrib.any((1, 2))
    # the restatement and the oracle agree on which Gaussians are blended at all: their rows, and only theirs, have units
    for k in ("dL_dcolors", "dL_dopacities"):
        has = (ref.units[k].reshape(len(blended), -1) > 0).any(1)
        assert np.array_equal(has, blended), k
    assert np.allclose(w.final_T, ref.final_T, rtol=1e-9, atol=0)


def measure_literal(name, oracle32, oracle64):
    """{tensor: the fp32 oracle's largest error in units} on a scene; unit-0 entries must be exactly 0 (asserted)."""
    sc = ru.scene(name)
    ref = ru.reference(oracle64, sc)
    full, M, _ = ru.per_pixel(oracle32, sc, ref.w)
    assert np.array_equal(full["radii"], ref.radii)
    got = {k: full[k] for k in ru.GRADS}
    got["image"] = full["color"]
    got["absgrad"] = M["dL_dmeans2D"][:, :2]
    return ru.compare(ref, got, ru.TENSORS)


@pytest.mark.parametrize("name", ru.SCENES)
def test_the_fp32_oracle_stays_within_the_literal(name, oracle32, oracle64):
    measured = measure_literal(name, oracle32, oracle64)
    print(f"[raster-units] {name} fp32 oracle, units (rounded up): " +
          ", ".join(f"{k} {v:.3g} ({ru.round_up_2(v):g})" for k, v in measured.items()))
    for k, v in measured.items():
        lit = ru.UNITS_LITERAL[name][k]
        assert v <= lit <= 1.25 * v, (name, k, v, lit)
        assert ru.UNITS_KERNEL[name][k] == 2 * lit
