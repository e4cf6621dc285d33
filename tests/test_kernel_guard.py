"""The kernel choice of a context across the blocking resample calls: each of them may override it for the one call (cpm_resample's
compat route takes the per-car kernel; a fallback takes a layout that cannot overflow) and must hand it back whichever way the call
ends.  Z = 3, T = 2, 2 cars per zone, synthetic tables; the failing calls are ordinary state errors (travel times without a
datamatrix)."""
import numpy as np
import pytest

from conftest import SIM_SEED, TABLE_SEED

gpu = pytest.mark.gpu
Z, T, CPZ = 3, 2, 2
AUTO, CAR, ZONE_LDS, GROUPED = 0, 1, 2, 5
ERR_STATE = -3
KERNELS = (AUTO, ZONE_LDS, GROUPED)


def _sampler(cpm, kernel):
    s = cpm.Sampler(Z, T=T)
    s.synth_tables(TABLE_SEED)
    s.init_states(Z * CPZ, CPZ)
    s.set_kernel(kernel)
    return s


def _would_run(s):
    from carparkingmaps_amd import _lib
    return s.get_info(_lib.CPM_INFO_KERNEL)


def _ran(s):
    from carparkingmaps_amd import _lib
    return s.get_info(_lib.CPM_INFO_LAST_KERNEL)


def _side_kwargs(cpm, kind):
    return {"flows": dict(flows=True), "csr": dict(flows="csr"), "stays": dict(stays=True), "paths": dict(paths=True),
            "charge": dict(charge=cpm.ChargeParams(capacity_wh=20000, power_wh=2300, initial_wh=6000, wh_per_km=25.0)),
            "compat": dict(want_state=True)}[kind]


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_the_compat_route_overrides_the_kernel_for_its_own_call_only(cpm, kernel):
    with _sampler(cpm, kernel) as s:
        before = _would_run(s)
        assert before == (CAR if kernel == AUTO else kernel)        # (6 cars: AUTO resolves to the per-car kernel)
        got = s.resample(SIM_SEED, want_state=True)
        assert got["state"].shape == (Z * CPZ, T)
        assert _ran(s) == CAR                                       # the override was applied ...
        assert _would_run(s) == before                              # ... and is gone


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind", ["compat", "flows", "stays", "paths", "charge", "csr"])
def test_a_blocking_call_that_fails_behind_its_guard_leaves_the_kernel_choice_alone(cpm, kernel, kind):
    with _sampler(cpm, kernel) as s:
        if kind == "charge":                                        # (a distance matrix, so that the travel check is the one that fails)
            s.set_distance(np.asfortranarray(np.ones((Z, Z)) - np.eye(Z)))
        first = s.resample(SIM_SEED)
        ran_first = _ran(s)
        before = _would_run(s)
        with pytest.raises(cpm.CpmError) as err:                    # no datamatrix: refused behind the guard (and the compat override)
            s.resample(SIM_SEED, travel=True, **_side_kwargs(cpm, kind))
        assert err.value.status == ERR_STATE and "CPM_FLAG_TRAVEL needs cpm_set_datamatrix" in str(err.value)
        assert _would_run(s) == before
        again = s.resample(SIM_SEED)
        assert _ran(s) == ran_first
        assert np.array_equal(again["parking"], first["parking"]) and np.array_equal(again["driving"], first["driving"])
