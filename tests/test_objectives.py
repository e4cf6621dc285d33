"""The sweep's objectives on the device (include/cpm_objectives.h), host side: the ABI list, the host restatement of the definition
against a scalar loop and against parking_density_error, the record reader, and the Evaluator / grid_sweep switches with stubs."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from objectives_cases import LADDER_T, LADDER_Z, bound, loop_zone_errors, make_case, scalar_of

T = 24


def _declared():
    text = open(os.path.join(ROOT, "include", "cpm_objectives.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_objectives_header_declares_exactly_the_two_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared()
    assert declared == sorted(["cpm_set_measured", "cpm_objectives_dev"]) == sorted(_lib.OBJECTIVES_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS, _lib.FLOWS_CSR_SYMBOLS, _lib.STAYS_SYMBOLS, _lib.PATHS_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_objectives.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_objectives.h")).read()
    assert not re.findall(r"#define (CPM_(?:OPT|INFO)\w+)", text)         # no new option or info key


@pytest.mark.parametrize("Tc", LADDER_T)
@pytest.mark.parametrize("Z", LADDER_Z)
def test_zone_errors_equal_a_scalar_loop_bit_for_bit_and_the_scalar_is_within_the_bound(Z, Tc):
    from carparkingmaps_amd import model_selection as ms
    c = make_case(Z, Tc)
    err, valid = ms.parking_density_zone_errors(c["parking"], c["n_cars"], c["measured"])
    want, want_valid = loop_zone_errors(c["parking"], c["n_cars"], c["measured"])
    assert err.dtype == np.float64 and valid.dtype == bool and err.shape == valid.shape == (Z,)
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(err.view(np.uint64), want.view(np.uint64))
    assert np.all(err[~valid] == -1.0) and np.all(err[valid] >= 0)
    got, ref = scalar_of(err, valid), ms.parking_density_error(c["parking"], c["n_cars"], c["measured"])
    if not valid.any():
        assert math.isnan(got) and math.isnan(ref)
    else:
        rel = abs(got - ref) / abs(ref)
        print(f"Z={Z} T={Tc}: relative difference {rel:.3e}, bound {bound(Z, Tc):.3e}")
        assert rel <= bound(Z, Tc)
    if Tc == 1:
        assert not valid.any()


def test_all_flat_and_all_unmeasured_inputs_give_nan_from_both_sides():
    from carparkingmaps_amd import model_selection as ms
    c = make_case(65, T)
    flat = np.repeat(c["parking"][:, :1], T, axis=1)
    for parking, measured in ((flat, c["measured"]), (c["parking"], np.zeros((65, T)))):
        err, valid = ms.parking_density_zone_errors(parking, c["n_cars"], measured)
        assert not valid.any() and np.all(err == -1.0)
        assert math.isnan(scalar_of(err, valid)) and math.isnan(ms.parking_density_error(parking, c["n_cars"], measured))
    err, valid = ms.parking_density_zone_errors(c["parking"], c["n_cars"], None)
    assert not valid.any() and np.all(err == -1.0)


def test_objectives_from_record_reads_a_hand_made_record():
    from carparkingmaps_amd import model_selection as ms
    Tc, C = 4, 50
    pt = ms.Point(0.5, 0.1, 0.9, 2)
    driving_sum, parking_sum = [3, 9, 6, 12], [50, 50, 50, 50]
    pe = 0.123456789
    rec = np.array([0, 7 * 65536 * 3600, 5, 0] + driving_sum + parking_sum, dtype=np.int64)
    rec[3:4] = np.array([pe]).view(np.int64)
    measured_act = np.array([0.0, 0.5, 0.25, 1.0])
    out = ms.objectives_from_record(rec, pt, C, Tc, measured_act)
    assert set(out) == {"e_drive", "p_min", "p_max", "e_dest", "A_drive", "traffic_activity", "activity_error", "parking_error",
                        "driving_total", "hours_hold_all_cars"}
    assert (out["e_drive"], out["p_min"], out["p_max"], out["e_dest"]) == (0.5, 0.1, 0.9, 2.0)
    assert out["A_drive"] == ms.a_drive(7 * 65536 * 3600, C, Tc)
    assert out["parking_error"] == pe
    assert out["driving_total"] == 30 and out["hours_hold_all_cars"] is True
    # bit-equal to the host path on any (Z, T) array with these column sums
    driving = np.array([[1, 4, 6, 2], [2, 5, 0, 10]], dtype=np.int64)
    assert np.array_equal(out["traffic_activity"], ms.traffic_activity(driving))
    assert out["activity_error"] == ms.traffic_activity_error(ms.traffic_activity(driving), measured_act)
    rec[4 + Tc + 2] = 49
    out = ms.objectives_from_record(rec, pt, C, Tc, with_parking_error=False)
    assert out["hours_hold_all_cars"] is False and "parking_error" not in out and "activity_error" not in out
    rec[3] = 0x7ff8000000000000
    assert math.isnan(ms.objectives_from_record(rec, pt, C, Tc)["parking_error"])


class _StubSampler:
    """What Evaluator.evaluate needs of a Sampler, without a device (no set_measured: the host path must not ask for it)."""
    Z, T = 6, T

    def __init__(self):
        rng = np.random.default_rng(11)
        self.parking = np.asfortranarray(rng.integers(50, 150, size=(self.Z, self.T)).astype(np.int64))
        self.driving = np.asfortranarray(rng.integers(0, 60, size=(self.Z, self.T)).astype(np.int64))
        self.calls = []

    def build_p_drive(self, *a, **k):
        self.calls.append("p_drive")

    def build_p_dest(self, *a, **k):
        self.calls.append("p_dest")

    def resample(self, seed, travel=False):
        self.calls.append("resample")
        return dict(parking=self.parking, driving=self.driving, sum_tt_q16=123456789)


def test_evaluator_without_the_flag_keeps_its_fields_and_results():
    from carparkingmaps_amd import model_selection as ms
    import dataclasses
    names = [f.name for f in dataclasses.fields(ms.Evaluator)]
    assert names[:7] == ["sampler", "C", "seed", "measured_activity", "measured_parking", "travel", "fallbacks"]
    assert {f.name: f.default for f in dataclasses.fields(ms.Evaluator)}["device_objectives"] is False
    rng = np.random.default_rng(12)
    s = _StubSampler()
    act, park = rng.uniform(0, 1, T), rng.uniform(0, 1, (s.Z, T))
    ev = ms.Evaluator(s, 600, 1, act, park, travel=True)
    assert ev.device_objectives is False and ev.fallbacks == 0
    pt = ms.Point(0.5, 0.1, 0.9, 2)
    out = ev.evaluate(pt)
    assert s.calls == ["p_drive", "p_dest", "resample"]
    assert set(out) == {"e_drive", "p_min", "p_max", "e_dest", "A_drive", "traffic_activity", "parking", "driving", "activity_error",
                        "parking_error"}
    assert out["parking"] is s.parking and out["driving"] is s.driving
    assert out["A_drive"] == ms.a_drive(123456789, 600, T)
    assert out["activity_error"] == ms.traffic_activity_error(ms.traffic_activity(s.driving), act)
    assert out["parking_error"] == ms.parking_density_error(s.parking, 600, park)


def test_evaluator_with_the_flag_installs_the_measured_densities_once():
    from carparkingmaps_amd import model_selection as ms

    class Stub(_StubSampler):
        def set_measured(self, m):
            self.calls.append(("set_measured", None if m is None else np.array(m)))

    s = Stub()
    park = np.random.default_rng(13).uniform(0, 1, (s.Z, T))
    ms.Evaluator(s, 600, 1, None, park, device_objectives=True)
    assert len(s.calls) == 1 and s.calls[0][0] == "set_measured" and np.array_equal(s.calls[0][1], park)
    s = Stub()
    ms.Evaluator(s, 600, 1, device_objectives=True)
    assert s.calls == [("set_measured", None)]


class _RecordLane:
    """A lane whose results hold no count arrays, as an Evaluator with device_objectives returns them."""
    C = 10

    def __init__(self, device_objectives=True):
        self.device_objectives = device_objectives

    def begin(self, pt, slot):
        pass

    def finish(self, pt, slot):
        return {"e_drive": pt.e_drive, "A_drive": 0.5, "traffic_activity": np.zeros(T), "driving_total": int(pt.e_drive) + 7,
                "hours_hold_all_cars": pt.e_drive != 2.0}

    def begin_batch(self, pts, slot):
        pass

    def finish_batch(self, pts, slot):
        return [self.finish(pt, slot) for pt in pts]


@pytest.mark.parametrize("batch", [None, 2])
def test_grid_sweep_takes_the_two_figures_from_the_dict_when_the_arrays_are_absent(batch):
    from carparkingmaps_amd import model_selection as ms
    grid = [ms.Point(float(i), 0.1, 0.9, 2) for i in range(5)]
    res = ms.grid_sweep(_RecordLane(), grid, batch=batch)
    assert [r["driving_total"] for r in res] == [7, 8, 9, 10, 11]
    assert [r["hours_hold_all_cars"] for r in res] == [True, True, False, True, True]
    assert all(r["fallback"] is False and "traffic_activity" not in r for r in res)


def test_checksums_together_with_device_objectives_raise():
    from carparkingmaps_amd import model_selection as ms
    grid = [ms.Point(1.0, 0.1, 0.9, 2)]
    with pytest.raises(ValueError, match="checksums"):
        ms.grid_sweep(_RecordLane(), grid, checksums=True)
    with pytest.raises(ValueError, match="checksums"):
        ms.grid_sweep([_RecordLane(False), _RecordLane(True)], grid, checksums=True)
