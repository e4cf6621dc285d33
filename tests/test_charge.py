"""EV state of charge, hourly charging load per zone and uncovered trips from the fused resample (include/cpm_charge.h,
csrc/cpm_charge.h).

Expected values come from the oracle only: tests/side_reference.reference runs O.initializestates -> O.solveinitialvalueproblem ->
O.resampling with a datamatrix, so that column 4 of the transition matrix holds the drawn distances, and
tests/charge_reference.charge_of, a numpy restatement of the definition, turns the matrices into the four arrays.  Every comparison is
exact.  Before anything is compared, the census of the reference must show every one of the six branches of the recurrence on at least
2 % of the car-hours: a parity test cannot pass on a day that skips a branch.
GPU tests are marked `gpu` and wrap every step in `pinned`; the host-only tests at the end run without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import charge_reference as CR
import side_reference as SR
from conftest import ROOT, SIM_SEED, TABLE_SEED
from product_form import CAR, GROUPED, MODE_FORM, ZONE_LDS, pinned

gpu = pytest.mark.gpu
T24 = 24
ZONE_POWER = (0, 2300, 3700, 11000)


def _params(Z, C, kind, capacity=20000, wh_per_km=25.0, initial=6000, power_div=1):
    """the standard parameters; kind "scalar": every car starts with `initial`, "array": soc_in[i] = (i * 2654435761) mod 24001,
    whose values above the capacity exercise the clamp"""
    p = dict(capacity_wh=capacity, power_wh=0, initial_wh=initial, wh_per_km=wh_per_km,
             zone_power_wh=np.array([ZONE_POWER[z % 4] // power_div for z in range(Z)], dtype=np.uint32), soc_in=None)
    if kind == "array":
        p["soc_in"] = ((np.arange(C, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(24001)).astype(np.uint32)
    return p


_REFS = {}
_SHAPES = {"dense192": (192, 120, T24), "long": (192, 120, T24), "t7": (67, 40, 7), "z67": (67, 40, T24), "z67x8": (67, 8, T24), "heavy": (64, 300, T24)}


def _ref(O, case):
    """The oracle's day of a named case with drawn distances, computed once and shared (read-only): what side_reference.reference
    returns + dist."""
    if case in _REFS:
        return _REFS[case]
    if case == "diag":      # tests/test_gpu_parity.py's random tables 3: many all-zero p_dest rows, so many trips inside a zone
        tb = SR.random_tables(3, T=T24)
        Z, cpz, T, p_drive, p_dest = tb["Z"], tb["cpz"], tb["T"], tb["p_drive"], tb["p_dest"]
        rng = np.random.default_rng(77)
        dist = O.distance_matrix(-37.8 + 0.3 * rng.random(Z), 144.9 + 0.4 * rng.random(Z))
        dm = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.3)[0]
    else:
        Z, cpz, T = _SHAPES[case]
        p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
        p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
        dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.3)
        if case == "long":
            p_drive[20:24, 3:7] = 0.0
            p_drive[30, :] = 1.0
            p_drive[10, 21:] = 0.0
        if case == "heavy":  # every origin sends 0.4 of its drivers to zone 6: more than 128 of one zone's drivers in one run
            p_dest[:] = 0.6 / (Z - 1)
            p_dest[:, 5, :] = 0.4
    ref = SR.reference(O, p_drive, p_dest, Z, cpz, T, SIM_SEED, dm=dm, dist=dist)
    dist.setflags(write=False)
    dm.setflags(write=False)
    ref.update(dist=dist, dm=dm, want={})
    _REFS[case] = ref
    return ref


def _want(ref, kind, threshold=0.02, **kw):
    """(params, the arrays charge_of gives for them) of a reference, once per kind; the census is asserted first"""
    key = (kind, tuple(sorted(kw.items())))
    if key not in ref["want"]:
        Z, C = ref["Z"], ref["Z"] * ref["cpz"]
        p = _params(Z, C, kind, **kw)
        shares = CR.census(ref["state"], ref["trans"], Z, p)
        print(f"census Z = {Z} x {ref['cpz']}, T = {ref['T']}, {kind}: " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in shares.items()))
        assert sorted(shares) == sorted(CR.BRANCHES) and min(shares.values()) >= threshold, shares
        want = CR.charge_of(ref["state"], ref["trans"], Z, p)
        CR.check_identities(want, ref["parking"], ref["driving"], p, Z)
        for v in want.values():
            v.setflags(write=False)
        ref["want"][key] = (p, want)
    return ref["want"][key]


def _sampler(cpm, ref, travel=False, **kw):
    s = cpm.Sampler(ref["Z"], ref["T"], **kw)
    s.set_p_drive(ref["p_drive"])
    s.set_p_dest(ref["p_dest"])
    if travel:
        s.set_datamatrix(ref["dm"], ref["dist"])
    else:
        s.set_distance(ref["dist"])      # (no datamatrix, no travel flag: the distance matrix alone)
    return s


def _same_counts(a, b):
    return np.array_equal(a["parking"], b["parking"]) and np.array_equal(a["driving"], b["driving"])


def _check(r, ref, want, where=None, cars=slice(None)):
    """shape, dtype and order; exact equality of the four arrays with the reference's; the identities against the counts of the
    same call"""
    Z, T = ref["Z"], ref["T"]
    for k, dt in (("charge", np.int64), ("used", np.int64), ("short", np.int32)):
        a = r[k]
        assert isinstance(a, np.ndarray) and a.shape == (Z, T) and a.dtype == dt and a.flags["C_CONTIGUOUS"], (where, k)
    assert r["soc"].dtype == np.uint32 and r["soc"].shape == want["soc"].shape, where
    if cars == slice(None):
        assert _same_counts(r, ref), where
    for k in ("short", "used", "charge", "soc"):
        assert np.array_equal(r[k], want[k]), (where, k, int((r[k] != want[k]).sum()))
    assert (r["short"] <= r["driving"]).all(), where
    assert int(want["e0"].sum()) + int(r["charge"].sum()) - int(r["used"].sum()) == int(r["soc"].astype(np.int64).sum()), where


def _both(s, O, ref, where=None, threshold=0.02, **pin):
    """resample(charge=...) for both initial states, each pinned"""
    for kind in ("scalar", "array"):
        p, want = _want(ref, kind, threshold)
        with pinned(s, **pin):
            r = s.resample(SIM_SEED, charge=p)
        _check(r, ref, want, (where, kind))


# ------------------------------------------------------------------------------------------------ 7: the test that fails without the feature
@gpu
def test_charge_of_all_hours_equals_the_reference_in_every_hour_form(cpm, O):
    """Z = 192 x 120, dense synthetic tables, AUTO: the grouped family, no repeat; all four arrays, both initial states.  Then the same
    under CPM_OPT_FUSED 0, 1, 3 and 6 (6 keeps the runs of all hours: T launches in hour order at the end).  Counts equal a plain
    resample's, and a plain resample afterwards is unchanged.  Without the feature the library has no cpm_resample_charge."""
    ref = _ref(O, "dense192")
    Z, cpz = ref["Z"], ref["cpz"]
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED):
            plain = s.resample(SIM_SEED)
        assert "charge" not in plain and _same_counts(plain, ref)
        _both(s, O, ref, "auto", kernel=0, family=GROUPED)
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 0           # (hour T ran in its run-producing form)
        for mode in (0, 1, 3, 6):
            s.set_fused(mode)
            if mode != 0 and s.get_info(cpm.CPM_INFO_FUSED) != MODE_FORM[mode]:      # (as tests/test_stays.py: a form the shape has no instantiation for)
                print(f"Z = {Z}: no instantiation for fused mode {mode} (CPM_INFO_FUSED {s.get_info(cpm.CPM_INFO_FUSED)})")
                continue
            _both(s, O, ref, mode, kernel=0, family=GROUPED, fused=mode)
        s.set_fused(5)
        with pinned(s, 0, family=GROUPED):
            assert _same_counts(s.resample(SIM_SEED), plain)


# ------------------------------------------------------------------------------------------------ 8: rows off the 16-byte grid, the other families
@gpu
@pytest.mark.parametrize("case", ["t7", "z67"])
def test_rows_of_seven_and_of_24_hours_on_the_grouped_family(cpm, O, case):
    """Z = 67 x 40 at T = 7 (int32 rows of 7 words are off the 16-byte grid) and at T = 24."""
    ref = _ref(O, case)
    Z, cpz = ref["Z"], ref["cpz"]
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _both(s, O, ref, case, kernel=0, family=GROUPED, repeats=0)


@gpu
@pytest.mark.parametrize("kernel", [ZONE_LDS, CAR])
def test_the_exact_layout_and_the_per_car_kernel(cpm, O, kernel):
    ref = _ref(O, "z67")
    Z, cpz = ref["Z"], ref["cpz"]
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        s.set_kernel(kernel)
        with pinned(s, kernel):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _both(s, O, ref, kernel, kernel=kernel, repeats=0)


@gpu
def test_a_small_fleet_under_auto_takes_the_per_car_kernel(cpm, O):
    """8 cars per zone: AUTO picks CPM_KERNEL_CAR."""
    ref = _ref(O, "z67x8")
    Z, cpz = ref["Z"], ref["cpz"]
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=CAR):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _both(s, O, ref, "small", kernel=0, family=CAR, repeats=0)


# ------------------------------------------------------------------------------------------------ 9: long stays
@gpu
def test_long_stays_hold_full_rate_hours_a_remainder_hour_and_empty_hours(cpm, O):
    """The `long` day of tests/test_stays.py: zones 21 .. 24 hold their cars for four hours, zone 31 sends every car on at once, zone
    11 keeps what arrives in the last three hours.  A 2,300 Wh charger fills 14,000 Wh in seven hours: full-rate hours, the
    remainder hour and the empty hours behind it all occur inside one stay, which the reference must show."""
    ref = _ref(O, "long")
    Z, cpz = ref["Z"], ref["cpz"]
    p, want = _want(ref, "scalar")
    lazy = CR.charge_lazy(ref["state"], ref["trans"], Z, p)
    assert lazy["three_phase_stays"] > 0 and CR.same(lazy, want)
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _both(s, O, ref, "long", kernel=0, family=GROUPED, repeats=0)


# ------------------------------------------------------------------------------------------------ 10: trips inside a zone
@gpu
def test_trips_inside_a_zone_cost_one_kilometre(cpm, O):
    """Random tables 3 of tests/side_reference.py at T = 24 (Z = 45 x 40: about a third of the trips lie on the diagonal) with the
    distance matrix of random centroids; capacity 3000, 60 Wh per km, initial 1500, a tenth of the standard powers.  The census
    threshold is 0.5 % per branch here.  The family falls where AUTO puts it."""
    ref = _ref(O, "diag")
    Z, cpz = ref["Z"], ref["cpz"]
    drove = ref["trans"][:, :, 0] == 1
    inside = drove & (ref["trans"][:, :, 1] == ref["state"])
    assert inside.sum() > 0.2 * drove.sum() and (ref["trans"][:, :, 3][inside] == 1.0).all()
    print(f"Z = {Z} x {cpz}: {int(inside.sum())} of {int(drove.sum())} trips inside a zone")
    kw = dict(capacity=3000, wh_per_km=60.0, initial=1500, power_div=10)
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        for kind in ("scalar", "array"):
            key = (kind, tuple(sorted(kw.items())))
            if key not in ref["want"]:
                p = _params(Z, Z * cpz, kind, **kw)
                shares = CR.census(ref["state"], ref["trans"], Z, p)
                print(f"census {kind}: " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in shares.items()))
                assert min(shares.values()) >= 0.005, shares
                ref["want"][key] = (p, CR.charge_of(ref["state"], ref["trans"], Z, p))
            p, want = ref["want"][key]
            with pinned(s, 0, repeats=None) as step:
                r = s.resample(SIM_SEED, charge=p)
            print(f"trips inside a zone, {kind}: the step ended on {step}")
            _check(r, ref, want, kind)


# ------------------------------------------------------------------------------------------------ 11: long runs, heavy buckets, a repaired step
@gpu
def test_one_popular_destination_long_runs_and_a_repaired_step(cpm, O):
    """Z = 64 x 300, every p_dest row puts 0.4 on zone 6 (0.9 leaves under 2 % of the car-hours for two of the six branches): an
    origin sends more than 128 drivers to one destination group in one hour (a second pass of the reader), zone 6 becomes a heavy
    bucket and may outgrow its region.  Whichever attempt counted, the arrays
    are the reference's; then again with no repeat, on the grown regions."""
    ref = _ref(O, "heavy")
    Z, cpz = ref["Z"], ref["cpz"]
    f = ref["flows"]
    assert f[:, :, 5].max() > 128 and ref["parking"][5].max() > 4 * cpz
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        s.set_state(ref["zone0"])
        for kind in ("scalar", "array"):
            p, want = _want(ref, kind)
            r = s.resample(SIM_SEED, charge=p)        # (not pinned: a repair may end on the exact layout)
            print(f"popular destination, {kind}: the step ended on {s.last_step()}")
            _check(r, ref, want, kind)
        fam = s.get_info(cpm.CPM_INFO_LAST_KERNEL)
        _both(s, O, ref, "again", kernel=0, family=fam, repeats=0)


# ------------------------------------------------------------------------------------------------ 12: with travel times
@gpu
def test_charge_of_a_travel_resample(cpm, O):
    """A travel resample keeps the runs of all hours (T launches in hour order at the end).  The arrays equal the non-travel ones and
    the travel-time sum the oracle's."""
    ref = _ref(O, "z67")
    Z, cpz = ref["Z"], ref["cpz"]
    p, want = _want(ref, "array")
    with _sampler(cpm, ref, travel=True) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None):
            plain = s.resample(SIM_SEED, travel=True)
        assert plain["sum_tt_q16"] == ref["sum_tt_q16"] != 0
        with pinned(s, 0, family=GROUPED, repeats=0):
            r = s.resample(SIM_SEED, travel=True, charge=p)
        assert r["sum_tt_q16"] == ref["sum_tt_q16"]
        _check(r, ref, want, "travel")
        with pinned(s, 0, family=GROUPED, repeats=0):
            r0 = s.resample(SIM_SEED, charge=p)
        assert r0["sum_tt_q16"] == 0 and CR.same(r0, r)
        _check(r0, ref, want, "no travel")


# ------------------------------------------------------------------------------------------------ 13: shards
@gpu
def test_two_strided_shards_sum_to_the_whole_fleet(cpm, O):
    ref = _ref(O, "dense192")
    Z, cpz, T = ref["Z"], ref["cpz"], ref["T"]
    C = Z * cpz
    p, whole = _want(ref, "array")
    total = {k: np.zeros((Z, T), dtype=np.int64) for k in ("charge", "used", "short")}
    soc = np.zeros(C, dtype=np.uint32)
    for first in (0, 1):
        cars = slice(first, None, 2)
        want = CR.charge_of(ref["state"], ref["trans"], Z, p, cars)       # (a shard against the reference as well: its cars alone)
        with _sampler(cpm, ref) as s:
            s.init_states(C, cpz, first, car_stride=2)
            assert s.car_count == C // 2
            with pinned(s, 0, family=GROUPED):
                assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"][cars])
            with pinned(s, 0, family=GROUPED):
                r = s.resample(SIM_SEED, charge=dict(p, soc_in=p["soc_in"][cars]))
            _check(r, ref, want, first, cars)
            for k in total:
                total[k] += r[k]
            soc[cars] = r["soc"]
    for k in total:
        assert np.array_equal(total[k], whole[k]), k
    assert np.array_equal(soc, whole["soc"])


# ------------------------------------------------------------------------------------------------ 14: the device-resident form
@gpu
def test_device_resident_charge_on_a_callers_stream(cpm, O):
    """Into torch tensors filled with a sentinel, guard words either side of every array: every word is overwritten, the status word
    is 0, nothing around the arrays moved."""
    import torch
    ref = _ref(O, "dense192")
    Z, cpz, T = ref["Z"], ref["cpz"], ref["T"]
    n, G = Z * cpz, 64
    p, want = _want(ref, "array")
    stream = torch.cuda.Stream()
    with _sampler(cpm, ref, stream=stream) as s:
        s.init_states(n, cpz)
        with pinned(s, 0, family=GROUPED):
            s.solve_ivp(SIM_SEED, want=False)
        d_counts = torch.full((s.counts_words(),), -1, dtype=torch.int64, device="cuda")
        bufs = {k: torch.full((words + 2 * G,), -7, dtype=dt, device="cuda")
                for k, words, dt in (("charge", Z * T, torch.int64), ("used", Z * T, torch.int64), ("short", Z * T, torch.int32), ("soc", n, torch.int32))}
        ptr = {k: b.data_ptr() + G * b.element_size() for k, b in bufs.items()}
        d_zp = torch.from_numpy(p["zone_power_wh"].astype(np.int32)).cuda()
        d_si = torch.from_numpy(p["soc_in"].view(np.int32)).cuda()
        scal = dict(capacity_wh=p["capacity_wh"], power_wh=p["power_wh"], initial_wh=p["initial_wh"], wh_per_km=p["wh_per_km"])
        with pinned(s, 0, family=GROUPED):
            with torch.cuda.stream(stream):
                s.resample_charge_dev(SIM_SEED, d_counts.data_ptr(), ptr["charge"], ptr["used"], ptr["short"], ptr["soc"], d_zone_power_ptr=d_zp.data_ptr(),
                                      d_soc_in_ptr=d_si.data_ptr(), **scal)
            stream.synchronize()
        counts = d_counts.cpu().numpy()
        assert counts[-1] == 0
        host = {k: b.cpu().numpy() for k, b in bufs.items()}
        for k, a in host.items():
            assert (a[:G] == -7).all() and (a[-G:] == -7).all(), k           # nothing around the arrays moved
        dev = dict(parking=counts[:Z * T].reshape(T, Z).T, driving=counts[Z * T:2 * Z * T].reshape(T, Z).T,
                   charge=np.ascontiguousarray(host["charge"][G:-G].reshape(Z, T)), used=np.ascontiguousarray(host["used"][G:-G].reshape(Z, T)),
                   short=np.ascontiguousarray(host["short"][G:-G].reshape(Z, T)), soc=np.ascontiguousarray(host["soc"][G:-G]).view(np.uint32))
        _check(dev, ref, want, "dev")                                        # (equal to the reference: every word was overwritten)
        with pinned(s, 0, family=GROUPED):                                   # soc may be NULL
            with torch.cuda.stream(stream):
                s.resample_charge_dev(SIM_SEED, d_counts.data_ptr(), ptr["charge"], ptr["used"], ptr["short"], 0, d_zone_power_ptr=d_zp.data_ptr(),
                                      d_soc_in_ptr=d_si.data_ptr(), **scal)
            stream.synchronize()
        assert np.array_equal(bufs["charge"].cpu().numpy()[G:-G].reshape(Z, T), want["charge"])
        for k in ("charge", "used", "short"):
            args = dict(ptr, **{k: 0})
            with pytest.raises(cpm.CpmError) as err:                         # a NULL array is an argument error
                s.resample_charge_dev(SIM_SEED, d_counts.data_ptr(), args["charge"], args["used"], args["short"], args["soc"], **scal)
            assert err.value.status == -1


# ------------------------------------------------------------------------------------------------ 15: error paths
@gpu
def test_error_paths_return_their_code_with_a_message(cpm, O):
    from carparkingmaps_amd import _lib
    ref = _ref(O, "z67x8")
    Z, cpz, T = ref["Z"], ref["cpz"], ref["T"]
    L = _lib.load()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pk = np.zeros((Z, T), dtype=np.int64, order="F")
    dr = np.zeros((Z, T), dtype=np.int64, order="F")
    P = lambda **kw: ctypes.byref(_lib.ChargeParamsC(**dict(dict(capacity_wh=20000, power_wh=2300, initial_wh=6000, wh_per_km=25.0), **kw)))
    with cpm.Sampler(Z, T) as s:                                             # no distance matrix
        s.set_p_drive(ref["p_drive"])
        s.set_p_dest(ref["p_dest"])
        s.init_states(Z * cpz, cpz)
        ch, us, sh = s.charge_empty(), s.used_empty(), s.short_empty()
        assert L.cpm_resample_charge(s._h, SIM_SEED, 0, P(), vp(pk), vp(dr), None, vp(ch), vp(us), vp(sh), None) == -3
        assert b"distance matrix" in L.cpm_last_error()
    with _sampler(cpm, ref) as s:
        s.init_states(Z * cpz, cpz)
        s.set_state(ref["zone0"])
        ch, us, sh = s.charge_empty(), s.used_empty(), s.short_empty()
        call = lambda params, c=ch, u=us, h=sh: L.cpm_resample_charge(s._h, SIM_SEED, 0, params, vp(pk), vp(dr), None, c if c is None else vp(c),
                                                                      u if u is None else vp(u), h if h is None else vp(h), None)
        assert call(None) == -1 and b"params" in L.cpm_last_error()
        assert call(P(), c=None) == -1 and b"charge_out" in L.cpm_last_error()
        assert call(P(), u=None) == -1 and b"used_out" in L.cpm_last_error()
        assert call(P(), h=None) == -1 and b"short_out" in L.cpm_last_error()
        assert call(P(initial_wh=20001)) == -1 and b"initial_wh" in L.cpm_last_error()
        assert call(P(capacity_wh=0, initial_wh=0)) == -1 and b"capacity_wh" in L.cpm_last_error()
        for bad in (-1.0, float("nan"), float("inf")):
            assert call(P(wh_per_km=bad)) == -1 and b"wh_per_km" in L.cpm_last_error()
        p, want = _want(ref, "scalar")
        with pinned(s, 0, family=CAR):                                       # (the context still works; soc_out = NULL is accepted)
            zp = p["zone_power_wh"]
            assert call(P(zone_power_wh=zp.ctypes.data)) == 0
        assert np.array_equal(ch, want["charge"]) and np.array_equal(us, want["used"]) and np.array_equal(sh, want["short"])
    with cpm.Sampler(4, 256) as s:                                           # the hour of the last drive is kept in 8 bits
        s.set_distance(np.ones((4, 4)))
        a64, a32 = np.zeros(4 * 256, dtype=np.int64), np.zeros(4 * 256, dtype=np.int32)
        assert L.cpm_resample_charge(s._h, SIM_SEED, 0, P(), vp(a64), vp(a64), None, vp(a64), vp(a64), vp(a32), None) == -1
        assert b"T = 256" in L.cpm_last_error()


# ------------------------------------------------------------------------------------------------ host only
# Ten cars, Z = 3, T = 4, written out by hand (the trajectories of tests/test_stays.py): (zone in hours 0 .. 3, drove in hours 0 .. 3,
# (destination, km) of each drive, initial Wh).  capacity 100 Wh, 4 Wh per km, chargers: zone 1 none, zone 2 30 Wh, zone 3 20 Wh.
_NAN = float("nan")
_HAND = [
    ((1, 1, 1, 1), (0, 0, 0, 0), (), 50),                                       # 0 never drives, no charger: 50
    ((1, 2, 2, 2), (1, 0, 0, 0), ((2, 5.125),), 50),                            # 1 20.5 -> 20 Wh (half to even): 30; zone 2 gives 30, 30, 10: 100
    ((2, 2, 2, 2), (0, 1, 0, 1), ((2, 1.0), (3, 17.5)), 50),                    # 2 +30: 80; inside the zone, 1 km: 76; +24 (the remainder): 100; -70: 30
    ((1, 2, 3, 1), (1, 1, 1, 1), ((2, 3.75), (3, 6.25), (1, 7.5), (2, _NAN)), 50),  # 3 -15: 35; -25: 10; 30 > 10, short: 0; NaN costs nothing: 0
    ((3, 3, 3, 1), (0, 0, 1, 0), ((1, 10.0),), 95),                             # 4 +5 (the remainder at once), then full; -40: 60; no charger: 60
    ((3, 3, 3, 2), (1, 0, 1, 0), ((3, 1.0), (2, 0.875)), 50),                   # 5 -4: 46; +20: 66; 3.5 -> 4 Wh: 62; +30: 92
    ((2, 2, 2, 2), (0, 0, 0, 0), (), 120),                                      # 6 clamped to 100, full all day
    ((1, 1, 1, 1), (0, 0, 0, 1), ((2, 15.0),), 50),                             # 7 60 > 50, short: 0
    ((2, 2, 1, 1), (0, 1, 0, 0), ((1, 0.625),), 50),                            # 8 +30: 80; 2.5 -> 2 Wh: 78; no charger: 78
    ((1, 3, 1, 1), (1, 1, 0, 0), ((3, 1.25), (1, 1.0)), 8),                     # 9 -5: 3; 4 > 3, short: 0
]
_HAND_PARAMS = dict(capacity_wh=100, power_wh=7, initial_wh=0, wh_per_km=4.0, zone_power_wh=np.array([0, 30, 20], dtype=np.uint32),
                    soc_in=np.array([c[3] for c in _HAND], dtype=np.uint32))
_HAND_CHARGE = {(1, 0): 60, (1, 1): 30, (1, 2): 54, (1, 3): 40, (2, 0): 5, (2, 1): 20}        # (z, t): Wh
_HAND_USED = {(0, 0): 40, (0, 3): 50, (1, 1): 31, (1, 3): 70, (2, 0): 4, (2, 1): 3, (2, 2): 54}
_HAND_SHORT = {(2, 2): 1, (0, 3): 1, (2, 1): 1}
_HAND_SOC = [50, 100, 30, 0, 60, 92, 100, 0, 78, 0]


def _hand_matrices():
    st = np.array([c[0] for c in _HAND], dtype=np.int64)
    tr = np.zeros((10, 4, 4), dtype=np.float64)
    for i, (zones, drove, trips, _) in enumerate(_HAND):
        it = iter(trips)
        for t in range(4):
            tr[i, t, 0] = drove[t]
            tr[i, t, 1], tr[i, t, 3] = next(it) if drove[t] else (zones[t], 0.0)
            if t < 3:
                assert zones[t + 1] == tr[i, t, 1]
    return st, tr


def test_both_restatements_on_ten_cars_written_out_by_hand():
    st, tr = _hand_matrices()
    want = dict(charge=np.zeros((3, 4), dtype=np.int64), used=np.zeros((3, 4), dtype=np.int64), short=np.zeros((3, 4), dtype=np.int32),
                soc=np.array(_HAND_SOC, dtype=np.uint32))
    for name, cells in (("charge", _HAND_CHARGE), ("used", _HAND_USED), ("short", _HAND_SHORT)):
        for k, v in cells.items():
            want[name][k] = v
    for f in (CR.charge_of, CR.charge_lazy):
        got = f(st, tr, 3, _HAND_PARAMS)
        assert CR.same(got, want), f.__name__
        assert got["e0"].tolist() == [50, 50, 50, 50, 95, 50, 100, 50, 50, 8]
        assert got["e0"].sum() + got["charge"].sum() - got["used"].sum() == got["soc"].astype(np.int64).sum() == 510
        # the even and the odd cars alone add up to the fleet
        parts = [f(st, tr, 3, _HAND_PARAMS, slice(k, None, 2)) for k in (0, 1)]
        for k in ("charge", "used", "short"):
            assert np.array_equal(parts[0][k] + parts[1][k], want[k])
        assert np.array_equal(parts[0]["soc"], want["soc"][0::2]) and np.array_equal(parts[1]["soc"], want["soc"][1::2])
    # without soc_in and zone_power_wh: one charge and one power for all
    flat = dict(_HAND_PARAMS, soc_in=None, zone_power_wh=None, initial_wh=100, power_wh=7)
    a, b = CR.charge_of(st, tr, 3, flat), CR.charge_lazy(st, tr, 3, flat)
    assert CR.same(a, b) and a["e0"].tolist() == [100] * 10 and a["charge"][1, 1] == 7     # (car 1 alone charges in zone 2 in hour 1: 20 Wh short of full)
    shares = CR.census(st, tr, 3, _HAND_PARAMS)
    assert {k: round(v * 40) for k, v in shares.items()} == dict(short=3, covered=11, full_rate=6, remainder=3, full=5, no_charger=12)


@pytest.mark.parametrize("kind", ["scalar", "array"])
def test_the_two_restatements_agree_on_the_oracles_day(O, kind):
    """Z = 67 x 40, T = 24; the census and the three identities on the reference (in _want) first."""
    ref = _ref(O, "z67")
    p, want = _want(ref, kind)
    lazy = CR.charge_lazy(ref["state"], ref["trans"], ref["Z"], p)
    assert CR.same(lazy, want) and np.array_equal(lazy["e0"], want["e0"])
    if kind == "array":
        assert (p["soc_in"] > p["capacity_wh"]).any() and want["e0"].max() == p["capacity_wh"]      # (the clamp is exercised)


def test_the_identities_hold_on_the_reference_at_seven_hours(O):
    ref = _ref(O, "t7")
    for kind in ("scalar", "array"):
        p, want = _want(ref, kind)                                          # (check_identities runs in _want)
        assert want["charge"].sum() > 0 and want["used"].sum() > 0 and want["short"].sum() > 0
        assert int(want["e0"].sum()) + int(want["charge"].sum()) - int(want["used"].sum()) == int(want["soc"].astype(np.int64).sum())


def _declared_charge():
    text = open(os.path.join(ROOT, "include", "cpm_charge.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_charge_header_declares_exactly_the_charge_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared_charge()
    assert declared == ["cpm_resample_charge", "cpm_resample_charge_dev"] == sorted(_lib.CHARGE_SYMBOLS)
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS, _lib.FLOWS_CSR_SYMBOLS, _lib.STAYS_SYMBOLS, _lib.PATHS_SYMBOLS, _lib.OBJECTIVES_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_charge.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_charge.h")).read()
    assert not re.findall(r"#define (CPM_(?:OPT|INFO)\w+)", text)         # no new option or info key
    assert ctypes.sizeof(_lib.ChargeParamsC) == 40 and _lib.ChargeParamsC.wh_per_km.offset == 16 and _lib.ChargeParamsC.soc_in.offset == 32
    buf = np.zeros(4, dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    assert L.cpm_resample_charge(None, 1, 0, None, buf, buf, None, buf, buf, buf, None) == -1
    assert L.cpm_resample_charge_dev(None, 1, 0, None, buf, buf, buf, buf, None) == -1


def _bare_sampler(cpm, Z=37, T=7, n=11):
    s = object.__new__(cpm.Sampler)
    s._h = None
    s.Z, s.T, s.car_count = Z, T, n
    return s


def test_the_python_mirror_refuses_every_forbidden_combination(cpm):
    s = _bare_sampler(cpm)
    p = cpm.ChargeParams(capacity_wh=20000, power_wh=2300, initial_wh=6000, wh_per_km=25.0)
    for kw in (dict(flows=True), dict(flows="csr"), dict(stays=True), dict(paths=True), dict(want_state=True), dict(want_trans=True)):
        with pytest.raises(ValueError):
            s.resample(1, charge=p, **kw)
        with pytest.raises(ValueError):
            s.resample(1, charge=dataclass_dict(p), **kw)
    with pytest.raises(ValueError):                                         # arrays of the wrong length
        s._charge_params(dict(capacity_wh=1, zone_power_wh=np.zeros(36, dtype=np.uint32)))
    with pytest.raises(ValueError):
        s._charge_params(dict(capacity_wh=1, soc_in=np.zeros(12, dtype=np.uint32)))
    c, keep = s._charge_params(dict(capacity_wh=5, power_wh=6, initial_wh=4, wh_per_km=0.5, zone_power_wh=np.arange(37), soc_in=np.arange(11)))
    assert (c.capacity_wh, c.power_wh, c.initial_wh, c.wh_per_km) == (5, 6, 4, 0.5)
    assert keep[0].dtype == np.uint32 and c.zone_power_wh == keep[0].ctypes.data and c.soc_in == keep[1].ctypes.data


def dataclass_dict(p):
    import dataclasses
    return dataclasses.asdict(p)


def test_the_python_mirror_allocates_c_ordered_arrays_of_the_stated_dtypes(cpm):
    s = _bare_sampler(cpm)
    for a, dt in ((s.charge_empty(), np.int64), (s.used_empty(), np.int64), (s.short_empty(), np.int32)):
        assert a.shape == (37, 7) and a.dtype == dt and a.strides == (7 * a.itemsize, a.itemsize)
    assert s.soc_empty().shape == (11,) and s.soc_empty().dtype == np.uint32
