"""Hourly origin-destination trip counts from the fused resample (include/cpm_flows.h, csrc/cpm_flows.h): flows[t, o, d] = cars that
drove from zone o + 1 to zone d + 1 in hour t + 1.

Expected values come from the oracle, never from the library alone.  Two recipes:
  faithful   O.initializestates -> O.solveinitialvalueproblem -> O.resampling, then per hour a histogram of (state[:, t], trans[:, t, 1])
             over the cars with trans[:, t, 0] == 1: all T hours, small fleets.
  fast twin  O.fast_run(..., want_state=True): a car whose zone differs between columns t and t + 1 made the off-diagonal trip
             (state[t], state[t + 1]); the diagonal is driving[o, t] minus the row's off-diagonal sum.  Hours 1 .. T - 1, any size
             (hour T is sampled and not applied: the state holds no column behind it).
GPU tests are marked `gpu` and wrap every step in `pinned`, so that a silent fallback cannot pass; the host-only tests at the end run
without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SIM_SEED, TABLE_SEED
from product_form import GROUPED, MODE_FORM, ZONE_LDS, at_least, pinned

gpu = pytest.mark.gpu
T = 24


def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


def _faithful(O, p_drive, p_dest, Z, cpz, dm=None, dist=None):
    """The reference's three passes on the oracle: dict(flows (T, Z, Z) int32, parking, driving (Z, T) int64, sum_tt_q16, zone0, and the
    state / transition matrices they were counted from)."""
    C = Z * cpz
    st, tr = O.initializestates(C, cpz, T)
    init = O.solveinitialvalueproblem(st, tr, p_drive, p_dest, C, Z, SIM_SEED)
    st, tr = O.initializestates(C, cpz, T)
    st[:, 0] = init
    O.resampling(st, tr, C, Z, p_drive, p_dest, dm, dist, SIM_SEED)
    flows = _flows_of(st, tr, Z)
    pk, dr, _ = O.histogram(Z, st, tr)
    return dict(flows=flows, parking=pk.astype(np.int64), driving=dr.astype(np.int64), sum_tt_q16=O.sum_travel_time_q16(tr), zone0=init,
                state=st, trans=tr)


def _flows_of(st, tr, Z, cars=slice(None)):
    """histogram of (state[:, t], trans[:, t, 1]) over the cars with trans[:, t, 0] == 1"""
    flows = np.zeros((T, Z, Z), dtype=np.int32)
    for t in range(T):
        o, drove, d = st[cars, t], tr[cars, t, 0] == 1, tr[cars, t, 1].astype(np.int64)
        flows[t] = np.bincount((o[drove] - 1) * Z + (d[drove] - 1), minlength=Z * Z).reshape(Z, Z)
    return flows


def _twin_hour(ref, t, Z):
    """hour t (0-based, t < T - 1) of the fast twin's recipe: (Z, Z) int64"""
    a, b = ref["state"][:, t], ref["state"][:, t + 1]
    moved = a != b
    f = np.bincount((a[moved] - 1) * Z + (b[moved] - 1), minlength=Z * Z).reshape(Z, Z)
    diag = ref["driving"][:, t] - f.sum(axis=1)
    assert (diag >= 0).all()
    f[np.arange(Z), np.arange(Z)] += diag
    return f


def _same_counts(a, b):
    return np.array_equal(a["parking"], b["parking"]) and np.array_equal(a["driving"], b["driving"])


def _dense192(O):
    Z, cpz = 192, 120
    return Z, cpz, O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)


def _check_flows_array(f, Z):
    assert isinstance(f, np.ndarray) and f.shape == (T, Z, Z) and f.dtype == np.int32 and f.flags["C_CONTIGUOUS"]


# ------------------------------------------------------------------------------------------------ 1: the test that fails without the feature
@gpu
def test_flows_of_all_hours_equal_the_faithful_oracle(cpm, O):
    """Z = 192 x 120 cars per zone, dense synthetic tables, AUTO: the grouped family, no repeat.  Without the feature the library has
    no cpm_resample_flows."""
    Z, cpz, p_drive, p_dest = _dense192(O)
    C = Z * cpz
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    assert ref["flows"].sum() == ref["driving"].sum() > 0
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED):
            plain = s.resample(SIM_SEED)
        assert "flows" not in plain
        with pinned(s, 0, family=GROUPED):
            r = s.resample(SIM_SEED, flows=True)
        _check_flows_array(r["flows"], Z)
        assert _same_counts(r, plain) and _same_counts(r, ref)
        for t in range(T):
            assert np.array_equal(r["flows"][t], ref["flows"][t]), t
        # the other form of the OD kernel (one launch over the kept runs of all hours): the same flows
        s.set_flows_kept(True)
        with pinned(s, 0, family=GROUPED):
            rk = s.resample(SIM_SEED, flows=True)
        assert np.array_equal(rk["flows"], ref["flows"]) and _same_counts(rk, ref)
        with pinned(s, 0, family=GROUPED):              # the state is unchanged: a plain resample still gives the same counts
            assert _same_counts(s.resample(SIM_SEED), ref)


# ------------------------------------------------------------------------------------------------ 2: the diagonal
@gpu
def test_trips_inside_a_zone_count_on_the_diagonal(cpm, O):
    """p_dest[17, :, 3] = 0 and p_dest[40, :, T - 1] = 0: single all-zero rows keep the origin (src/resampling.jl:35-36), so zones 18
    and 41 see trips inside the zone, one of them in hour T.  The oracle gives 11 and 179 such trips (190 on the diagonal in all);
    the largest bucket is 285 against a region of 1,024: no repeat."""
    Z, cpz, p_drive, p_dest = _dense192(O)
    C = Z * cpz
    p_dest[17, :, 3] = 0.0
    p_dest[40, :, T - 1] = 0.0
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    assert ref["flows"][3, 17, 17] > 0 and ref["flows"][T - 1, 40, 40] > 0      # (the case is not vacuous)
    assert int(np.trace(ref["flows"].sum(axis=0))) == ref["flows"][3, 17, 17] + ref["flows"][T - 1, 40, 40]
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED):
            r = s.resample(SIM_SEED, flows=True)
    assert r["flows"][3, 17, 17] == ref["flows"][3, 17, 17] != 0 and r["flows"][T - 1, 40, 40] == ref["flows"][T - 1, 40, 40] != 0
    assert np.array_equal(r["flows"], ref["flows"]) and _same_counts(r, ref)


# ------------------------------------------------------------------------------------------------ 3: a sink zone
@gpu
def test_a_sink_zone_keeps_every_car_that_arrives(cpm, O):
    """p_dest[5, :, :] = 0: zone 6 keeps every car that arrives (the faithful oracle: 1,455 cars after the IVP, 2,739 at most; 23,824
    trips on the diagonal over the 24 hours, the largest cell 1,710).  The bucket regions must grow, so the steps are pinned with repeats=None.  Observed: the regions grow to
    64x the mean bucket (four repeats between the IVP and the first resample), the sink becomes a heavy bucket (11 workgroups: two
    launches per hour) and the grouped family produces IVP, counts and flows: pinned as such."""
    Z, cpz, p_drive, p_dest = _dense192(O)
    C = Z * cpz
    p_dest[5, :, :] = 0.0
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    assert int(ref["flows"][:, 5, 5].sum()) == int(np.trace(ref["flows"].sum(axis=0))) > 20000 and ref["flows"].max() > 1024
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None) as step:
            r = s.resample(SIM_SEED, flows=True)
        print(f"sink zone: the first flows resample ended on {step}")
        with pinned(s, 0, family=GROUPED, repeats=0, parts=at_least(2)):      # (again, on the grown regions: heavy buckets, no repeat)
            r2 = s.resample(SIM_SEED, flows=True)
    for got in (r, r2):
        assert np.array_equal(got["flows"], ref["flows"]) and _same_counts(got, ref)


# ------------------------------------------------------------------------------------------------ 4: every family and form
def _every_family_and_form(cpm, s, ref, Z, travel):
    for kernel in (1, 2, 5):
        s.set_kernel(kernel)
        if travel:
            # (the grouped family's first resample that needs hour T's runs -- travel times or flows -- is where the sparse shape
            #  outgrows its regions: the plain travel call goes first and is the one step that may repeat)
            with pinned(s, kernel, repeats=None if kernel == 5 else 0):
                plain = s.resample(SIM_SEED, travel=True)
            assert plain["sum_tt_q16"] == ref["sum_tt_q16"] and _same_counts(plain, ref), kernel
        modes = (0, 1, 3, 6, 8) if kernel == 5 else (5,)
        for mode in modes:
            if kernel == 5:
                s.set_fused(mode)
                if mode != 0 and s.get_info(cpm.CPM_INFO_FUSED) != MODE_FORM[mode]:
                    print(f"Z = {Z}: no instantiation for fused mode {mode} (CPM_INFO_FUSED {s.get_info(cpm.CPM_INFO_FUSED)})")
                    continue
            for kept in ((False, True) if kernel == 5 and mode in (0, 1) else (False,)):
                s.set_flows_kept(kept)
                with pinned(s, kernel, fused=mode, repeats=0):
                    r = s.resample(SIM_SEED, flows=True)
                assert np.array_equal(r["flows"], ref["flows"]) and _same_counts(r, ref), (kernel, mode, kept)
        if travel:
            s.set_fused(5)
            with pinned(s, kernel, repeats=0):
                r = s.resample(SIM_SEED, travel=True, flows=True)
            assert r["sum_tt_q16"] == plain["sum_tt_q16"], kernel
            assert np.array_equal(r["flows"], ref["flows"]) and _same_counts(r, ref), kernel
    s.set_kernel(0)
    s.set_fused(5)


@gpu
def test_every_family_and_form_on_sparse_packs(cpm, O):
    """Z = 700 x 60 with the sparse datamatrix of tests/test_sparse_upload.py (sparse packs, general destination groups): kernels 1, 2
    and 5, for 5 the two-launch hour and every one-launch mode the shape has an instantiation for (both forms of the OD kernel where
    the mode leaves the choice), each against the faithful oracle; then once per family with travel times, whose sum must equal the
    plain call's.  The shape outgrows its regions in the first travel resample (tests/test_sparse_upload.py::
    test_counts_of_every_family_with_travel_times_and_a_batch): that step is pinned with repeats=None, every other with 0."""
    Z, cpz = 700, 60
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        p_dest = s.build_p_dest(2)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        assert np.array_equal(p_dest, O.createpdestin(dm, Z, T, 2))
        np.testing.assert_allclose(p_drive, O.createpdrive(dm, dist, Z, T, 0.1, 0.9, 0.5), rtol=4e-16, atol=0, equal_nan=True)
        ref = _faithful(O, p_drive, p_dest, Z, cpz, dm, dist)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _every_family_and_form(cpm, s, ref, Z, travel=True)


@gpu
def test_every_family_and_form_on_dense_packs(cpm, O):
    """The same at Z = 192 x 120 on dense synthetic tables (dense packs, power-of-two destination groups), without travel times."""
    Z, cpz, p_drive, p_dest = _dense192(O)
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _every_family_and_form(cpm, s, ref, Z, travel=False)


# ------------------------------------------------------------------------------------------------ 5: the device-resident form
def _overflow_context(cpm, O):
    """the datamatrix of tests/test_batch.py::_overflow_context: trips end in 6 of 192 zones; no IVP"""
    Z, cpz = 192, 120
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.9)
    dm[:, 6:, :, :] = 0.0
    dm = np.asfortranarray(dm)
    s = cpm.Sampler(Z, T)
    s.set_datamatrix(dm, dist)
    p_drive = s.build_p_drive(0.1, 0.9, 0.5)
    p_dest = s.build_p_dest(2)
    s.init_states(Z * cpz, cpz)
    return s, p_drive, p_dest


@gpu
def test_device_resident_flows_on_a_callers_stream(cpm, O):
    import torch
    Z, cpz, p_drive, p_dest = _dense192(O)
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    stream = torch.cuda.Stream()
    with cpm.Sampler(Z, T, stream=stream) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            s.solve_ivp(SIM_SEED, want=False)
        assert s.flows_words() == T * Z * Z
        d_counts = torch.full((s.counts_words(),), -1, dtype=torch.int64, device="cuda")
        d_flows = torch.full((s.flows_words(),), -1, dtype=torch.int32, device="cuda")     # (the call writes every word)
        with pinned(s, 0, family=GROUPED):
            with torch.cuda.stream(stream):
                s.resample_flows_dev(SIM_SEED, d_counts.data_ptr(), d_flows.data_ptr())
            stream.synchronize()
        counts = d_counts.cpu().numpy()
        assert counts[-1] == 0
        assert np.array_equal(counts[:Z * T].reshape(T, Z).T, ref["parking"]) and np.array_equal(counts[Z * T:2 * Z * T].reshape(T, Z).T, ref["driving"])
        dev = d_flows.cpu().numpy().reshape(T, Z, Z)
        with pinned(s, 0, family=GROUPED):
            blocking = s.resample(SIM_SEED, flows=True)
        assert np.array_equal(dev, blocking["flows"]) and np.array_equal(dev, ref["flows"])
        with pytest.raises(cpm.CpmError) as err:                     # a NULL d_flows is an argument error
            s.resample_flows_dev(SIM_SEED, d_counts.data_ptr(), 0)
        assert err.value.status == -1


@gpu
def test_an_overflowed_device_step_is_flagged_and_the_blocking_call_repairs_it(cpm, O):
    """Trips end in 6 of 192 zones and no IVP has run: the first hours outgrow the regions.  The asynchronous step leaves a non-zero
    status word (counts and flows invalid); the blocking call that follows repeats itself on grown regions and, when they cannot grow further, on the
    exact layout (observed: four repeats, CPM_KERNEL_ZONE_LDS produced the results -- pinned as such: its flows come from the generic
    per-car kernel) and returns the oracle's flows.  The oracle side: the fast twin from the initial state (hours 1 .. T - 1) and, for hour T, the
    row sums."""
    import torch
    s, p_drive, p_dest = _overflow_context(cpm, O)
    Z, cpz = 192, 120
    C = Z * cpz
    try:
        ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), do_ivp=False, want_state=True)
        stream = torch.cuda.Stream()
        s.set_stream(stream)
        d_counts = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
        d_flows = torch.zeros(s.flows_words(), dtype=torch.int32, device="cuda")
        with torch.cuda.stream(stream):
            s.resample_flows_dev(SIM_SEED, d_counts.data_ptr(), d_flows.data_ptr())
        stream.synchronize()
        assert s.get_info(cpm.CPM_INFO_LAST_KERNEL) == GROUPED
        assert int(d_counts[-1].item()) != 0
        with pinned(s, 0, family=ZONE_LDS, repeats=at_least(1)) as step:
            r = s.resample(SIM_SEED, flows=True)
        print(f"overflow: the blocking flows resample ended on {step}")
        with pinned(s, 0, family=ZONE_LDS, repeats=0):                # (AUTO has left the grouped layout for this context)
            r2 = s.resample(SIM_SEED, flows=True)
    finally:
        s.close()
    for got in (r, r2):
        assert _same_counts(got, ref)
        for t in range(T - 1):
            assert np.array_equal(got["flows"][t], _twin_hour(ref, t, Z)), t
        assert np.array_equal(got["flows"][T - 1].sum(axis=1), ref["driving"][:, T - 1])


# ------------------------------------------------------------------------------------------------ 6: a strided shard
@gpu
def test_two_strided_shards_sum_to_the_whole_fleet(cpm, O):
    Z, cpz, p_drive, p_dest = _dense192(O)
    C = Z * cpz
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    total = np.zeros((T, Z, Z), dtype=np.int64)
    for first in (0, 1):
        with cpm.Sampler(Z, T) as s:
            s.set_p_drive(p_drive)
            s.set_p_dest(p_dest)
            s.init_states(C, cpz, first, car_stride=2)
            assert s.car_count == C // 2
            with pinned(s, 0, family=GROUPED):
                assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"][first::2])
            with pinned(s, 0, family=GROUPED):
                r = s.resample(SIM_SEED, flows=True)
            # (a shard against the oracle as well: the cars of the shard alone)
            assert np.array_equal(r["flows"], _flows_of(ref["state"], ref["trans"], Z, slice(first, None, 2))), first
            total += r["flows"]
    assert np.array_equal(total, ref["flows"])


# ------------------------------------------------------------------------------------------------ 7: full size
def _full_size_checks(r, ref, p_dest, Z):
    """hours 1 .. T - 1 against the fast twin; all hours: row sums = driving; t < T: the parking balance; no trip where p_dest is zero
    except on the diagonal of all-zero rows"""
    f = r["flows"]
    _check_flows_array(f, Z)
    assert _same_counts(r, ref)
    idx = np.arange(Z)
    for t in range(T):
        ft = f[t].astype(np.int64)
        assert ft.min() >= 0
        assert np.array_equal(ft.sum(axis=1), ref["driving"][:, t]), t
        if t < T - 1:
            assert np.array_equal(ft, _twin_hour(ref, t, Z)), t
            assert np.array_equal(ref["parking"][:, t + 1], ref["parking"][:, t] - ref["driving"][:, t] + ft.sum(axis=0)), t
        no_way = p_dest[:, :, t] == 0                      # [origin, destination]
        zero_row = no_way.all(axis=1)
        no_way[idx[zero_row], idx[zero_row]] = False       # an all-zero row keeps the origin
        assert not ft[no_way].any(), t


@gpu
def test_flows_at_the_headline_shape(cpm, O):
    """Z = 4,096 x 1,000 cars per zone, the tables and seeds of tests/test_gpu_parity.py::test_headline_config_full_size, pinned to the
    form bench.py times (the grouped family in the form CPM_INFO_FUSED predicts, regions at 4x the mean, no repeat).  Hour T is
    covered against the oracle by the small tests above only (the fast twin's state holds no column behind it); here it is held to
    its row sums and to p_dest's zeros."""
    Z, cpz = 4096, 1000
    C = Z * cpz
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    cdf = O.build_cdf(p_dest)
    ref = O.fast_run(p_drive, cdf, C, SIM_SEED, _zone0(C, cpz), want_state=True)
    del cdf
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(TABLE_SEED)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, form=1, cap_mult=4, parts=1):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, form=1, cap_mult=4, parts=1, repeats=0):
            r = s.resample(SIM_SEED, flows=True)
    _full_size_checks(r, ref, p_dest, Z)


@gpu
def test_flows_at_melbournes_shape_with_travel_times(cpm, O):
    """Z = 2,357 x 1,000 cars per zone (Z is not a multiple of 4: rows start off a 16-byte boundary), sparse packs, travel times on.
    Hour T as in the headline test."""
    Z, cpz = 2357, 1000
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        p_dest = s.build_p_dest(2)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        cdf = O.build_cdf(p_dest)
        ref = O.fast_run(p_drive, cdf, C, SIM_SEED, _zone0(C, cpz), want_state=True, datamatrix=dm, dist=dist)
        del cdf
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=0):
            r = s.resample(SIM_SEED, travel=True, flows=True)
    assert r["sum_tt_q16"] == ref["sum_tt_q16"]
    _full_size_checks(r, ref, p_dest, Z)


# ------------------------------------------------------------------------------------------------ 8: host only
def _declared_flows():
    text = open(os.path.join(ROOT, "include", "cpm_flows.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_flows_header_declares_exactly_the_flows_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared_flows()
    assert declared and sorted(_lib.FLOWS_SYMBOLS) == declared
    assert not set(declared) & set(_lib.SYMBOLS) and not set(declared) & set(_lib.BATCH_SYMBOLS)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_flows.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_flows.h")).read()
    assert {k: int(v) for k, v in re.findall(r"#define (CPM_\w+) (\d+)", text)} == {"CPM_OPT_FLOWS_KEPT": _lib.CPM_OPT_FLOWS_KEPT}


def test_null_arguments_are_argument_errors(cpm):
    from carparkingmaps_amd import _lib
    L = _lib.load()
    buf = np.zeros(4, dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    assert L.cpm_resample_flows(None, 1, 0, buf, buf, None, buf) == -1
    assert L.cpm_resample_flows_dev(None, 1, 0, buf, buf) == -1
    assert b"null context" in L.cpm_last_error()


def test_flows_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "flows_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_flows.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    int64_t counts[4] = {0};
    int32_t flows[4] = {0};
    int32_t rc = cpm_resample_flows(ctx, 1u, CPM_FLAG_TRAVEL, counts, counts, NULL, flows) + cpm_resample_flows_dev(ctx, 1u, 0u, counts, flows);
    return (rc == 2 * CPM_ERR_ARG && CPM_OPT_FLOWS_KEPT == 16) ? 0 : 1;
}
""")
    exe = str(tmp_path / "flows_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == 0


def test_the_python_mirror_allocates_t_z_z_int32_in_c_order(cpm):
    """Sampler.flows_words / flows_empty without a context (no GPU): the shape, dtype and size of the array the library fills."""
    s = object.__new__(cpm.Sampler)
    s._h = None
    s.Z, s.T = 37, 24
    assert s.flows_words() == 24 * 37 * 37
    a = s.flows_empty()
    _check_flows_array(a, 37)
    assert a.size == s.flows_words() and a.nbytes == 4 * s.flows_words()
    assert a.strides == (37 * 37 * 4, 37 * 4, 4)             # hour-major, then origin, destination fastest


def test_the_oracles_two_recipes_agree(O):
    """The faithful form's flows and the fast twin's recipe on Z = 37 (hours 1 .. T - 1), with an all-zero row in one hour: what the
    full-size tests rely on."""
    Z, cpz = 37, 40
    C = Z * cpz
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    p_dest[3, :, 5] = 0.0
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    twin = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), want_state=True)
    assert _same_counts(ref, twin) and ref["flows"][5, 3, 3] > 0
    for t in range(T - 1):
        assert np.array_equal(ref["flows"][t], _twin_hour(twin, t, Z)), t
    assert np.array_equal(ref["flows"].sum(axis=2).T, ref["driving"])
