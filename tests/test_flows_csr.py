"""The hourly origin-destination trip counts as compressed sparse rows (include/cpm_flows_csr.h, csrc/cpm_flows_csr.h): the non-zero
cells of flows[t, o, d] (tests/test_flows.py), row t * Z + o, destinations 0-based and ascending.

Expected values come from the oracle by the two recipes of tests/test_flows.py (whose helpers are imported, not copied), and the
layout from numpy: the CSR of a dense tensor is np.nonzero in row-major order.  All comparisons are on integers and exact.  GPU
tests wrap every step in `pinned`; the host-only tests at the end run without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SIM_SEED, TABLE_SEED
from product_form import GROUPED, MODE_FORM, ZONE_LDS, at_least, pinned
from test_flows import T, _dense192, _faithful, _flows_of, _full_size_checks, _overflow_context, _same_counts, _twin_hour, _zone0

gpu = pytest.mark.gpu


def _csr_of_dense(dense):
    """canonical CSR of a (T, Z, Z) tensor: np.nonzero walks it in row-major order"""
    Tn, Z, _ = dense.shape
    flat = dense.reshape(Tn * Z, Z)
    rows, cols = np.nonzero(flat)
    row_ptr = np.zeros(Tn * Z + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=Tn * Z), out=row_ptr[1:])
    return dict(row_ptr=row_ptr, dest=cols.astype(np.int32), count=flat[rows, cols].astype(np.int32), shape=(Tn, Z, Z))


def _same_csr(a, b):
    return (tuple(a["shape"]) == tuple(b["shape"]) and np.array_equal(a["row_ptr"], b["row_ptr"]) and np.array_equal(a["dest"], b["dest"])
            and np.array_equal(a["count"], b["count"]))


def _check_canonical(csr, Z, nnz=None):
    rp, dest, count = csr["row_ptr"], csr["dest"], csr["count"]
    assert tuple(csr["shape"]) == (T, Z, Z)
    assert rp.dtype == np.int64 and dest.dtype == np.int32 and count.dtype == np.int32
    assert rp.shape == (T * Z + 1,) and dest.shape == count.shape == (int(rp[-1]),)
    assert rp[0] == 0 and (np.diff(rp) >= 0).all()
    if nnz is not None:
        assert rp[-1] == nnz
    if dest.size:
        assert dest.min() >= 0 and dest.max() < Z and count.min() > 0
        rising = np.diff(dest.astype(np.int64)) > 0           # strictly ascending, except across a row's first entry
        starts = rp[1:-1][(rp[1:-1] > 0) & (rp[1:-1] < dest.size)]
        rising[starts - 1] = True
        assert rising.all()


# ------------------------------------------------------------------------------------------------ 1: the test that fails without the feature
@gpu
def test_csr_flows_of_all_hours_equal_the_faithful_oracle(cpm, O):
    """Z = 192 x 120, dense synthetic tables, AUTO: the grouped family, no repeat.  Without the feature Sampler.resample knows no
    flows="csr" and the library no cpm_resample_flows_csr."""
    Z, cpz, p_drive, p_dest = _dense192(O)
    C = Z * cpz
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED):
            plain = s.resample(SIM_SEED)
        with pinned(s, 0, family=GROUPED):
            r = s.resample(SIM_SEED, flows="csr")
        with pinned(s, 0, family=GROUPED):
            rd = s.resample(SIM_SEED, flows=True)
        assert "flows" not in r and "flows_csr" not in rd and "flows_csr" not in plain
        csr = r["flows_csr"]
        dense = cpm.flows_csr_to_dense(csr)
        assert dense.dtype == np.int32 and dense.shape == (T, Z, Z)
        for t in range(T):
            assert np.array_equal(dense[t], ref["flows"][t]), t
        assert np.array_equal(dense, rd["flows"])
        assert _same_counts(r, plain) and _same_counts(r, ref) and _same_counts(rd, ref)
        _check_canonical(csr, Z, nnz=np.count_nonzero(dense))
        assert csr["row_ptr"][-1] == csr["dest"].size == np.count_nonzero(ref["flows"])
        assert (csr["count"] > 1).any()                       # (not passing on all-ones)
        assert _same_csr(csr, _csr_of_dense(ref["flows"]))
        for t in (0, 7, T - 1):                                # an hour's view, rebased
            indptr, indices, data = cpm.flows_csr_hour(csr, t)
            assert indptr[0] == 0 and indptr.shape == (Z + 1,)
            hour = _csr_of_dense(ref["flows"][t:t + 1])
            assert np.array_equal(indptr, hour["row_ptr"]) and np.array_equal(indices, hour["dest"]) and np.array_equal(data, hour["count"])
        # the other form (one set of launches over the kept runs of all hours): the same three arrays
        s.set_flows_kept(True)
        with pinned(s, 0, family=GROUPED):
            rk = s.resample(SIM_SEED, flows="csr")
        assert _same_csr(rk["flows_csr"], csr) and _same_counts(rk, ref)
        with pinned(s, 0, family=GROUPED):              # the state is unchanged: a plain resample still gives the same counts
            assert _same_counts(s.resample(SIM_SEED), ref)
        with pytest.raises(ValueError):
            s.resample(SIM_SEED, flows="csr", want_state=True)
        with pytest.raises(ValueError):
            s.resample(SIM_SEED, flows="coo")


# ------------------------------------------------------------------------------------------------ 2: every family and form
def _every_family_and_form_csr(cpm, s, ref, Z, travel):
    """the matrix of tests/test_flows.py::_every_family_and_form with flows="csr": every result's arrays equal the first one's and
    the CSR of the oracle's dense flows"""
    want = _csr_of_dense(ref["flows"])
    for kernel in (1, 2, 5):
        s.set_kernel(kernel)
        if travel:
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
                    r = s.resample(SIM_SEED, flows="csr")
                _check_canonical(r["flows_csr"], Z)
                assert _same_csr(r["flows_csr"], want) and _same_counts(r, ref), (kernel, mode, kept)
        if travel:
            s.set_fused(5)
            with pinned(s, kernel, repeats=0):
                r = s.resample(SIM_SEED, travel=True, flows="csr")
            assert r["sum_tt_q16"] == plain["sum_tt_q16"], kernel
            assert _same_csr(r["flows_csr"], want) and _same_counts(r, ref), kernel
    s.set_kernel(0)
    s.set_fused(5)


@gpu
def test_every_family_and_form_on_sparse_packs(cpm, O):
    """Z = 700 x 60, the sparse datamatrix of tests/test_flows.py's test of the same name, with travel times."""
    Z, cpz = 700, 60
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        p_dest = s.build_p_dest(2)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        ref = _faithful(O, p_drive, p_dest, Z, cpz, dm, dist)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _every_family_and_form_csr(cpm, s, ref, Z, travel=True)


@gpu
def test_every_family_and_form_on_dense_packs(cpm, O):
    Z, cpz, p_drive, p_dest = _dense192(O)
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        _every_family_and_form_csr(cpm, s, ref, Z, travel=False)


# ------------------------------------------------------------------------------------------------ 3: edges
@gpu
def test_zero_rows_empty_zones_and_a_row_length_off_four(cpm, O):
    """Z = 190 (not a multiple of 4) x 120.  No trip ends in zones 151 .. 190 (their p_dest columns are zero, the rows renormalised)
    and no car starts there: their rows are empty in every hour.  p_dest[17, :, 3] = 0 and p_dest[40, :, T - 1] = 0: single all-zero
    rows keep the origin, so rows (3, 17) and (T - 1, 40) hold one entry each, on the diagonal, one of them in hour T.  All cars in
    150 of 190 zones: buckets start at 1.27x the mean the regions are sized for -- pinned with repeats=None, family grouped."""
    Z, cpz, lo = 190, 120, 150
    C = Z * cpz
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    p_dest[:, lo:, :] = 0.0
    p_dest /= p_dest.sum(axis=1, keepdims=True)
    p_dest[17, :, 3] = 0.0
    p_dest[40, :, T - 1] = 0.0
    p_dest = np.asfortranarray(p_dest)
    zone0 = np.arange(C, dtype=np.int64) % lo + 1
    st, tr = O.initializestates(C, cpz, T)
    st[:, 0] = zone0
    init = O.solveinitialvalueproblem(st, tr, p_drive, p_dest, C, Z, SIM_SEED)
    st, tr = O.initializestates(C, cpz, T)
    st[:, 0] = init
    O.resampling(st, tr, C, Z, p_drive, p_dest, None, None, SIM_SEED)
    flows = _flows_of(st, tr, Z)
    assert init.max() <= lo and flows[3, 17, 17] > 0 and flows[T - 1, 40, 40] > 0 and not flows[:, lo:, :].any() and not flows[:, :, lo:].any()
    want = _csr_of_dense(flows)
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        s.set_state(zone0)
        with pinned(s, 0, family=GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), init)
        with pinned(s, 0, family=GROUPED, repeats=None):
            r = s.resample(SIM_SEED, flows="csr")
        with pinned(s, 0, family=GROUPED, repeats=0):
            rd = s.resample(SIM_SEED, flows=True)
        for kernel in (1, 2):                            # the dense-row path of the other two families, rows off a 16-byte boundary
            s.set_kernel(kernel)
            with pinned(s, kernel, repeats=0):
                rk = s.resample(SIM_SEED, flows="csr")
            assert _same_csr(rk["flows_csr"], want), kernel
    csr = r["flows_csr"]
    _check_canonical(csr, Z, nnz=np.count_nonzero(flows))
    assert _same_csr(csr, want) and np.array_equal(rd["flows"], flows)
    rp = csr["row_ptr"]
    for t in range(T):
        assert (rp[t * Z + lo:(t + 1) * Z + 1] == rp[t * Z + lo]).all(), t          # empty rows: equal consecutive row_ptr
    for t, o in ((3, 17), (T - 1, 40)):
        a, b = rp[t * Z + o], rp[t * Z + o + 1]
        assert b - a == 1 and csr["dest"][a] == o and csr["count"][a] == flows[t, o, o]
    assert rp[-1] > rp[(T - 1) * Z]                                                 # hour T is present


@gpu
def test_a_sink_zone(cpm, O):
    """p_dest[5, :, :] = 0 (tests/test_flows.py::test_a_sink_zone_keeps_every_car_that_arrives): row (t, 5) is one entry on the diagonal
    with a count above 1,024, the regions grow (repeats=None), then the sink is a heavy bucket and nothing repeats."""
    Z, cpz, p_drive, p_dest = _dense192(O)
    C = Z * cpz
    p_dest[5, :, :] = 0.0
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    want = _csr_of_dense(ref["flows"])
    assert want["count"].max() > 1024
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None):
            r = s.resample(SIM_SEED, flows="csr")
        with pinned(s, 0, family=GROUPED, repeats=0, parts=at_least(2)):
            r2 = s.resample(SIM_SEED, flows="csr")
    for got in (r, r2):
        assert _same_csr(got["flows_csr"], want) and _same_counts(got, ref)
    rp = want["row_ptr"]
    for t in range(T):
        assert rp[t * Z + 6] - rp[t * Z + 5] == 1 and r["flows_csr"]["dest"][rp[t * Z + 5]] == 5


# ------------------------------------------------------------------------------------------------ 4: the device-resident form
@gpu
def test_device_resident_csr_on_a_callers_stream(cpm, O):
    import torch
    Z, cpz, p_drive, p_dest = _dense192(O)
    ref = _faithful(O, p_drive, p_dest, Z, cpz)
    want = _csr_of_dense(ref["flows"])
    nnz = int(want["row_ptr"][-1])
    stream = torch.cuda.Stream()
    with cpm.Sampler(Z, T, stream=stream) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(Z * cpz, cpz)
        with pinned(s, 0, family=GROUPED):
            s.solve_ivp(SIM_SEED, want=False)
        L, h = s._L, s._h
        dummy = np.zeros(4, dtype=np.int32)
        assert L.cpm_get_flows_csr(h, dummy.ctypes.data_as(ctypes.c_void_p), dummy.ctypes.data_as(ctypes.c_void_p), 0) == -1   # no blocking call yet
        with pinned(s, 0, family=GROUPED):
            blocking = s.resample(SIM_SEED, flows="csr")
        assert _same_csr(blocking["flows_csr"], want)
        assert L.cpm_get_flows_csr(h, dummy.ctypes.data_as(ctypes.c_void_p), dummy.ctypes.data_as(ctypes.c_void_p), nnz + 1) == -1  # not the reported size
        GUARD, PAD = -7, 64

        def run(cap, kept=False, sizes_only=False):
            s.set_flows_kept(kept)
            d_counts = torch.full((s.counts_words(),), -1, dtype=torch.int64, device="cuda")
            d_row_ptr = torch.full((T * Z + 1,), -1, dtype=torch.int64, device="cuda")
            d_dest = torch.full((cap + PAD,), GUARD, dtype=torch.int32, device="cuda")
            d_count = torch.full((cap + PAD,), GUARD, dtype=torch.int32, device="cuda")
            with pinned(s, 0, family=GROUPED):
                with torch.cuda.stream(stream):
                    if sizes_only:
                        s.resample_flows_csr_dev(SIM_SEED, d_counts.data_ptr(), d_row_ptr.data_ptr(), 0, 0, 0)
                    else:
                        s.resample_flows_csr_dev(SIM_SEED, d_counts.data_ptr(), d_row_ptr.data_ptr(), d_dest.data_ptr(), d_count.data_ptr(), cap)
                stream.synchronize()
            counts = d_counts.cpu().numpy()
            assert counts[-1] == 0
            assert np.array_equal(counts[:Z * T].reshape(T, Z).T, ref["parking"]) and np.array_equal(counts[Z * T:2 * Z * T].reshape(T, Z).T, ref["driving"])
            return d_row_ptr.cpu().numpy(), d_dest.cpu().numpy(), d_count.cpu().numpy()

        for kept in (False, True):
            rp, dest, count = run(nnz, kept)                                   # exact cap
            assert np.array_equal(rp, want["row_ptr"]) and np.array_equal(dest[:nnz], want["dest"]) and np.array_equal(count[:nnz], want["count"])
            assert (dest[nnz:] == GUARD).all() and (count[nnz:] == GUARD).all()
            for cap in (nnz // 2, nnz // 2 + 1, nnz // 2 + 2, nnz // 2 + 3):   # about half (every alignment of the cut): the cut falls inside a row
                rp, dest, count = run(cap, kept)
                assert np.array_equal(rp, want["row_ptr"]) and rp[-1] == nnz > cap
                assert np.array_equal(dest[:cap], want["dest"][:cap]) and np.array_equal(count[:cap], want["count"][:cap])
                assert (dest[cap:] == GUARD).all() and (count[cap:] == GUARD).all()    # nothing stored at or behind cap
            rp, dest, count = run(0, kept, sizes_only=True)                    # cap = 0, null entry pointers: sizes only
            assert np.array_equal(rp, want["row_ptr"]) and (dest == GUARD).all() and (count == GUARD).all()
        d_counts = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
        d_row_ptr = torch.zeros(T * Z + 1, dtype=torch.int64, device="cuda")
        for args in ((0, d_row_ptr.data_ptr(), 0, 0, 0), (d_counts.data_ptr(), 0, 0, 0, 0), (d_counts.data_ptr(), d_row_ptr.data_ptr(), 0, 0, 16),
                     (d_counts.data_ptr(), d_row_ptr.data_ptr(), 0, 0, -1)):
            with pytest.raises(cpm.CpmError) as err:
                s.resample_flows_csr_dev(SIM_SEED, *args)
            assert err.value.status == -1


@gpu
def test_an_overflowed_device_step_is_flagged_and_the_blocking_call_repairs_it(cpm, O):
    """The context of tests/test_flows.py's test of the same name: the asynchronous step leaves a non-zero status word (all three arrays
    invalid, nothing stored behind cap); the blocking call repeats itself, ends on CPM_KERNEL_ZONE_LDS (whose rows come through the
    dense hour block) and returns the oracle's flows: the fast twin for hours 1 .. T - 1, the row sums for hour T."""
    import torch
    s, p_drive, p_dest = _overflow_context(cpm, O)
    Z, cpz = 192, 120
    C = Z * cpz
    try:
        ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), do_ivp=False, want_state=True)
        stream = torch.cuda.Stream()
        s.set_stream(stream)
        cap, GUARD = 4096, -7
        d_counts = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
        d_row_ptr = torch.zeros(T * Z + 1, dtype=torch.int64, device="cuda")
        d_dest = torch.full((cap + 64,), GUARD, dtype=torch.int32, device="cuda")
        d_count = torch.full((cap + 64,), GUARD, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(stream):
            s.resample_flows_csr_dev(SIM_SEED, d_counts.data_ptr(), d_row_ptr.data_ptr(), d_dest.data_ptr(), d_count.data_ptr(), cap)
        stream.synchronize()
        assert s.get_info(cpm.CPM_INFO_LAST_KERNEL) == GROUPED
        assert int(d_counts[-1].item()) != 0
        assert (d_dest[cap:] == GUARD).all().item() and (d_count[cap:] == GUARD).all().item()
        with pinned(s, 0, family=ZONE_LDS, repeats=at_least(1)) as step:
            r = s.resample(SIM_SEED, flows="csr")
        print(f"overflow: the blocking csr resample ended on {step}")
        with pinned(s, 0, family=ZONE_LDS, repeats=0):
            r2 = s.resample(SIM_SEED, flows="csr")
    finally:
        s.close()
    assert _same_csr(r["flows_csr"], r2["flows_csr"])
    for got in (r, r2):
        assert _same_counts(got, ref)
        _check_canonical(got["flows_csr"], Z)
        dense = cpm.flows_csr_to_dense(got["flows_csr"])
        for t in range(T - 1):
            assert np.array_equal(dense[t], _twin_hour(ref, t, Z)), t
        assert np.array_equal(dense[T - 1].sum(axis=1), ref["driving"][:, T - 1])


# ------------------------------------------------------------------------------------------------ 5: shards
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
            with pinned(s, 0, family=GROUPED):
                assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"][first::2])
            with pinned(s, 0, family=GROUPED):
                r = s.resample(SIM_SEED, flows="csr")
            assert _same_csr(r["flows_csr"], _csr_of_dense(_flows_of(ref["state"], ref["trans"], Z, slice(first, None, 2)))), first
            total += cpm.flows_csr_to_dense(r["flows_csr"])
    assert np.array_equal(total, ref["flows"])


# ------------------------------------------------------------------------------------------------ 6: full size
def _csr_equals_nonzero_of(csr, dense):
    """the CSR against np.nonzero of the dense tensor of the same context, hour by hour (row-major order)"""
    Tn, Z, _ = dense.shape
    _check_canonical(csr, Z)
    rp = csr["row_ptr"]
    for t in range(Tn):
        rows, cols = np.nonzero(dense[t])
        a, b = rp[t * Z], rp[(t + 1) * Z]
        assert b - a == rows.size, t
        assert np.array_equal(np.diff(rp[t * Z:(t + 1) * Z + 1]), np.bincount(rows, minlength=Z)), t
        assert np.array_equal(csr["dest"][a:b], cols) and np.array_equal(csr["count"][a:b], dense[t][rows, cols]), t


@gpu
def test_csr_flows_at_the_headline_shape(cpm, O):
    """Z = 4,096 x 1,000, pinned as tests/test_flows.py::test_flows_at_the_headline_shape pins it."""
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
            r = s.resample(SIM_SEED, flows="csr")
        with pinned(s, 0, family=GROUPED, form=1, cap_mult=4, parts=1, repeats=0):
            rd = s.resample(SIM_SEED, flows=True)
    csr = r["flows_csr"]
    print(f"headline: nnz {csr['row_ptr'][-1]:,} of {T * Z * Z:,} cells ({csr['row_ptr'][-1] / (T * Z * Z):.2%})")
    _csr_equals_nonzero_of(csr, rd["flows"])
    del rd
    _full_size_checks(dict(r, flows=cpm.flows_csr_to_dense(csr)), ref, p_dest, Z)


@gpu
def test_csr_flows_at_melbournes_shape_with_travel_times(cpm, O):
    """Z = 2,357 x 1,000 (Z is not a multiple of 4), sparse packs, travel times on: the kept form."""
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
        with pinned(s, 0, family=GROUPED, repeats=None):     # (the first travel resample may outgrow its regions, as in tests/test_flows.py)
            s.resample(SIM_SEED, travel=True)
        with pinned(s, 0, family=GROUPED, repeats=0):
            r = s.resample(SIM_SEED, travel=True, flows="csr")
        with pinned(s, 0, family=GROUPED, repeats=0):
            rd = s.resample(SIM_SEED, travel=True, flows=True)
    csr = r["flows_csr"]
    print(f"melbourne x 1,000: nnz {csr['row_ptr'][-1]:,} of {T * Z * Z:,} cells ({csr['row_ptr'][-1] / (T * Z * Z):.2%})")
    assert r["sum_tt_q16"] == ref["sum_tt_q16"] == rd["sum_tt_q16"]
    _csr_equals_nonzero_of(csr, rd["flows"])
    del rd
    _full_size_checks(dict(r, flows=cpm.flows_csr_to_dense(csr)), ref, p_dest, Z)


# ------------------------------------------------------------------------------------------------ 7: the size the dense tensor could not serve
@gpu
def test_csr_flows_at_8192_zones(cpm, O):
    """Z = 8,192 x 500 cars per zone: the dense tensor would be 6.4 GB; blocking CSR only, against the fast twin with its state.  Hours
    t < T: the (origin, destination, count) triples are np.unique over the moved cars' (state[t], state[t + 1]) plus the diagonal
    remainder driving - moved.  All hours: row sums = driving.  The oracle's dense tables (2 x 12.9 GB on the host) dominate the
    test's duration."""
    Z, cpz = 8192, 500
    C = Z * cpz
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    cdf = O.build_cdf(p_dest)
    del p_dest
    ref = O.fast_run(p_drive, cdf, C, SIM_SEED, _zone0(C, cpz), want_state=True)
    del cdf
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(TABLE_SEED)
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None):
            r = s.resample(SIM_SEED, flows="csr")
    assert _same_counts(r, ref)
    csr = r["flows_csr"]
    _check_canonical(csr, Z)
    rp, nnz = csr["row_ptr"], int(csr["row_ptr"][-1])
    print(f"Z = 8,192: nnz {nnz:,} of {T * Z * Z:,} cells ({nnz / (T * Z * Z):.2%})")
    assert nnz * 8 + (T * Z + 1) * 8 < (T * Z * Z * 4) // 4           # host memory: far below the dense tensor's
    row_of = np.repeat(np.arange(T * Z, dtype=np.int64), np.diff(rp))
    sums = np.bincount(row_of, weights=csr["count"], minlength=T * Z).astype(np.int64).reshape(T, Z)
    assert np.array_equal(sums.T, ref["driving"])                      # all hours: row sums = driving
    idx = np.arange(Z, dtype=np.int64)
    for t in range(T - 1):
        a, b = ref["state"][:, t], ref["state"][:, t + 1]
        moved = a != b
        keys, cnt = np.unique((a[moved] - 1) * Z + (b[moved] - 1), return_counts=True)
        diag = ref["driving"][:, t] - np.bincount(a[moved] - 1, minlength=Z)
        assert (diag >= 0).all()
        keys = np.concatenate([keys, (idx * Z + idx)[diag > 0]])
        cnt = np.concatenate([cnt, diag[diag > 0]])
        order = np.argsort(keys, kind="stable")
        indptr, indices, data = cpm.flows_csr_hour(csr, t)
        got_keys = np.repeat(idx, np.diff(indptr)) * Z + indices
        assert np.array_equal(got_keys, keys[order]) and np.array_equal(data, cnt[order]), t


# ------------------------------------------------------------------------------------------------ 8: host only
def _declared():
    text = open(os.path.join(ROOT, "include", "cpm_flows_csr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cpm_[a-z0-9_]+)\s*\(", text)))


def test_csr_header_declares_exactly_the_csr_symbols_and_the_library_exports_them(cpm):
    from carparkingmaps_amd import _lib
    declared = _declared()
    assert declared and sorted(_lib.FLOWS_CSR_SYMBOLS) == declared
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.FLOWS_SYMBOLS):
        assert not set(declared) & set(other)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/cpm_flows_csr.h but not exported"
    text = open(os.path.join(ROOT, "include", "cpm_flows_csr.h")).read()
    assert "SparseMatrixCSC(Z, Z*T, row_ptr .+ 1, dest .+ 1, count)" in text
    assert "SparseMatrixCSC(Z, Z*T, row_ptr .+ 1, dest .+ 1, count)" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_argument_errors(cpm):
    from carparkingmaps_amd import _lib
    L = _lib.load()
    buf = np.zeros(4, dtype=np.int64).ctypes.data_as(ctypes.c_void_p)
    nnz = ctypes.c_int64(0)
    assert L.cpm_resample_flows_csr(None, 1, 0, buf, buf, None, buf, ctypes.byref(nnz)) == -1
    assert b"null context" in L.cpm_last_error()
    assert L.cpm_resample_flows_csr_dev(None, 1, 0, buf, buf, buf, buf, 4) == -1
    assert b"null context" in L.cpm_last_error()
    assert L.cpm_get_flows_csr(None, buf, buf, 0) == -1
    assert b"null context" in L.cpm_last_error()


def test_csr_header_compiles_under_a_strict_c_compiler(cpm, tmp_path):
    from carparkingmaps_amd import _lib
    src = tmp_path / "flows_csr_header.c"
    src.write_text("""#include <stddef.h>
#include "cpm_flows.h"
#include "cpm_flows_csr.h"
int main(void)
{
    cpm_ctx *ctx = NULL;
    int64_t counts[4] = {0}, row_ptr[4] = {0}, nnz = 0;
    int32_t entries[4] = {0};
    int32_t rc = cpm_resample_flows_csr(ctx, 1u, CPM_FLAG_TRAVEL, counts, counts, NULL, row_ptr, &nnz)
               + cpm_resample_flows_csr_dev(ctx, 1u, 0u, counts, row_ptr, entries, entries, 4)
               + cpm_get_flows_csr(ctx, entries, entries, nnz);
    return (rc == 3 * CPM_ERR_ARG && CPM_OPT_FLOWS_KEPT == 16) ? 0 : 1;
}
""")
    exe = str(tmp_path / "flows_csr_header")
    csrc = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + csrc, "-lcpm_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath-link,/opt/rocm/lib"])
    assert subprocess.run([exe]).returncode == 0


def _hand_made():
    """T = 24 hours x Z = 5: hour 2 is empty, hour 1 has empty rows, one cell above 1, entries in the first and the last row"""
    Z = 5
    dense = np.zeros((T, Z, Z), dtype=np.int32)
    dense[0, 0, 0] = 3
    dense[0, 0, 4] = 1
    dense[0, 3, 2] = 7
    dense[2, 1, 0] = 2
    dense[2, 1, 1] = 1
    dense[2, 4, 3] = 5
    dense[T - 1, 4, 4] = 11
    return Z, dense


def test_the_python_helpers_round_trip_a_hand_made_tensor(cpm, tmp_path):
    Z, dense = _hand_made()
    csr = _csr_of_dense(dense)
    _check_canonical(csr, Z, nnz=7)
    assert csr["row_ptr"][Z] == csr["row_ptr"][2 * Z] == 3                     # hour 2 (index 1) is empty
    back = cpm.flows_csr_to_dense(csr)
    assert back.dtype == np.int32 and back.shape == (T, Z, Z) and np.array_equal(back, dense)
    indptr, indices, data = cpm.flows_csr_hour(csr, 2)
    assert indptr.tolist() == [0, 0, 2, 2, 2, 3] and indices.tolist() == [0, 1, 3] and data.tolist() == [2, 1, 5]
    assert np.shares_memory(indices, csr["dest"]) and np.shares_memory(data, csr["count"])      # views
    indptr, indices, data = cpm.flows_csr_hour(csr, 1)
    assert indptr.tolist() == [0] * (Z + 1) and indices.size == 0 and data.size == 0
    with pytest.raises(IndexError):
        cpm.flows_csr_hour(csr, T)
    path = tmp_path / "flows.csv"
    assert cpm.save_flows_csv(str(path), csr) == 7
    lines = path.read_text().split("\n")
    assert lines[0] == "hour,origin,destination,trips" and lines[-1] == ""
    assert lines[1:-1] == ["1,1,1,3", "1,1,5,1", "1,4,3,7", "3,2,1,2", "3,2,2,1", "3,5,4,5", f"{T},5,5,11"]
    table = np.array([[int(v) for v in ln.split(",")] for ln in lines[1:-1]])
    again = np.zeros_like(dense)
    again[table[:, 0] - 1, table[:, 1] - 1, table[:, 2] - 1] = table[:, 3]
    assert np.array_equal(again, dense)
    empty = _csr_of_dense(np.zeros((T, Z, Z), dtype=np.int32))
    assert not cpm.flows_csr_to_dense(empty).any() and cpm.save_flows_csv(str(path), empty) == 0


def test_the_package_does_not_import_scipy(cpm):
    out = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import carparkingmaps_amd; print('scipy' in sys.modules)" % ROOT],
                         capture_output=True, text=True)
    assert out.stdout.strip() == "False", out
