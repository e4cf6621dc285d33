"""Sparse row packs for an UPLOADED p_destin (CPM_OPT_SPARSE_UPLOAD, csrc/cpm_upload.h): cpm_set_p_dest compacts the dense array on the
device and installs the packs cpm_build_p_dest gives a sparse datamatrix's tables, when the table qualifies (no (hour, origin) row with
more than 512 non-zero entries, the sparse pack of the longest row at most 60 % of the dense one); dense packs otherwise.

Expected values come from the oracle (O.fast_run on O.build_cdf(p_dest); first j with u <= np.cumsum), never from the library's
other route alone; where both routes run they are compared with each other in addition.  GPU tests are marked `gpu`; the restatement
of the pack's definition and the host-layer checks at the end run without one."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SIM_SEED, TABLE_SEED
from dataset_edges import _probe_k53, _ref_categorical
from product_form import GROUPED, pinned

gpu = pytest.mark.gpu
INFO_SPARSE = 6      # CPM_INFO_SPARSE_TABLES
ERR_TABLE = -4       # CPM_ERR_TABLE


def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


def _row_cells(p_dest):
    """non-zero entries of the longest (origin, hour) row (numpy: -0.0 != 0 is False, as on the device)"""
    return int((p_dest != 0).sum(axis=1).max())


def _z700(O):
    Z, T = 700, 24
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06)
    return Z, T, dm, dist


def _same_counts(a, b):
    return np.array_equal(a["parking"], b["parking"]) and np.array_equal(a["driving"], b["driving"])


# ------------------------------------------------------------------------------------------------ 1: the route
@gpu
def test_an_uploaded_sparse_table_gets_sparse_row_packs(cpm, O):
    """The test that fails without the feature: cpm_set_option knows no option 7 there, and CPM_INFO_SPARSE_TABLES is 0 after any upload.
    The generator fills each cell independently with probability 0.06 (oracle/cpm_oracle.c), so a row holds Binomial(700, 0.06) cells:
    mean 42, sigma 6.3, the longest of 16,800 rows about 70; the dense pack is 868 words, a sparse one of up to 192 cells 372 <= 520."""
    Z, T, dm, dist = _z700(O)
    p_dest = O.createpdestin(dm, Z, T, 2)
    assert _row_cells(p_dest) <= 192                         # the input qualifies (checked before anything touches the GPU)
    with cpm.Sampler(Z, T) as s:
        s.set_sparse_upload(True)
        s.set_p_dest(p_dest)
        info_upload = s.get_info(INFO_SPARSE)
        assert info_upload > 0
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        s.build_p_dest(2, want=False)
        info_built = s.get_info(INFO_SPARSE)
    # (the dataset keeps cells of weight zero -- the pair's minimum over the day -- that the upload drops)
    assert 0 < info_upload <= info_built, (info_upload, info_built)


# ------------------------------------------------------------------------------------------------ 2: draws
@gpu
def test_draws_on_below_and_above_every_breakpoint(cpm, O):
    Z, T, dm, dist = _z700(O)
    p_dest = O.createpdestin(dm, Z, T, 2)
    rng = np.random.default_rng(6)
    with cpm.Sampler(Z, T) as s:
        s.set_sparse_upload(True)
        s.set_p_dest(p_dest)
        assert s.get_info(INFO_SPARSE) > 0
        total_exact = 0
        for (o, t) in [(1, 1), (8, 3), (Z, T), (100, 12), (12, 6)]:
            cdf = np.cumsum(p_dest[o - 1, :, t - 1])
            k53 = _probe_k53(cdf, rng)
            got, n_exact = s.debug_categorical(o, t, k53)
            assert np.array_equal(got, _ref_categorical(cdf, k53)), (o, t)
            total_exact += n_exact
            assert np.array_equal(s.get_cdf_row(o, t), cdf), (o, t)   # the f64 rows of the uploaded bytes, bit for bit
        assert total_exact > 100                                      # (ties walk the uploaded cells)
        assert s.get_info(INFO_SPARSE) > 0


# ------------------------------------------------------------------------------------------------ 3: counts, families, travel, batch
@gpu
def test_counts_of_every_family_with_travel_times_and_a_batch(cpm, O):
    """The datamatrix, fleet and seed of tests/test_gpu_parity.py::test_sparse_dataset_tables_equal_the_dense_ones (an origin without
    data and a (mean 0, std > 0) cell included), its p_destin computed by the ORACLE and uploaded.  The step record is the one that
    test documents -- it depends on the bucket regions, not on the pack: one context serves the three kernel passes, the first
    travel resample (AUTO) meets a run longer than the regions at the 1,024-slot floor and is repeated three times up to 32x the
    mean bucket, every other step runs on the regions as they are.  (Observed on the uploaded packs: exactly that record -- AUTO's IVP at
    4x without a repeat, its travel resample 3 repeats to 32x, kernels 2 and 5 no repeat -- so the shorter rows change nothing here.)"""
    Z, T, cpz = 700, 24, 60
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06)
    dm[7, :, :, :] = 0.0
    dm[11, 13, 5, 0], dm[11, 13, 5, 1] = 0.0, 5.0
    dm = np.asfortranarray(dm)
    p_dest = O.createpdestin(dm, Z, T, 2)
    assert _row_cells(p_dest) <= 192
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)                           # travel times come from the datamatrix, whichever way the tables arrived
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        np.testing.assert_allclose(p_drive, O.createpdrive(dm, dist, Z, T, 0.1, 0.9, 0.5), rtol=4e-16, atol=0, equal_nan=True)
        s.set_sparse_upload(True)
        s.set_p_dest(p_dest)
        assert s.get_info(INFO_SPARSE) > 0
        ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), datamatrix=dm, dist=dist)
        for kernel in (0, 2, 5):
            s.set_kernel(kernel)
            s.init_states(C, cpz)
            first = kernel == 0
            with pinned(s, kernel, cap_mult=4 if first else 32) as ivp:
                assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"]), kernel
            with pinned(s, kernel, repeats=3 if first else 0, cap_mult=32) as step:
                r = s.resample(SIM_SEED, travel=True)
            print(f"kernel {kernel}: ivp {ivp} resample {step}")
            assert _same_counts(r, ref), kernel
            assert r["sum_tt_q16"] == ref["sum_tt_q16"], kernel
        assert s.get_info(INFO_SPARSE) > 0
        # one batched resample on the uploaded packs: each fleet equals its single resample
        s.set_kernel(0)
        rng = np.random.default_rng(3)
        # (fleets that drive no more than the fleet above: a fleet whose runs outgrow the regions, which cannot grow beyond 64x here,
        #  is handed to the single path by the batch call -- include/cpm_batch.h -- and would say nothing about the batched kernels)
        tables = np.asfortranarray(np.stack([p_drive, p_drive * rng.uniform(0.5, 1.0, (Z, T)), p_drive * 0.75], axis=2))
        seeds = np.array([SIM_SEED, SIM_SEED, SIM_SEED + 1], dtype=np.uint64)
        s.set_p_drive_batch(tables)
        rb = s.resample_batch(seeds, travel=True)
        assert s.get_info(cpm.CPM_INFO_LAST_KERNEL) == GROUPED and s.get_info(cpm.CPM_INFO_LAST_FORM) == cpm.CPM_FORM_BATCH
        fleets = s.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS)
        print(f"fleets the batched kernels produced: {fleets} of 3")
        assert fleets >= 1
        for b in range(3):
            s.set_p_drive(np.asfortranarray(tables[:, :, b]))
            one = s.resample(int(seeds[b]), travel=True)
            assert np.array_equal(rb["parking"][:, :, b], one["parking"]) and np.array_equal(rb["driving"][:, :, b], one["driving"]), b
            assert int(rb["sum_tt_q16"][b]) == one["sum_tt_q16"], b
        assert np.array_equal(rb["parking"][:, :, 0], ref["parking"]) and int(rb["sum_tt_q16"][0]) == ref["sum_tt_q16"]


# ------------------------------------------------------------------------------------------------ 4: edge rows
def _edge_table(Z, T, rng):
    w = rng.random((Z, Z, T)) ** 2
    w[rng.random((Z, Z, T)) >= 0.1] = 0.0                    # ordinary sparse rows: Binomial(403, 0.1) cells, mean 40, sigma 6
    w[:, 77, :] = 0.0                                        # a zone no row leads to
    tot = w.sum(axis=1, keepdims=True)
    p = np.divide(w, tot, out=np.zeros_like(w), where=tot > 0)
    p[5, :, :] = 0.0                                         # an all-zero row: destination = origin, still driving
    p[9, :, :] = 0.0
    p[9, 17, :] = 1.0                                        # a single-destination row
    p[20, :, :] *= 0.5                                       # a row summing to 0.5 and one to 1.5: D1 at both ends
    p[21, :, :] *= 1.5
    blk = p[30:40]
    blk[blk == 0.0] = -0.0                                   # entries of -0.0: no cell, no change to any sum
    p[50, :, :] = 0.0
    p[50, Z - 1, :] = 1.0                                    # a row whose only weight is the last zone
    p[Z - 1, :, 0] = 0.0
    p[Z - 1, 0, 0] = 0.25                                    # (the last origin: Z is not a multiple of 64)
    p[Z - 1, Z - 1, 0] = 0.75
    return np.asfortranarray(p)


@gpu
def test_edge_rows_of_a_hand_made_table(cpm, O):
    """Z = 403, T = 6, 40 cars per zone: T != 24, Z not a multiple of 32, AUTO takes the grouped path.  The dense pack is 516 words and a
    sparse one of <= 96 cells 256 <= 309: the table qualifies."""
    Z, T, cpz = 403, 6, 40
    C = Z * cpz
    rng = np.random.default_rng(41)
    p_dest = _edge_table(Z, T, rng)
    assert _row_cells(p_dest) <= 96
    assert np.signbit(p_dest[30:40]).any() and not (p_dest[:, 77, :] != 0).any() and not (p_dest[5] != 0).any()
    p_drive = np.asfortranarray(rng.random((Z, T)))
    p_drive[rng.random((Z, T)) < 0.05] = 0.0
    p_drive[rng.random((Z, T)) < 0.05] = 1.0
    p_drive[rng.random((Z, T)) < 0.02] = np.nan
    p_drive[[5, 9, 20, 21, 50, Z - 1], :] = 0.8              # (the special rows are drawn from)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz))
    got = {}
    for sparse in (True, False):
        with cpm.Sampler(Z, T) as s:
            s.set_sparse_upload(sparse)
            s.set_p_drive(p_drive)
            s.set_p_dest(p_dest)
            assert (s.get_info(INFO_SPARSE) > 0) == sparse
            for kernel in (0, 5):
                s.set_kernel(kernel)
                s.init_states(C, cpz)
                with pinned(s, kernel, family=GROUPED, repeats=None):
                    assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"]), (sparse, kernel)
                with pinned(s, kernel, family=GROUPED, repeats=None):
                    r = s.resample(SIM_SEED)
                assert _same_counts(r, ref), (sparse, kernel)
                got[sparse, kernel] = r
            for (o, t) in [(6, 1), (10, 2), (21, 3), (22, 4), (35, 5), (51, 6), (Z, 1)]:
                cdf = np.cumsum(p_dest[o - 1, :, t - 1])
                k53 = _probe_k53(cdf, rng)
                assert np.array_equal(s.debug_categorical(o, t, k53)[0], _ref_categorical(cdf, k53)), (sparse, o, t)
                assert np.array_equal(s.get_cdf_row(o, t), cdf), (sparse, o, t)
    for kernel in (0, 5):
        assert _same_counts(got[True, kernel], got[False, kernel]), kernel


# ------------------------------------------------------------------------------------------------ 5: fallbacks
def _sparse_table(Z, T, rng, density=0.06):
    w = rng.random((Z, Z, T))
    w[rng.random((Z, Z, T)) >= density] = 0.0
    tot = w.sum(axis=1, keepdims=True)
    return np.asfortranarray(np.divide(w, tot, out=np.zeros_like(w), where=tot > 0))


@gpu
def test_tables_that_do_not_qualify_take_the_dense_packs(cpm, O):
    Z, T, cpz = 700, 6, 40
    C = Z * cpz
    rng = np.random.default_rng(17)
    base = _sparse_table(Z, T, rng)
    assert _row_cells(base) <= 192
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    # (i) ONE row with 513 non-zero entries: counted, never stored -- the whole table takes the dense packs
    long_row = base.copy(order="F")
    long_row[123, :, 2] = 0.0
    long_row[123, :513, 2] = 1.0 / 513
    assert _row_cells(long_row) == 513
    ref = O.fast_run(p_drive, O.build_cdf(long_row), C, SIM_SEED, _zone0(C, cpz))
    with cpm.Sampler(Z, T) as s:
        s.set_sparse_upload(True)
        s.set_p_drive(p_drive)
        s.set_p_dest(long_row)
        assert s.get_info(INFO_SPARSE) == 0
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None):
            r = s.resample(SIM_SEED)
        assert _same_counts(r, ref)
        # (ii) rows of 400 non-zero entries: the sparse pack would be 740 words against 60 % of 868 = 520
        wide = np.zeros((Z, Z, T), order="F")
        wide[:, :400, :] = 1.0 / 400
        assert _row_cells(wide) == 400
        s.set_p_dest(wide)
        assert s.get_info(INFO_SPARSE) == 0
        # ... and a table that qualifies, behind them in the same context
        s.set_p_dest(base)
        assert s.get_info(INFO_SPARSE) > 0
    # (iii) NaN, then a negative entry: CPM_ERR_TABLE on the sparse route too, no table left behind; a valid upload installs cleanly
    ref = O.fast_run(p_drive, O.build_cdf(base), C, SIM_SEED, _zone0(C, cpz))
    with cpm.Sampler(Z, T) as s:
        s.set_sparse_upload(True)
        s.set_p_drive(p_drive)
        s.init_states(C, cpz)
        for bad_value in (np.nan, -0.25):
            bad = base.copy(order="F")
            bad[Z - 1, 3, T - 1] = bad_value
            with pytest.raises(cpm.CpmError) as e:
                s.set_p_dest(bad)
            assert e.value.status == ERR_TABLE
            with pytest.raises(cpm.CpmError):                # (the context is left without a table)
                s.resample(SIM_SEED)
        s.set_p_dest(base)
        assert s.get_info(INFO_SPARSE) > 0
        with pinned(s, 0, family=GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None):
            r = s.resample(SIM_SEED)
        assert _same_counts(r, ref)


# ------------------------------------------------------------------------------------------------ 6: life cycle
@gpu
def test_refresh_and_a_new_datamatrix_leave_the_uploaded_tables_whole(cpm, O):
    Z, T, dm, dist = _z700(O)
    cpz = 60
    C = Z * cpz
    p_dest = O.createpdestin(dm, Z, T, 2)
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz))
    rng = np.random.default_rng(9)
    with cpm.Sampler(Z, T) as s:
        s.set_sparse_upload(True)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        info = s.get_info(INFO_SPARSE)
        assert info > 0
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, repeats=None):
            init = s.solve_ivp(SIM_SEED)
        assert np.array_equal(init, ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=None):
            r0 = s.resample(SIM_SEED)
        assert _same_counts(r0, ref)
        s.refresh_tables()                                   # NO datamatrix in the context: the packs come from the table's own cells
        assert s.get_info(INFO_SPARSE) == info
        with pinned(s, 0, family=GROUPED):
            r1 = s.resample(SIM_SEED)
        assert _same_counts(r1, ref)
        # another dataset swept into the compact rows behind the installed tables: they are the upload's, not dm2's
        dm2, dist2 = O.synth_datamatrix(Z, T, TABLE_SEED + 1, density=0.06)
        s.set_datamatrix(dm2, dist2)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.set_p_drive(p_drive)
        s.refresh_tables()
        assert s.get_info(INFO_SPARSE) == info
        total_exact = 0
        for (o, t) in [(1, 1), (8, 3), (Z, T), (100, 12), (12, 6)]:
            cdf = np.cumsum(p_dest[o - 1, :, t - 1])
            k53 = _probe_k53(cdf, rng)
            got, n_exact = s.debug_categorical(o, t, k53)
            assert np.array_equal(got, _ref_categorical(cdf, k53)), (o, t)
            total_exact += n_exact
        assert total_exact > 100
        with pinned(s, 0, family=GROUPED):
            r2 = s.resample(SIM_SEED)
        assert _same_counts(r2, ref)
        # the option back to 0 and the same array again: dense packs, the same counts
        s.set_sparse_upload(False)
        assert s.get_info(INFO_SPARSE) == info               # (read when a table is installed, not afterwards)
        s.set_p_dest(p_dest)
        assert s.get_info(INFO_SPARSE) == 0
        with pinned(s, 0, family=GROUPED):
            r3 = s.resample(SIM_SEED)
        assert _same_counts(r3, ref)


# ------------------------------------------------------------------------------------------------ 7: full size
@gpu
def test_full_size_melbourne_shape_uploaded(cpm, O):
    """configs[0]'s shape, Z = 2,357 x 100 cars per zone, the datamatrix of tests/test_full_size.py: the oracle's createpdestin uploaded
    with the option on, travel times from the datamatrix.  Rows hold Binomial(2,357, 0.0868) cells: mean 205, sigma 13.7, the longest
    of 56,568 about 265."""
    Z, T, cpz = 2357, 24, 100
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED)
    p_dest = O.createpdestin(dm, Z, T, 2)
    assert _row_cells(p_dest) <= 512                         # (before anything touches the GPU)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        np.testing.assert_allclose(p_drive, O.createpdrive(dm, dist, Z, T, 0.1, 0.9, 0.5), rtol=4e-16, atol=0, equal_nan=True)
        s.set_sparse_upload(True)
        s.set_p_dest(p_dest)
        assert s.get_info(INFO_SPARSE) > 0
        cdf = O.build_cdf(p_dest)
        del p_dest
        ref = O.fast_run(p_drive, cdf, C, SIM_SEED, _zone0(C, cpz), datamatrix=dm, dist=dist)
        del cdf
        s.init_states(C, cpz)
        with pinned(s, 0, family=GROUPED, repeats=0):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, 0, family=GROUPED, repeats=0) as step:
            r = s.resample(SIM_SEED, travel=True)
        print(f"step record {step}, sparse pack words {s.get_info(INFO_SPARSE)}")
    assert _same_counts(r, ref)
    assert r["sum_tt_q16"] == ref["sum_tt_q16"]
    assert (r["parking"].sum(axis=0) == C).all()


# ------------------------------------------------------------------------------------------------ without a GPU
def _pack_of_row(row, nc):
    """compact, running sum, high words: the sparse pack's definition (csrc/cpm_upload.h) restated for one dense row"""
    j = np.flatnonzero(row != 0)                             # cells in destination order; -0.0 is no cell
    run = np.cumsum(row[j])                                  # range_up = range_up + distribution[j], left to right
    hi = np.where(run < 1.0, np.floor(np.minimum(run, 1.0) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint64)
    total = run[-1] if len(j) else 0.0
    last_hi = hi[-1] if len(j) else np.uint64(2 ** 32 - 1)
    hi = np.concatenate([hi, np.full(nc - len(j), last_hi, dtype=np.uint64)])
    idx = np.concatenate([j, np.full(nc - len(j), j[-1] if len(j) else 0)])
    return j, run, total, hi, idx


def test_the_pack_definition_against_the_oracle_cdf(O):
    """What k_up_compact / k_up_pack compute, in numpy, against O.build_cdf: the running sum over the kept cells equals the dense
    row's at every cell, bit for bit (the zeros in between add nothing), the row total is its last value, and `first entry with
    hi[e] >= khi` mapped through idx is `first destination with hi_dense[j] >= khi` for every khi that is no tie -- the pack's definition, pinned without a GPU."""
    Z, T = 403, 6
    rng = np.random.default_rng(41)
    p_dest = _edge_table(Z, T, rng)
    cdf = O.build_cdf(p_dest)                                # [t][o][d]
    nc = _row_cells(p_dest)
    assert 0 < nc <= 96
    for (o, t) in [(0, 0), (5, 1), (9, 2), (20, 3), (21, 4), (33, 5), (50, 0), (Z - 1, 0), (200, 3)]:
        row, dense = p_dest[o, :, t], cdf[t, o, :]
        j, run, total, hi, idx = _pack_of_row(row, nc)
        assert np.array_equal(run, dense[j]) and total == dense[-1], (o, t)
        if len(j) == 0:
            assert (dense == 0).all()
            continue
        hi_dense = np.where(dense < 1.0, np.floor(np.minimum(dense, 1.0) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint64)
        keys = np.unique(np.concatenate([hi[: len(j)] + 1, np.maximum(hi[: len(j)], 1) - 1, rng.integers(0, 2 ** 32, size=500).astype(np.uint64)]))
        keys = keys[keys <= hi_dense[-1]]                    # (beyond the row's total D1 clamps the draw: not the search's business)
        keys = keys[~np.isin(keys, hi)]                      # (a key that EQUALS a high word is a tie: the f64 walk over the cells decides it)
        e = np.searchsorted(hi, keys, side="left")
        d = np.searchsorted(hi_dense, keys, side="left")
        assert (e < nc).all() and np.array_equal(idx[e], d), (o, t)


def test_host_layers_know_the_option():
    from carparkingmaps_amd import _lib
    from carparkingmaps_amd.sampler import Sampler
    header = open(os.path.join(ROOT, "include", "cpm.h")).read()
    assert int(re.search(r"#define\s+CPM_OPT_SPARSE_UPLOAD\s+(\d+)", header).group(1)) == _lib.CPM_OPT_SPARSE_UPLOAD == 7
    assert int(re.search(r"#define\s+CPM_INFO_SPARSE_TABLES\s+(\d+)", header).group(1)) == _lib.CPM_INFO_SPARSE_TABLES == INFO_SPARSE
    assert callable(Sampler.set_sparse_upload)
    shim = open(os.path.join(ROOT, "julia", "CarParkingMapsAMD.jl")).read()
    assert re.search(r"cpm_set_option.*CPM_OPT_SPARSE_UPLOAD|CPM_OPT_SPARSE_UPLOAD.*cpm_set_option", shim), "the Julia shim's context() turns the option on"
