"""The batched resample (include/cpm_batch.h) on the GPU: every fleet of a batch bit for bit what the single resample of the same
context returns with that fleet's p_drive installed and its seed -- counts with np.array_equal, travel-time sums exactly -- on dense and
sparse row packs, with and without travel times, through overflow, fallback, the asynchronous form and the sweep.  The step record is
read directly (CPM_INFO_LAST_KERNEL / _LAST_FORM / _LAST_BATCH_FLEETS / _STEPS_REPEATED)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import ROOT, SIM_SEED, TABLE_SEED

pytestmark = pytest.mark.gpu

T = 24


def _record(s):
    from carparkingmaps_amd import _lib
    return dict(kernel=s.get_info(_lib.CPM_INFO_LAST_KERNEL), form=s.get_info(_lib.CPM_INFO_LAST_FORM),
                repeats=s.get_info(_lib.CPM_INFO_STEPS_REPEATED), fleets=s.get_info(_lib.CPM_INFO_LAST_BATCH_FLEETS))


def _singles(s, tables, seeds, travel):
    """fleet b through the single path of the same context: tables[:, :, b] installed as its own p_drive, seeds[b]"""
    keep = s.get_p_drive()
    out = []
    for b in range(tables.shape[2]):
        s.set_p_drive(np.asfortranarray(tables[:, :, b]))
        out.append(s.resample(int(seeds[b]), travel=travel))
    s.set_p_drive(keep)
    return out


def _assert_fleets_equal(r, singles):
    for b, one in enumerate(singles):
        assert np.array_equal(r["parking"][:, :, b], one["parking"]), f"fleet {b}: parking"
        assert np.array_equal(r["driving"][:, :, b], one["driving"]), f"fleet {b}: driving"
        assert int(r["sum_tt_q16"][b]) == one["sum_tt_q16"], f"fleet {b}: travel-time sum"


def _pinned_batch(cpm, s, fleets):
    rec = _record(s)
    assert rec["kernel"] == cpm.CPM_KERNEL_ZONE_GROUPED and rec["form"] == cpm.CPM_FORM_BATCH and rec["fleets"] == fleets, rec


def _dense_tables(O, Z):
    rng = np.random.default_rng(11)
    synth = O.synth_p_drive(Z, T, TABLE_SEED)
    nan_rows = synth.copy()
    nan_rows[::7, :] = np.nan                                # never drives there
    tables = np.stack([synth, np.zeros((Z, T)), np.ones((Z, T)), nan_rows, rng.uniform(0, 1, (Z, T)), rng.uniform(0.2, 0.9, (Z, T))], axis=2)
    seeds = np.array([SIM_SEED] * 5 + [SIM_SEED + 1], dtype=np.uint64)   # (the last fleet: a seed of its own)
    return np.asfortranarray(tables), seeds


@pytest.mark.parametrize("travel", [False, True], ids=["counts", "travel"])
def test_dense_fleets_equal_their_single_resamples_and_the_oracle(cpm, O, travel):
    Z, cpz = 192, 120
    C = Z * cpz
    tables, seeds = _dense_tables(O, Z)
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.3)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        s.set_p_drive(tables[:, :, 0])
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        s.set_p_drive_batch(tables)
        assert s.get_info(cpm.CPM_INFO_BATCH) == 6
        assert np.array_equal(s.get_p_drive_batch(), tables, equal_nan=True)
        repeats = s.get_info(cpm.CPM_INFO_STEPS_REPEATED)
        r = s.resample_batch(seeds, travel=travel)
        _pinned_batch(cpm, s, 6)
        assert s.get_info(cpm.CPM_INFO_STEPS_REPEATED) == repeats
        assert r["parking"].shape == (Z, T, 6) and r["parking"].flags.f_contiguous
        singles = _singles(s, tables, seeds, travel)
    _assert_fleets_equal(r, singles)
    assert (r["driving"][:, :, 1] == 0).all() and (r["driving"][::7, :, 3] == 0).all()
    assert (r["parking"].sum(axis=0) == C).all()
    cdf = O.build_cdf(p_dest)
    for b in (0, 4):
        ref = O.fast_run(np.asfortranarray(tables[:, :, b]), cdf, C, int(seeds[b]), zone0, do_ivp=False,
                         datamatrix=dm if travel else None, dist=dist if travel else None)
        assert np.array_equal(r["parking"][:, :, b], ref["parking"]) and np.array_equal(r["driving"][:, :, b], ref["driving"])
        if travel:
            assert int(r["sum_tt_q16"][b]) == ref["sum_tt_q16"]


def test_the_single_path_is_as_it_was_around_a_batch(cpm, O):
    Z, cpz = 192, 120
    C = Z * cpz
    tables, seeds = _dense_tables(O, Z)
    with cpm.Sampler(Z, T) as s:
        p_drive = O.synth_p_drive(Z, T, TABLE_SEED + 1)
        s.set_p_drive(p_drive)
        s.set_p_dest(O.synth_p_dest_dense(Z, T, TABLE_SEED))
        s.init_states(C, cpz)
        s.solve_ivp(SIM_SEED)
        before = s.resample(SIM_SEED)
        info = {k: s.get_info(k) for k in (cpm.CPM_INFO_CAP_MULT, cpm.CPM_INFO_FUSED, cpm.CPM_INFO_PARTS, cpm.CPM_INFO_FUSED_BAILOUTS)}
        s.set_p_drive_batch(tables)
        s.resample_batch(seeds)
        _pinned_batch(cpm, s, 6)
        assert np.array_equal(s.get_p_drive(), p_drive)
        assert {k: s.get_info(k) for k in info} == info
        after = s.resample(SIM_SEED)
        assert s.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS) == 0 and s.get_info(cpm.CPM_INFO_LAST_FORM) != cpm.CPM_FORM_BATCH
    assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])


def test_sparse_packs_melbourne_shaped(cpm, O):
    Z, cpz = 700, 300
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED)
    pts = [(0.1, 0.9, 0.5), (0.0, 1.0, 2.0), (0.2, 0.7, 0.25), (0.05, 0.5, 1.0), (0.1, 0.9, 0.5)]
    seeds = np.array([SIM_SEED, SIM_SEED, SIM_SEED + 7, SIM_SEED, SIM_SEED + 1], dtype=np.uint64)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        s.init_states(C, cpz)
        s.solve_ivp(SIM_SEED, want=False)
        tables = s.build_p_drive_batch(*zip(*pts), want=True)
        for b, (lo, hi, e) in enumerate(pts):
            assert np.array_equal(tables[:, :, b], s.build_p_drive(lo, hi, e), equal_nan=True), b
        r = s.resample_batch(seeds, travel=True)
        _pinned_batch(cpm, s, len(pts))
        singles = _singles(s, tables, seeds, True)
    _assert_fleets_equal(r, singles)
    assert (r["sum_tt_q16"] > 0).all()


def test_headline_shape_batch_of_eight(cpm):
    c = json.load(open(os.path.join(ROOT, "tests", "golden", "big_checksums.json")))["s4k_dense_z4096_cpz1000"]
    Z, cpz, C = c["Z"], c["cpz"], c["C"]
    rng = np.random.default_rng(8)
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(c["table_seed"])
        s.init_states(C, cpz)
        s.solve_ivp(c["sim_seed"], want=False)
        synth = s.get_p_drive()
        tables = np.stack([synth] + [np.clip(synth * rng.uniform(0.3, 1.2), 0, 1) for _ in range(4)] +
                          [rng.uniform(0.05, 0.95, (Z, T)) for _ in range(3)], axis=2)
        seeds = np.array([c["sim_seed"]] * 5 + [c["sim_seed"] + k for k in (1, 2, 3)], dtype=np.uint64)
        s.set_p_drive_batch(tables)
        repeats = s.get_info(cpm.CPM_INFO_STEPS_REPEATED)
        r = s.resample_batch(seeds)
        _pinned_batch(cpm, s, 8)
        assert s.get_info(cpm.CPM_INFO_STEPS_REPEATED) == repeats
        singles = _singles(s, tables[:, :, 1:], seeds[1:], False)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert sha(r["parking"][:, :, 0].ravel(order="F")) == c["parking_sha256"]
    assert sha(r["driving"][:, :, 0].ravel(order="F")) == c["driving_sha256"]
    assert int(r["driving"][:, :, 0].sum()) == c["driving_total"]
    for b, one in enumerate(singles, start=1):
        assert np.array_equal(r["parking"][:, :, b], one["parking"]) and np.array_equal(r["driving"][:, :, b], one["driving"]), b


def _overflow_context(cpm, O, tables):
    """the datamatrix of test_pipelined_points_that_overflow_are_evaluated_again: trips end in 6 of 192 zones; no IVP"""
    Z, cpz = 192, 120
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.9)
    dm[:, 6:, :, :] = 0.0
    s = cpm.Sampler(Z, T)
    s.set_datamatrix(np.asfortranarray(dm), dist)
    s.build_p_drive(0.1, 0.9, 0.5, want=False)
    s.build_p_dest(2, want=False)
    s.init_states(Z * cpz, cpz)
    s.set_p_drive_batch(tables)
    return s


def test_overflowed_fleets_are_repeated_by_the_blocking_call_and_flagged_by_the_async_one(cpm, O):
    import torch
    Z = 192
    rng = np.random.default_rng(5)
    tables = np.asfortranarray(np.stack([np.zeros((Z, T)), rng.uniform(0.3, 0.9, (Z, T)), np.full((Z, T), 0.5), rng.uniform(0, 1, (Z, T))], axis=2))
    seeds = np.array([SIM_SEED, SIM_SEED, SIM_SEED + 1, SIM_SEED + 2], dtype=np.uint64)
    s = _overflow_context(cpm, O, tables)
    try:
        repeats = s.get_info(cpm.CPM_INFO_STEPS_REPEATED)
        r = s.resample_batch(seeds, travel=True)
        assert s.get_info(cpm.CPM_INFO_STEPS_REPEATED) > repeats
    finally:
        s.close()
    s = _overflow_context(cpm, O, tables)
    try:
        singles = _singles(s, tables, seeds, True)
    finally:
        s.close()
    _assert_fleets_equal(r, singles)
    s = _overflow_context(cpm, O, tables)
    try:
        stream = torch.cuda.Stream()
        s.set_stream(stream)
        nw = s.counts_words()
        d = torch.zeros(s.batch_counts_words(), dtype=torch.int64, device="cuda")
        with torch.cuda.stream(stream):
            s.resample_batch_dev(seeds, d.data_ptr(), travel=True)
        stream.synchronize()
        _pinned_batch(cpm, s, 4)
        flat = d.cpu().numpy().reshape(4, nw)
    finally:
        s.close()
    status = flat[:, -1]
    assert status[0] == 0 and (status[1:] != 0).any(), status     # no car of fleet 0 drives: its regions cannot overflow
    zt = Z * T
    assert np.array_equal(flat[0, :zt].reshape(T, Z).T, singles[0]["parking"])


@pytest.mark.parametrize("case", ["few_cars_per_zone", "zone_lds"])
def test_fallback_to_the_single_fleet_step(cpm, O, case):
    Z = 192
    cpz = 20 if case == "few_cars_per_zone" else 120
    tables, seeds = _dense_tables(O, Z)
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(tables[:, :, 0])
        s.set_p_dest(O.synth_p_dest_dense(Z, T, TABLE_SEED))
        s.init_states(Z * cpz, cpz)
        if case == "zone_lds":
            s.set_kernel(cpm.CPM_KERNEL_ZONE_LDS)
        s.set_p_drive_batch(tables)
        r = s.resample_batch(seeds)
        rec = _record(s)
        assert rec["fleets"] == 0 and rec["form"] != cpm.CPM_FORM_BATCH
        assert rec["kernel"] == (cpm.CPM_KERNEL_CAR if case == "few_cars_per_zone" else cpm.CPM_KERNEL_ZONE_LDS)
        singles = _singles(s, tables, seeds, False)
    _assert_fleets_equal(r, singles)


def test_async_batch_equals_the_blocking_one_and_one_fleet_equals_resample(cpm, O):
    import torch
    Z, cpz = 192, 120
    tables, seeds = _dense_tables(O, Z)
    stream = torch.cuda.Stream()
    with cpm.Sampler(Z, T, stream=stream) as s:
        s.set_p_drive(tables[:, :, 0])
        s.set_p_dest(O.synth_p_dest_dense(Z, T, TABLE_SEED))
        s.init_states(Z * cpz, cpz)
        s.solve_ivp(SIM_SEED, want=False)
        s.set_p_drive_batch(tables)
        blocking = s.resample_batch(seeds)
        nw = s.counts_words()
        d = torch.full((s.batch_counts_words(),), -1, dtype=torch.int64, device="cuda")
        with torch.cuda.stream(stream):
            s.resample_batch_dev(seeds, d.data_ptr())
        stream.synchronize()
        _pinned_batch(cpm, s, 6)
        flat = d.cpu().numpy().reshape(6, nw)
        one = s.resample(SIM_SEED)
        s.set_p_drive_batch(tables[:, :, :1])
        r1 = s.resample_batch(SIM_SEED)
        _pinned_batch(cpm, s, 1)
    zt = Z * T
    assert (flat[:, -1] == 0).all()
    for b in range(6):
        assert np.array_equal(flat[b, :zt].reshape(T, Z).T, blocking["parking"][:, :, b])
        assert np.array_equal(flat[b, zt:2 * zt].reshape(T, Z).T, blocking["driving"][:, :, b])
    assert np.array_equal(r1["parking"][:, :, 0], one["parking"]) and np.array_equal(r1["driving"][:, :, 0], one["driving"])


def _sweep_lanes(cpm, O, lanes):
    import torch
    from carparkingmaps_amd import model_selection as ms
    Z, cpz = 192, 60
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.4)
    rng = np.random.default_rng(3)
    act, park = rng.uniform(0, 1, T), rng.uniform(0, 1, (Z, T))
    samplers, evs = [], []
    for _ in range(lanes):
        s = cpm.Sampler(Z, T, stream=torch.cuda.Stream())
        s.set_datamatrix(dm, dist)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)
        s.init_states(C, cpz)
        s.solve_ivp(SIM_SEED, want=False)
        samplers.append(s)
        evs.append(ms.Evaluator(s, C, SIM_SEED, act, park, travel=True))
    return samplers, evs


def _same_sweeps(got, plain, grid, B):
    for a, b, pt in zip(got, plain, grid):
        assert a is not None and b is not None, pt
        for k in ("parking_crc32", "driving_crc32", "A_drive", "activity_error", "parking_error", "driving_total", "hours_hold_all_cars"):
            assert a[k] == b[k], (B, pt, k)


@pytest.mark.parametrize("lanes", [1, 2])
def test_batched_sweep_equals_the_sweep(cpm, O, lanes):
    from carparkingmaps_amd import model_selection as ms
    grid = [ms.Point(a, b, c, d) for d in (2, 0.5) for a in (0.5, 2.0) for b in (0.0, 0.1) for c in (0.8, 1.0)]
    assert len(grid) == 16
    samplers, evs = _sweep_lanes(cpm, O, lanes)
    try:
        plain = ms.grid_sweep(evs, grid, checksums=True)
        for B in (4, 5):
            _same_sweeps(ms.grid_sweep(evs, grid, checksums=True, batch=B), plain, grid, B)
            assert all(s.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS) > 0 for s in samplers)
    finally:
        for s in samplers:
            s.close()


@pytest.mark.parametrize("B", [4, 8])
def test_batched_sweep_whose_first_batch_is_the_shortest(cpm, O, B):
    """A lane whose first batch is shorter than a later one (3 points of one e_dest, then 8 of another: batches of 3, 4, 4 or of 3, 8):
    the pipeline grows while the batch before is still in flight, and every point's results are those of the unbatched sweep.  The
    batched sweep runs first, on fresh evaluators."""
    from carparkingmaps_amd import model_selection as ms
    grid = [ms.Point(a, 0.1, 0.9, 0.5) for a in (0.5, 1.0, 2.0)] + [ms.Point(a, b, 0.9, 2) for a in (0.5, 1.0, 2.0, 4.0) for b in (0.0, 0.1)]
    by_e_dest = sorted(range(len(grid)), key=lambda i: (float(grid[i].e_dest), type(grid[i].e_dest).__name__, i))
    assert [len(c) for c in ms.batch_cuts(grid, by_e_dest, B)] == ([3, 4, 4] if B == 4 else [3, 8])
    samplers, evs = _sweep_lanes(cpm, O, 1)
    try:
        got = ms.grid_sweep(evs, grid, checksums=True, batch=B)
        assert samplers[0].get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS) > 0
        plain = ms.grid_sweep(evs, grid, checksums=True)
        _same_sweeps(got, plain, grid, B)
        assert all(r["driving_total"] > 0 for r in got)
    finally:
        for s in samplers:
            s.close()


def test_async_batches_grow_their_regions_after_an_overflow(cpm, O):
    """The asynchronous batch step cannot repeat itself, but the context learns from its status words: the steps that follow it run on
    grown regions, until no fleet overflows -- and those counts are the single path's."""
    import torch
    Z = 192
    rng = np.random.default_rng(5)
    # (drivers few enough that grown regions hold the buckets of the 6 zones -- ~30 x the mean -- and the runs behind them)
    tables = np.asfortranarray(np.stack([np.full((Z, T), 0.1), rng.uniform(0.05, 0.2, (Z, T))], axis=2))
    seeds = np.array([SIM_SEED, SIM_SEED + 1], dtype=np.uint64)
    s = _overflow_context(cpm, O, tables)
    try:
        stream = torch.cuda.Stream()
        s.set_stream(stream)
        nw = s.counts_words()
        d = torch.zeros(s.batch_counts_words(), dtype=torch.int64, device="cuda")
        flagged = []
        for _ in range(8):
            with torch.cuda.stream(stream):
                s.resample_batch_dev(seeds, d.data_ptr(), travel=True)
            stream.synchronize()
            _pinned_batch(cpm, s, 2)                                 # (the batched kernels ran every step)
            flat = d.cpu().numpy().reshape(2, nw)
            flagged.append(int((flat[:, -1] != 0).sum()))
            if flagged[-1] == 0:
                break
    finally:
        s.close()
    s = _overflow_context(cpm, O, tables)                            # (a fresh context: its single path grows its own regions)
    try:
        singles = _singles(s, tables, seeds, True)
    finally:
        s.close()
    assert flagged[0] > 0 and flagged[-1] == 0, flagged
    zt = Z * T
    for b in range(2):
        assert np.array_equal(flat[b, :zt].reshape(T, Z).T, singles[b]["parking"]), b
        assert np.array_equal(flat[b, zt:2 * zt].reshape(T, Z).T, singles[b]["driving"]), b
        assert int(flat[b, 2 * zt]) == singles[b]["sum_tt_q16"], b


def test_headline_shape_sixty_four_fleets_in_sub_batches(cpm):
    """B = 64 at the headline shape: more fleets than one run's workspace budget takes (~0.69 GB per fleet against 24 GiB), so the
    call runs them in sub-batches -- every fleet equals its single resample, blocking and asynchronous."""
    import torch
    c = json.load(open(os.path.join(ROOT, "tests", "golden", "big_checksums.json")))["s4k_dense_z4096_cpz1000"]
    Z, cpz, C = c["Z"], c["cpz"], c["C"]
    B = cpm.CPM_MAX_BATCH
    rng = np.random.default_rng(64)
    stream = torch.cuda.Stream()
    with cpm.Sampler(Z, T, stream=stream) as s:
        s.synth_tables(c["table_seed"])
        s.init_states(C, cpz)
        s.solve_ivp(c["sim_seed"], want=False)
        synth = s.get_p_drive()
        tables = np.asfortranarray(np.stack([synth] + [np.clip(synth * rng.uniform(0.2, 1.2), 0, 1) for _ in range(B - 1)], axis=2))
        seeds = np.array([c["sim_seed"] + (k % 5) for k in range(B)], dtype=np.uint64)
        s.set_p_drive_batch(tables)
        r = s.resample_batch(seeds)
        _pinned_batch(cpm, s, B)
        nw = s.counts_words()
        d = torch.zeros(s.batch_counts_words(), dtype=torch.int64, device="cuda")
        with torch.cuda.stream(stream):
            s.resample_batch_dev(seeds, d.data_ptr())
        stream.synchronize()
        flat = d.cpu().numpy().reshape(B, nw)
        singles = _singles(s, tables, seeds, False)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert sha(r["parking"][:, :, 0].ravel(order="F")) == c["parking_sha256"]
    _assert_fleets_equal(r, singles)
    zt = Z * T
    assert (flat[:, -1] == 0).all()
    for b in range(B):
        assert np.array_equal(flat[b, :zt].reshape(T, Z).T, r["parking"][:, :, b]) and np.array_equal(flat[b, zt:2 * zt].reshape(T, Z).T, r["driving"][:, :, b]), b
