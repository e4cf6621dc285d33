"""The sweep's objectives on the device (include/cpm_objectives.h), on the GPU.  The kernels read any int64 tensor, so the edge cases
run on count tensors made with numpy and uploaded through torch: no tables, no cars, no resample.  The end-to-end and sharded cases
run at tests/golden/small_z24.npz's shape."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from objectives_cases import LADDER_T, LADDER_Z, bound, make_case, scalar_of, tensor

gpu = pytest.mark.gpu
T = 24
GUARD = 16                                   # words on either side of both outputs
SENT = 0x5A5A5A5A5A5A5A5A                    # what the guards hold (as f64: 2.9e130, not a value the kernels write)
NAN_BITS = 0x7FF8000000000000
CPM_ERR_ARG = -1


def _run(s, counts, n_cars, zone_err=True):
    """objectives_dev on `counts` ((B, 2*T*Z + 2) int64): (records (B, 4 + 2*T) int64, zone errors (B, Z) float64 or None).  Both
    outputs lie between guard words, which must come back untouched; the counts are read only."""
    import torch
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1, s.counts_words())
    B, ow = counts.shape[0], s.objective_words()
    dev = torch.from_numpy(counts).cuda()
    obj = torch.full((2 * GUARD + B * ow,), SENT, dtype=torch.int64, device="cuda")
    zerr = torch.full((2 * GUARD + B * s.Z,), SENT, dtype=torch.int64, device="cuda") if zone_err else None
    torch.cuda.synchronize()                 # (the context enqueues on a stream of its own)
    s.objectives_dev(dev.data_ptr(), B, n_cars, obj.data_ptr() + 8 * GUARD, zerr.data_ptr() + 8 * GUARD if zone_err else 0)
    s.sync()
    obj = obj.cpu().numpy()
    assert np.all(obj[:GUARD] == SENT) and np.all(obj[-GUARD:] == SENT), "a store outside d_obj"
    assert np.array_equal(dev.cpu().numpy(), counts), "the counts are read only"
    ze = None
    if zone_err:
        z = zerr.cpu().numpy()
        assert np.all(z[:GUARD] == SENT) and np.all(z[-GUARD:] == SENT), "a store outside d_zone_err"
        ze = z[GUARD:-GUARD].reshape(B, s.Z).view(np.float64)
    return obj[GUARD:-GUARD].reshape(B, ow), ze


def _check_fleet(rec, ze, case, status=0, measured=True):
    """One fleet's record and zone errors against the host restatement."""
    from carparkingmaps_amd import model_selection as ms
    Tc, Z = case["T"], case["Z"]
    err, valid = ms.parking_density_zone_errors(case["parking"], case["n_cars"], case["measured"] if measured else None)
    assert rec[0] == status and rec[1] == case["sum_tt_q16"]
    assert rec[2] == valid.sum()
    assert np.array_equal(rec[4:4 + Tc], case["driving"].sum(axis=0)) and np.array_equal(rec[4 + Tc:], case["parking"].sum(axis=0))
    if ze is not None:
        assert np.array_equal(ze.view(np.uint64), err.view(np.uint64))
    got = float(rec[3:4].view(np.float64)[0])
    if status != 0 or not valid.any():
        assert rec[3] == NAN_BITS
    else:
        want = scalar_of(err, valid)
        rel = abs(got - want) / abs(want)
        print(f"Z={Z} T={Tc}: parking_error {got!r} against {want!r}, relative {rel:.3e}, bound {bound(Z, Tc):.3e}")
        assert rel <= bound(Z, Tc)
    return got


# ------------------------------------------------------------------------------------------------ 1: the ladder
@gpu
@pytest.mark.parametrize("Tc", LADDER_T)
@pytest.mark.parametrize("Z", LADDER_Z)
def test_ladder_of_made_up_tensors(cpm, Z, Tc):
    c = make_case(Z, Tc)
    counts = tensor(c["parking"], c["driving"], c["sum_tt_q16"])
    with cpm.Sampler(Z, Tc) as s:
        assert s.objective_words() == 4 + 2 * Tc
        s.set_measured(c["measured"])
        rec, ze = _run(s, counts, c["n_cars"])
        _check_fleet(rec[0], ze[0], c)
        if Tc == 1:
            assert rec[0, 2] == 0 and rec[0, 3] == NAN_BITS
        again, ze2 = _run(s, counts, c["n_cars"])
        assert np.array_equal(rec, again) and np.array_equal(ze.view(np.uint64), ze2.view(np.uint64))
        without, none = _run(s, counts, c["n_cars"], zone_err=False)      # the zone errors are optional
        assert none is None and np.array_equal(rec, without)


# ------------------------------------------------------------------------------------------------ 2: batches
@gpu
@pytest.mark.parametrize("B", [1, 3, 64])
def test_fleet_b_of_a_batch_gives_the_bits_of_a_single_call(cpm, B):
    Z = 257
    cases = [make_case(Z, T, seed=7 * b + 1) for b in range(B)]
    measured, n_cars = cases[0]["measured"], cases[0]["n_cars"]
    bad = 1 if B > 1 else None                # one fleet with its status word set
    counts = np.stack([tensor(c["parking"], c["driving"], c["sum_tt_q16"], status=(2 if b == bad else 0)) for b, c in enumerate(cases)])
    with cpm.Sampler(Z, T) as s:
        s.set_measured(measured)
        rec, ze = _run(s, counts, n_cars)
        for b, c in enumerate(cases):
            one, ze1 = _run(s, counts[b], n_cars)
            assert np.array_equal(rec[b], one[0]), b
            assert np.array_equal(ze[b].view(np.uint64), ze1[0].view(np.uint64)), b
            _check_fleet(rec[b], ze[b], dict(c, measured=measured), status=(2 if b == bad else 0))
        if bad is not None:                   # NaN and the status copied; the neighbours are those of the batch without the flag
            assert rec[bad, 0] == 2 and rec[bad, 3] == NAN_BITS
            clean = counts.copy()
            clean[bad, -1] = 0
            rec0, ze0 = _run(s, clean, n_cars)
            keep = [b for b in range(B) if b != bad]
            assert np.array_equal(rec[keep], rec0[keep]) and np.array_equal(ze.view(np.uint64), ze0.view(np.uint64))
            assert np.array_equal(rec[bad, 4:], rec0[bad, 4:]) and rec[bad, 1] == rec0[bad, 1] and rec[bad, 2] == rec0[bad, 2]
            assert rec0[bad, 3] != NAN_BITS


# ------------------------------------------------------------------------------------------------ 3: measured data and arguments
@gpu
def test_without_measured_data_and_after_forgetting_it(cpm):
    Z = 65
    c = make_case(Z, T)
    counts = tensor(c["parking"], c["driving"], c["sum_tt_q16"])
    with cpm.Sampler(Z, T) as s:
        rec, ze = _run(s, counts, c["n_cars"])
        assert rec[0, 2] == 0 and rec[0, 3] == NAN_BITS and np.all(ze == -1.0)
        _check_fleet(rec[0], ze[0], c, measured=False)
        s.set_measured(c["measured"])
        with_m, _ = _run(s, counts, c["n_cars"])
        assert with_m[0, 2] > 0 and with_m[0, 3] != NAN_BITS
        s.set_measured(None)
        rec2, ze2 = _run(s, counts, c["n_cars"])
        assert np.array_equal(rec, rec2) and np.array_equal(ze.view(np.uint64), ze2.view(np.uint64))


@gpu
def test_nan_or_infinite_measured_entries_and_bad_arguments_are_refused(cpm):
    import torch
    from carparkingmaps_amd import _lib
    Z = 65
    c = make_case(Z, T)
    counts = tensor(c["parking"], c["driving"], c["sum_tt_q16"])
    with cpm.Sampler(Z, T) as s:
        s.set_measured(c["measured"])
        want, _ = _run(s, counts, c["n_cars"])
        for poison in (float("nan"), float("inf"), -float("inf")):
            m = c["measured"].copy()
            m[Z - 1, T - 1] = poison
            with pytest.raises(_lib.CpmError) as e:
                s.set_measured(m)
            assert e.value.status == CPM_ERR_ARG
        got, _ = _run(s, counts, c["n_cars"])             # what was installed is still there
        assert np.array_equal(got, want)
        with pytest.raises(ValueError):
            s.set_measured(c["measured"][:, :T - 1])
        dev = torch.from_numpy(counts).cuda()
        obj = torch.zeros(s.objective_words(), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for args in ((0, 1, 10, obj.data_ptr()), (dev.data_ptr(), 1, 10, 0), (dev.data_ptr(), 0, 10, obj.data_ptr()),
                     (dev.data_ptr(), -1, 10, obj.data_ptr()), (dev.data_ptr(), cpm.CPM_MAX_BATCH + 1, 10, obj.data_ptr()),
                     (dev.data_ptr(), 1, 0, obj.data_ptr()), (dev.data_ptr(), 1, -5, obj.data_ptr())):
            with pytest.raises(_lib.CpmError) as e:
                s.objectives_dev(*args)
            assert e.value.status == CPM_ERR_ARG, args
        s.sync()
        assert not obj.cpu().numpy().any()                # a refused call enqueues nothing
    L = _lib.load()
    assert L.cpm_set_measured(None, None) == CPM_ERR_ARG and L.cpm_objectives_dev(None, None, 1, 1, None, None) == CPM_ERR_ARG


@gpu
def test_the_last_zone_of_a_partial_workgroup_is_the_only_valid_zone(cpm):
    from carparkingmaps_amd import model_selection as ms
    Z = 257
    c = make_case(Z, T)
    c["parking"] = np.random.default_rng(5).integers(0, 3000, size=(Z, T)).astype(np.int64)   # no flat zone
    c["measured"][:256] = 0.0
    c["measured"][256] = np.random.default_rng(6).uniform(0.1, 1, T)
    with cpm.Sampler(Z, T) as s:
        s.set_measured(c["measured"])
        rec, ze = _run(s, tensor(c["parking"], c["driving"], c["sum_tt_q16"]), c["n_cars"])
    err, valid = ms.parking_density_zone_errors(c["parking"], c["n_cars"], c["measured"])
    assert valid.sum() == 1 and valid[256]
    _check_fleet(rec[0], ze[0], c)
    assert rec[0, 2] == 1 and rec[0, 3] == err[256:257].view(np.int64)[0]      # one term: the scalar IS the zone's error


@gpu
@pytest.mark.parametrize("base", [2 ** 31, 2 ** 40])
def test_large_counts_give_exact_hour_sums(cpm, base):
    Z = 257
    c = make_case(Z, T)
    c["parking"] = c["parking"] + base
    c["driving"] = c["driving"] + base
    c["n_cars"] = int(c["parking"].sum(axis=0).max())
    assert int(c["parking"].sum(axis=0).max()) > 2 ** 31 * Z and c["parking"].max() < 2 ** 53
    with cpm.Sampler(Z, T) as s:
        s.set_measured(c["measured"])
        rec, ze = _run(s, tensor(c["parking"], c["driving"], c["sum_tt_q16"]), c["n_cars"])
    _check_fleet(rec[0], ze[0], c)


# ------------------------------------------------------------------------------------------------ 4: end to end, the sweep
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_z24.npz"))
    return g, int(g["Z"]), int(g["cpz"]), int(g["sim_seed"])


def _lane(cpm, g, Z, cpz, seed, first=0, stride=1):
    import torch
    s = cpm.Sampler(Z, T, stream=torch.cuda.Stream())
    s.set_datamatrix(np.asfortranarray(g["datamatrix"]), np.asfortranarray(g["dist"]))
    s.build_p_drive(0.1, 0.9, 0.5, want=False)
    s.build_p_dest(2, want=False)
    s.init_states(Z * cpz, cpz, first, car_stride=stride)
    s.solve_ivp(seed, want=False)
    return s


@gpu
def test_sweep_with_device_objectives_equals_the_host_sweep(cpm):
    from carparkingmaps_amd import model_selection as ms
    g, Z, cpz, seed = _golden()
    C = Z * cpz
    rng = np.random.default_rng(9)
    act, park = rng.uniform(0, 1, T), rng.uniform(0, 1, (Z, T))
    park[rng.random(Z) < 0.3] = 0.0
    grid = [ms.Point(a, b, 0.9, d) for d in (2, 1) for a in (0.5, 2.0) for b in (0.0, 0.1)]      # 2 x 2 x 1 x 2
    s = _lane(cpm, g, Z, cpz, seed)
    try:
        host = ms.Evaluator(s, C, seed, act, park, travel=True)
        dev = ms.Evaluator(s, C, seed, act, park, travel=True, device_objectives=True)
        assert dev.device_objectives and not host.device_objectives
        for batch in (None, 4):
            want = ms.grid_sweep(host, grid, batch=batch)
            got = ms.grid_sweep(dev, grid, batch=batch)
            for a, b, pt in zip(got, want, grid):
                for k in ("activity_error", "A_drive", "driving_total", "hours_hold_all_cars", "fallback"):
                    assert a[k] == b[k], (batch, pt, k)
                rel = abs(a["parking_error"] - b["parking_error"]) / abs(b["parking_error"])
                print(f"batch={batch} {pt}: parking_error {a['parking_error']!r} against {b['parking_error']!r}, relative {rel:.3e}")
                assert rel <= bound(Z, T), (batch, pt)
                assert a["hours_hold_all_cars"] and a["driving_total"] > 0 and a["A_drive"] > 0
        # the blocking form: its host counts go through objectives_dev as well, and word 1 is the travel-time sum
        pt = grid[3]
        e_dev, e_host = dev.evaluate(pt), host.evaluate(pt)
        assert "parking" not in e_dev and "driving" not in e_dev
        assert e_dev["A_drive"] == e_host["A_drive"] == ms.a_drive(s.resample(seed, travel=True)["sum_tt_q16"], C, T)
        assert e_dev["activity_error"] == e_host["activity_error"] and np.array_equal(e_dev["traffic_activity"], e_host["traffic_activity"])
        assert abs(e_dev["parking_error"] - e_host["parking_error"]) <= bound(Z, T) * abs(e_host["parking_error"])
        assert e_dev["parking_error"] == [r for r, p in zip(got, grid) if p is pt][0]["parking_error"]   # one definition, pipelined or blocking
        with pytest.raises(ValueError, match="checksums"):
            ms.grid_sweep(dev, grid, checksums=True)
    finally:
        s.close()


@gpu
def test_record_of_a_resample_with_travel_times_carries_sum_tt_q16(cpm):
    import torch
    g, Z, cpz, seed = _golden()
    s = _lane(cpm, g, Z, cpz, seed)
    try:
        r = s.resample(seed, travel=True)
        with torch.cuda.stream(s._stream_obj):
            counts = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
            obj = torch.zeros(s.objective_words(), dtype=torch.int64, device="cuda")
            s.resample_dev(seed, counts.data_ptr(), travel=True)
            s.objectives_dev(counts.data_ptr(), 1, Z * cpz, obj.data_ptr())
            rec = obj.cpu().numpy()
        assert rec[0] == 0 and rec[1] == r["sum_tt_q16"] and r["sum_tt_q16"] > 0
        assert np.array_equal(rec[4:4 + T], r["driving"].sum(axis=0)) and np.all(rec[4 + T:] == Z * cpz)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ 5: shards
@gpu
def test_two_shards_summed_give_the_bits_of_the_whole_fleet(cpm):
    import torch
    g, Z, cpz, seed = _golden()
    C = Z * cpz
    measured = np.random.default_rng(10).uniform(0, 1, (Z, T))
    lanes = [_lane(cpm, g, Z, cpz, seed), _lane(cpm, g, Z, cpz, seed, 0, 2), _lane(cpm, g, Z, cpz, seed, 1, 2)]
    try:
        tensors = []
        for s in lanes:
            with torch.cuda.stream(s._stream_obj):
                t = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda")
                s.resample_dev(seed, t.data_ptr(), travel=True)
            s.sync()
            tensors.append(t)
        torch.cuda.synchronize()
        whole, summed = tensors[0].cpu().numpy(), (tensors[1] + tensors[2]).cpu().numpy()   # (the all-reduce of two ranks)
        assert whole[-1] == 0 and summed[-1] == 0
        assert np.array_equal(whole, summed)
        assert lanes[1].car_count + lanes[2].car_count == C
        s = lanes[1]                               # a shard's context reduces the summed tensor with the fleet's car count
        s.set_measured(measured)
        lanes[0].set_measured(measured)
        rec_sum, ze_sum = _run(s, summed, C)
        rec_whole, ze_whole = _run(lanes[0], whole, C)
        assert np.array_equal(rec_sum, rec_whole) and np.array_equal(ze_sum.view(np.uint64), ze_whole.view(np.uint64))
        assert rec_whole[0, 2] > 0 and rec_whole[0, 3] != NAN_BITS
        shard, _ = _run(s, tensors[1].cpu().numpy(), s.car_count)     # before the reduce the divisor is the shard's count
        assert np.all(shard[0, 4 + T:] == s.car_count)
    finally:
        for s in lanes:
            s.close()
