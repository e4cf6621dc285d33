"""Expected travel time and distance per zone and hour (include/cpm_expected_travel.h) on the GPU: the trip weights and a fleet's
seconds, kilometres and totals against the exact (rational) form within the header's bounds, against the numpy form within twice
those at the sizes the exact form is too slow for, on uploaded and dataset-built tables; the device entries between guard words; fleet
b of a batch bit for bit the single call; the cache of the weights and every change that must empty it; the device sampler's sums
within the 5.5 cap; the errors, no trace in a later resample, and the Evaluator's noise-free A_drive.

Shapes: Z = 2, 5, 67 put rows off the 16-byte grid (odd Z: the 8-byte form of k_exp_trip) and leave the last strip of 128 origins
partly empty; Z = 192 has fewer 16-byte pairs than a workgroup has lanes, Z = 513 more (and five strips, the last with one origin),
Z = 1,031 is a prime with more than one round of the unrolled destination loop in every segment."""
import functools
import math

import numpy as np
import pytest

import expected_reference as R
import expected_travel_reference as V

gpu = pytest.mark.gpu
T = 24
SEED = 20240611
CAP = 5.5
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4


@functools.lru_cache(maxsize=None)
def _inputs(Z, Tc):
    """(p_drive, p_dest, datamatrix, dist, row tables) -- computed once and shared; nobody writes to them"""
    from oracle import oracle as O
    O.build()
    p_drive, p_dest = V.planted_tables(O, Z, Tc)
    dm, dist = V.planted_datamatrix(O, Z, Tc)
    for a in (p_drive, p_dest, dm, dist):
        a.setflags(write=False)
    return p_drive, p_dest, dm, dist, R.row_tables(p_dest)


def _sampler(cpm, Z, Tc, p_drive, p_dest, dm, dist):
    s = cpm.Sampler(Z, Tc)
    s.set_p_drive(p_drive)
    s.set_p_dest(p_dest)
    s.set_datamatrix(dm, dist)
    return s


def _pi0(Z, given):
    return np.random.default_rng(Z).uniform(0.0, 2.0, Z) if given else None


def _ratio(got, want, tol):
    """max |got - want| / (tol |want|) over f64 arrays; a word whose reference is 0 must be 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.all(got[want == 0.0] == 0.0), "a word whose reference is 0 is not 0"
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(want != 0.0, np.abs(got - want) / (np.broadcast_to(tol, want.shape) * np.abs(want)), 0.0)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ 1: the exact form
@gpu
@pytest.mark.parametrize("Tc", [1, 2, 24])
@pytest.mark.parametrize("Z", [2, 5, 67])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, Tc):
    p_drive, p_dest, dm, dist, tables = _inputs(Z, Tc)
    ew_sec, ew_km = V.exact_trip(p_dest, dm, dist, tables)
    with _sampler(cpm, Z, Tc, p_drive, p_dest, dm, dist) as s:
        w_sec, w_km = s.expected_trip()
        ws, zs = R.worst_ratio(w_sec, ew_sec, V.bound_trip(Z))
        wk, zk = R.worst_ratio(w_km, ew_km, V.bound_trip(Z))
        print(f"Z={Z} T={Tc}: worst error / bound: w_sec {ws:.3f}, w_km {wk:.3f}")
        assert zs and zk, "a weight whose exact value is 0 is not 0"
        assert ws <= 1.0 and wk <= 1.0
        n_sec, n_km = V.numpy_trip(p_dest, dm, dist, tables)
        print(f"  bit-equal to the numpy form in the documented order: {np.array_equal(w_sec, n_sec) and np.array_equal(w_km, n_km)}")
        variants = ((False, False), (True, True), (False, True), (True, False))       # (pi0 given, ivp)
        for given, ivp in variants[:2] if Z * Tc > 1000 else variants:               # (the exact form of 47 operators at Z = 67 takes a second)
            pi0, flags = _pi0(Z, given), R.IVP if ivp else 0
            r = s.expected_travel(pi0, ivp=ivp)
            _, edrv, _ = R.exact_expected(p_drive, p_dest, pi0, flags, tables)
            esec, ekm, etot_s, etot_k = V.exact_travel(edrv, ew_sec, ew_km)
            h = R.operators_behind(Tc, flags)
            tol = np.array([V.bound_travel(Z, k) for k in h])[None, :]
            w1, z1 = R.worst_ratio(r["seconds"], esec, tol)
            w2, z2 = R.worst_ratio(r["km"], ekm, tol)
            w3, z3 = R.worst_ratio(np.array([r["total_seconds"], r["total_km"]]), np.array([etot_s, etot_k], dtype=object),
                                   V.bound_total(Z, Tc, h[-1]))
            print(f"  pi0 given={given} ivp={ivp}: worst error / bound: seconds {w1:.3f}, km {w2:.3f}, totals {w3:.3f}")
            assert z1 and z2 and z3, "a word whose exact value is 0 is not 0"
            assert w1 <= 1.0 and w2 <= 1.0 and w3 <= 1.0
            assert r["A_drive"] == r["total_seconds"] / (Tc * 3600.0)
            _, drv = s.expected(pi0, ivp=ivp)                                          # the densities are those of expected(), bit for bit
            assert np.array_equal(r["seconds"], drv * w_sec) and np.array_equal(r["km"], drv * w_km)


# ------------------------------------------------------------------------------------------------ 2: the numpy form
def _against_numpy(s, p_drive, p_dest, dm, dist, tables, what):
    Z, Tc = p_drive.shape
    n_sec, n_km = V.numpy_trip(p_dest, dm, dist, tables)
    w_sec, w_km = s.expected_trip()
    a, b = _ratio(w_sec, n_sec, 2 * V.bound_trip(Z)), _ratio(w_km, n_km, 2 * V.bound_trip(Z))
    print(f"{what} Z={Z} T={Tc}: worst error / (2 x bound): w_sec {a:.3f}, w_km {b:.3f}; "
          f"bit-equal: {np.array_equal(w_sec, n_sec) and np.array_equal(w_km, n_km)}")
    assert a <= 1.0 and b <= 1.0
    for given, ivp in ((False, False), (True, True)):
        pi0, flags = _pi0(Z, given), R.IVP if ivp else 0
        r = s.expected_travel(pi0, ivp=ivp)
        _, ndrv, _ = R.numpy_expected(p_drive, p_dest, pi0, flags, tables)
        nsec, nkm, ntot_s, ntot_k = V.numpy_travel(ndrv, n_sec, n_km)
        h = R.operators_behind(Tc, flags)
        tol = 2 * np.array([V.bound_travel(Z, k) for k in h])[None, :]
        c, d = _ratio(r["seconds"], nsec, tol), _ratio(r["km"], nkm, tol)
        e = _ratio([r["total_seconds"], r["total_km"]], [ntot_s, ntot_k], 2 * V.bound_total(Z, Tc, h[-1]))
        print(f"  pi0 given={given} ivp={ivp}: seconds {c:.3f}, km {d:.3f}, totals {e:.3f}")
        assert c <= 1.0 and d <= 1.0 and e <= 1.0
    return w_sec, w_km


@gpu
@pytest.mark.parametrize("Z", [192, 513, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc = 3
    p_drive, p_dest, dm, dist, tables = _inputs(Z, Tc)
    assert V.segments(Z, Tc)[0] > 1                                    # (several destination segments at these sizes)
    with _sampler(cpm, Z, Tc, p_drive, p_dest, dm, dist) as s:
        _against_numpy(s, p_drive, p_dest, dm, dist, tables, "uploaded")


# ------------------------------------------------------------------------------------------------ 3: the device entries
@gpu
@pytest.mark.parametrize("Z,Tc", [(5, 2), (67, 24), (192, 3)])
def test_device_entries_write_every_word_and_nothing_else(cpm, Z, Tc):
    import torch
    p_drive, p_dest, dm, dist, _ = _inputs(Z, Tc)
    zt = Z * Tc
    with _sampler(cpm, Z, Tc, p_drive, p_dest, dm, dist) as s:
        w_sec, w_km = s.expected_trip()
        ref = s.expected_travel()
        park, drv = s.expected()

        def guarded(words):
            return torch.full((2 * GUARD + words,), SENT, dtype=torch.int64, device="cuda")

        def body(t, words, written=True):
            a = t.cpu().numpy()
            assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
            if not written:
                assert np.all(a == SENT)
                return None
            assert a.size == 2 * GUARD + words and not np.any(a[GUARD:-GUARD] == SENT), "a word was not written"
            return a[GUARD:-GUARD].view(np.float64)

        d_w = guarded(2 * zt)
        exp = torch.from_numpy(np.concatenate([park.ravel(order="F"), drv.ravel(order="F")])).cuda()
        torch.cuda.synchronize()
        s.expected_trip_dev(d_w.data_ptr() + 8 * GUARD)
        s.sync()
        w = body(d_w, 2 * zt).reshape(2, Tc, Z)
        assert np.array_equal(w[0].T, w_sec) and np.array_equal(w[1].T, w_km)
        for want_travel, want_totals in ((True, True), (True, False), (False, True)):
            d_trav, d_tot = guarded(2 * zt), guarded(2)
            torch.cuda.synchronize()
            s.expected_travel_dev(exp.data_ptr(), 1, d_trav.data_ptr() + 8 * GUARD if want_travel else 0,
                                  d_tot.data_ptr() + 8 * GUARD if want_totals else 0)
            s.sync()
            trav, tot = body(d_trav, 2 * zt, want_travel), body(d_tot, 2, want_totals)
            if want_travel:
                trav = trav.reshape(2, Tc, Z)
                assert np.array_equal(trav[0].T, ref["seconds"]) and np.array_equal(trav[1].T, ref["km"])
            if want_totals:
                assert tot[0] == ref["total_seconds"] and tot[1] == ref["total_km"]
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_dev(exp.data_ptr(), 1, 0, 0)
        assert e.value.status == ERR_ARG
        # any driving density will do: sampled counts / C in the driving half, whatever the parking half holds
        counts = np.random.default_rng(7).integers(0, 50, (Tc, Z)).astype(np.float64) / 4096.0
        exp2 = torch.from_numpy(np.concatenate([np.full(zt, np.nan), counts.ravel()])).cuda()
        d_trav, d_tot = guarded(2 * zt), guarded(2)
        torch.cuda.synchronize()
        s.expected_travel_dev(exp2.data_ptr(), 1, d_trav.data_ptr() + 8 * GUARD, d_tot.data_ptr() + 8 * GUARD)
        s.sync()
        trav = body(d_trav, 2 * zt).reshape(2, Tc, Z)
        assert np.array_equal(trav[0].T, counts.T * w_sec) and np.array_equal(trav[1].T, counts.T * w_km)
        assert body(d_tot, 2)[0] == V.numpy_travel(counts.T, w_sec, w_km)[2]


# ------------------------------------------------------------------------------------------------ 4: the batch contract
@gpu
@pytest.mark.parametrize("Z,Tc", [(67, 24), (513, 3)])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_fleet_b_of_a_batch_gives_the_bits_of_the_single_call(cpm, Z, Tc, B):
    p_drive, p_dest, dm, dist, _ = _inputs(Z, Tc)
    p_drives = np.asfortranarray(np.random.default_rng(100 * B + Z).uniform(0.0, 1.0, (Z, Tc, B)))
    p_drives[:, :, 0] = p_drive
    with _sampler(cpm, Z, Tc, p_drive, p_dest, dm, dist) as s:
        s.set_p_drive_batch(p_drives)
        for ivp in (False, True):
            r = s.expected_travel_batch(ivp=ivp)
            r2 = s.expected_travel_batch(ivp=ivp)
            assert r["seconds"].shape == r["km"].shape == (Z, Tc, B) and r["total_seconds"].shape == r["A_drive"].shape == (B,)
            for k in r:
                assert np.array_equal(r[k], r2[k]), k
            for b in range(B):
                s.set_p_drive(p_drives[:, :, b])
                one = s.expected_travel(ivp=ivp)
                assert np.array_equal(one["seconds"], r["seconds"][:, :, b]) and np.array_equal(one["km"], r["km"][:, :, b]), (b, ivp)
                assert one["total_seconds"] == r["total_seconds"][b] and one["total_km"] == r["total_km"][b], (b, ivp)
                assert one["A_drive"] == r["A_drive"][b]
        assert s.expected_trip_builds() == 1                            # (p_drive does not enter the weights)


# ------------------------------------------------------------------------------------------------ 5: the dataset route
@gpu
def test_tables_built_from_a_datamatrix_go_through_the_dense_array(cpm, O):
    Z, Tc = 358, 24
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.06)
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        s.build_p_dest(2, want=False)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        first = s.expected_travel()                                     # (before anything else asked for the dense array)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        builds = s.expected_trip_builds()
        p_dest = s.build_p_dest(2, want=True)                           # the same tables again, and their array for the references
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        tables = R.row_tables(p_dest)
        assert (tables[1] != Z - 1).mean() > 0.5                        # sparse rows end early: the residuals land all over the destinations
        _against_numpy(s, p_drive, p_dest, dm, dist, tables, "dataset")
        assert s.expected_trip_builds() == builds + 1
        again = s.expected_travel()
        for k in first:
            assert np.array_equal(first[k], again[k]), k


# ------------------------------------------------------------------------------------------------ 6: the cache
@gpu
def test_weights_are_cached_and_rebuilt_after_every_change_of_their_inputs(cpm, O):
    Z, Tc = 67, 24
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    dm, dist = np.asfortranarray(dm), np.asfortranarray(dist)
    p_drive, p_dest = V.planted_tables(O, Z, Tc)

    def check(s, p_dest, dm, dist, builds):
        w_sec, w_km = s.expected_trip()
        assert s.expected_trip_builds() == builds
        n_sec, n_km = V.numpy_trip(p_dest, dm, dist)
        tol = 2 * V.bound_trip(Z)
        assert _ratio(w_sec, n_sec, tol) <= 1.0 and _ratio(w_km, n_km, tol) <= 1.0
        return w_sec, w_km

    with cpm.Sampler(Z, Tc) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.set_datamatrix(dm, dist)
        assert s.expected_trip_builds() == 0
        w0 = check(s, p_dest, dm, dist, 1)
        check(s, p_dest, dm, dist, 1)
        s.set_p_drive(np.asfortranarray(p_drive * 0.5))
        s.expected_travel()
        assert s.expected_trip_builds() == 1
        n = 1
        p2 = np.array(p_dest, order="F")
        p2[1, :, :] *= 0.5
        s.set_p_dest(p2)                                               # -- set_p_dest
        n += 1
        w1 = check(s, p2, dm, dist, n)
        assert not np.array_equal(w0[0], w1[0])
        p3 = s.build_p_dest(2, want=True)                              # -- build_p_dest
        n += 1
        check(s, p3, dm, dist, n)
        s.refresh_tables()                                             # -- refresh_tables: the same tables, built again
        n += 1
        check(s, p3, dm, dist, n)
        dm2 = np.array(dm, order="F")
        dm2[:, :, :, 0] *= 1.5
        s.set_datamatrix(dm2)                                          # -- set_datamatrix with a changed mean (p_dest stays as uploaded)
        n += 1
        w2 = check(s, p3, dm2, dist, n)
        dist2 = np.asfortranarray(dist * 2.0)
        s.set_datamatrix(dm2, dist2)                                   # -- set_datamatrix(dm, dist2)
        n += 1
        w3 = check(s, p3, dm2, dist2, n)
        assert np.array_equal(w2[0], w3[0]) and not np.array_equal(w2[1], w3[1])
        dist3 = np.asfortranarray(dist * 3.0)
        s.set_distance(dist3)                                          # -- set_distance
        n += 1
        check(s, p3, dm2, dist3, n)
        s.synth_datamatrix(12, 0.2)                                    # -- synth_datamatrix: another datamatrix and other distances
        n += 1
        dm4, dist4 = s.get_datamatrix(), s.get_distance()
        assert not np.array_equal(dm4, dm2) and not np.array_equal(dist4, dist3)
        check(s, p3, dm4, dist4, n)
        check(s, p3, dm4, dist4, n)


# ------------------------------------------------------------------------------------------------ 7: the sampler on the device
@gpu
@pytest.mark.parametrize("density", [0.3, 0.06])
def test_device_sampler_lies_within_the_cap_of_the_device_expectation(cpm, O, density):
    d = V.statistical_inputs(O, density)
    Z, C, cpz = d["Z"], d["C"], d["cpz"]
    _, _, v_sec, v_km = d["moments"]
    with _sampler(cpm, Z, T, d["p_drive"], d["p_dest"], d["dm"], d["dist"]) as s:
        s.init_states(C, cpz)
        r = s.resample(SEED, travel=True, want_state=True, want_trans=True)
        w_sec, w_km = s.expected_trip()
        e = s.expected_travel()
        _, drv = s.expected()
    N, S, D = V.sums_per_cell(r["state"], r["trans"], Z)
    assert np.array_equal(N, r["driving"])
    V.check_cells(N, S, D, w_sec, w_km, v_sec, v_km, CAP, f"device, density {density}")
    # the whole day: the sampled sum against C * total_seconds, with the device's own expected N and the Bernoulli variance of N
    var = (C * drv * v_sec + C * drv * (1.0 - drv) * w_sec * w_sec).sum()
    got, want = r["sum_tt_q16"] / 65536.0, C * e["total_seconds"]
    z = abs(got - want) / math.sqrt(var)
    print(f"density {density}: travel-time sum {got:.1f} s against {want:.1f} s expected: {z:.2f} sigma; A_drive {e['A_drive']:.6f}")
    assert z <= CAP


# ------------------------------------------------------------------------------------------------ 8: errors and side effects
@gpu
def test_errors_name_what_is_missing(cpm):
    Z, Tc = 24, 24
    p_drive, p_dest, dm, dist, _ = _inputs(Z, Tc)
    big = np.array(p_dest)
    big[2, :, 4] *= 1.25
    with cpm.Sampler(Z, Tc) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        for call in (s.expected_trip, s.expected_travel):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "datamatrix" in str(e.value)
        s.set_datamatrix(dm)                                            # (no distance matrix yet)
        for call in (s.expected_trip, s.expected_travel):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "distance matrix" in str(e.value)
        s.set_distance(dist)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_batch()
        assert e.value.status == ERR_STATE and "batch" in str(e.value)
        s.set_p_dest(big)
        for _ in range(2):                                              # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected_trip()
            assert e.value.status == ERR_TABLE and "hour 5, origin 3" in str(e.value)
        assert s.expected_trip_builds() == 0
        s.set_p_dest(p_dest)
        w_sec, _ = s.expected_trip()
        assert np.all(np.isfinite(w_sec)) and s.expected_trip_builds() == 1
    with cpm.Sampler(Z, Tc) as s:                                       # no p_dest
        s.set_p_drive(p_drive)
        s.set_datamatrix(dm, dist)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_trip()
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)


@gpu
def test_expected_travel_leaves_no_trace_in_a_later_resample(cpm):
    Z, cpz = 67, 200
    C = Z * cpz
    p_drive, p_dest, dm, dist, _ = _inputs(Z, T)
    with _sampler(cpm, Z, T, p_drive, p_dest, dm, dist) as s:
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        before, step = s.resample(SEED, travel=True), s.last_step()
        s.set_p_drive_batch(np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (Z, T, 3))))
        s.expected_trip()
        s.expected_travel()
        s.expected_travel(ivp=True)
        s.expected_travel_batch()
        assert s.last_step() == step
        after = s.resample(SEED, travel=True)
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert before["sum_tt_q16"] == after["sum_tt_q16"]
        assert s.last_step() == step


# ------------------------------------------------------------------------------------------------ 9: the Evaluator
@gpu
def test_evaluator_returns_the_noise_free_a_drive(cpm, O):
    from carparkingmaps_amd import model_selection as ms
    Z = 67
    dm, dist = O.synth_datamatrix(Z, T, 11, density=0.3)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, T), rng.uniform(0, 1, (Z, T))
    pts = [ms.Point(0.5, 0.1, 0.9, 2), ms.Point(1.0, 0.05, 0.7, 2), ms.Point(0.25, 0.2, 1.0, 2)]
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        ev = ms.Evaluator(s, C=Z * 100, seed=SEED, measured_activity=m_act, measured_parking=m_park)
        singles = []
        for pt in pts:
            out = ev.evaluate_expected(pt)
            ref = s.expected_travel(ivp=True)                           # the point's tables are installed
            park, drv = s.expected(ivp=True)
            assert out["A_drive"] == ref["A_drive"] and out["total_seconds"] == ref["total_seconds"] and out["total_km"] == ref["total_km"]
            assert np.array_equal(out["parking"], park) and np.array_equal(out["driving"], drv)
            want = ms.expected_objectives(park, drv, m_act, m_park, seconds=ref["total_seconds"])
            assert out["activity_error"] == want["activity_error"] and out["parking_error"] == want["parking_error"]
            assert 0.0 < out["A_drive"] < 1.0
            singles.append(out)
        assert len({o["A_drive"] for o in singles}) == len(pts)
        batch = ev.evaluate_expected_batch(pts)
        for one, b in zip(singles, batch):
            assert one["A_drive"] == b["A_drive"] and one["total_km"] == b["total_km"]
            assert np.array_equal(one["parking"], b["parking"]) and np.array_equal(one["driving"], b["driving"])
            assert one["activity_error"] == b["activity_error"] and one["parking_error"] == b["parking_error"]
        no_ivp = ev.evaluate_expected(pts[0], ivp=False)
        assert no_ivp["A_drive"] == s.expected_travel()["A_drive"]
        # tune_p_min_max as it is, on the noise-free value
        pm, px, A, hist = ms.tune_p_min_max(lambda a, b: ev.evaluate_expected(ms.Point(0.5, a, b, 2))["A_drive"], A_set=0.07, max_iter=4)
        print(f"tune_p_min_max on the expected A_drive: p_min {pm:.3f}, p_max {px:.3f}, A_drive {A:.4f} after {len(hist)} evaluations")
        assert 0.0 <= pm <= px <= 1.0 and A > 0.0
