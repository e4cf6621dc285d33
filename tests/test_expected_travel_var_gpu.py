"""The exact seed variance of travel seconds, kilometres and count functionals (include/cpm_expected_travel_var.h) on the GPU: bit for
bit the integer reference on dyadic tables; within the header's bound of the exact form (fed the device's own v_sec words); the bits
of the numpy form at the sizes the exact form is too slow for; v_sec within its bound of mpmath on the travel ladder; functional k of
K bit for bit the K = 1 call; S = D = 0 bit for bit cpm_expected_linear_var_dev; exactly 0 for a constant functional; the S = 1 mean
against C x expected_travel; determinism, guard words, no trace in a later call, the cache and its build counter, sparse tables, NULL
d_zone and NULL trip arrays, every refusal; the Python layers bit for bit; and the device sampler's spread over 400 seeds.

Shapes: the product's strip is 128 origins (two per lane), a segment at least 32 destinations dealt over four waves, four
destinations of a wave in flight, a pass NB = 2 functionals.  Z = 16, 17 sit in one partial strip (even: 16-byte loads; odd: the
8-byte path, origins lane and lane + 64); 33 has one segment with a partial round; 65 two segments; 127 / 128 / 129 sit on and either
side of a strip; 130 / 257 / 518 / 1,031 take several strips and up to 32 segments, odd and even."""
import ctypes
import functools

import numpy as np
import pytest

import expected_reference as R
import expected_travel_reference as TR
import expected_var_reference as V
import expected_linear_var_reference as LV
import expected_travel_var_reference as TV
import travel_ladder as TL

gpu = pytest.mark.gpu
T = 24
NB = 2                                       # kEtvNB of csrc/cpm_expected_travel_var.h
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4
KEYS = ("mean", "var", "zone_mean", "zone_var")


def _sampler(cpm, p_drive, p_dest, dm=None, dist=None):
    s = cpm.Sampler(*p_drive.shape)
    s.set_p_drive(p_drive)
    s.set_p_dest(p_dest)
    if dm is not None:
        s.set_datamatrix(dm, dist)
    return s


def _guarded(words):
    import torch
    return torch.full((2 * GUARD + words,), SENT, dtype=torch.int64, device="cuda")


def _body(buf, what):
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), f"a store outside {what}"
    assert not np.any(a[GUARD:-GUARD] == SENT), f"a word of {what} was not written"
    return a[GUARD:-GUARD].view(np.float64)


def _dev_call(s, f, w, ivp, zone=True, linear=False):
    """expected_travel_var_dev (linear: expected_linear_var_dev on A, B alone) between guard words on sentinel-filled outputs: every
    word written, none outside.  f: (A, B, S, D), each (Z, T, K).  Returns dict(mean (K,), var (K,), zone_mean (Z, K), zone_var (Z, K))."""
    import torch
    K = f[0].shape[2]
    coeff = np.ascontiguousarray(np.stack([x.transpose(2, 1, 0) for x in (f[:2] if linear else f)], axis=1))   # [K][4 or 2][T][Z]
    d_coeff = torch.from_numpy(coeff).cuda()
    out, zn = _guarded(2 * K), _guarded(2 * K * s.Z)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    call = s.expected_linear_var_dev if linear else s.expected_travel_var_dev
    call(K, d_coeff.data_ptr(), out.data_ptr() + 8 * GUARD, 0 if w is None else d_w.data_ptr(), ivp, zn.data_ptr() + 8 * GUARD if zone else 0)
    s.sync()
    o = _body(out, "d_out").reshape(K, 2)
    res = {"mean": o[:, 0].copy(), "var": o[:, 1].copy()}
    if zone:
        z = _body(zn, "d_zone").reshape(K, 2, s.Z)
        res["zone_mean"], res["zone_var"] = z[:, 0].T.copy(), z[:, 1].T.copy()
    else:
        assert np.all(zn.cpu().numpy() == SENT)
    return res


def _vsec_dev(s):
    """expected_trip_var_dev between guard words: (Z, T)"""
    buf = _guarded(s.Z * s.T)
    s.expected_trip_var_dev(buf.data_ptr() + 8 * GUARD)
    s.sync()
    return np.asfortranarray(_body(buf, "d_v").reshape(s.T, s.Z).T)


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _one(res, k):
    return {"mean": res["mean"][k], "var": res["var"][k], "zone_mean": res["zone_mean"][:, k], "zone_var": res["zone_var"][:, k]}


def _pick(f, k):
    return [np.asfortranarray(x[:, :, k]) for x in f]


def _cut(f, a, b):
    return [np.asfortranarray(x[:, :, a:b]) for x in f]


@functools.lru_cache(maxsize=None)
def _tables(Z, Tc):
    from oracle import oracle as O
    O.build()
    p_drive, p_dest = TR.planted_tables(O, Z, Tc) if Z > 2 else R.modified_tables(O, Z, Tc)
    k = min(Z, 5)
    p_drive[:k, 1 % Tc] = [np.nan, -0.1, 0.0, 1.0, 1.5][:k]      # entries the Bernoulli maps to 0, 0, 0, 1, 1
    dm, dist = TR.planted_datamatrix(O, Z, Tc)                    # (standard deviations of 10 .. 40 % and none; a planted diagonal)
    for a in (p_drive, p_dest, dm, dist):
        a.setflags(write=False)
    sec, km = TR.trip_values(dm, dist)
    return p_drive, p_dest, R.row_tables(p_dest), dm, dist, sec, km


def _w(Z, kind="given"):
    if kind == "ones":
        return None
    w = np.random.default_rng(Z).integers(0, 50, Z).astype(np.float64)
    w[Z // 2] = 0.0
    return w


# ------------------------------------------------------------------------------------------------ 1: exact equality
@gpu
@pytest.mark.parametrize("Z", [16, 17, 33, 65, 130])
def test_dyadic_tables_give_the_integer_reference_bit_for_bit(cpm, Z):
    """T = 3 without the IVP, tables in multiples of 2^-3 (p_drive: 2^-2), means and distances in halves, negative standard deviations
    (var_sec exactly 0), coefficients in {-2 .. 2} and {-1 .. 1}: the reference asserts that every intermediate and every partial sum
    in any order fits 53 bits, so any lane-map, strip-edge, diagonal, residual or zero-row error shows with no tolerance"""
    p_drive, p_dest, w = V.dyadic_tables(Z, 3)
    dm, dist = TV.dyadic_datamatrix(Z, 3)
    sec, km = TR.trip_values(dm, dist)
    f = TV.small_functionals(Z, 3, 3, Z)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        got = _dev_call(s, f, w, False)
        vsec = _vsec_dev(s)
    assert np.all(vsec == 0.0)
    for k in range(3):
        want = TV.int_tv(p_drive, p_dest, *_pick(f, k), sec, km, vsec, w, 0, bits=53)
        assert got["mean"][k] == float(want["mean"]) and got["var"][k] == float(want["var"]), (k, got["var"][k], float(want["var"]))
        assert np.array_equal(got["zone_mean"][:, k], [float(x) for x in want["zone_mean"]])
        zv = np.array([float(x) for x in want["zone_var"]])
        assert np.array_equal(got["zone_var"][:, k], zv), np.argwhere(got["zone_var"][:, k] != zv)[:8].tolist()
        assert want["var"] > 0


# ------------------------------------------------------------------------------------------------ 2: the bound
def _check_exact(cpm, Z, Tc, flags, K):
    p_drive, p_dest, tables, dm, dist, sec, km = _tables(Z, Tc)
    w = _w(Z, "ones" if Z % 2 == 0 else "given")
    f = TV.signed_functionals(Z, Tc, K, 7 * Z + Tc)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        got = _dev_call(s, f, w, bool(flags))
        blk = s.expected_travel_var(*f, start=w, ivp=bool(flags), per_zone=True)
        vsec = _vsec_dev(s)
        assert np.array_equal(vsec, s.expected_trip_var())
    assert _same(got, blk)                                             # the blocking form is the device form
    assert np.any(vsec > 0)
    for k in range(K):
        exact = TV.int_tv(p_drive, p_dest, *_pick(f, k), sec, km, vsec, w, flags, tables)
        mag = TV.int_tv(p_drive, p_dest, *_pick(f, k), sec, km, vsec, w, flags, tables, magnitude=True)
        worst, zeros_ok = TV.worst(_one(got, k), exact, TV.bounds(Z, Tc, flags, mag, w))
        print(f"Z={Z} T={Tc} flags={flags} k={k}: worst error / bound {worst}")
        assert zeros_ok and max(worst.values()) <= 1.0


@gpu
@pytest.mark.parametrize("flags", [0, TV.IVP])
@pytest.mark.parametrize("Z", [2, 3, 8, 16, 17, 33, 65])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, flags):
    _check_exact(cpm, Z, 4, flags, 2)


@gpu
@pytest.mark.parametrize("flags", [0, TV.IVP])
def test_device_meets_the_bound_over_a_whole_day(cpm, flags):
    _check_exact(cpm, 65, T, flags, 1)


@gpu
@pytest.mark.parametrize("Z", [127, 128, 129, 257, 518, 1031])
def test_device_has_the_bits_of_the_numpy_form(cpm, Z):
    Tc, K = 4, NB + 1                                                  # (a full pass and a pass of one)
    p_drive, p_dest, tables, dm, dist, sec, km = _tables(Z, Tc)
    w = _w(Z)
    f = TV.signed_functionals(Z, Tc, K, Z)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        vsec = _vsec_dev(s)
        for flags in (0, TV.IVP):
            got = _dev_call(s, f, w, bool(flags))
            for k in (0, K - 1):
                want = TV.numpy_tv(p_drive, p_dest, *_pick(f, k), sec, km, vsec, w, flags, tables)
                for key in KEYS:
                    g, e = np.atleast_1d(_one(got, k)[key]), np.atleast_1d(want[key])
                    assert np.array_equal(g, e), (key, flags, k, float(np.max(np.abs(g - e) / np.maximum(np.abs(e), 1e-300))))
                assert want["var"] > 0


# ------------------------------------------------------------------------------------------------ 3: v_sec
@gpu
@pytest.mark.parametrize("Z", [16, 17])
def test_trip_variance_weights_on_the_travel_ladder(cpm, O, Z):
    """standard deviations from 4 x the mean down to 1e-6 x, none, negative and infinite: every exit and both forms of v(a); within
    the header's bound of the mpmath form, the bits of the f64 restatement on the oracle's kit in the documented order, and exactly 0
    where every destination's draw is the mean"""
    import mpmath as mp
    Tc = 3
    dm, dist, idx = TL.ladder_datamatrix(O, Z, Tc, 5, 0.7)
    p_drive, p_dest = TR.planted_tables(O, Z, Tc)
    tables = R.row_tables(p_dest)
    dm[Z - 2, :, 1, 1] = -1.0                                         # (a row whose every draw is the mean)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        got = _vsec_dev(s)
    vs = TV.var_sec_array(O, dm)
    assert np.array_equal(got, TV.vsec_numpy(p_dest, vs, tables)), "not the documented form or order"
    with mp.workdps(40):
        vm = [[[TV.var_sec_mp(dm[o, d, t, 0], dm[o, d, t, 1]) if d != o else 0 for t in range(Tc)] for d in range(Z)] for o in range(Z)]
        exact = TV.vsec_exact(p_dest, vm, tables, conv=lambda x: mp.mpf(float(x)))
        worst = 0.0
        for t in range(Tc):
            for o in range(Z):
                e = exact[o, t]
                if e == 0:
                    assert got[o, t] == 0.0
                    continue
                err = float(abs(mp.mpf(float(got[o, t])) - e) / e)
                worst = max(worst, err)
                assert err <= TV.bound_vsec(Z), (o, t, err / TV.bound_vsec(Z))
    print(f"Z={Z}: v_sec worst relative error {worst:.3e} = {worst / TV.bound_vsec(Z):.4f} of the bound")
    assert got[Z - 2, 1] == 0.0 and np.all(got[tables[0].T == 0.0] == 0.0) and np.any(got > 0)
    assert len(set(idx[idx >= 0].tolist())) == len(TL.RUNGS)


# ------------------------------------------------------------------------------------------------ 4: functional k of K
@gpu
def test_functional_k_of_K_carries_the_bits_of_a_call_on_it_alone(cpm):
    Z, Tc = 257, 4
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    w = _w(Z)
    f = TV.signed_functionals(Z, Tc, 64, 1)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        singles = [_dev_call(s, _cut(f, k, k + 1), w, True) for k in range(64)]
        for K in (1, 3, 4, 5, 9, 24, 64):                              # partial passes, a second and a third pass
            got = _dev_call(s, _cut(f, 0, K), w, True)
            for k in range(K):
                assert _same(_one(got, k), _one(singles[k], 0)), (K, k)
        got = _dev_call(s, _cut(f, 5, 12), w, True)                    # ... wherever the functional stands in its pass
        assert all(_same(_one(got, k), _one(singles[5 + k], 0)) for k in range(7))
    assert len({float(r["var"][0]) for r in singles}) == 64


# ------------------------------------------------------------------------------------------------ 5: against the other calls
@gpu
@pytest.mark.parametrize("Z", [17, 130, 257])
def test_no_trip_coefficients_give_the_bits_of_the_linear_call(cpm, Z):
    Tc = 6
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    w = _w(Z)
    A, B = LV.signed_functionals(Z, Tc, 5, Z)
    zero = np.zeros((Z, Tc, 5), order="F")
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        for ivp in (False, True):
            lin = _dev_call(s, (A, B), w, ivp, linear=True)
            got = _dev_call(s, (A, B, zero, zero), w, ivp)
            assert _same(got, lin)
            blk = s.expected_travel_var(A, B, start=w, ivp=ivp, per_zone=True)     # (NULL trip arrays: zeros)
            assert _same(blk, lin)
            one = s.expected_travel_var(A, B, None, zero, start=w, ivp=ivp, per_zone=True)
            assert _same(one, lin)
        assert np.all(lin["var"] > 0)


@gpu
@pytest.mark.parametrize("Z", [65, 257])
def test_a_functional_constant_over_the_zones_has_variance_exactly_zero(cpm, Z):
    Tc = 6
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    w = _w(Z)
    hours = np.arange(1.0, Tc + 1.0) * 0.3                             # (constant over the zones, not over the hours)
    A = np.stack([np.broadcast_to(c * hours[None, :], (Z, Tc)) for c in (1.0, 1e6)], axis=2)
    A = np.asfortranarray(np.concatenate([A, A[:, :, :1]], axis=2))    # (the third: with seconds, a check of the check)
    zero = np.zeros((Z, Tc, 3), order="F")
    S = zero.copy(order="F")
    S[:, :, 2] = 1e-3
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        for ivp in (False, True):
            got = _dev_call(s, (A, zero, S, zero), w, ivp)
            assert got["var"][0] == 0.0 and got["var"][1] == 0.0 and np.all(got["zone_var"][:, :2] == 0.0)
            assert got["var"][2] > 0.0
            assert abs(got["mean"][0] - hours.sum() * w.sum()) <= 1e-9 * hours.sum() * w.sum()


@gpu
@pytest.mark.parametrize("Z", [33, 130])
def test_mean_of_the_seconds_and_kilometres_agrees_with_expected_travel(cpm, Z):
    """S = 1 alone and D = 1 alone: the means are C x expected_travel()'s totals (another kernel family), within the sum of the two
    headers' bounds"""
    Tc = 6
    p_drive, p_dest, tables, dm, dist, sec, km = _tables(Z, Tc)
    w = _w(Z)
    C = float(w.sum())
    zero, one = np.zeros((Z, Tc, 2), order="F"), np.zeros((Z, Tc, 2), order="F")
    S, D = zero.copy(order="F"), zero.copy(order="F")
    S[:, :, 0], D[:, :, 1] = 1.0, 1.0
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        vsec = _vsec_dev(s)
        for flags in (0, TV.IVP):
            got = _dev_call(s, (zero, zero, S, D), w, bool(flags))
            tr = s.expected_travel(w / C, ivp=bool(flags))
            hmax = R.operators_behind(Tc, flags)[-1]
            for k, total in ((0, tr["total_seconds"]), (1, tr["total_km"])):
                mag = TV.numpy_tv(p_drive, p_dest, zero[:, :, k], zero[:, :, k], S[:, :, k], D[:, :, k], sec, km, vsec, w, flags, tables, magnitude=True)
                tol = TV.bounds(Z, Tc, flags, mag, w)["mean"] + (TR.bound_total(Z, Tc, hmax) + 4 * TV.EPS) * C * abs(total)
                assert abs(got["mean"][k] - C * total) <= tol, (k, flags, abs(got["mean"][k] - C * total) / tol)
                assert got["var"][k] > 0 and total > 0


# ------------------------------------------------------------------------------------------------ 6: the family's checks
@gpu
def test_ones_are_the_null_start_and_null_zone_output(cpm):
    Z, Tc = 130, 6
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    w = _w(Z)
    f = TV.signed_functionals(Z, Tc, 3, 2)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        for ivp in (False, True):
            none, ones, given = _dev_call(s, f, None, ivp), _dev_call(s, f, np.ones(Z), ivp), _dev_call(s, f, w, ivp)
            assert _same(none, ones)
            assert _same(none, given, ("zone_mean", "zone_var"))       # (the per-zone outputs do not read the start)
            no_zone = _dev_call(s, f, w, ivp, zone=False)              # NULL d_zone: the same totals from the context's own buffer
            assert _same(no_zone, given, ("mean", "var"))


@gpu
def test_same_bits_on_a_repeated_call_and_in_a_second_context(cpm):
    Z, Tc = 257, 6
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    w = _w(Z)
    f = TV.signed_functionals(Z, Tc, 5, 4)
    g = (f[1], f[0], f[2], f[3])
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s, _sampler(cpm, p_drive, p_dest, dm, dist) as s2:
        for ivp in (False, True):
            a = _dev_call(s, f, w, ivp)
            other = _dev_call(s, g, None, not ivp)                     # (another call in between leaves nothing behind)
            b = _dev_call(s, f, w, ivp)
            c = _dev_call(s2, f, w, ivp)
            assert _same(a, b) and _same(a, c) and not _same(a, other)
        assert np.array_equal(_vsec_dev(s), _vsec_dev(s2))


@gpu
def test_no_trace_in_a_later_call_or_resample(cpm):
    Z, cpz, seed = 67, 200, 20240611
    C = Z * cpz
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, T)
    f = TV.signed_functionals(Z, T, 3, 6)
    with _sampler(cpm, np.nan_to_num(p_drive), p_dest, dm, dist) as s:
        s.init_states(C, cpz)
        s.solve_ivp(seed, want=False)
        before, step = s.resample(seed, travel=True), s.last_step()
        exp_before, lin_before = s.expected(ivp=True), s.expected_linear_var(f[0], f[1], ivp=True, per_zone=True)
        trav_before = s.expected_travel(ivp=True)
        state = s.get_state()
        s.expected_travel_var(*f)
        s.expected_travel_var(*f, start=np.bincount(state - 1, minlength=Z).astype(np.float64), ivp=True)
        s.expected_trip_var()
        assert s.last_step() == step and np.array_equal(s.get_state(), state)
        exp_after, lin_after = s.expected(ivp=True), s.expected_linear_var(f[0], f[1], ivp=True, per_zone=True)
        trav_after = s.expected_travel(ivp=True)
        after = s.resample(seed, travel=True)
        assert np.array_equal(exp_before[0], exp_after[0]) and np.array_equal(exp_before[1], exp_after[1])
        assert _same(lin_before, lin_after)
        assert np.array_equal(trav_before["seconds"], trav_after["seconds"]) and trav_before["total_km"] == trav_after["total_km"]
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert before["sum_tt_q16"] == after["sum_tt_q16"] and s.last_step() == step


@gpu
def test_cache_and_build_counter_follow_the_tables(cpm, O):
    Z, Tc = 33, 6
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    f = TV.signed_functionals(Z, Tc, 2, 3)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        assert s.expected_trip_var_builds() == 0
        v0 = s.expected_trip_var()
        r0 = s.expected_travel_var(*f)
        s.expected_trip_var()
        assert s.expected_trip_var_builds() == 1                       # (built once, whatever asks)
        dm2 = np.array(dm)
        dm2[..., 1] *= 0.5
        s.set_datamatrix(dm2)                                          # a new datamatrix, the distances kept
        v1 = s.expected_trip_var()
        assert s.expected_trip_var_builds() == 2 and not np.array_equal(v0, v1)
        r1 = s.expected_travel_var(*f)
        assert not np.array_equal(r0["var"], r1["var"]) and np.array_equal(r0["mean"], r1["mean"])   # (the means read no std word)
        s.set_distance(np.asfortranarray(2.0 * np.array(dist)))        # new distances: v_sec is rebuilt with the trip weights, the same words
        r2 = s.expected_travel_var(*f)
        assert s.expected_trip_var_builds() == 3 and np.array_equal(s.expected_trip_var(), v1)
        assert not np.array_equal(r1["mean"], r2["mean"])
        p2 = np.array(p_dest)
        p2[4, :, :] *= 0.5
        s.set_p_dest(p2)                                               # a new p_destin
        v3 = s.expected_trip_var()
        assert s.expected_trip_var_builds() == 4 and not np.array_equal(v1[4], v3[4]) and np.array_equal(np.delete(v1, 4, 0), np.delete(v3, 4, 0))
        s.set_p_drive(np.full((Z, Tc), 0.25, order="F"))               # p_drive does not enter
        s.expected_travel_var(*f)
        assert s.expected_trip_var_builds() == 4
    with _sampler(cpm, p_drive, p_dest, dm2, 2.0 * np.array(dist)) as d:
        assert _same(d.expected_travel_var(*f), r2, ("mean", "var"))   # (a fresh context on the final tables of r2)


@gpu
def test_sparse_tables_against_a_dense_context(cpm, O):
    """tables built on the dataset route hold sparse row packs: the call expands them to the dense array first"""
    Z = 358                                                            # (the compact-row route takes T = 24 only)
    dm, dist = O.synth_datamatrix(Z, T, 11, density=0.06)
    w = _w(Z)
    f = TV.signed_functionals(Z, T, 3, 3)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        s.build_p_dest(2, want=False)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        first = s.expected_travel_var(*f, start=w, per_zone=True)      # (before anything else asked for the dense array)
        v_first = s.expected_trip_var()
        p_dest = s.build_p_dest(2, want=True)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        again = s.expected_travel_var(*f, start=w, per_zone=True)
    assert _same(first, again)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as d:
        assert d.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        dense = d.expected_travel_var(*f, start=w, per_zone=True)
        assert np.array_equal(d.expected_trip_var(), v_first)
    assert _same(first, dense)
    assert np.all(first["var"] > 0)


@gpu
def test_blocking_form_shapes_and_null_outputs(cpm):
    Z, Tc = 33, 6
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    f = TV.signed_functionals(Z, Tc, 3, 8)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        full = s.expected_travel_var(*f, per_zone=True)
        plain = s.expected_travel_var(*f)
        assert set(plain) == {"mean", "var"} and _same(full, plain, ("mean", "var")) and full["zone_var"].shape == (Z, 3)
        one = s.expected_travel_var(*[x[:, :, 1] for x in f], per_zone=True)                # (Z, T) inputs: scalars and (Z,)
        assert isinstance(one["mean"], float) and one["zone_mean"].shape == (Z,)
        assert one["mean"] == full["mean"][1] and one["var"] == full["var"][1] and np.array_equal(one["zone_var"], full["zone_var"][:, 1])
        c_order = s.expected_travel_var(*[np.ascontiguousarray(x) for x in f])               # (any memory order)
        assert _same(c_order, plain, ("mean", "var"))


@gpu
def test_every_refusal(cpm):
    Z, Tc = 24, 24
    p_drive, p_dest, _, dm, dist, _, _ = _tables(Z, Tc)
    big = np.array(p_dest)
    big[2, :, 4] *= 1.25
    f = TV.signed_functionals(Z, Tc, 2, 9)
    buf = np.zeros(2 * 4 * Z * Tc)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    with cpm.Sampler(Z, Tc) as s:
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_var(*f)
        assert e.value.status == ERR_STATE and "p_drive" in str(e.value)
        s.set_p_drive(p_drive)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_var(*f)
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_trip_var()
        assert e.value.status == ERR_STATE
        s.set_p_dest(p_dest)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_var(*f)
        assert e.value.status == ERR_STATE and "datamatrix" in str(e.value)
        assert s._L.cpm_expected_travel_var_dev(s._h, None, 0, 1, vp, vp, None) == ERR_STATE
        assert s._L.cpm_expected_trip_var_dev(s._h, vp) == ERR_STATE
        s.set_datamatrix(dm)                                            # (no distances yet)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_var(*f)
        assert e.value.status == ERR_STATE and "distance" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_trip_var()
        assert e.value.status == ERR_STATE and "distance" in str(e.value)
        assert s.expected_trip_var_builds() == 0
        s.set_distance(dist)
        s.set_p_dest(big)
        for _ in range(2):                                          # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected_travel_var(*f)
            assert e.value.status == ERR_TABLE and "hour 5, origin 3" in str(e.value)
        s.set_p_dest(p_dest)
        assert np.all(np.isfinite(s.expected_travel_var(*f)["var"]))
        for bad in (np.nan, np.inf, -1e-9):
            w = np.ones(Z)
            w[3] = bad
            with pytest.raises(cpm.CpmError) as e:
                s.expected_travel_var(*f, start=w)
            assert e.value.status == ERR_ARG and "zone 4" in str(e.value)
        for bad in (np.nan, np.inf, -np.inf):
            for which in range(4):
                c = [x.copy(order="F") for x in f]
                c[which][6, 2, 1] = bad
                with pytest.raises(cpm.CpmError) as e:
                    s.expected_travel_var(*c)
                assert e.value.status == ERR_ARG and "functional 2, zone 7, hour 3" in str(e.value)
        with pytest.raises(ValueError):
            s.expected_travel_var(*f, start=np.ones(Z + 1))
        with pytest.raises(ValueError):
            s.expected_travel_var(f[0], f[1], f[2][:, :, :1])
        for K in (0, -1, 65):
            assert s._L.cpm_expected_travel_var_dev(s._h, None, 0, K, vp, vp, None) == ERR_ARG
            assert s._L.cpm_expected_travel_var(s._h, None, 0, K, vp, vp, vp, vp, vp, vp, None, None) == ERR_ARG
            assert b"K = " in s._L.cpm_last_error()
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_var_dev(1, 0, buf.ctypes.data)
        assert e.value.status == ERR_ARG and "d_coeff" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_var_dev(1, buf.ctypes.data, 0)
        assert e.value.status == ERR_ARG and "d_out" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_trip_var_dev(0)
        assert e.value.status == ERR_ARG and "d_v" in str(e.value)
        assert s._L.cpm_expected_trip_var(s._h, None) == ERR_ARG
        assert s._L.cpm_expected_travel_var(s._h, None, 0, 1, None, vp, vp, vp, vp, vp, None, None) == ERR_ARG
        assert s._L.cpm_expected_travel_var(s._h, None, 0, 1, vp, vp, None, None, None, vp, None, None) == ERR_ARG
        for flags in (2, 0x100, 0x80000001):
            assert s._L.cpm_expected_travel_var_dev(s._h, None, flags, 1, vp, vp, None) == ERR_ARG
            assert s._L.cpm_expected_travel_var(s._h, None, flags, 1, vp, vp, vp, vp, vp, vp, None, None) == ERR_ARG
        assert b"flag" in s._L.cpm_last_error()
        assert s._L.cpm_expected_travel_var_dev(None, None, 0, 1, vp, vp, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ 7: the Python layers
@gpu
def test_travel_noise_and_expected_noise_are_the_explicit_functionals(cpm, O):
    from carparkingmaps_amd import model_selection as ms
    Z, Tc, C = 24, 24, 4800
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, Tc), np.asfortranarray(rng.uniform(0, 1, (Z, Tc)))
    pt = ms.Point(e_drive=0.6, p_min=0.15, p_max=0.8, e_dest=2)
    start = np.full(Z, C / Z)
    zero, one = np.zeros((Z, Tc), order="F"), np.ones((Z, Tc), order="F")
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        ev = ms.Evaluator(s, C=C, seed=1, measured_activity=m_act, measured_parking=m_park)
        plain = ev.expected_noise(pt, ivp=True)                        # (installs the point)
        noise = ev.expected_noise(pt, ivp=True, travel=True)
        assert set(noise) == set(plain) | {"A_drive"} and all(np.array_equal(noise[k]["var"], plain[k]["var"]) if k == "activity" else noise[k] == plain[k] for k in plain)
        for ivp in (False, True):
            tn = ms.travel_noise(s, start, ivp=ivp)
            sec = s.expected_travel_var(zero, zero, one, zero, start=start, ivp=ivp)
            km = s.expected_travel_var(zero, zero, zero, one, start=start, ivp=ivp)
            assert tn["seconds_mean"] == sec["mean"] and tn["seconds_std"] == float(np.sqrt(sec["var"]))
            assert tn["km_mean"] == km["mean"] and tn["km_std"] == float(np.sqrt(km["var"]))
            assert tn["A_drive_mean"] == sec["mean"] / (C * Tc * 60 * 60) and tn["A_drive_std"] == float(np.sqrt(sec["var"])) / (C * Tc * 60 * 60)
            assert tn["A_drive_mean"] == ms.a_drive(sec["mean"] * 65536.0, C, Tc)
            tr = s.expected_travel(None, ivp=ivp)                      # (the noise-free A_drive of the same tables)
            assert abs(tn["A_drive_mean"] - tr["A_drive"]) <= 1e-9 * tr["A_drive"] and 0 < tn["A_drive_std"] < tn["A_drive_mean"]
            if ivp:
                assert noise["A_drive"] == tn


# ------------------------------------------------------------------------------------------------ 8: the sampler's spread
def _device_runs(cpm, s, C, ivp):
    runs = []
    s.init_states(C, TV.STAT_CPZ)
    family = s.get_info(cpm.CPM_INFO_KERNEL)                # (what AUTO resolves to for these tables and cars: no set_kernel anywhere)
    assert family != cpm.CPM_KERNEL_AUTO
    for seed in range(1, TV.RUNS + 1):
        if ivp:
            s.init_states(C, TV.STAT_CPZ)
            s.solve_ivp(seed, want=False)
        r = s.resample(seed, travel=True)
        assert s.get_info(cpm.CPM_INFO_LAST_KERNEL) == family, "not the default kernel family"
        runs.append((r["parking"], r["driving"], r["sum_tt_q16"] / 65536.0))
    return runs


@gpu
@pytest.mark.parametrize("ivp", [False, True])
def test_spread_of_the_device_sampler(cpm, O, ivp):
    """R = 400 seeds of Sampler.resample(travel=True) on the device's own default kernel family: the total seconds, and the total
    seconds plus a random signed count functional, against the device's expected_travel_var; the caps of tests/test_expected_travel_var.py"""
    p_drive, p_dest, zone0, w, dm, dist = TV.stat_setup(O)
    funcs = TV.stat_functionals(TV.STAT_Z, TV.STAT_T)
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        res = s.expected_travel_var(*TV.stack4(funcs), start=w, ivp=ivp)
        runs = _device_runs(cpm, s, len(zone0), ivp)
    TV.check_stat(TV.stat_values(runs, funcs), res["mean"], res["var"], "device ivp" if ivp else "device")


@gpu
@pytest.mark.parametrize("which", ["no_draw", "no_cov"])
def test_spread_on_the_planted_tables_and_the_two_mutants(cpm, O, which):
    """the tables of tests/test_expected_travel_var.py on which all noise is draw noise, and on which half of the variance is the
    covariance of destination and duration: the device's variance stays inside the cap of the device's sampler, the mutant does not"""
    p_drive, p_dest, zone0, w, dm, dist = TV.draw_only_setup(O) if which == "no_draw" else TV.cov_setup(O)
    Z, Tc = p_drive.shape
    zero, one = np.zeros((Z, Tc), order="F"), np.ones((Z, Tc), order="F")
    with _sampler(cpm, p_drive, p_dest, dm, dist) as s:
        res = s.expected_travel_var(zero, zero, one, zero, start=w)
        vsec = s.expected_trip_var()
        runs = _device_runs(cpm, s, len(zone0), False)
    sec, km = TR.trip_values(dm, dist)
    mut = TV.plain_tv(p_drive, p_dest, zero, zero, one, zero, sec, km, vsec, w, 0, None, mutant=which)
    L = np.array([[r[2]] for r in runs])
    TV.check_stat(L, np.array([res["mean"]]), np.array([res["var"]]), "device " + which, [(which, 0, np.array([mut["var"]]))])
