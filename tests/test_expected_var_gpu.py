"""Exact variances of a resample's counts (include/cpm_expected_var.h) on the GPU: bit for bit the integer reference on dyadic
tables at every tile edge; within the header's bound of the exact (rational) form, and within twice it of the numpy form at the sizes
the exact form is too slow for; the means against cpm_expected_dev (another kernel family); sparse tables against a dense context;
the same bits every time; guard words; no trace in a later call; the blocking form, NULL outputs and every refusal; and the device
sampler's spread: the mean over the cells of (N - mean)^2 / var is 1 within 5.5 standard errors with the exact variance and is not
with the binomial one.

Shapes: the product's tile is 128 x 128 over slices of 16 of the summed index, a wave's 64 x 64, an MFMA's 16 x 16 x 4.  Z = 2, 3, 15
are K remainders of 2, 3, 3 in one partial MFMA tile; 16, 17, 31, 33 sit on and either side of an MFMA tile and of a slice; 65 crosses
a wave's quarter; 130 takes four workgroups (and three partial sums); 255 / 257 / 1,031 cross workgroup tiles with K remainders 3, 1, 3."""
import ctypes
import functools

import numpy as np
import pytest

import expected_reference as R
import expected_var_reference as V

gpu = pytest.mark.gpu
T = 24
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4


def _sampler(cpm, p_drive, p_dest):
    s = cpm.Sampler(*p_drive.shape)
    s.set_p_drive(p_drive)
    s.set_p_dest(p_dest)
    return s


def _dev_call(s, w, ivp):
    """expected_var_dev between guard words on a sentinel-filled output: every word written, none outside"""
    import torch
    out = torch.full((2 * GUARD + s.expected_var_words(),), SENT, dtype=torch.int64, device="cuda")
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    s.expected_var_dev(out.data_ptr() + 8 * GUARD, 0 if w is None else d_w.data_ptr(), ivp)
    s.sync()
    out = out.cpu().numpy()
    assert np.all(out[:GUARD] == SENT) and np.all(out[-GUARD:] == SENT), "a store outside the output"
    body = out[GUARD:-GUARD]
    assert not np.any(body == SENT), "a word of d_out was not written"
    four = body.view(np.float64).reshape(4, s.T, s.Z)
    return {k: four[i].T for i, k in enumerate(V.KEYS)}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in V.KEYS)


@functools.lru_cache(maxsize=None)
def _tables(Z, Tc):
    from oracle import oracle as O
    O.build()
    p_drive, p_dest = R.modified_tables(O, Z, Tc)
    k = min(Z, 5)
    p_drive[:k, 1 % Tc] = [np.nan, -0.1, 0.0, 1.0, 1.5][:k]      # entries the Bernoulli maps to 0, 0, 0, 1, 1
    for a in (p_drive, p_dest):
        a.setflags(write=False)
    return p_drive, p_dest, R.row_tables(p_dest)


def _w(Z, kind):
    if kind == "ones":
        return None
    w = np.random.default_rng(Z).integers(0, 50, Z).astype(np.float64)
    w[Z // 2] = 0.0
    return w


# ------------------------------------------------------------------------------------------------ 1: exact equality
@gpu
@pytest.mark.parametrize("Z", [2, 3, 15, 16, 17, 31, 33, 65, 130])
def test_dyadic_tables_give_the_integer_reference_bit_for_bit(cpm, Z):
    """every product and sum is exact in f64 (expected_var_reference.dyadic_tables), so any lane-map or tile-edge error shows with
    no tolerance.  T = 3 without the IVP; T = 2 with it (four operators of a T = 3 day would leave the 53 bits)."""
    p_drive, p_dest, w = V.dyadic_tables(Z, 3)
    for Tc, ivp in ((3, False), (2, True)):
        pd, pp = np.asfortranarray(p_drive[:, :Tc]), np.asfortranarray(p_dest[:, :, :Tc])
        want = V.int_var(pd, pp, w, V.IVP if ivp else 0)
        with _sampler(cpm, pd, pp) as s:
            got = _dev_call(s, w, ivp)
        for k in V.KEYS:
            f, exact = V.to_f64(want[k])
            assert exact, "the reference left f64"
            assert np.array_equal(got[k], f), (k, Tc, np.argwhere(got[k] != f)[:8].tolist())
        assert Z == 2 or ivp or (want["var_parking"] != 0).any()   # (at Z = 2 the cars that count never move)


# ------------------------------------------------------------------------------------------------ 2: the bound
@functools.lru_cache(maxsize=None)
def _exact(Z, flags, kind):
    p_drive, p_dest, tables = _tables(Z, T)
    return V.exact_var(p_drive, p_dest, _w(Z, kind), flags, tables)


@gpu
@pytest.mark.parametrize("flags", [0, V.IVP])
@pytest.mark.parametrize("Z", [2, 3, 8, 16, 17, 33])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, flags):
    p_drive, p_dest, tables = _tables(Z, T)
    kind = "ones" if Z % 2 == 0 else "given"
    w = _w(Z, kind)
    with _sampler(cpm, p_drive, p_dest) as s:
        got = s.expected_var(w, ivp=bool(flags))
        dev = _dev_call(s, w, bool(flags))
    assert _same(got, dev)                                             # the blocking form is the device form
    worst, zeros_ok = V.worst(got, _exact(Z, flags, kind), Z, T, flags)
    print(f"Z={Z} flags={flags}: worst error / bound {worst}")
    assert zeros_ok, "a word whose exact value is 0 is not 0"
    assert max(worst.values()) <= 1.0
    if not flags:
        assert np.all(got["var_parking"][:, 0] == 0.0)                 # hour 0 without the IVP: no spread


@gpu
@pytest.mark.parametrize("Z", [255, 257, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc = 6
    p_drive, p_dest, tables = _tables(Z, Tc)
    w = _w(Z, "given")
    with _sampler(cpm, p_drive, p_dest) as s:
        for flags in (0, V.IVP):
            got = s.expected_var(w, ivp=bool(flags))
            want = V.numpy_var(p_drive, p_dest, w, flags, tables)
            worst, zeros_ok = V.worst_f64(got, want, Z, Tc, flags, factor=2.0)
            print(f"Z={Z} flags={flags}: worst error / (2 x bound) {worst}")
            assert zeros_ok and max(worst.values()) <= 1.0


@gpu
@pytest.mark.parametrize("Z", [17, 130, 257])
def test_means_agree_with_the_expected_densities(cpm, Z):
    """two independent kernel families: sum over s of w[s] * P_t[s, z] against pi_t propagated from pi_0 = w (cpm_expected_dev is
    linear in pi_0), within the sum of the two bounds"""
    Tc = 6
    p_drive, p_dest, _ = _tables(Z, Tc)
    w = _w(Z, "given")
    with _sampler(cpm, p_drive, p_dest) as s:
        for flags in (0, V.IVP):
            got = s.expected_var(w, ivp=bool(flags))
            park, drv = s.expected(w, ivp=bool(flags))
            h = V.operators_behind(Tc, flags)
            tol = np.array([R.bound(Z, k) + V.bound(Z, k) for k in h])[None, :]
            tol_d = np.array([R.bound_driving(Z, k) + V.bound(Z, k) for k in h])[None, :]
            for a, b, t in ((got["mean_parking"], park, tol), (got["mean_driving"], drv, tol_d)):
                assert np.all((a == 0.0) == (b == 0.0))
                assert np.all(np.abs(a - b) <= t * np.maximum(a, b))


@gpu
def test_sparse_tables_against_a_dense_context(cpm, O):
    """tables built on the dataset route hold sparse row packs: the call expands them to the dense array first"""
    Z = 358                                                            # (the compact-row route takes T = 24 only)
    dm, dist = O.synth_datamatrix(Z, T, 11, density=0.06)
    w = _w(Z, "given")
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        s.build_p_dest(2, want=False)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        first = s.expected_var(w)                                      # (before anything else asked for the dense array)
        p_dest = s.build_p_dest(2, want=True)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        again = s.expected_var(w)
    assert _same(first, again)
    with _sampler(cpm, p_drive, p_dest) as d:
        assert d.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        dense = d.expected_var(w)
    worst, zeros_ok = V.worst_f64(first, dense, Z, T, 0)
    print(f"sparse against dense: worst error / bound {worst}")
    assert zeros_ok and max(worst.values()) <= 1.0
    want = V.numpy_var(p_drive, p_dest, w, 0)
    worst, zeros_ok = V.worst_f64(first, want, Z, T, 0, factor=2.0)
    assert zeros_ok and max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ 3: determinism, side effects
@gpu
def test_same_bits_on_a_repeated_call_and_in_a_second_context(cpm):
    Z, Tc = 257, 6
    p_drive, p_dest, _ = _tables(Z, Tc)
    w = _w(Z, "given")
    with _sampler(cpm, p_drive, p_dest) as s, _sampler(cpm, p_drive, p_dest) as s2:
        for ivp in (False, True):
            a = _dev_call(s, w, ivp)
            other = _dev_call(s, None, not ivp)                        # (another call in between leaves nothing behind)
            b = _dev_call(s, w, ivp)
            c = _dev_call(s2, w, ivp)
            assert _same(a, b) and _same(a, c) and not _same(a, other)
    # linear in w
    with _sampler(cpm, p_drive, p_dest) as s:
        a, b = s.expected_var(w), s.expected_var(4.0 * w)
        assert all(np.array_equal(4.0 * a[k], b[k]) for k in V.KEYS)


@gpu
def test_no_trace_in_a_later_expected_dev_or_resample(cpm):
    Z, cpz, seed = 67, 200, 20240611
    C = Z * cpz
    p_drive, p_dest, _ = _tables(Z, T)
    with _sampler(cpm, np.nan_to_num(p_drive), p_dest) as s:
        s.init_states(C, cpz)
        s.solve_ivp(seed, want=False)
        before, step = s.resample(seed), s.last_step()
        exp_before = s.expected(ivp=True)
        state = s.get_state()
        s.expected_var()
        s.expected_var(np.bincount(state - 1, minlength=Z).astype(np.float64), ivp=True)
        assert s.last_step() == step and np.array_equal(s.get_state(), state)
        exp_after = s.expected(ivp=True)
        after = s.resample(seed)
        assert np.array_equal(exp_before[0], exp_after[0]) and np.array_equal(exp_before[1], exp_after[1])
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step


@gpu
def test_null_outputs_of_the_blocking_form(cpm):
    Z, Tc = 33, 6
    p_drive, p_dest, _ = _tables(Z, Tc)
    with _sampler(cpm, p_drive, p_dest) as s:
        full = s.expected_var()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for keep in range(4):
            arrs = [np.full((Z, Tc), np.nan, order="F") if i == keep else None for i in range(4)]
            assert s._L.cpm_expected_var(s._h, None, 0, *[None if a is None else vp(a) for a in arrs]) == 0
            assert np.array_equal(arrs[keep], full[V.KEYS[keep]])
        assert s._L.cpm_expected_var(s._h, None, 0, None, None, None, None) == 0


@gpu
def test_every_refusal(cpm):
    Z, Tc = 24, 24
    p_drive, p_dest, _ = _tables(Z, Tc)
    big = np.array(p_dest)
    big[2, :, 4] *= 1.25
    out = np.zeros(4 * Z * Tc)
    vp = out.ctypes.data_as(ctypes.c_void_p)
    with cpm.Sampler(Z, Tc) as s:
        with pytest.raises(cpm.CpmError) as e:
            s.expected_var()
        assert e.value.status == ERR_STATE and "p_drive" in str(e.value)
        s.set_p_drive(p_drive)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_var()
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        assert s._L.cpm_expected_var_dev(s._h, None, 0, vp) == ERR_STATE
        s.set_p_dest(big)
        for _ in range(2):                                          # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected_var()
            assert e.value.status == ERR_TABLE and "hour 5, origin 3" in str(e.value)
        s.set_p_dest(p_dest)
        assert np.all(np.isfinite(s.expected_var()["var_parking"]))
        for bad in (np.nan, np.inf, -1e-9):
            w = np.ones(Z)
            w[3] = bad
            with pytest.raises(cpm.CpmError) as e:
                s.expected_var(w)
            assert e.value.status == ERR_ARG and "zone 4" in str(e.value)
        with pytest.raises(ValueError):
            s.expected_var(np.ones(Z + 1))
        with pytest.raises(cpm.CpmError) as e:
            s.expected_var_dev(0)
        assert e.value.status == ERR_ARG and "d_out" in str(e.value)
        for flags in (2, 0x100, 0x80000001):
            assert s._L.cpm_expected_var_dev(s._h, None, flags, vp) == ERR_ARG      # (refused before the pointer is looked at)
            assert s._L.cpm_expected_var(s._h, None, flags, vp, None, None, None) == ERR_ARG
        assert b"flag" in s._L.cpm_last_error()
        assert s._L.cpm_expected_var_dev(None, None, 0, vp) == ERR_ARG


# ------------------------------------------------------------------------------------------------ 4: the sampler's spread
def _device_runs(cpm, s, C, cpz, ivp):
    runs = []
    s.init_states(C, cpz)
    family = s.get_info(cpm.CPM_INFO_KERNEL)            # (what AUTO resolves to for these tables and cars: no set_kernel anywhere)
    assert family != cpm.CPM_KERNEL_AUTO
    for seed in range(1, V.RUNS + 1):
        if ivp:
            s.init_states(C, cpz)
            s.solve_ivp(seed, want=False)
        r = s.resample(seed)
        assert s.get_info(cpm.CPM_INFO_LAST_KERNEL) == family, "not the default kernel family"
        runs.append((r["parking"], r["driving"]))
    return runs


@gpu
def test_spread_of_the_device_sampler_and_the_binomial_mutant(cpm, O):
    """R = 400 seeds of Sampler.resample on the device's own default kernel family (no set_kernel; checked per run) against the
    device's expected_var: the caps and the failing mutant of tests/test_expected_var.py"""
    p_drive, p_dest, zone0, w = V.stat_setup(O)
    C = len(zone0)
    with _sampler(cpm, p_drive, p_dest) as s:
        ev = s.expected_var(w)
        runs = _device_runs(cpm, s, C, V.STAT_CPZ, False)
        assert np.array_equal(np.bincount(s.get_state() - 1, minlength=V.STAT_Z), w)
        from carparkingmaps_amd import model_selection as ms
        z = ms.count_zscores(runs[0][0], runs[0][1], ev)
        assert z["parking_fixed_ok"] and z["driving_fixed_ok"] and z["parking_fixed"][:, 0].all()
        assert np.isfinite(z["parking"][~z["parking_fixed"]]).all() and np.isfinite(z["driving"][~z["driving_fixed"]]).all()
    V.check_statistic(runs, ev, C, "device")


@gpu
def test_spread_with_the_ivp_on_the_device(cpm, O):
    p_drive, p_dest, zone0, w = V.stat_setup(O)
    C = len(zone0)
    with _sampler(cpm, p_drive, p_dest) as s:
        ev = s.expected_var(w, ivp=True)
        runs = _device_runs(cpm, s, C, V.STAT_CPZ, True)
    mean = np.stack([ev["mean_parking"], ev["mean_driving"]])
    var = np.stack([ev["var_parking"], ev["var_driving"]])
    g, kept = V.g_with(runs, mean, var, var)
    ok, m, half = V.within_cap(g, kept, list(range(T)))
    print(f"device ivp: all hours: exact {m:.4f} +- {half:.4f}")
    assert ok
    for t in range(0, 7):
        ok, m, half = V.within_cap(g, kept, [t])
        assert ok, f"hour {t}: {m:.4f} +- {half:.4f}"
