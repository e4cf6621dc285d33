"""The exact seed variance of linear functionals of a resample's counts (include/cpm_expected_linear_var.h) on the GPU: bit for bit
the integer reference on dyadic tables; within the header's bound of the exact form, and within twice it of the numpy form (whose
bits it also carries: the documented order of the sums) at the sizes the exact form is too slow for; functional k of K bit for bit the
K = 1 call; V_0 against the adjoint's grad_pi0 and indicator functionals against cpm_expected_var_dev (two other kernel families);
exactly 0 for a functional constant over the zones; linearity in the start; sparse tables, determinism, guard words, no trace in a later call, NULL d_zone, the blocking form, every refusal; the
Python layers bit for bit; and the device sampler's spread: over 400 seeds the mean of (L - mean)^2 / var is 1 within 5.5 standard
errors, and is not when the covariances between the cells are dropped.

Shapes: the product's strip is 128 origins (two per lane), a segment at least 32 destinations dealt over four waves, a pass NB = 4
functionals.  Z = 16, 17 sit in one partial strip (even: 16-byte loads; odd: the 8-byte path, origins lane and lane + 64); 33 has one
segment with a partial round; 65 two segments; 127 / 128 / 129 sit on and either side of a strip; 130 / 257 / 518 / 1,031 take several
strips and up to 32 segments, odd and even."""
import ctypes
import functools

import numpy as np
import pytest

import expected_grad_reference as G
import expected_reference as R
import expected_var_reference as V
import expected_linear_var_reference as LV

gpu = pytest.mark.gpu
T = 24
NB = 4                                       # kElvNB of csrc/cpm_expected_linear_var.h
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4
KEYS = ("mean", "var", "zone_mean", "zone_var")


def _sampler(cpm, p_drive, p_dest):
    s = cpm.Sampler(*p_drive.shape)
    s.set_p_drive(p_drive)
    s.set_p_dest(p_dest)
    return s


def _guarded(words):
    import torch
    return torch.full((2 * GUARD + words,), SENT, dtype=torch.int64, device="cuda")


def _body(buf, what):
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), f"a store outside {what}"
    assert not np.any(a[GUARD:-GUARD] == SENT), f"a word of {what} was not written"
    return a[GUARD:-GUARD].view(np.float64)


def _dev_call(s, A, B, w, ivp, zone=True):
    """expected_linear_var_dev between guard words on sentinel-filled outputs: every word written, none outside.  A, B: (Z, T, K).
    Returns dict(mean (K,), var (K,), zone_mean (Z, K), zone_var (Z, K))."""
    import torch
    K = A.shape[2]
    coeff = np.ascontiguousarray(np.stack([A.transpose(2, 1, 0), B.transpose(2, 1, 0)], axis=1))       # [K][2][T][Z]
    d_coeff = torch.from_numpy(coeff).cuda()
    out, zn = _guarded(2 * K), _guarded(2 * K * s.Z)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    s.expected_linear_var_dev(K, d_coeff.data_ptr(), out.data_ptr() + 8 * GUARD, 0 if w is None else d_w.data_ptr(), ivp,
                              zn.data_ptr() + 8 * GUARD if zone else 0)
    s.sync()
    o = _body(out, "d_out").reshape(K, 2)
    res = {"mean": o[:, 0].copy(), "var": o[:, 1].copy()}
    if zone:
        z = _body(zn, "d_zone").reshape(K, 2, s.Z)
        res["zone_mean"], res["zone_var"] = z[:, 0].T.copy(), z[:, 1].T.copy()
    else:
        assert np.all(zn.cpu().numpy() == SENT)
    return res


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _one(res, k):
    return {"mean": res["mean"][k], "var": res["var"][k], "zone_mean": res["zone_mean"][:, k], "zone_var": res["zone_var"][:, k]}


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
    """T = 3 without the IVP, tables in multiples of 2^-3 (p_drive: 2^-2), coefficients in {-2 .. 2}: the reference asserts that
    every intermediate and every partial sum in any order fits 53 bits, so any lane-map, strip-edge, residual or zero-row error shows
    with no tolerance"""
    p_drive, p_dest, w = V.dyadic_tables(Z, 3)
    A, B = LV.small_functionals(Z, 3, 3, Z)
    with _sampler(cpm, p_drive, p_dest) as s:
        got = _dev_call(s, A, B, w, False)
    for k in range(3):
        want = LV.int_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, 0, bits=53)
        assert got["mean"][k] == float(want["mean"]) and got["var"][k] == float(want["var"]), (k, got["var"][k], float(want["var"]))
        assert np.array_equal(got["zone_mean"][:, k], [float(x) for x in want["zone_mean"]])
        zv = np.array([float(x) for x in want["zone_var"]])
        assert np.array_equal(got["zone_var"][:, k], zv), np.argwhere(got["zone_var"][:, k] != zv)[:8].tolist()
        assert want["var"] > 0


# ------------------------------------------------------------------------------------------------ 2: the bound
def _check_exact(cpm, Z, Tc, flags, K):
    p_drive, p_dest, tables = _tables(Z, Tc)
    w = _w(Z, "ones" if Z % 2 == 0 else "given")
    A, B = LV.signed_functionals(Z, Tc, K, 7 * Z + Tc)
    with _sampler(cpm, p_drive, p_dest) as s:
        got = _dev_call(s, A, B, w, bool(flags))
        blk = s.expected_linear_var(A, B, start=w, ivp=bool(flags), per_zone=True)
    assert _same(got, blk)                                             # the blocking form is the device form
    for k in range(K):
        exact = LV.int_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables)
        mag = LV.int_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables, magnitude=True)
        worst, zeros_ok = LV.worst(_one(got, k), exact, LV.bounds(Z, Tc, flags, mag, w))
        print(f"Z={Z} T={Tc} flags={flags} k={k}: worst error / bound {worst}")
        assert zeros_ok and max(worst.values()) <= 1.0


@gpu
@pytest.mark.parametrize("flags", [0, LV.IVP])
@pytest.mark.parametrize("Z", [2, 3, 8, 16, 17, 33, 65])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, flags):
    _check_exact(cpm, Z, 4, flags, 2)


@gpu
@pytest.mark.parametrize("flags", [0, LV.IVP])
def test_device_meets_the_bound_over_a_whole_day(cpm, flags):
    _check_exact(cpm, 65, T, flags, 1)


@gpu
@pytest.mark.parametrize("Z", [127, 128, 129, 257, 518, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc, K = 4, NB + 1                                                  # (a full pass and a pass of one)
    p_drive, p_dest, tables = _tables(Z, Tc)
    w = _w(Z)
    A, B = LV.signed_functionals(Z, Tc, K, Z)
    with _sampler(cpm, p_drive, p_dest) as s:
        for flags in (0, LV.IVP):
            got = _dev_call(s, A, B, w, bool(flags))
            for k in (0, K - 1):
                want = LV.numpy_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables)
                mag = LV.numpy_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables, magnitude=True)
                bound = {key: 2.0 * np.asarray(v) for key, v in LV.bounds(Z, Tc, flags, mag, w).items()}
                for key in KEYS:
                    g, e, b = np.atleast_1d(_one(got, k)[key]), np.atleast_1d(want[key]), np.atleast_1d(bound[key])
                    assert np.all(np.abs(g - e) <= b), (key, flags, k, float(np.max(np.abs(g - e) / np.where(b > 0, b, 1.0))))
                assert _same(_one(got, k), want), "not the documented order of the sums"   # (the numpy form follows it step by step)


# ------------------------------------------------------------------------------------------------ 3: functional k of K
@gpu
def test_functional_k_of_K_carries_the_bits_of_a_call_on_it_alone(cpm):
    Z, Tc = 257, 4
    p_drive, p_dest, _ = _tables(Z, Tc)
    w = _w(Z)
    A, B = LV.signed_functionals(Z, Tc, 64, 1)
    with _sampler(cpm, p_drive, p_dest) as s:
        singles = [_dev_call(s, A[:, :, k:k + 1], B[:, :, k:k + 1], w, True) for k in range(64)]
        for K in (1, NB - 1, NB, NB + 1, 2 * NB + 1, 24, 64):          # partial passes, a second and a third pass
            got = _dev_call(s, np.asfortranarray(A[:, :, :K]), np.asfortranarray(B[:, :, :K]), w, True)
            for k in range(K):
                assert _same(_one(got, k), _one(singles[k], 0)), (K, k)
        # ... wherever the functional stands in its pass
        got = _dev_call(s, np.asfortranarray(A[:, :, 5:12]), np.asfortranarray(B[:, :, 5:12]), w, True)
        assert all(_same(_one(got, k), _one(singles[5 + k], 0)) for k in range(7))
    assert len({float(r["var"][0]) for r in singles}) == 64


# ------------------------------------------------------------------------------------------------ 4: two other kernel families
@gpu
@pytest.mark.parametrize("Z", [17, 130, 257])
def test_zone_means_agree_with_the_adjoint(cpm, Z):
    """V_0 is grad_pi0 of cpm_expected_grad_dev with the coefficients as cotangents (the mean is linear in pi_0), within the sum of
    the two headers' bounds"""
    Tc = 6
    p_drive, p_dest, tables = _tables(Z, Tc)
    A, B = LV.signed_functionals(Z, Tc, 2, Z)
    with _sampler(cpm, p_drive, p_dest) as s:
        for flags in (0, LV.IVP):
            got = _dev_call(s, A, B, None, bool(flags))
            for k in range(2):
                a, b = np.asfortranarray(A[:, :, k]), np.asfortranarray(B[:, :, k])
                g = s.expected_grad(a, b, ivp=bool(flags))["grad_pi0"]
                mag = LV.numpy_lv(p_drive, p_dest, a, b, None, flags, tables, magnitude=True)
                tol = np.asarray(LV.bounds(Z, Tc, flags, mag)["zone_mean"]) + G.numpy_adjoint(p_drive, p_dest, a, b, None, flags, None, tables, 1.0)[1]
                assert np.all(np.abs(got["zone_mean"][:, k] - g) <= tol)
                assert np.any(g != 0.0)


@gpu
@pytest.mark.parametrize("Z", [33, 130])
def test_indicators_agree_with_the_per_cell_variances(cpm, Z):
    """the indicator of one parking or driving cell is that cell's count: 16 cells against cpm_expected_var_dev's words, within the
    sum of the two bounds; and the mean of signed functionals against <coefficients, its means>"""
    Tc = 6
    p_drive, p_dest, tables = _tables(Z, Tc)
    w = _w(Z)
    rng = np.random.default_rng(Z)
    cells = [("parking" if i % 2 else "driving", int(rng.integers(0, Z)), int(rng.integers(0, Tc))) for i in range(16)]
    AB = [LV.indicator(Z, Tc, *c) for c in cells]
    A, B = np.asfortranarray(np.stack([a for a, _ in AB], axis=2)), np.asfortranarray(np.stack([b for _, b in AB], axis=2))
    S1, S2 = LV.signed_functionals(Z, Tc, 3, Z + 1)
    with _sampler(cpm, p_drive, p_dest) as s:
        for flags in (0, LV.IVP):
            ev = s.expected_var(w, ivp=bool(flags))
            got = _dev_call(s, A, B, w, bool(flags))
            h = V.operators_behind(Tc, flags)
            for k, (kind, z, t) in enumerate(cells):
                mag = LV.numpy_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables, magnitude=True)
                b = LV.bounds(Z, Tc, flags, mag, w)
                E = V.bound(Z, h[t]) * ev["mean_" + kind][z, t]
                assert abs(got["mean"][k] - ev["mean_" + kind][z, t]) <= b["mean"] + E, (kind, z, t)
                assert abs(got["var"][k] - ev["var_" + kind][z, t]) <= b["var"] + E, (kind, z, t)
            sg = _dev_call(s, S1, S2, w, bool(flags))
            E = np.array([V.bound(Z, k) for k in h])[None, :]
            for k in range(3):
                terms = S1[:, :, k] * ev["mean_parking"], S2[:, :, k] * ev["mean_driving"]
                inner = float(terms[0].sum() + terms[1].sum())
                mag = LV.numpy_lv(p_drive, p_dest, S1[:, :, k], S2[:, :, k], w, flags, tables, magnitude=True)
                # (the means' own bound on every term, and the 2 Z T roundings of the inner product formed here)
                tol = LV.bounds(Z, Tc, flags, mag, w)["mean"] + float(((E + 2 * Z * Tc * LV.EPS) * (np.abs(terms[0]) + np.abs(terms[1]))).sum())
                assert abs(sg["mean"][k] - inner) <= tol


# ------------------------------------------------------------------------------------------------ 5: the centring
@gpu
@pytest.mark.parametrize("Z", [65, 257])
def test_a_functional_constant_over_the_zones_has_variance_exactly_zero(cpm, Z):
    Tc = 6
    p_drive, p_dest, _ = _tables(Z, Tc)
    w = _w(Z)
    hours = np.arange(1.0, Tc + 1.0) * 0.3                             # (constant over the zones, not over the hours)
    A = np.stack([np.broadcast_to(c * hours[None, :], (Z, Tc)) for c in (1.0, 1e6)], axis=2)
    A = np.asfortranarray(np.concatenate([A, A[:, :, :1]], axis=2))    # (the third: with a driving term, a check of the check)
    B = np.zeros((Z, Tc, 3), order="F")
    B[:, :, 2] = 1.0
    with _sampler(cpm, p_drive, p_dest) as s:
        for ivp in (False, True):
            got = _dev_call(s, A, B, w, ivp)
            assert got["var"][0] == 0.0 and got["var"][1] == 0.0 and np.all(got["zone_var"][:, :2] == 0.0)
            assert got["var"][2] > 0.0
            assert abs(got["mean"][0] - hours.sum() * w.sum()) <= 1e-9 * hours.sum() * w.sum()


# ------------------------------------------------------------------------------------------------ 6: linearity in the start
@gpu
def test_ones_are_the_null_start_and_the_per_zone_output_reweighs(cpm):
    Z, Tc = 130, 6
    p_drive, p_dest, tables = _tables(Z, Tc)
    w = _w(Z)
    A, B = LV.signed_functionals(Z, Tc, 3, 2)
    with _sampler(cpm, p_drive, p_dest) as s:
        for ivp in (False, True):
            none, ones, given = _dev_call(s, A, B, None, ivp), _dev_call(s, A, B, np.ones(Z), ivp), _dev_call(s, A, B, w, ivp)
            assert _same(none, ones)
            assert _same(none, given, ("zone_mean", "zone_var"))       # (the per-zone outputs do not read the start)
            for k in range(3):
                mag = LV.numpy_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, LV.IVP if ivp else 0, tables, magnitude=True)
                b = LV.bounds(Z, Tc, LV.IVP if ivp else 0, mag, w)
                assert abs(float(w @ none["zone_mean"][:, k]) - given["mean"][k]) <= b["mean"]
                assert abs(float(w @ none["zone_var"][:, k]) - given["var"][k]) <= b["var"]
            no_zone = _dev_call(s, A, B, w, ivp, zone=False)           # NULL d_zone: the same totals from the context's own buffer
            assert _same(no_zone, given, ("mean", "var"))


# ------------------------------------------------------------------------------------------------ 7: the family's checks
@gpu
def test_sparse_tables_against_a_dense_context(cpm, O):
    """tables built on the dataset route hold sparse row packs: the call expands them to the dense array first"""
    Z = 358                                                            # (the compact-row route takes T = 24 only)
    dm, dist = O.synth_datamatrix(Z, T, 11, density=0.06)
    w = _w(Z)
    A, B = LV.signed_functionals(Z, T, 3, 3)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        s.build_p_dest(2, want=False)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        first = s.expected_linear_var(A, B, start=w, per_zone=True)    # (before anything else asked for the dense array)
        p_dest = s.build_p_dest(2, want=True)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        again = s.expected_linear_var(A, B, start=w, per_zone=True)
    assert _same(first, again)
    with _sampler(cpm, p_drive, p_dest) as d:
        assert d.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        dense = d.expected_linear_var(A, B, start=w, per_zone=True)
    assert _same(first, dense)
    assert np.all(first["var"] > 0)


@gpu
def test_same_bits_on_a_repeated_call_and_in_a_second_context(cpm):
    Z, Tc = 257, 6
    p_drive, p_dest, _ = _tables(Z, Tc)
    w = _w(Z)
    A, B = LV.signed_functionals(Z, Tc, 6, 4)
    with _sampler(cpm, p_drive, p_dest) as s, _sampler(cpm, p_drive, p_dest) as s2:
        for ivp in (False, True):
            a = _dev_call(s, A, B, w, ivp)
            other = _dev_call(s, B, A, None, not ivp)                  # (another call in between leaves nothing behind)
            b = _dev_call(s, A, B, w, ivp)
            c = _dev_call(s2, A, B, w, ivp)
            assert _same(a, b) and _same(a, c) and not _same(a, other)


@gpu
def test_no_trace_in_a_later_call_or_resample(cpm):
    Z, cpz, seed = 67, 200, 20240611
    C = Z * cpz
    p_drive, p_dest, _ = _tables(Z, T)
    A, B = LV.signed_functionals(Z, T, 5, 6)
    with _sampler(cpm, np.nan_to_num(p_drive), p_dest) as s:
        s.init_states(C, cpz)
        s.solve_ivp(seed, want=False)
        before, step = s.resample(seed), s.last_step()
        exp_before, var_before = s.expected(ivp=True), s.expected_var(ivp=True)
        grad_before = s.expected_grad(np.asfortranarray(A[:, :, 0]), np.asfortranarray(B[:, :, 0]), ivp=True)
        state = s.get_state()
        s.expected_linear_var(A, B)
        s.expected_linear_var(A, B, start=np.bincount(state - 1, minlength=Z).astype(np.float64), ivp=True)
        assert s.last_step() == step and np.array_equal(s.get_state(), state)
        exp_after, var_after = s.expected(ivp=True), s.expected_var(ivp=True)
        grad_after = s.expected_grad(np.asfortranarray(A[:, :, 0]), np.asfortranarray(B[:, :, 0]), ivp=True)
        after = s.resample(seed)
        assert np.array_equal(exp_before[0], exp_after[0]) and np.array_equal(exp_before[1], exp_after[1])
        assert all(np.array_equal(var_before[k], var_after[k]) for k in V.KEYS)
        assert all(np.array_equal(grad_before[k], grad_after[k]) for k in ("grad_p_drive", "grad_pi0"))
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step


@gpu
def test_blocking_form_shapes_and_null_outputs(cpm):
    Z, Tc = 33, 6
    p_drive, p_dest, _ = _tables(Z, Tc)
    A, B = LV.signed_functionals(Z, Tc, 3, 8)
    with _sampler(cpm, p_drive, p_dest) as s:
        full = s.expected_linear_var(A, B, per_zone=True)
        plain = s.expected_linear_var(A, B)
        assert set(plain) == {"mean", "var"} and _same(full, plain, ("mean", "var")) and full["zone_var"].shape == (Z, 3)
        one = s.expected_linear_var(A[:, :, 1], B[:, :, 1], per_zone=True)                 # (Z, T) inputs: scalars and (Z,)
        assert isinstance(one["mean"], float) and one["zone_mean"].shape == (Z,)
        assert one["mean"] == full["mean"][1] and one["var"] == full["var"][1] and np.array_equal(one["zone_var"], full["zone_var"][:, 1])
        c_order = s.expected_linear_var(np.ascontiguousarray(A), np.ascontiguousarray(B))  # (any memory order)
        assert _same(c_order, plain, ("mean", "var"))


@gpu
def test_every_refusal(cpm):
    Z, Tc = 24, 24
    p_drive, p_dest, _ = _tables(Z, Tc)
    big = np.array(p_dest)
    big[2, :, 4] *= 1.25
    A, B = LV.signed_functionals(Z, Tc, 2, 9)
    buf = np.zeros(2 * 2 * Z * Tc)
    vp = buf.ctypes.data_as(ctypes.c_void_p)
    with cpm.Sampler(Z, Tc) as s:
        with pytest.raises(cpm.CpmError) as e:
            s.expected_linear_var(A, B)
        assert e.value.status == ERR_STATE and "p_drive" in str(e.value)
        s.set_p_drive(p_drive)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_linear_var(A, B)
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        assert s._L.cpm_expected_linear_var_dev(s._h, None, 0, 1, vp, vp, None) == ERR_STATE
        s.set_p_dest(big)
        for _ in range(2):                                          # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected_linear_var(A, B)
            assert e.value.status == ERR_TABLE and "hour 5, origin 3" in str(e.value)
        s.set_p_dest(p_dest)
        assert np.all(np.isfinite(s.expected_linear_var(A, B)["var"]))
        for bad in (np.nan, np.inf, -1e-9):
            w = np.ones(Z)
            w[3] = bad
            with pytest.raises(cpm.CpmError) as e:
                s.expected_linear_var(A, B, start=w)
            assert e.value.status == ERR_ARG and "zone 4" in str(e.value)
        for bad in (np.nan, np.inf, -np.inf):
            for which in (0, 1):
                c = [A.copy(order="F"), B.copy(order="F")]
                c[which][6, 2, 1] = bad
                with pytest.raises(cpm.CpmError) as e:
                    s.expected_linear_var(*c)
                assert e.value.status == ERR_ARG and "functional 2, zone 7, hour 3" in str(e.value)
        with pytest.raises(ValueError):
            s.expected_linear_var(A, B, start=np.ones(Z + 1))
        with pytest.raises(ValueError):
            s.expected_linear_var(A, B[:, :, :1])
        for K in (0, -1, 65):
            assert s._L.cpm_expected_linear_var_dev(s._h, None, 0, K, vp, vp, None) == ERR_ARG
            assert s._L.cpm_expected_linear_var(s._h, None, 0, K, vp, vp, vp, vp, None, None) == ERR_ARG
            assert b"K = " in s._L.cpm_last_error()
        with pytest.raises(cpm.CpmError) as e:
            s.expected_linear_var_dev(1, 0, buf.ctypes.data)
        assert e.value.status == ERR_ARG and "d_coeff" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_linear_var_dev(1, buf.ctypes.data, 0)
        assert e.value.status == ERR_ARG and "d_out" in str(e.value)
        assert s._L.cpm_expected_linear_var(s._h, None, 0, 1, None, vp, vp, vp, None, None) == ERR_ARG
        assert s._L.cpm_expected_linear_var(s._h, None, 0, 1, vp, vp, None, vp, None, None) == ERR_ARG
        for flags in (2, 0x100, 0x80000001):
            assert s._L.cpm_expected_linear_var_dev(s._h, None, flags, 1, vp, vp, None) == ERR_ARG
            assert s._L.cpm_expected_linear_var(s._h, None, flags, 1, vp, vp, vp, vp, None, None) == ERR_ARG
        assert b"flag" in s._L.cpm_last_error()
        assert s._L.cpm_expected_linear_var_dev(None, None, 0, 1, vp, vp, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------ 8: the Python layers
@gpu
def test_activity_noise_and_objective_noise_are_the_explicit_functionals(cpm, O):
    from carparkingmaps_amd import model_selection as ms
    Z, Tc, C = 24, 24, 4800
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, Tc), np.asfortranarray(rng.uniform(0, 1, (Z, Tc)))     # (the Evaluator's own memory order: its sums')
    pt = ms.Point(e_drive=0.6, p_min=0.15, p_max=0.8, e_dest=2)
    start = np.full(Z, C / Z)
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        ev = ms.Evaluator(s, C=C, seed=1, measured_activity=m_act, measured_parking=m_park)
        noise = ev.expected_noise(pt, ivp=True)                        # (installs the point)
        for ivp in (False, True):
            act = ms.activity_noise(s, start, ivp=ivp)
            Bk = np.zeros((Z, Tc, Tc), order="F")
            for k in range(Tc):
                Bk[:, k, k] = 1.0
            want = s.expected_linear_var(np.zeros((Z, Tc, Tc), order="F"), Bk, start=start, ivp=ivp)
            assert _same(act, want, ("mean", "var")) and act["mean"].shape == (Tc,)
            park, drv = s.expected(None, ivp=ivp)
            assert np.all(np.abs(act["mean"] - C * drv.sum(axis=0)) <= 1e-9 * C)          # (the mean of driving_sum[t])
            assert np.all(act["var"] > 0) and np.all(act["var"] < act["mean"])          # (a sum of Bernoullis: below the Poisson's)
            on = ms.objective_noise(s, (park, drv), C, start, m_act, m_park, ivp=ivp)
            ga = ms.traffic_activity_error_grad(drv, m_act) / float(C)
            gp = ms.parking_density_error_grad(park, m_park) / float(C)
            zero = np.zeros((Z, Tc), order="F")
            va = s.expected_linear_var(zero, ga, start=start, ivp=ivp)["var"]
            vq = s.expected_linear_var(gp, zero, start=start, ivp=ivp)["var"]
            assert on == {"activity_error_std": float(np.sqrt(va)), "parking_error_std": float(np.sqrt(vq))}
            assert on["activity_error_std"] > 0 and on["parking_error_std"] > 0
            only = ms.objective_noise(s, (park, drv), C, start, measured_parking=m_park, ivp=ivp)
            assert only == {"parking_error_std": on["parking_error_std"]}
            if ivp:
                assert _same(noise["activity"], act, ("mean", "var"))
                assert {k: noise[k] for k in on} == on and set(noise) == {"activity", *on}


# ------------------------------------------------------------------------------------------------ 9: the sampler's spread
@gpu
@pytest.mark.parametrize("ivp", [False, True])
def test_spread_of_the_device_sampler_and_the_mutant_without_covariances(cpm, O, ivp):
    """R = 400 seeds of Sampler.resample on the device's own default kernel family (no set_kernel; checked per run): the functionals
    of the device's own counts against the device's expected_linear_var, the caps and the failing mutant of
    tests/test_expected_linear_var.py"""
    p_drive, p_dest, zone0, w = LV.stat_setup(O)
    C = len(zone0)
    funcs = LV.stat_functionals(V.STAT_Z, V.STAT_T)
    A, B = LV.stat_stack(funcs)
    with _sampler(cpm, p_drive, p_dest) as s:
        res = s.expected_linear_var(A, B, start=w, ivp=ivp)
        mut = LV.mutant_var(funcs, s.expected_var(w, ivp=ivp))
        runs = []
        s.init_states(C, V.STAT_CPZ)
        family = s.get_info(cpm.CPM_INFO_KERNEL)            # (what AUTO resolves to for these tables and cars: no set_kernel anywhere)
        assert family != cpm.CPM_KERNEL_AUTO
        for seed in range(1, V.RUNS + 1):
            if ivp:
                s.init_states(C, V.STAT_CPZ)
                s.solve_ivp(seed, want=False)
            r = s.resample(seed)
            assert s.get_info(cpm.CPM_INFO_LAST_KERNEL) == family, "not the default kernel family"
            runs.append((r["parking"], r["driving"]))
    LV.check_stat(LV.stat_values(runs, funcs), funcs, res["mean"], res["var"], mut, "device ivp" if ivp else "device")
