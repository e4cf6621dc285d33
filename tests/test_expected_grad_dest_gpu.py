"""The adjoint along a tangent of p_destin (include/cpm_expected_grad_dest.h) on the GPU: grad_dest against the exact (rational) form
within the header's bound and against the numpy form within twice that; grad_p_drive and grad_pi0 with expected_grad's bits; the device
entry between guard words; the same bits every time; exact zeros; no trace in a later expected, expected_grad or resample; the builder
of d p_destin / d e_dest on both routes against its definition in mpmath and against central differences of build_p_dest; the tangent
of the trip weights; the errors and what drops the tangent; and Evaluator.expected_gradient(dest=True) against central differences of
evaluate_expected in e_dest.

Shapes are those of tests/test_expected_grad_gpu.py: Z = 2, 3, 5, 67 reach rows off a 16-byte boundary and a last strip that is not
full; Z = 127, 128, 129 the edge of a 128-origin strip; Z = 1,031 several segments and more than one round of the unrolled loop."""

import mpmath
import numpy as np
import pytest

import expected_reference as R
import expected_grad_reference as G
import expected_grad_dest_reference as D
from test_expected_gpu import GUARD, SENT, _pi0, _sampler, _tables

gpu = pytest.mark.gpu
SEED = 20240611
ERR_ARG, ERR_STATE = -1, -3
INFO_SPARSE = 6      # CPM_INFO_SPARSE_TABLES


def _same(a, b):
    """bit for bit"""
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _tangent(p_dest, tables, seed, plant=True):
    """a signed random dP; plant: zeros on every zero row"""
    dP = D.signed_tangent(p_dest, seed)
    if plant:
        for t, o in np.argwhere(tables[0] == 0.0):
            dP[o, :, t] = 0.0
    return dP


def _dev_call(s, gp, gd, pi0, ivp, gn):
    """expected_grad_dest_dev between guard words on sentinel-filled outputs: every word written, none outside"""
    import torch
    Z, Tc = s.Z, s.T
    cot = torch.from_numpy(np.concatenate([gp.ravel(order="F"), gd.ravel(order="F")])).cuda()       # [2][T][Z]
    outs = [torch.full((2 * GUARD + n,), SENT, dtype=torch.int64, device="cuda") for n in (Z * Tc, Z, Z * Tc)]
    d_pi0 = None if pi0 is None else torch.from_numpy(np.ascontiguousarray(pi0)).cuda()
    d_gn = None if gn is None else torch.from_numpy(np.ascontiguousarray(gn)).cuda()
    torch.cuda.synchronize()
    at = lambda x: x.data_ptr() + 8 * GUARD
    s.expected_grad_dest_dev(cot.data_ptr(), at(outs[0]), at(outs[2]), 0 if pi0 is None else d_pi0.data_ptr(), ivp,
                             0 if gn is None else d_gn.data_ptr(), at(outs[1]))
    s.sync()
    outs = [a.cpu().numpy() for a in outs]
    for a in outs:
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
        assert not np.any(a[GUARD:-GUARD] == SENT), "a word of an output was not written"
    body = [a[GUARD:-GUARD].view(np.float64) for a in outs]
    return body[0].reshape(Tc, Z).T, body[1], body[2].reshape(Tc, Z).T


def _properties(s, got, gp, gd, pi0, ivp, gn):
    """what holds on every case: expected_grad's bits, the device entry's bits, the same bits twice"""
    plain = s.expected_grad(gp, gd, pi0, ivp=ivp, g_next=gn)
    assert _same(got["grad_p_drive"], plain["grad_p_drive"]) and _same(got["grad_pi0"], plain["grad_pi0"])
    dgrad, dpi0, ddest = _dev_call(s, gp, gd, pi0, ivp, gn)
    assert _same(dgrad, got["grad_p_drive"]) and _same(dpi0, got["grad_pi0"]) and _same(ddest, got["grad_dest"])
    again = s.expected_grad_dest(gp, gd, pi0, ivp=ivp, g_next=gn)
    assert all(_same(again[k], got[k]) for k in got)


def _zero_cases(s, dP, Z, Tc):
    gp, gd, gn = G.signed_cotangents(Z, Tc, 3)
    zp, zd, _ = G.signed_cotangents(Z, Tc, 1, "zero")
    for ivp in (False, True):
        assert not s.expected_grad_dest(zp, zd, ivp=ivp)["grad_dest"].any()          # an all-zero cotangent
    s.set_p_dest_tangent(np.zeros_like(dP))
    for ivp in (False, True):
        assert not s.expected_grad_dest(gp, gd, ivp=ivp, g_next=gn)["grad_dest"].any()   # an all-zero tangent
    s.set_p_dest_tangent(dP)


# ------------------------------------------------------------------------------------------------ 1: against the references
@gpu
@pytest.mark.parametrize("Tc", [1, 2, 24])
@pytest.mark.parametrize("Z", [2, 3, 5, 67])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, Tc):
    p_drive, p_dest, tables = _tables(Z, Tc)
    dP = _tangent(p_dest, tables, 11 * Z + Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(dP)
        assert _same(s.get_p_dest_tangent(), dP)
        variants = [(0, "uniform", False, "random"), (R.IVP, "given", True, "random")]
        if Z * Tc <= 1000:
            variants += [(f, k, n, "random") for f in (0, R.IVP) for k in ("uniform", "given") for n in (False, True)
                         if (f, k, n) not in ((0, "uniform", False), (R.IVP, "given", True))]
            variants += [(R.IVP, "uniform", False, "single"), (0, "given", True, "single")]
        for flags, kind, with_next, cot in variants:
            pi0 = _pi0(Z, kind)
            gp, gd, gn = G.signed_cotangents(Z, Tc, 7 * Z + Tc, cot)
            gn = gn if with_next else None
            got = s.expected_grad_dest(gp, gd, pi0, ivp=bool(flags), g_next=gn)
            exact, bound, _, _ = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables)
            w, z = G.worst_ratio(got["grad_dest"], exact, bound)
            print(f"Z={Z} T={Tc} flags={flags} pi0={kind} g_next={with_next} {cot}: grad_dest worst error / bound {w:.4f}")
            assert z, "a word whose magnitude is 0 is not 0"
            assert w <= 1.0
            _properties(s, got, gp, gd, pi0, bool(flags), gn)
        _zero_cases(s, dP, Z, Tc)


@gpu
def test_a_zero_row_carries_no_tangent_whatever_the_table_holds_there(cpm):
    Z, Tc = 67, 24
    p_drive, p_dest, tables = _tables(Z, Tc)
    assert (tables[0] == 0.0).any()
    dP = _tangent(p_dest, tables, 5, plant=False)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 8)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(dP)
        got = s.expected_grad_dest(gp, gd, ivp=True, g_next=gn)
        exact, bound, _, _ = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, R.IVP, gn, tables)
        w, z = G.worst_ratio(got["grad_dest"], exact, bound)
        print(f"unplanted zero row: grad_dest worst error / bound {w:.4f}")
        assert z and w <= 1.0
        for t, o in np.argwhere(tables[0] == 0.0):
            assert got["grad_dest"][o, t] == 0.0


@gpu
@pytest.mark.parametrize("Z", [127, 128, 129, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc = 3
    p_drive, p_dest, tables = _tables(Z, Tc)
    dP = _tangent(p_dest, tables, Z)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(dP)
        for flags, kind, with_next, cot in ((0, "uniform", False, "random"), (R.IVP, "given", True, "random"), (R.IVP, "uniform", False, "single")):
            pi0 = _pi0(Z, kind)
            gp, gd, gn = G.signed_cotangents(Z, Tc, 7 * Z + Tc, cot)
            gn = gn if with_next else None
            got = s.expected_grad_dest(gp, gd, pi0, ivp=bool(flags), g_next=gn)
            want = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables)[0]
            tol = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables, bound_factor=2.0)[0]
            g = got["grad_dest"]
            assert np.all(g[tol == 0.0] == 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(tol != 0.0, np.abs(g - want) / tol, 0.0)
            print(f"Z={Z} T={Tc} flags={flags} {cot}: grad_dest worst error / (2 x bound) {ratio.max():.4f}")
            assert np.all(np.isfinite(g)) and ratio.max() <= 1.0
            _properties(s, got, gp, gd, pi0, bool(flags), gn)
        _zero_cases(s, dP, Z, Tc)


# ------------------------------------------------------------------------------------------------ 2: no trace
@gpu
def test_the_call_leaves_no_trace_in_a_later_expected_gradient_or_resample(cpm):
    Z, Tc, cpz = 67, 24, 50
    C = Z * cpz
    p_drive, p_dest, tables = _tables(Z, Tc)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 4)
    with _sampler(cpm, Z, Tc, np.nan_to_num(p_drive), p_dest) as s:
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        before, step = s.resample(SEED), s.last_step()
        e0, e1 = s.expected(want_next=True), s.expected(_pi0(Z, "given"), ivp=True, want_next=True)
        g0 = s.expected_grad(gp, gd, _pi0(Z, "given"), ivp=True, g_next=gn)
        s.set_p_dest_tangent(_tangent(p_dest, tables, 9))
        s.expected_grad_dest(gp, gd)
        s.expected_grad_dest(gp, gd, _pi0(Z, "given"), ivp=True, g_next=gn)
        assert s.last_step() == step
        f0, f1 = s.expected(want_next=True), s.expected(_pi0(Z, "given"), ivp=True, want_next=True)
        for x, y in zip(e0 + e1, f0 + f1):
            assert _same(x, y)
        g1 = s.expected_grad(gp, gd, _pi0(Z, "given"), ivp=True, g_next=gn)
        assert _same(g0["grad_p_drive"], g1["grad_p_drive"]) and _same(g0["grad_pi0"], g1["grad_pi0"])
        after = s.resample(SEED)
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step


# ------------------------------------------------------------------------------------------------ 3: the builder
def _check_against_mpmath(dP, p, x, rows):
    """(worst |dP - definition| / bound over the cells with p > 0 of the given (origin, hour) rows); cells with p == 0 are exactly 0"""
    worst = mpmath.mpf(0)
    for o, t in rows:
        want, bound = D.tangent_mp(x[o, :, t], p[o, :, t])
        for d in range(p.shape[1]):
            if p[o, d, t] > 0.0 and bound[d] == 0:                   # (every cell of the row has x == 1: l, m and the tangent are 0)
                assert dP[o, d, t] == 0.0 and want[d] == 0
            elif p[o, d, t] > 0.0:
                worst = max(worst, abs(mpmath.mpf(float(dP[o, d, t])) - want[d]) / bound[d])
            else:
                assert dP[o, d, t] == 0.0
    return float(worst)


def _check_against_differences(s, e, dP):
    """dP against central differences of build_p_dest in e at h = 2^-10 and 2^-11, per row: 4 |FD(h) - FD(h / 2)| + 2^-30 max |dP|"""
    fd = {}
    for h in (2.0 ** -10, 2.0 ** -11):
        fd[h] = (s.build_p_dest(float(e) + h) - s.build_p_dest(float(e) - h)) / (2 * h)
    a, b = fd[2.0 ** -10], fd[2.0 ** -11]
    tol = 4 * np.abs(a - b) + 2.0 ** -30 * np.abs(dP).max(axis=1, keepdims=True)
    ratio = np.abs(dP - b) / np.where(tol > 0, tol, 1.0)
    assert np.all(np.abs(dP - b) <= tol), float(ratio.max())
    return float(ratio.max())


@gpu
@pytest.mark.parametrize("e", [2, 0.5, 1.7])
@pytest.mark.parametrize("Z,Tc,density,compact", [(5, 24, 0.3, False), (24, 24, 0.3, False), (67, 24, 1.0, False), (5, 3, 0.3, False),
                                                  (358, 24, 0.06, True)])
def test_builder_against_its_definition_and_against_central_differences(cpm, O, Z, Tc, density, compact, e):
    """Both routes of build_p_dest.  The compact-row route needs a row pack above the 1 KiB floor to pay (Z in the hundreds), so the
    small datamatrices all take the dense route; Z = 358 at Melbourne's density takes the compact one (as tests/test_expected_gpu.py
    relies on).  The route is asserted, not assumed."""
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=density)
    x = D.e_dest_x(dm)
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        p = s.build_p_dest(e)
        assert (s.get_info(INFO_SPARSE) != 0) == compact
        dP = s.build_p_dest_tangent(want=True)
        assert (s.get_info(INFO_SPARSE) != 0) == compact
        assert _same(dP, s.get_p_dest_tangent())
        assert np.all(dP[p == 0.0] == 0.0) and np.all(np.isfinite(dP)) and np.any(dP != 0.0)
        # the definition: every row where that takes a second or two, else the rows of three hours / every 12th origin
        hours = range(Tc) if Z <= 24 else (0, Tc // 2, Tc - 1)
        rows = [(o, t) for o in range(0, Z, 12 if Z > 100 else 1) for t in hours]
        worst = _check_against_mpmath(dP, p, x, rows)
        print(f"Z={Z} T={Tc} density={density} e_dest={e!r} compact={compact}: tangent worst error / bound {worst:.4f}")
        assert worst <= 1.0
        with np.errstate(divide="ignore"):
            mbar = (p * np.abs(np.where(p > 0.0, np.log(np.where(p > 0.0, x, 1.0)), 0.0))).sum(axis=1)
        assert np.all(np.abs(dP.sum(axis=1)) <= 8 * Z * R.EPS * mbar)              # rows sum to 0 up to rounding: |dP| <= p (|l| + m~)
        again = s.build_p_dest_tangent(want=True)
        assert _same(again, dP)
        ratio = _check_against_differences(s, e, dP)
        print(f"Z={Z} T={Tc} density={density} e_dest={e!r}: worst |dP - FD(h/2)| / tolerance {ratio:.4f}")


# ------------------------------------------------------------------------------------------------ 4: the tangent of the trip weights
@gpu
@pytest.mark.parametrize("Z", [3, 67, 129])
def test_trip_tangent_against_the_rational_form(cpm, O, Z):
    Tc = 3
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.5)
    p_drive = O.synth_p_drive(Z, Tc, 11)
    # rows of 64ths that sum to 1 exactly: no row carries a residual, so the linearity check below covers every row but the zero one
    rng = np.random.default_rng(Z)
    p_dest = np.asfortranarray(np.stack([rng.multinomial(64, np.full(Z, 1.0 / Z), size=Z) / 64.0 for _ in range(Tc)], axis=2))
    p_dest[Z - 1, :, 1] = 0.0                                          # a zero row
    tables = R.row_tables(p_dest)
    dP = _tangent(p_dest, tables, Z, plant=False)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_datamatrix(dm, dist)
        s.set_p_dest(p_dest)                                           # (a new datamatrix dropped nothing that was installed: no tangent yet)
        s.set_p_dest_tangent(dP)
        dw_sec, dw_km = s.expected_trip_tangent()
        e_sec, e_km, b_sec, b_km = D.exact_trip_tangent(dP, dm, dist, tables)
        for name, got, exact, bound in (("dw_sec", dw_sec, e_sec, b_sec), ("dw_km", dw_km, e_km, b_km)):
            w, z = G.worst_ratio(got, exact, bound)
            print(f"Z={Z}: {name} worst error / bound {w:.4f}")
            assert z and w <= 1.0
        assert dw_sec[Z - 1, 1] == 0.0 and dw_km[Z - 1, 1] == 0.0
        # the operator is linear: the tangent p itself gives the trip weights on the rows that carry no residual
        s.set_p_dest_tangent(p_dest)
        t_sec, t_km = s.expected_trip_tangent()
        w_sec, w_km = s.expected_trip()
        plain = ((tables[2] == 0.0) & (tables[0] != 0.0)).T            # (Z, T)
        assert plain.sum() == Z * Tc - 1
        _, _, pb_sec, pb_km = D.exact_trip_tangent(p_dest, dm, dist, tables)
        assert np.all(np.abs(t_sec - w_sec)[plain] <= np.array(pb_sec, dtype=np.float64)[plain])
        assert np.all(np.abs(t_km - w_km)[plain] <= np.array(pb_km, dtype=np.float64)[plain])
        import torch
        dev = torch.full((2 * GUARD + 2 * Z * Tc,), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.expected_trip_tangent_dev(dev.data_ptr() + 8 * GUARD)
        s.sync()
        dev = dev.cpu().numpy()
        assert np.all(dev[:GUARD] == SENT) and np.all(dev[-GUARD:] == SENT) and not np.any(dev[GUARD:-GUARD] == SENT)
        body = dev[GUARD:-GUARD].view(np.float64).reshape(2, Tc, Z)
        assert _same(body[0].T, t_sec) and _same(body[1].T, t_km)


# ------------------------------------------------------------------------------------------------ 5: errors, and what drops the tangent
@gpu
def test_errors_and_invalidation(cpm, O):
    Z, Tc = 24, 24
    p_drive, p_dest, tables = _tables(Z, Tc)
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 2)
    dP = _tangent(p_dest, tables, 1)

    def refused(call, status, word=None):
        with pytest.raises(cpm.CpmError) as e:
            call()
        assert e.value.status == status, str(e.value)
        assert word is None or word in str(e.value)

    with cpm.Sampler(Z, Tc) as s:
        refused(lambda: s.set_p_dest_tangent(dP), ERR_STATE, "p_dest")                     # no tables to belong to
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        grad = lambda: s.expected_grad_dest(gp, gd, g_next=gn)
        refused(grad, ERR_STATE, "tangent")                                                 # before any tangent
        refused(s.get_p_dest_tangent, ERR_STATE, "tangent")
        refused(s.build_p_dest_tangent, ERR_STATE, "cpm_build_p_dest")                      # after set_p_dest: nothing to differentiate
        s.set_p_dest_tangent(dP)
        good = grad()
        # every call that installs tables drops the tangent, and so does a new datamatrix
        s.set_p_dest(p_dest)
        refused(grad, ERR_STATE, "tangent")
        s.set_p_dest_tangent(dP)
        s.set_datamatrix(dm, dist)
        refused(grad, ERR_STATE, "tangent")
        refused(s.expected_trip_tangent, ERR_STATE, "tangent")
        s.set_p_dest_tangent(dP)
        s.build_p_dest(2, want=False)
        refused(grad, ERR_STATE, "tangent")
        s.build_p_dest_tangent()
        assert np.all(np.isfinite(grad()["grad_dest"]))
        s.set_datamatrix(dm, dist)                                                          # the tables no longer come from the resident datamatrix
        refused(s.build_p_dest_tangent, ERR_STATE, "cpm_build_p_dest")
        s.build_p_dest(0, want=False)
        refused(s.build_p_dest_tangent, ERR_STATE, "e_dest")
        s.build_p_dest(1.7, want=False)
        s.build_p_dest_tangent()
        s.synth_tables(11)
        refused(grad, ERR_STATE, "tangent")
        refused(s.build_p_dest_tangent, ERR_STATE, "cpm_build_p_dest")
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.set_p_dest_tangent(dP)
        assert all(_same(grad()[k], good[k]) for k in good)
        # CPM_ERR_ARG: refused calls leave nothing behind
        bad = np.array(dP)
        bad[3, 4, 5] = np.nan
        refused(lambda: s.set_p_dest_tangent(bad), ERR_ARG, "origin 4, destination 5, hour 6")
        for value in (np.nan, np.inf):
            for which in range(3):
                arrs = [np.array(gp), np.array(gd), np.array(gn)]
                arrs[which].flat[5] = value
                refused(lambda: s.expected_grad_dest(arrs[0], arrs[1], g_next=arrs[2]), ERR_ARG)
        a = np.zeros((Z, Tc), order="F")
        vp = lambda v: v.ctypes.data
        L, h = s._L, s._h
        for flags in (2, 0x80000001):                                                       # unknown flag bits, refused before anything is enqueued
            assert L.cpm_expected_grad_dest(h, None, flags, vp(gp), vp(gd), None, vp(a), None, vp(a)) == ERR_ARG
            assert L.cpm_expected_grad_dest_dev(h, None, flags, vp(a), None, vp(a), None, vp(a)) == ERR_ARG
        assert L.cpm_expected_grad_dest(h, None, 0, None, vp(gd), None, vp(a), None, vp(a)) == ERR_ARG
        assert L.cpm_expected_grad_dest(h, None, 0, vp(gp), vp(gd), None, None, None, vp(a)) == ERR_ARG
        assert L.cpm_expected_grad_dest(h, None, 0, vp(gp), vp(gd), None, vp(a), None, None) == ERR_ARG
        assert L.cpm_expected_grad_dest_dev(h, None, 0, None, None, vp(a), None, vp(a)) == ERR_ARG
        assert L.cpm_expected_grad_dest_dev(h, None, 0, vp(a), None, None, None, vp(a)) == ERR_ARG
        assert L.cpm_expected_grad_dest_dev(h, None, 0, vp(a), None, vp(a), None, None) == ERR_ARG
        assert L.cpm_set_p_dest_tangent(h, None) == ERR_ARG and L.cpm_get_p_dest_tangent(h, None) == ERR_ARG
        assert L.cpm_expected_trip_tangent(h, None, vp(a)) == ERR_ARG and L.cpm_expected_trip_tangent_dev(h, None) == ERR_ARG
        assert all(_same(grad()[k], good[k]) for k in good)


# ------------------------------------------------------------------------------------------------ 6: end to end
@gpu
def test_evaluator_d_e_dest_against_central_differences_of_evaluate_expected(cpm, O):
    from carparkingmaps_amd import model_selection as ms
    Z, Tc = 24, 24
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, Tc), rng.uniform(0, 1, (Z, Tc))
    pt = ms.Point(e_drive=0.6, p_min=0.15, p_max=0.8, e_dest=1.7)
    objectives = ("activity_error", "parking_error", "A_drive")
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        ev = ms.Evaluator(s, C=1, seed=SEED, measured_activity=m_act, measured_parking=m_park)
        old = {ob: ev.expected_gradient(pt, ob) for ob in objectives}
        new = {ob: ev.expected_gradient(pt, ob, dest=True) for ob in objectives}
        for ob in objectives:
            assert set(new[ob]) == set(old[ob]) | {"grad_dest", "d_e_dest"}
            for k in old[ob]:                                        # the three old derivatives, bit for bit
                assert _same(np.asarray(old[ob][k], dtype=np.float64), np.asarray(new[ob][k], dtype=np.float64)) if k != "objective" else old[ob][k] == new[ob][k]
            assert new[ob]["grad_dest"].shape == (Z, Tc)
        base = ev.evaluate_expected(pt)
        on = G.inside(s.get_p_drive())
        arg = lambda r: (r["driving"].sum(axis=0).argmin(), r["driving"].sum(axis=0).argmax(), tuple(r["parking"].argmin(axis=1)),
                         tuple(r["parking"].argmax(axis=1)))
        fd = {ob: {} for ob in objectives}
        for h in (2.0 ** -10, 2.0 ** -11):
            vals = []
            for sgn in (1.0, -1.0):
                q = ms.Point(pt.e_drive, pt.p_min, pt.p_max, pt.e_dest + sgn * h)
                r = ev.evaluate_expected(q)
                # the point is one where nothing clips and no argmin / argmax hour changes between the steps
                assert np.array_equal(G.inside(s.get_p_drive()), on), h
                assert arg(r) == arg(base), h
                vals.append(r)
            for ob in objectives:
                fd[ob][h] = (vals[0][ob] - vals[1][ob]) / (2 * h)
        for ob in objectives:
            d, a, b = new[ob]["d_e_dest"], fd[ob][2.0 ** -10], fd[ob][2.0 ** -11]
            floor = 2.0 ** -30 * max(abs(new[ob]["d_" + name]) for name in ("p_min", "p_max", "e_drive", "e_dest"))
            tol = 4 * abs(a - b) + floor
            print(f"{ob} d/de_dest: adjoint {d:.12e}, FD(h/2) {b:.12e}, |difference| / tolerance {abs(d - b) / tol:.4f}")
            assert abs(d - b) <= tol, ob
