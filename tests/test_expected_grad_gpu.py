"""The adjoint of the expected densities (include/cpm_expected_grad.h) on the GPU: the device against the exact (rational) form of the
definition within the header's bound, against the numpy form within twice that at the sizes the exact form is too slow for; exactly 0
where p_drive is clipped; the device entry between guard words; the same bits every time; no trace in a later cpm_expected or
resample; the transposition against the library's own forward pass; the errors; and Evaluator.expected_gradient against central
differences of evaluate_expected.

Shapes: Z = 2, 3, 5, 67 reach rows off a 16-byte boundary (odd Z) and a last strip that is not full; Z = 127, 128, 129 the edge of a
128-origin strip; Z = 1,031 more than one segment and more than one round of the unrolled loop."""
from fractions import Fraction

import numpy as np
import pytest

import expected_reference as R
import expected_grad_reference as G
from test_expected_gpu import GUARD, SENT, SPECIAL, _pi0, _sampler, _tables

gpu = pytest.mark.gpu
SEED = 20240611
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4


def _dev_call(s, gp, gd, pi0, ivp, gn, want_pi0=True):
    """expected_grad_dev between guard words on sentinel-filled outputs: every word written, none outside"""
    import torch
    Z, Tc = s.Z, s.T
    cot = torch.from_numpy(np.concatenate([gp.ravel(order="F"), gd.ravel(order="F")])).cuda()       # [2][T][Z]
    grad = torch.full((2 * GUARD + Z * Tc,), SENT, dtype=torch.int64, device="cuda")
    gpi0 = torch.full((2 * GUARD + Z,), SENT, dtype=torch.int64, device="cuda")
    d_pi0 = None if pi0 is None else torch.from_numpy(np.ascontiguousarray(pi0)).cuda()
    d_gn = None if gn is None else torch.from_numpy(np.ascontiguousarray(gn)).cuda()
    torch.cuda.synchronize()
    s.expected_grad_dev(cot.data_ptr(), grad.data_ptr() + 8 * GUARD, 0 if pi0 is None else d_pi0.data_ptr(), ivp,
                        0 if gn is None else d_gn.data_ptr(), gpi0.data_ptr() + 8 * GUARD if want_pi0 else 0)
    s.sync()
    grad, gpi0 = grad.cpu().numpy(), gpi0.cpu().numpy()
    for a in (grad, gpi0):
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
    assert not np.any(grad[GUARD:-GUARD] == SENT), "a word of d_grad_p_drive was not written"
    if want_pi0:
        assert not np.any(gpi0[GUARD:-GUARD] == SENT), "a word of d_grad_pi0 was not written"
    else:
        assert np.all(gpi0 == SENT)
    return grad[GUARD:-GUARD].view(np.float64).reshape(Tc, Z).T, gpi0[GUARD:-GUARD].view(np.float64)


def _special(Z, Tc):
    return [(z, 1 % Tc) for z in range(min(Z, len(SPECIAL)))]


def _same(a, b):
    """bit for bit"""
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ------------------------------------------------------------------------------------------------ 1: against the references
@gpu
@pytest.mark.parametrize("Tc", [1, 2, 24])
@pytest.mark.parametrize("Z", [2, 3, 5, 67])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, Tc):
    p_drive, p_dest, tables = _tables(Z, Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        # (flags, pi0, with G_next, cotangent): both of each at every size; all eight combinations where the exact form is quick
        variants = [(0, "uniform", False, "random"), (R.IVP, "given", True, "random")]
        if Z * Tc <= 1000:
            variants += [(f, k, n, "random") for f in (0, R.IVP) for k in ("uniform", "given") for n in (False, True)
                         if (f, k, n) not in ((0, "uniform", False), (R.IVP, "given", True))]
            variants += [(R.IVP, "uniform", False, "single"), (0, "given", True, "single")]
        for flags, kind, with_next, cot in variants:
            pi0 = _pi0(Z, kind)
            gp, gd, gn = G.signed_cotangents(Z, Tc, 7 * Z + Tc, cot)
            if cot == "single" and with_next:
                gp[:], gd[:], gn[1:] = 0.0, 0.0, 0.0               # the single word is one of G_next
                gn[0] = -0.625
            gn = gn if with_next else None
            got = s.expected_grad(gp, gd, pi0, ivp=bool(flags), g_next=gn)
            egrad, epi0, bg, bp = G.exact_with_bounds(p_drive, p_dest, gp, gd, pi0, flags, gn, tables)
            wg, zg = G.worst_ratio(got["grad_p_drive"], egrad, bg)
            wp, zp = G.worst_ratio(got["grad_pi0"], epi0, bp)
            print(f"Z={Z} T={Tc} flags={flags} pi0={kind} g_next={with_next} {cot}: worst error / bound: grad_p_drive {wg:.4f}, grad_pi0 {wp:.4f}")
            assert zg and zp, "a word whose magnitude is 0 is not 0"
            assert wg <= 1.0 and wp <= 1.0
            for z, t in _special(Z, Tc):                              # clipped entries: exactly 0
                assert got["grad_p_drive"][z, t] == 0.0
            dgrad, dpi0 = _dev_call(s, gp, gd, pi0, bool(flags), gn)  # the asynchronous entry: the same bits
            assert _same(dgrad, got["grad_p_drive"]) and _same(dpi0, got["grad_pi0"])
        gp, gd, _ = G.signed_cotangents(Z, Tc, 1, "zero")             # an all-zero cotangent: exactly 0
        for ivp in (False, True):
            got = s.expected_grad(gp, gd, ivp=ivp)
            assert not got["grad_p_drive"].any() and not got["grad_pi0"].any()


@gpu
@pytest.mark.parametrize("Z", [127, 128, 129, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc = 3
    p_drive, p_dest, tables = _tables(Z, Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        for flags, kind, with_next, cot in ((0, "uniform", False, "random"), (R.IVP, "given", True, "random"), (R.IVP, "uniform", False, "single")):
            pi0 = _pi0(Z, kind)
            gp, gd, gn = G.signed_cotangents(Z, Tc, 7 * Z + Tc, cot)
            gn = gn if with_next else None
            got = s.expected_grad(gp, gd, pi0, ivp=bool(flags), g_next=gn)
            ngrad, npi0 = G.numpy_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables)
            bg, bp = G.numpy_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables, bound_factor=2.0)
            for name, g, want, tol in (("grad_p_drive", got["grad_p_drive"], ngrad, bg), ("grad_pi0", got["grad_pi0"], npi0, bp)):
                assert np.all(g[tol == 0.0] == 0.0), name
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(tol != 0.0, np.abs(g - want) / tol, 0.0)
                print(f"Z={Z} T={Tc} flags={flags} {cot}: {name} worst error / (2 x bound) {ratio.max():.4f}")
                assert np.all(np.isfinite(g)) and ratio.max() <= 1.0, name
            for z, t in _special(Z, Tc):
                assert got["grad_p_drive"][z, t] == 0.0
            dgrad, dpi0 = _dev_call(s, gp, gd, pi0, bool(flags), gn)
            assert _same(dgrad, got["grad_p_drive"]) and _same(dpi0, got["grad_pi0"])
        gp, gd, _ = G.signed_cotangents(Z, Tc, 1, "zero")
        got = s.expected_grad(gp, gd, ivp=True)
        assert not got["grad_p_drive"].any() and not got["grad_pi0"].any()


# ------------------------------------------------------------------------------------------------ 2: the device entry, determinism, no trace
@gpu
@pytest.mark.parametrize("Z,Tc", [(67, 24), (129, 2), (1031, 3)])
def test_device_entry_writes_every_word_and_two_calls_give_the_same_bits(cpm, Z, Tc):
    p_drive, p_dest, _ = _tables(Z, Tc)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 3)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        for ivp in (False, True):
            a = s.expected_grad(gp, gd, ivp=ivp, g_next=gn)
            b = s.expected_grad(gp, gd, ivp=ivp, g_next=gn)
            assert _same(a["grad_p_drive"], b["grad_p_drive"]) and _same(a["grad_pi0"], b["grad_pi0"])
            dgrad, dpi0 = _dev_call(s, gp, gd, None, ivp, gn)
            assert _same(dgrad, a["grad_p_drive"]) and _same(dpi0, a["grad_pi0"])
            dgrad, _ = _dev_call(s, gp, gd, None, ivp, gn, want_pi0=False)       # a NULL d_grad_pi0: that array is untouched
            assert _same(dgrad, a["grad_p_drive"])
        assert np.any(a["grad_p_drive"] != 0.0) and np.any(a["grad_pi0"] != 0.0)


@gpu
def test_gradient_leaves_no_trace_in_a_later_expected_or_resample(cpm):
    Z, Tc, cpz = 67, 24, 50
    C = Z * cpz
    p_drive, p_dest, _ = _tables(Z, Tc)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 4)
    with _sampler(cpm, Z, Tc, np.nan_to_num(p_drive), p_dest) as s:
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        before, step = s.resample(SEED), s.last_step()
        e0, e1 = s.expected(want_next=True), s.expected(_pi0(Z, "given"), ivp=True, want_next=True)
        s.expected_grad(gp, gd)
        s.expected_grad(gp, gd, _pi0(Z, "given"), ivp=True, g_next=gn)
        assert s.last_step() == step
        f0, f1 = s.expected(want_next=True), s.expected(_pi0(Z, "given"), ivp=True, want_next=True)
        for x, y in zip(e0 + e1, f0 + f1):
            assert _same(x, y)
        after = s.resample(SEED)
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step


# ------------------------------------------------------------------------------------------------ 3: transposition
@gpu
@pytest.mark.parametrize("Z,Tc,flags", [(5, 3, R.IVP), (67, 24, 0)])
def test_transposition_against_the_librarys_own_forward(cpm, Z, Tc, flags):
    """<G, expected(pi0 = d)> + <G_next, pi_next> is linear in d, and grad_pi0 is its gradient: both from the device's words, compared
    in Fractions, within the forward bound on the densities plus the backward bound on grad_pi0"""
    p_drive, p_dest, tables = _tables(Z, Tc)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 9)
    F = lambda v: Fraction(float(v))
    eps = Fraction(R.EPS)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        gpi0 = s.expected_grad(gp, gd, ivp=bool(flags), g_next=gn)["grad_pi0"]
        _, lam_bar = G.magnitudes(p_drive, p_dest, gp, gd, None, flags, gn, tables)
        N, h = len(R.schedule(Tc, flags)[1]), R.operators_behind(Tc, flags)
        for k in range(3):
            d = np.random.default_rng(50 + k).uniform(0.0, 2.0, Z)
            park, drv, nxt = s.expected(d, ivp=bool(flags), want_next=True)
            lhs = sum(F(gp[z, t]) * F(park[z, t]) + F(gd[z, t]) * F(drv[z, t]) for z in range(Z) for t in range(Tc)) + sum(F(gn[z]) * F(nxt[z]) for z in range(Z))
            rhs = sum(F(gpi0[z]) * F(d[z]) for z in range(Z))
            # a device word w of the forward pass lies within b w / (1 - b) of its exact value, b its relative bound
            rel = lambda b: Fraction(float(b)) / (1 - Fraction(float(b)))
            fwd = sum(abs(F(gp[z, t])) * F(park[z, t]) * rel(R.bound(Z, h[t])) + abs(F(gd[z, t])) * F(drv[z, t]) * rel(R.bound_driving(Z, h[t]))
                      for z in range(Z) for t in range(Tc)) + sum(abs(F(gn[z])) * F(nxt[z]) * rel(R.bound(Z, h[-1] + 1)) for z in range(Z))
            bwd = sum(N * G.K(Z) * eps * lam_bar[z] * F(d[z]) for z in range(Z))
            print(f"Z={Z} T={Tc} flags={flags} direction {k}: |lhs - rhs| / (forward + backward bound) = {float(abs(lhs - rhs) / (fwd + bwd)):.4f}")
            assert abs(lhs - rhs) <= fwd + bwd


# ------------------------------------------------------------------------------------------------ 4: errors
@gpu
def test_errors(cpm):
    Z, Tc = 24, 24
    p_drive, p_dest, _ = _tables(Z, Tc)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 2)
    big = np.array(p_dest)
    big[2, :, 4] *= 1.25
    with cpm.Sampler(Z, Tc) as s:
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad(gp, gd)
        assert e.value.status == ERR_STATE
        s.set_p_drive(p_drive)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad(gp, gd)
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        s.set_p_dest(big)
        for _ in range(2):                                          # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected_grad(gp, gd)
            assert e.value.status == ERR_TABLE and "hour 5, origin 3" in str(e.value)
        s.set_p_dest(p_dest)
        good = s.expected_grad(gp, gd, g_next=gn)
        assert np.all(np.isfinite(good["grad_p_drive"]))
        for bad in (np.nan, np.inf):
            for which in range(3):
                arrs = [np.array(gp), np.array(gd), np.array(gn)]
                arrs[which].flat[5] = bad
                with pytest.raises(cpm.CpmError) as e:
                    s.expected_grad(arrs[0], arrs[1], g_next=arrs[2])
                assert e.value.status == ERR_ARG
        a = np.zeros((Z, Tc), order="F")
        vp = lambda x: x.ctypes.data
        for flags in (2, 0x80000001):                               # unknown flag bits, in both forms
            assert s._L.cpm_expected_grad(s._h, None, flags, vp(gp), vp(gd), None, vp(a), None) == ERR_ARG
            assert s._L.cpm_expected_grad_dev(s._h, None, flags, vp(a), None, vp(a), None) == ERR_ARG   # (refused before anything is enqueued)
        assert s._L.cpm_expected_grad(s._h, None, 0, None, vp(gd), None, vp(a), None) == ERR_ARG
        assert s._L.cpm_expected_grad(s._h, None, 0, vp(gp), vp(gd), None, None, None) == ERR_ARG
        assert s._L.cpm_expected_grad_dev(s._h, None, 0, None, None, vp(a), None) == ERR_ARG
        assert s._L.cpm_expected_grad_dev(s._h, None, 0, vp(a), None, None, None) == ERR_ARG
        again = s.expected_grad(gp, gd, g_next=gn)                  # the refused calls left nothing behind
        assert _same(again["grad_p_drive"], good["grad_p_drive"]) and _same(again["grad_pi0"], good["grad_pi0"])


# ------------------------------------------------------------------------------------------------ 5: end to end
@gpu
def test_evaluator_gradient_against_central_differences_of_evaluate_expected(cpm, O):
    from carparkingmaps_amd import model_selection as ms
    Z, Tc = 24, 24
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, Tc), rng.uniform(0, 1, (Z, Tc))
    pt = ms.Point(e_drive=0.6, p_min=0.15, p_max=0.8, e_dest=2)
    names = ("p_min", "p_max", "e_drive")
    objectives = ("activity_error", "parking_error", "A_drive")
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        ev = ms.Evaluator(s, C=1, seed=SEED, measured_activity=m_act, measured_parking=m_park)
        grads = {ob: ev.expected_gradient(pt, ob) for ob in objectives}
        assert _same(s.build_p_drive(pt.p_min, pt.p_max, pt.e_drive), s.get_p_drive())       # the point's own table is installed again
        base = ev.evaluate_expected(pt)
        on = G.inside(s.get_p_drive())
        for ob in objectives:
            assert grads[ob]["value"] == base[ob]
            assert not grads[ob]["grad_p_drive"][~on].any()
        arg = lambda r: (r["driving"].sum(axis=0).argmin(), r["driving"].sum(axis=0).argmax(), tuple(r["parking"].argmin(axis=1)),
                         tuple(r["parking"].argmax(axis=1)))
        fd = {ob: {} for ob in objectives}
        for name in names:
            for h in (2.0 ** -10, 2.0 ** -11):
                vals = []
                for sgn in (1.0, -1.0):
                    q = ms.Point(pt.e_drive, pt.p_min, pt.p_max, pt.e_dest)
                    setattr(q, name, getattr(pt, name) + sgn * h)
                    r = ev.evaluate_expected(q)
                    # the point is one where no parameter clips and no argmin / argmax hour changes between the steps
                    assert np.array_equal(G.inside(s.get_p_drive()), on), (name, h)
                    assert arg(r) == arg(base), (name, h)
                    vals.append(r)
                for ob in objectives:
                    fd[ob][(name, h)] = (vals[0][ob] - vals[1][ob]) / (2 * h)
        for ob in objectives:
            d = {name: grads[ob]["d_" + name] for name in names}
            floor = 2.0 ** -30 * max(abs(v) for v in d.values())
            for name in names:
                a, b = fd[ob][(name, 2.0 ** -10)], fd[ob][(name, 2.0 ** -11)]
                tol = 4 * abs(a - b) + floor
                print(f"{ob} d/d{name}: adjoint {d[name]:.12e}, FD(h/2) {b:.12e}, |difference| / tolerance {abs(d[name] - b) / tol:.4f}")
                assert abs(d[name] - b) <= tol, (ob, name)
