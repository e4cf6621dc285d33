"""Forward tangent of the expected densities (include/cpm_expected_tangent.h) on the GPU: d parking, d driving and d pi_next against
the exact (rational) tangent within the header's bound and, at the sizes the exact form is too slow for, against the numpy form within
twice that; exact zeros under clipping; the primal with expected_dev's bits; direction k of K bit for bit the K = 1 call over every
instantiation and a second and third pass; what the dP pass shares; the transposition identity <G, J v> = <J^T G, v> between this
kernel and the adjoint kernels of expected_grad_dest_dev; the builder of d p_drive / d (p_min, p_max, e_drive) against mpmath and
central differences; forward against reverse mode for the four parameters of the objectives (Evaluator.expected_jacobian against
expected_fit); guard words, repeatability, no trace in later calls, the refusals; and refine_expected_lm on the device.

Shapes: Z = 2, 3, 4, 5 reach odd rows and a single partial row group of 4; 63, 64, 65 a last partial group and both parities; 255,
256, 257 one 256-lane stride of pairs and its edges; 1,031 several strides.  T = 3 and 5, with and without the IVP."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import expected_reference as R
import expected_grad_reference as G
import expected_grad_dest_reference as D
import expected_tangent_reference as TG
from test_expected_gpu import GUARD, SENT, _pi0, _sampler, _tables
from test_expected_tangent import LM_CPU_RATIO, lm_check, lm_run

gpu = pytest.mark.gpu
SEED = 20240611
ERR_ARG, ERR_STATE = -1, -3
SMALL, LARGE = [2, 3, 4, 5, 63, 64, 65], [255, 256, 257, 1031]
C3 = np.array([0.0, -0.75, 1.5])


def _same(a, b):
    """bit for bit"""
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _dev_call(s, K, d_pi0, d_pd, c, pi0, ivp):
    """expected_tangent_dev between guard words on sentinel-filled outputs: every word written, none outside.  Returns the blocking
    call's dict (d_parking, d_driving (Z, T, K), d_pi_next (Z, K), parking, driving (Z, T))."""
    import torch
    Z, Tc = s.Z, s.T
    outs = [torch.full((2 * GUARD + n,), SENT, dtype=torch.int64, device="cuda") for n in (K * 2 * Z * Tc, K * Z, 2 * Z * Tc)]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a).ravel(order="F"))).cuda()
    d_a, d_b, d_c = up(d_pd), up(d_pi0), up(pi0)
    ptr = lambda x: 0 if x is None else x.data_ptr()
    at = lambda x: x.data_ptr() + 8 * GUARD
    torch.cuda.synchronize()
    s.expected_tangent_dev(K, at(outs[0]), ptr(d_a), ptr(d_b), c, ptr(d_c), ivp, at(outs[1]), at(outs[2]))
    s.sync()
    outs = [a.cpu().numpy() for a in outs]
    for a in outs:
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
        assert not np.any(a[GUARD:-GUARD] == SENT), "a word of an output was not written"
    body = [a[GUARD:-GUARD].view(np.float64) for a in outs]
    both, prim = body[0].reshape(K, 2, Tc, Z), body[2].reshape(2, Tc, Z)
    return dict(d_parking=both[:, 0].transpose(2, 1, 0), d_driving=both[:, 1].transpose(2, 1, 0), d_pi_next=body[1].reshape(K, Z).T,
                parking=prim[0].T, driving=prim[1].T)


def _call(s, K, d_pi0, d_pd, c, pi0, ivp):
    """the blocking call with every output; the device entry between guard words and a second call give the same bits, and the
    primal carries expected()'s"""
    got = s.expected_tangent(K, d_pd, d_pi0, c, pi0, ivp, want_next=True, want_expected=True)
    dev = _dev_call(s, K, d_pi0, d_pd, c, pi0, ivp)
    again = s.expected_tangent(K, d_pd, d_pi0, c, pi0, ivp, want_next=True, want_expected=True)
    for k in got:
        assert _same(got[k], dev[k]), f"{k}: the device entry differs from the blocking call"
        assert _same(got[k], again[k]), f"{k}: a second call gives other bits"
    parking, driving, _ = s.expected(pi0, ivp=ivp, want_next=True)
    assert _same(got["parking"], parking) and _same(got["driving"], driving), "the primal does not carry expected()'s bits"
    return got


def _case(Z, Tc, seed):
    p_drive, p_dest, tables = _tables(Z, Tc)
    d_pi0, d_pd = TG.directions(Z, Tc, 3, seed)      # (finite everywhere: the clipped entries hold values the library must ignore)
    return p_drive, p_dest, tables, d_pi0, d_pd, D.signed_tangent(p_dest, seed + 1)


# ------------------------------------------------------------------------------------------------ 1: against the references
@gpu
@pytest.mark.parametrize("Tc", [3, 5])
@pytest.mark.parametrize("Z", SMALL)
def test_device_meets_the_bound_against_the_exact_tangent(cpm, Z, Tc):
    p_drive, p_dest, tables, d_pi0, d_pd, dP = _case(Z, Tc, 11 * Z + Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(dP)                       # (zero rows left unplanted: the library must ignore the table there)
        for flags, kind in ((0, "uniform"), (R.IVP, "given")):
            pi0 = _pi0(Z, kind)
            got = _call(s, 3, d_pi0, d_pd, C3, pi0, bool(flags))
            for k in (range(3) if Z <= 5 else (2,)):   # (the exact form of a direction takes seconds at Z = 65: the one with every part)
                args = (p_drive, p_dest, pi0, flags, d_pi0[:, k], d_pd[:, :, k], C3[k], dP, tables)
                exact = TG.exact_direction(*args)
                bound = TG.exact_bounds(Z, Tc, flags, TG.magnitude(*args))
                for name, g, e, b in zip(("d_parking", "d_driving", "d_pi_next"), (got["d_parking"][:, :, k], got["d_driving"][:, :, k], got["d_pi_next"][:, k]),
                                         exact, bound):
                    w, z = TG.worst_ratio(g, e, b)
                    print(f"Z={Z} T={Tc} flags={flags} k={k} {name}: worst error / bound {w:.4f}")
                    assert z, "a word whose bound is 0 is not the exact value"
                    assert w <= 1.0


@gpu
@pytest.mark.parametrize("Tc", [3, 5])
@pytest.mark.parametrize("Z", LARGE)
def test_device_meets_twice_the_bound_against_the_numpy_tangent(cpm, Z, Tc):
    p_drive, p_dest, tables, d_pi0, d_pd, dP = _case(Z, Tc, 13 * Z + Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(dP)
        for flags, kind in ((0, "given"), (R.IVP, "uniform")):
            pi0 = _pi0(Z, kind)
            got = _call(s, 3, d_pi0, d_pd, C3, pi0, bool(flags))
            coef = TG.bounds(Z, Tc, flags)
            for k in range(3):
                args = (p_drive, p_dest, pi0, flags, d_pi0[:, k], d_pd[:, :, k], C3[k], dP, tables)
                want, mags = TG.numpy_tangent(*args), TG.numpy_tangent(*args, magnitude=True)
                for name, g, w_, m, cf in zip(("d_parking", "d_driving", "d_pi_next"), (got["d_parking"][:, :, k], got["d_driving"][:, :, k], got["d_pi_next"][:, k]),
                                              want, mags, coef):
                    tol = 2.0 * np.asarray(cf) * m
                    assert np.all(np.isfinite(g)) and np.all(g[m == 0.0] == 0.0)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ratio = np.where(tol != 0.0, np.abs(g - w_) / tol, np.where(g == w_, 0.0, np.inf))
                    print(f"Z={Z} T={Tc} flags={flags} k={k} {name}: worst error / (2 x bound) {ratio.max():.4f}")
                    assert ratio.max() <= 1.0


@gpu
@pytest.mark.parametrize("Z,Tc", [(5, 3), (65, 5), (257, 3)])
def test_clipped_directions_and_the_zero_direction_give_exact_zeros(cpm, Z, Tc):
    p_drive, p_dest, tables = _tables(Z, Tc)
    off = ~G.inside(p_drive)
    assert off.any()
    rng = np.random.default_rng(Z)
    d_pd = np.zeros((Z, Tc, 3), order="F")
    d_pd[:, :, 0][off] = rng.uniform(-1.0, 1.0, off.sum())      # confined to the clipped entries
    d_pd[:, :, 1][off] = np.inf                                  # ... whatever they hold (the device entry reads no word of it)
    d_pd[:, :, 2][off] = np.nan
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        for ivp in (False, True):
            got = _dev_call(s, 3, None, d_pd, None, None, ivp)
            assert not got["d_parking"].any() and not got["d_driving"].any() and not got["d_pi_next"].any()
            got = _call(s, 2, np.zeros((Z, 2), order="F"), np.zeros((Z, Tc, 2), order="F"), np.zeros(2), _pi0(Z, "given"), ivp)
            assert not got["d_parking"].any() and not got["d_driving"].any() and not got["d_pi_next"].any()
            got = s.expected_tangent(1, ivp=ivp, want_next=True)     # every part NULL
            assert not got["d_parking"].any() and not got["d_driving"].any() and not got["d_pi_next"].any()


# ------------------------------------------------------------------------------------------------ 2: passes
@gpu
@pytest.mark.parametrize("Z,Tc,ivp", [(5, 3, False), (65, 5, True), (257, 3, True)])
def test_direction_k_of_K_carries_the_bits_of_the_K_1_call(cpm, Z, Tc, ivp):
    """K = 1, 3, 4, 7: the instantiations of 2, 4, 5 and 8 vectors; 8: a second pass of one direction (2 vectors); 15 and 16: a third
    pass of one and two directions (2 and 4 vectors)"""
    p_drive, p_dest, tables = _tables(Z, Tc)
    d_pi0, d_pd = TG.directions(Z, Tc, 16, 5 * Z)
    c = np.where(np.arange(16) % 3 == 0, 0.0, np.linspace(-2.0, 2.0, 16))     # (zero for k = 0, 3, ..: mixed within every pass)
    pi0 = _pi0(Z, "given")
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(D.signed_tangent(p_dest, Z))
        alone = [s.expected_tangent(1, d_pd[:, :, k:k + 1], d_pi0[:, k:k + 1], c[k:k + 1], pi0, ivp, want_next=True) for k in range(16)]
        assert not _same(alone[1]["d_parking"], alone[2]["d_parking"])
        for K in (1, 3, 4, 7, 8, 15, 16):
            got = _call(s, K, d_pi0[:, :K], d_pd[:, :, :K], c[:K], pi0, ivp)
            for k in range(K):
                for name in ("d_parking", "d_driving", "d_pi_next"):
                    assert _same(got[name][..., k], alone[k][name][..., 0]), f"K={K} k={k} {name}"
        # a direction's place does not matter either: the last one first
        back = s.expected_tangent(16, d_pd[:, :, ::-1], d_pi0[:, ::-1], c[::-1], pi0, ivp, want_next=True)
        for name in ("d_parking", "d_driving", "d_pi_next"):
            assert _same(back[name][..., 0], alone[15][name][..., 0]) and _same(back[name][..., 15], alone[0][name][..., 0])


@gpu
@pytest.mark.parametrize("Z,Tc", [(5, 3), (64, 5), (257, 3)])
def test_the_dP_pass_is_shared_and_skipped_without_a_c_dest(cpm, Z, Tc):
    p_drive, p_dest, tables, d_pi0, d_pd, dP = _case(Z, Tc, 17 * Z)
    pi0 = _pi0(Z, "given")
    names = ("d_parking", "d_driving", "d_pi_next")
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        for ivp in (False, True):
            bare = s.expected_tangent(3, d_pd, d_pi0, None, pi0, ivp, want_next=True)        # no tangent installed
            s.set_p_dest_tangent(dP)
            for c in (None, np.zeros(3)):
                got = s.expected_tangent(3, d_pd, d_pi0, c, pi0, ivp, want_next=True)
                assert all(_same(got[k], bare[k]) for k in names)
            # a direction that is c_dest alone: linear in c.  A power of two scales every operation exactly -- the same bits times c.
            # Any other c rounds c * u once where the c = 1 direction does not round, and behind one operator the Z-term sums of
            # the two round differently: one rounding holds for the first operator's result, d parking of hour 1 without the IVP
            # (d pi_1 = c * u_0, against c times the c = 1 direction's u_0: the same single product); everything behind it is held
            # within the bounds of the two results
            one = s.expected_tangent(1, c_dest=[1.0], pi0=pi0, ivp=ivp, want_next=True)
            assert one["d_pi_next"].any()
            for c in (-4.0, 0.5):
                got = s.expected_tangent(1, c_dest=[c], pi0=pi0, ivp=ivp, want_next=True)
                assert all(np.array_equal(got[k], c * one[k]) for k in names)
            got = s.expected_tangent(1, c_dest=[3.0], pi0=pi0, ivp=ivp, want_next=True)
            if not ivp:
                first, base = got["d_parking"][:, 1, 0], 3.0 * one["d_parking"][:, 1, 0]
                assert base.any() and (np.abs(first - base) <= 2.0 ** -53 * np.abs(base)).all()
            mags = TG.numpy_tangent(p_drive, p_dest, pi0, R.IVP if ivp else 0, None, None, 3.0, dP, tables, magnitude=True)
            for k, m, cf in zip(names, mags, TG.bounds(Z, Tc, R.IVP if ivp else 0)):
                m = m.reshape(got[k].shape)
                cf = np.asarray(cf).reshape((1, -1, 1)) if np.ndim(cf) else cf
                assert (np.abs(got[k] - 3.0 * one[k]) <= 2.0 * cf * m + 2.0 ** -52 * np.abs(got[k])).all()
            s.set_p_dest(p_dest)                                                             # drops the tangent


# ------------------------------------------------------------------------------------------------ 3: transposition
def _dot(a, b):
    """the exact inner product of two f64 arrays"""
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(np.asarray(a).ravel(), np.asarray(b).ravel())), Fraction(0))


@gpu
@pytest.mark.parametrize("Z,Tc", [(3, 3), (64, 5), (257, 3), (1031, 3)])
def test_transposition_identity_between_the_tangent_and_the_adjoint_kernels(cpm, Z, Tc):
    """<G, tangent> + <g_next, d pi_next> from this call against <grad_p_drive, dq> + <grad_pi0, d pi_0> + c * sum(grad_dest) from
    expected_grad_dest: two independent kernel families, within the sum of the two headers' bounds contracted with |G| and |v|"""
    p_drive, p_dest, tables, d_pi0, d_pd, dP = _case(Z, Tc, 19 * Z + Tc)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 23 * Z)
    on = G.inside(p_drive)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_dest_tangent(dP)
        for flags, kind in ((0, "given"), (R.IVP, "uniform")):
            pi0, ivp = _pi0(Z, kind), bool(flags)
            tan = s.expected_tangent(3, d_pd, d_pi0, C3, pi0, ivp, want_next=True)
            adj = s.expected_grad_dest(gp, gd, pi0, ivp=ivp, g_next=gn)
            b_pd, b_pi0 = G.numpy_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables, bound_factor=1.0)
            b_dest = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables, bound_factor=1.0)[0]
            coef = TG.bounds(Z, Tc, flags)
            for k in range(3):
                dq = np.where(on, d_pd[:, :, k], 0.0)
                lhs = _dot(gp, tan["d_parking"][:, :, k]) + _dot(gd, tan["d_driving"][:, :, k]) + _dot(gn, tan["d_pi_next"][:, k])
                rhs = _dot(adj["grad_p_drive"], dq) + _dot(adj["grad_pi0"], d_pi0[:, k]) + Fraction(float(C3[k])) * _dot(adj["grad_dest"], np.ones((Z, Tc)))
                mp, md, mn = TG.numpy_tangent(p_drive, p_dest, pi0, flags, d_pi0[:, k], d_pd[:, :, k], C3[k], dP, tables, magnitude=True)
                tol = (np.abs(gp) * coef[0] * mp).sum() + (np.abs(gd) * coef[1] * md).sum() + (np.abs(gn) * coef[2] * mn).sum()
                tol += (b_pd * np.abs(dq)).sum() + (b_pi0 * np.abs(d_pi0[:, k])).sum() + abs(C3[k]) * np.abs(b_dest).sum()
                print(f"Z={Z} T={Tc} flags={flags} k={k}: |lhs - rhs| / bound {abs(float(lhs - rhs)) / tol:.4f}  (lhs {float(lhs):.6e})")
                assert lhs != 0 and abs(float(lhs - rhs)) <= tol


# ------------------------------------------------------------------------------------------------ 4: the builder
def _data_sampler(cpm, Z, Tc, e_dest=2):
    """a sampler on the oracle's synthetic datamatrix with one zone that has no data (mx <= 0); (sampler, dm, dist)"""
    from oracle import oracle as O
    O.build()
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.5)
    dm, dist = np.asfortranarray(dm), np.asfortranarray(dist)
    dm[3, :, :, :] = 0.0
    s = cpm.Sampler(Z, Tc)
    s.set_datamatrix(dm, dist)
    s.build_p_dest(e_dest, want=False)
    return s, dm, dist


@gpu
@pytest.mark.parametrize("e_drive", [0.5, 1.0, 2.0, 0.7])
@pytest.mark.parametrize("Z,Tc", [(64, 3), (65, 5)])
def test_builder_matches_its_definition_and_central_differences(cpm, Z, Tc, e_drive):
    lo, hi = 0.15, 0.8
    u = 2.0 ** -52
    with _data_sampler(cpm, Z, Tc)[0] as s:
        sv = s.build_p_drive(0.0, 1.0, 1.0)                       # s itself: identity power, p_min = 0, p_max = 1
        dead = s.build_p_drive(0.3, 0.9, 1.0) == 0.0              # mx <= 0: the table is 0 whatever the parameters
        assert dead[3].all() and not dead[[0, 1, 2]].any() and (sv[~dead] == 0.0).any()
        installed = s.build_p_drive(lo, hi, e_drive)
        got = s.build_p_drive_tangent(lo, hi, e_drive)
        import torch
        dev = torch.full((2 * GUARD + 3 * Z * Tc,), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.build_p_drive_tangent_dev(lo, hi, e_drive, dev.data_ptr() + 8 * GUARD)
        s.sync()
        dev = dev.cpu().numpy()
        assert np.all(dev[:GUARD] == SENT) and np.all(dev[-GUARD:] == SENT) and not np.any(dev[GUARD:-GUARD] == SENT)
        assert _same(dev[GUARD:-GUARD].view(np.float64), got.ravel(order="F"))
        assert _same(s.get_p_drive(), installed), "the builder touched the installed p_drive"
        assert not got[dead].any()                                # all three exactly 0 where mx <= 0
        assert not got[:, :, 2][sv <= 0.0].any()                  # d / d e_drive exactly 0 where s <= 0
        worst = [0.0, 0.0, 0.0]
        for z, t in np.argwhere(~dead):
            x = mpmath.mpf(float(sv[z, t]))
            se = mpmath.power(x, mpmath.mpf(e_drive)) if x > 0 else mpmath.mpf(0)
            want = (1 - se, se, (mpmath.mpf(hi) - mpmath.mpf(lo)) * se * mpmath.log(x) if x > 0 else mpmath.mpf(0))
            tol = (16 * u * se + u * abs(1 - se), 16 * u * se, (16 + 4 + 2) * u * abs(want[2]))
            for i in range(3):
                err = abs(mpmath.mpf(float(got[z, t, i])) - want[i])
                if tol[i] == 0:
                    assert err == 0
                else:
                    worst[i] = max(worst[i], float(err / tol[i]))
        print(f"e_drive={e_drive}: worst error / tolerance (p_min, p_max, e_drive) {worst[0]:.4f} {worst[1]:.4f} {worst[2]:.4f}")
        assert max(worst) <= 1.0
        # central differences of build_p_drive at two steps: the gap between them judges the finer one
        for i, step in enumerate((lambda h: (lo + h, hi, e_drive), lambda h: (lo, hi + h, e_drive), lambda h: (lo, hi, e_drive + h))):
            fd = [(s.build_p_drive(*step(h)) - s.build_p_drive(*step(-h))) / (2 * h) for h in (2.0 ** -10, 2.0 ** -11)]
            err = 4 * np.abs(fd[0] - fd[1]) + 64 * u * 2.0 ** 11 + 1e-9 * np.abs(fd[1])
            live = ~dead & ((sv > 0.0) if i == 2 else True)       # (at s = 0 the power has no derivative in e from the left of 0^e)
            assert (np.abs(got[:, :, i] - fd[1])[live] <= err[live]).all(), i
    with cpm.Sampler(Z, Tc) as s:
        with pytest.raises(cpm.CpmError) as e:
            s.build_p_drive_tangent(lo, hi, e_drive)
        assert e.value.status == ERR_STATE


# ------------------------------------------------------------------------------------------------ 5: forward against reverse mode
@gpu
@pytest.mark.parametrize("dest", [False, True])
@pytest.mark.parametrize("ivp", [False, True])
@pytest.mark.parametrize("Z,Tc", [(64, 3), (65, 5)])
def test_four_parameter_derivatives_match_expected_fit(cpm, Z, Tc, ivp, dest):
    """dF / d (e_drive, p_min, p_max[, e_dest]) from Evaluator.expected_jacobian and the residual JVPs against words 5 .. 8 of
    expected_fit's record: forward against reverse mode across two kernel families.  Tolerance, per parameter: this header's bound
    contracted with the cotangent of F (the forward side); the adjoint headers' bounds of grad_p_drive / grad_dest contracted with
    the direction, and the fit header's chain-rule bound (96 + ceil(T Z / 65536)) 2^-53 M, M the sum of the absolute values of the
    word's terms with s^e and 1 - s^e counted as 1 (the reverse side); and 8 (T + Z) 2^-53 times the contraction of |cotangent| with
    the tangent's magnitude for the host's own residuals and sums, the constant tests/test_expected_fit.py gives the host functions."""
    from carparkingmaps_amd import model_selection as ms
    flags = R.IVP if ivp else 0
    w = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}
    wv = (0.7, 1.3, 2.1)
    rng = np.random.default_rng(3)
    m_a, m_p = rng.random(Tc), np.asfortranarray(rng.random((Z, Tc)))
    m_p[2] = 0.0
    pt = ms.Point(0.7, 0.15, 0.8, 2)
    s, dm, dist = _data_sampler(cpm, Z, Tc)
    with s:
        ev = ms.Evaluator(s, C=1, seed=SEED, measured_activity=m_a, measured_parking=m_p)
        s.set_measured_activity(m_a)
        s.set_measured(m_p)
        jac = ev.expected_jacobian(pt, ivp=ivp, dest=dest)
        P = 4 if dest else 3
        assert jac["d_parking"].shape == (P, Z, Tc) and jac["d_driving"].shape == (P, Z, Tc)
        parking, driving = s.expected(ivp=ivp)
        assert _same(jac["parking"], parking) and _same(jac["driving"], driving)
        w_sec = s.expected_trip()[0]
        dw_sec = s.expected_trip_tangent()[0] if dest else None
        ra, Ja = ms.activity_residual_jvp(jac["driving"], jac["d_driving"], m_a)
        rp, Jp = ms.parking_residual_jvp(jac["parking"], jac["d_parking"], m_p)
        fwd = 2 * wv[0] * (Ja * ra).sum(axis=1) + 2 * wv[1] * (Jp * rp).sum(axis=(1, 2)) + wv[2] * ms.a_drive_jvp(w_sec, jac["d_driving"], jac["driving"], dw_sec)
        fit = s.expected_fit([pt.p_min], [pt.p_max], [pt.e_drive], wv, ivp=ivp, dest=dest, want=("cotangent", "grad_p_drive") + (("grad_dest",) if dest else ()))
        rev = [fit["d_e_drive"][0], fit["d_p_min"][0], fit["d_p_max"][0]] + ([fit["d_e_dest"][0]] if dest else [])
        # the magnitudes of the tolerance, from the installed tables
        p_drive, p_dest = s.get_p_drive(), s.build_p_dest(2)
        tables = R.row_tables(p_dest)
        dirs = s.build_p_drive_tangent(pt.p_min, pt.p_max, pt.e_drive)[:, :, [2, 0, 1]]
        dP = s.build_p_dest_tangent(want=True) if dest else None
        gp, gd = fit["cotangent"][0, 0].T, fit["cotangent"][0, 1].T
        b_pd, _ = G.numpy_adjoint(p_drive, p_dest, gp, gd, None, flags, None, tables, bound_factor=1.0)
        coef = TG.bounds(Z, Tc, flags)
        chain = (96 + 1) * 2.0 ** -53
        on = G.inside(p_drive)
        g_pd = np.abs(fit["grad_p_drive"][:, :, 0])
        for i in range(P):
            d_pd, c = (dirs[:, :, i], 0.0) if i < 3 else (None, 1.0)
            mp, md, _ = TG.numpy_tangent(p_drive, p_dest, None, flags, None, d_pd, c, dP, tables, magnitude=True)
            M = (np.abs(gp) * mp).sum() + (np.abs(gd) * md).sum()
            tol = (np.abs(gp) * coef[0] * mp).sum() + (np.abs(gd) * coef[1] * md).sum() + 8 * (Tc + Z) * 2.0 ** -53 * M
            if i < 3:
                dq = np.where(on, d_pd, 0.0)
                counted = np.abs(dq) if i == 0 else on.astype(np.float64)      # (s^e and 1 - s^e both count as 1)
                tol += (b_pd * np.abs(dq)).sum() + chain * (g_pd * counted).sum()
            else:
                direct = wv[2] * (np.abs(driving) * np.abs(dw_sec)).sum() / (Tc * 3600.0)
                tol += np.abs(D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, flags, None, tables, bound_factor=1.0)[0]).sum()
                tol += chain * (np.abs(fit["grad_dest"][:, :, 0]).sum() + direct) + (Z / 4 + 16) * 2.0 ** -52 * direct
            print(f"Z={Z} T={Tc} ivp={ivp} dest={dest} parameter {i}: forward {fwd[i]:.12e} reverse {rev[i]:.12e} |difference| / tolerance "
                  f"{abs(fwd[i] - rev[i]) / tol:.3e}")
            assert fwd[i] != 0.0 and abs(fwd[i] - rev[i]) <= tol


# ------------------------------------------------------------------------------------------------ 6: hygiene and refusals
@gpu
@pytest.mark.parametrize("Z,Tc", [(64, 3), (65, 5)])
def test_the_call_leaves_no_trace_in_later_calls_and_the_tangent_drops_with_the_tables(cpm, Z, Tc):
    cpz = 50
    C = Z * cpz
    rng = np.random.default_rng(9)
    gp, gd, gn = G.signed_cotangents(Z, Tc, 4)
    wv = (0.7, 1.3, 2.1)
    s, dm, dist = _data_sampler(cpm, Z, Tc)
    with s:
        s.build_p_drive(0.15, 0.8, 0.7, want=False)
        s.set_measured_activity(rng.random(Tc))
        s.set_measured(np.asfortranarray(rng.random((Z, Tc))))
        s.build_p_dest_tangent()
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        pi0 = _pi0(Z, "given")
        before, step = s.resample(SEED), s.last_step()
        e0 = s.expected(pi0, ivp=True, want_next=True)
        g0 = s.expected_grad_dest(gp, gd, pi0, ivp=True, g_next=gn)
        f0 = s.expected_fit([0.15], [0.8], [0.7], wv, ivp=True, dest=True)["record"]
        d_pi0, d_pd = TG.directions(Z, Tc, 9, 1)
        c = np.linspace(-1.0, 1.0, 9)
        t0 = _call(s, 9, d_pi0, d_pd, c, pi0, True)
        _call(s, 2, d_pi0[:, :2], d_pd[:, :, :2], None, None, False)
        assert s.last_step() == step
        e1 = s.expected(pi0, ivp=True, want_next=True)
        g1 = s.expected_grad_dest(gp, gd, pi0, ivp=True, g_next=gn)
        f1 = s.expected_fit([0.15], [0.8], [0.7], wv, ivp=True, dest=True)["record"]
        assert all(_same(x, y) for x, y in zip(e0, e1)) and all(_same(g0[k], g1[k]) for k in g0) and _same(f0, f1)
        after = s.resample(SEED)
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step
        t1 = _call(s, 9, d_pi0, d_pd, c, pi0, True)           # (and the other calls leave none in this one)
        assert all(_same(t0[k], t1[k]) for k in t0)
        # installing p_destin tables drops the tangent: a non-zero c_dest is refused, pure p_drive directions keep working
        s.set_p_dest(s.build_p_dest(2))
        with pytest.raises(cpm.CpmError) as e:
            s.expected_tangent(9, d_pd, d_pi0, c, pi0, True)
        assert e.value.status == ERR_STATE
        t2 = s.expected_tangent(9, d_pd, d_pi0, np.zeros(9), pi0, True, want_next=True)
        t3 = s.expected_tangent(9, d_pd, d_pi0, None, pi0, True, want_next=True)
        assert all(_same(t2[k], t3[k]) for k in t2) and t2["d_parking"].any()


@gpu
def test_refusals(cpm):
    import torch
    Z, Tc = 5, 3
    p_drive, p_dest, tables = _tables(Z, Tc)
    d_pi0, d_pd = TG.directions(Z, Tc, 1, 1)
    out = torch.zeros(17 * 2 * Z * Tc, dtype=torch.float64, device="cuda")
    dirs = torch.zeros(17 * Z * Tc, dtype=torch.float64, device="cuda")

    def refused(status, f, *a, **kw):
        with pytest.raises(cpm.CpmError) as e:
            f(*a, **kw)
        assert e.value.status == status, e.value

    with cpm.Sampler(Z, Tc) as s:
        refused(ERR_STATE, s.expected_tangent_dev, 1, out.data_ptr(), dirs.data_ptr())          # no tables at all
        s.set_p_drive(p_drive)
        refused(ERR_STATE, s.expected_tangent_dev, 1, out.data_ptr(), dirs.data_ptr())          # no p_destin
        s.set_p_dest(p_dest)
        s.expected_tangent_dev(1, out.data_ptr(), dirs.data_ptr())
        s.sync()
        refused(ERR_ARG, s.expected_tangent_dev, 0, out.data_ptr(), dirs.data_ptr())
        refused(ERR_ARG, s.expected_tangent_dev, 17, out.data_ptr(), dirs.data_ptr())
        for K in (0, 17):                                   # (the library's refusal on either path, whatever the arrays' shapes)
            refused(ERR_ARG, s.expected_tangent, K, d_pd, d_pi0, [1.0])
            refused(ERR_ARG, s.expected_tangent_dev, K, out.data_ptr(), dirs.data_ptr(), c_dest=[1.0])
        refused(ERR_ARG, s.expected_tangent_dev, 1, 0, dirs.data_ptr())                         # NULL d_out
        refused(ERR_ARG, s.expected_tangent_dev, 1, out.data_ptr(), dirs.data_ptr(), flags=2)
        refused(ERR_ARG, s.expected_tangent_dev, 1, out.data_ptr(), dirs.data_ptr(), flags=0x100)
        for bad in (np.nan, np.inf):
            refused(ERR_ARG, s.expected_tangent_dev, 1, out.data_ptr(), dirs.data_ptr(), c_dest=[bad])
            refused(ERR_ARG, s.expected_tangent, 1, d_pd, d_pi0, [bad])
            v = d_pd.copy()
            v[Z - 1, Tc - 1, 0] = bad
            refused(ERR_ARG, s.expected_tangent, 1, v, d_pi0)
            v = d_pi0.copy()
            v[0, 0] = bad
            refused(ERR_ARG, s.expected_tangent, 1, d_pd, v)
            v = np.ones(Z)
            v[1] = bad
            refused(ERR_ARG, s.expected_tangent, 1, d_pd, d_pi0, None, v)
        refused(ERR_STATE, s.expected_tangent_dev, 1, out.data_ptr(), dirs.data_ptr(), c_dest=[1.0])   # no tangent installed
        refused(ERR_STATE, s.expected_tangent, 1, d_pd, d_pi0, [0.5])
        s.expected_tangent(1, d_pd, d_pi0, [0.0])
        refused(ERR_ARG, s.build_p_drive_tangent_dev, 0.1, 0.9, 0.5, 0)
        refused(ERR_STATE, s.build_p_drive_tangent_dev, 0.1, 0.9, 0.5, out.data_ptr())          # no datamatrix


# ------------------------------------------------------------------------------------------------ 7: Levenberg-Marquardt on the device
@gpu
def test_refine_expected_lm_reaches_the_cpu_tests_ratio_on_the_device(cpm):
    """The planted problem of tests/test_expected_tangent.py through Evaluator.expected_jacobian: the same bound on F(last) / F(start),
    10 times the numpy run's ratio, and the same properties of the path."""
    from carparkingmaps_amd import model_selection as ms
    from oracle import oracle as O
    O.build()
    prob = TG.lm_problem(O)
    with cpm.Sampler(TG.LM_Z, TG.LM_T) as s:
        s.set_datamatrix(prob["dm"], prob["dist"])
        ev = ms.Evaluator(s, C=1, seed=SEED, measured_activity=prob["measured_activity"], measured_parking=prob["measured_parking"])
        out = lm_run(ms, ev, None)
        lm_check(out, 10 * LM_CPU_RATIO, np.array([1e-3, 0.0, 0.0]), np.array([16.0, 1.0, 1.0]), 1e-3)
