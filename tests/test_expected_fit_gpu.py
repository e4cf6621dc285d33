"""Value and four-parameter gradient of the noise-free objectives (include/cpm_expected_fit.h) on the GPU.

Tables come from cpm_synth_datamatrix.  Z = 2, 3, 5, 67 reach odd Z and a last block that is not full, Z = 129 the edge of a 128-origin
strip, Z = 1,031 several blocks of 256 zones and several chunks of the chain rule; T = 24, and T = 5 at Z = 67.  B = 9 is a pass of
eight plus a pass of one, B = 5 a pass of the eight-fleet kernel that is not full, B = 1 the single-point form.

The reference (tests/expected_fit_reference.py) writes the header's ZONE SUM out, so wherever the header gives an order the device is
compared BIT FOR BIT -- which is inside every bound the header states; the chain rule's words 5 .. 8, whose terms go through pow and
log, are compared with the mpmath chain rule within the header's bound.

Measured parking holds an all-zero row (zone 3, where Z >= 3).  Checked on the CPU below for every case and every fleet that drives:
n_valid >= 1, and where Z >= 3 at least one zone is invalid."""
import functools

import numpy as np
import pytest

import expected_fit_reference as ref
from test_expected_gpu import GUARD, SENT

gpu = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
E_DEST = 1.7
IVP, DEST = 1, 0x100
OWN = (0.2, 0.7, 0.8)                                       # the context's own p_drive: (p_min, p_max, e_drive)

# fleet: (p_min, p_max, e_drive, (w_act, w_park, w_adrive)); e_drive 0.5, 1, 2 are pow_f64's exact branches; fleet 4 clips (p_min = 0,
# p_max = 1: entries at 0 and at 1); fleet 7 never drives: activity_error and parking_error are NaN there and carry weight 0
FLEETS = [(0.10, 0.90, 0.5, (1.0, 0.0, 0.0)), (0.15, 0.80, 1.0, (0.0, 1.0, 0.0)), (0.05, 0.70, 2.0, (0.0, 0.0, 1.0)),
          (0.20, 0.85, 0.73, (0.7, 1.3, 2.1)), (0.00, 1.00, 1.3, (1.5, 0.5, 0.25)), (0.30, 0.60, 0.5, (0.0, 2.0, 3.0)),
          (0.12, 0.95, 1.9, (2.0, 0.0, -1.0)), (0.00, 0.00, 1.0, (0.0, 0.0, 1.5)), (0.25, 0.75, 1.0, (0.3, 0.3, 0.3))]
NAN_FLEET = 7


def _same(a, b):
    """bit for bit"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def _measured(Z, Tc):
    rng = np.random.default_rng(100 * Z + Tc)
    m_act = rng.uniform(0.0, 1.0, Tc)
    m_park = np.asfortranarray(rng.uniform(0.0, 1.0, (Z, Tc)))
    if Z >= 3:
        m_park[2, :] = 0.0                                  # an all-zero row: an unmeasured zone
    for a in (m_act, m_park):
        a.setflags(write=False)
    return m_act, m_park


class _Ctx:
    """a sampler with the synthetic datamatrix, p_destin at E_DEST with its tangent, the measured arrays and a p_drive of its own"""
    def __init__(self, cpm, Z, Tc, measured=True, tangent=True):
        self.s = s = cpm.Sampler(Z, Tc)
        s.synth_datamatrix(11, density=1.0 if Z < 67 else 0.5 if Z < 200 else 0.1)
        s.build_p_dest(E_DEST, want=False)
        if tangent:
            s.build_p_dest_tangent()
        self.s_table = s.build_p_drive(0.0, 1.0, 1.0)       # (Z, T): the s of the chain rule, bit for bit (0 + 1 * s)
        self.own = s.build_p_drive(*OWN)
        self.m_act, self.m_park = _measured(Z, Tc)
        if measured:
            s.set_measured_activity(self.m_act)
            s.set_measured(self.m_park)

    def __enter__(self):
        self.s.__enter__()
        return self

    def __exit__(self, *a):
        return self.s.__exit__(*a)


def _fit_dev(s, fleets, flags, pi0=None, outputs=True):
    """expected_fit_dev between guard words on sentinel-filled outputs: every word written, none outside.  Returns numpy arrays:
    record (B, 16 + T), expected / cotangent (B, 2, T, Z), grad_p_drive / grad_dest (B, T, Z) (grad_dest None without DEST)."""
    import torch
    Z, Tc, B = s.Z, s.T, len(fleets)
    dest = bool(flags & DEST)
    sizes = dict(record=B * s.fit_words())
    if outputs:
        sizes.update(expected=B * 2 * Tc * Z, cotangent=B * 2 * Tc * Z, grad_p_drive=B * Tc * Z)
        if dest:
            sizes["grad_dest"] = B * Tc * Z
    bufs = {k: torch.full((2 * GUARD + n,), SENT, dtype=torch.int64, device="cuda") for k, n in sizes.items()}
    at = lambda k: bufs[k].data_ptr() + 8 * GUARD if k in bufs else 0
    d_pi0 = None if pi0 is None else torch.from_numpy(np.ascontiguousarray(pi0)).cuda()
    torch.cuda.synchronize()
    s.expected_fit_dev([f[0] for f in fleets], [f[1] for f in fleets], [f[2] for f in fleets], np.array([f[3] for f in fleets]), at("record"),
                       0 if pi0 is None else d_pi0.data_ptr(), bool(flags & IVP), dest, at("expected"), at("cotangent"), at("grad_p_drive"),
                       at("grad_dest"))
    s.sync()
    out = {"grad_dest": None}
    for k, buf in bufs.items():
        a = buf.cpu().numpy()
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), f"a store outside {k}"
        assert not np.any(a[GUARD:-GUARD] == SENT), f"a word of {k} was not written"
        out[k] = a[GUARD:-GUARD].view(np.float64)
    out["record"] = out["record"].reshape(B, s.fit_words())
    if outputs:
        out["expected"] = out["expected"].reshape(B, 2, Tc, Z)
        out["cotangent"] = out["cotangent"].reshape(B, 2, Tc, Z)
        out["grad_p_drive"] = out["grad_p_drive"].reshape(B, Tc, Z)
        if dest:
            out["grad_dest"] = out["grad_dest"].reshape(B, Tc, Z)
    return out


def _existing_calls(s, cot, flags, B):
    """expected_batch_dev, expected_travel_dev's totals and expected_grad[_dest]_batch_dev fed `cot`, on the installed batch tables"""
    import torch
    Z, Tc = s.Z, s.T
    exp = torch.empty(B * 2 * Tc * Z, dtype=torch.float64, device="cuda")
    tot = torch.empty(2 * B, dtype=torch.float64, device="cuda")
    d_cot = torch.from_numpy(np.ascontiguousarray(cot)).cuda()
    grad = torch.empty(B * Tc * Z, dtype=torch.float64, device="cuda")
    gdest = torch.empty(B * Tc * Z, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s.expected_batch_dev(exp.data_ptr(), 0, bool(flags & IVP))
    s.expected_travel_dev(exp.data_ptr(), B, 0, tot.data_ptr())
    if flags & DEST:
        s.expected_grad_dest_batch_dev(d_cot.data_ptr(), grad.data_ptr(), gdest.data_ptr(), 0, bool(flags & IVP))
    else:
        s.expected_grad_batch_dev(d_cot.data_ptr(), grad.data_ptr(), 0, bool(flags & IVP))
    s.sync()
    return (exp.cpu().numpy().reshape(B, 2, Tc, Z), tot.cpu().numpy().reshape(B, 2), grad.cpu().numpy().reshape(B, Tc, Z),
            gdest.cpu().numpy().reshape(B, Tc, Z) if flags & DEST else None)


WORST = {}


def _check_against_reference(c, fleets, flags, got, mp_fleets):
    """checks 1 .. 6 of the module's list for one call"""
    s = c.s
    Z, Tc, B = s.Z, s.T, len(fleets)
    rec = got["record"]
    exp, tot, grad, gdest = _existing_calls(s, got["cotangent"], flags, B)
    assert _same(got["expected"], exp), "d_expected is not expected_batch_dev's"
    assert _same(got["grad_p_drive"], grad), "d_grad_p_drive is not expected_grad_batch_dev's on d_cotangent"
    if flags & DEST:
        assert _same(got["grad_dest"], gdest), "d_grad_dest is not expected_grad_dest_batch_dev's on d_cotangent"
    assert _same(rec[:, 9], tot[:, 0]) and _same(rec[:, 10], tot[:, 1])
    assert not rec[:, 11:16].any()
    w_sec = s.expected_trip()[0].T                                  # (T, Z)
    dw_sec = s.expected_trip_tangent()[0].T if flags & DEST else None
    tables = s.get_p_drive_batch()
    want_tables = s.build_p_drive_batch([f[0] for f in fleets], [f[1] for f in fleets], [f[2] for f in fleets], want=True)
    assert _same(tables, want_tables), "the batch tables are not build_p_drive_batch's at these points"
    n_invalid = 0
    for b, (p_min, p_max, e_drive, w) in enumerate(fleets):
        park, drv = got["expected"][b, 0], got["expected"][b, 1]
        r = ref.fit_reference(park, drv, w, c.m_act, c.m_park.T, w_sec, tot[b, 0])
        if b != NAN_FLEET or fleets is not FLEETS:
            # stated for the chosen inputs: a valid zone exists, and where Z >= 3 an invalid one (the all-zero measured row)
            assert r["n_valid"] >= 1, (Z, Tc, b)
            n_invalid += int(Z - r["n_valid"])
        assert _same(got["cotangent"][b, 0], r["g_parking"]), f"fleet {b}: g_parking"
        assert _same(got["cotangent"][b, 1], r["g_driving"]), f"fleet {b}: g_driving"
        for word, key in ((0, "F"), (1, "activity_error"), (2, "parking_error"), (3, "A_drive")):
            assert _same(rec[b, word], r[key]) or (np.isnan(rec[b, word]) and np.isnan(r[key])), (b, key, rec[b, word], r[key])
        assert rec[b, 4] == r["n_valid"]
        assert _same(rec[b, 16:], r["traffic_activity"]) or (np.isnan(rec[b, 16:]).all() and np.isnan(r["traffic_activity"]).all())
        # the sums over zones also sit inside the header's bound of the exact sums
        a_exact = np.array([float(sum(map(ref.mpmath.mpf, map(float, drv[t])))) for t in range(Tc)]) if Z <= 129 else r["a"]
        assert (np.abs(r["a"] - a_exact) <= ref.zone_sum_bound(Z) * a_exact).all()
        if not flags & DEST:
            assert np.isnan(rec[b, 8])
        if b in mp_fleets:
            vals, mags = ref.chain_rule_mp(got["grad_p_drive"][b], c.s_table.T, np.ones(Z, dtype=bool), p_min, p_max, e_drive,
                                           got["grad_dest"][b] if flags & DEST else None, drv, dw_sec, w[2])
            for word, v, m in zip((5, 6, 7, 8), vals, mags):
                if v is None:
                    continue
                err, bound = abs(ref.mpmath.mpf(float(rec[b, word])) - v), ref.chain_bound(Tc, Z) * m
                assert err <= bound, (Z, Tc, b, word, float(rec[b, word]), float(v), float(err), float(bound))
                if m > 0:
                    WORST[word] = max(WORST.get(word, 0.0), float(err / bound))
    if fleets is FLEETS and Z >= 3:
        assert n_invalid >= 1
    assert np.isfinite(rec[:, 0]).all()
    if fleets is FLEETS and B > NAN_FLEET:
        assert np.isnan(rec[NAN_FLEET, 1]) and np.isnan(rec[NAN_FLEET, 2]) and rec[NAN_FLEET, 4] == 0 and rec[NAN_FLEET, 0] == 0.0
    print(f"Z={Z} T={Tc} B={B} flags={flags:#x}: worst chain-rule error / bound so far {WORST}")


# ------------------------------------------------------------------------------------------------ 1: against the references
@gpu
@pytest.mark.parametrize("Z,Tc", [(2, 24), (3, 24), (5, 24), (67, 24), (67, 5), (129, 24), (1031, 24)])
def test_device_against_the_reference_and_the_existing_calls(cpm, Z, Tc):
    with _Ctx(cpm, Z, Tc) as c:
        small = Z * Tc <= 2000
        for flags in ((0, IVP, DEST, IVP | DEST) if small else (IVP | DEST, 0)):
            got = _fit_dev(c.s, FLEETS, flags)
            _check_against_reference(c, FLEETS, flags, got, range(9) if small else (3, 4))
            if flags == IVP | DEST:
                nine = got
        # fleet b of B = 9 equals fleet b alone in a B = 1 call, for every word; and a pass of five
        for b in (range(9) if small else (0, 3, 8)):
            one = _fit_dev(c.s, [FLEETS[b]], IVP | DEST)
            for k in one:
                assert _same(one[k][0], nine[k][b]), f"fleet {b} alone differs in {k}"
        five = _fit_dev(c.s, FLEETS[2:7], IVP | DEST)
        for k in five:
            assert _same(five[k], nine[k][2:7]), f"the pass of five differs in {k}"
        # the same bits on a repeat, after the smaller batches, and with the outputs kept in the workspace
        again = _fit_dev(c.s, FLEETS, IVP | DEST)
        assert all(_same(again[k], nine[k]) for k in nine)
        assert _same(_fit_dev(c.s, FLEETS, IVP | DEST, outputs=False)["record"], nine["record"])
        # the blocking form
        host = c.s.expected_fit([f[0] for f in FLEETS], [f[1] for f in FLEETS], [f[2] for f in FLEETS], np.array([f[3] for f in FLEETS]), ivp=True,
                                dest=True, want=("expected", "cotangent", "grad_p_drive", "grad_dest"))
        assert _same(host["record"], nine["record"]) and _same(host["expected"], nine["expected"]) and _same(host["cotangent"], nine["cotangent"])
        assert _same(np.moveaxis(host["grad_p_drive"], (0, 1, 2), (2, 1, 0)), nine["grad_p_drive"])
        assert _same(np.moveaxis(host["grad_dest"], (0, 1, 2), (2, 1, 0)), nine["grad_dest"])
        assert _same(host["d_e_dest"], nine["record"][:, 8]) and _same(host["traffic_activity"], nine["record"][:, 16:])


@gpu
def test_a_given_pi0_and_no_measured_parking(cpm):
    Z, Tc = 67, 24
    with _Ctx(cpm, Z, Tc) as c:
        pi0 = np.random.default_rng(3).uniform(0.0, 2.0, Z)
        fleets = [FLEETS[0], FLEETS[2], FLEETS[6]]                  # no weight on parking_error
        with_parking = _fit_dev(c.s, fleets, IVP | DEST, pi0)
        assert not _same(with_parking["record"], _fit_dev(c.s, fleets, IVP | DEST)["record"])
        c.s.set_measured(None)
        got = _fit_dev(c.s, fleets, IVP | DEST, pi0)
        assert np.isnan(got["record"][:, 2]).all() and not got["record"][:, 4].any() and not got["cotangent"][:, 0].any()
        for k in ("expected", "grad_p_drive", "grad_dest"):
            assert _same(got[k], with_parking[k])
        assert _same(got["record"][:, [0, 1, 3, 5, 6, 7, 8]], with_parking["record"][:, [0, 1, 3, 5, 6, 7, 8]])


# ------------------------------------------------------------------------------------------------ 2: no trace
@gpu
def test_no_trace_in_later_calls_and_the_own_p_drive_is_untouched(cpm):
    Z, Tc = 67, 24
    with _Ctx(cpm, Z, Tc) as c:
        s = c.s
        s.init_states(Z * 40, 40)
        gp, gd = np.asfortranarray(np.random.default_rng(1).standard_normal((2, Z, Tc)))

        def snapshot():
            r = s.resample(77, travel=True)
            return (s.expected(ivp=True), s.expected_grad(gp, gd, ivp=True), s.expected_grad_dest(gp, gd, ivp=True), r["parking"], r["driving"],
                    r["sum_tt_q16"], s.get_p_drive())

        before = snapshot()
        _fit_dev(s, FLEETS, IVP | DEST)
        _fit_dev(s, FLEETS[:5], 0)
        after = snapshot()
        assert _same(before[0][0], after[0][0]) and _same(before[0][1], after[0][1])
        for i in (1, 2):
            assert all(_same(before[i][k], after[i][k]) for k in before[i])
        assert np.array_equal(before[3], after[3]) and np.array_equal(before[4], after[4]) and before[5] == after[5]
        assert _same(before[6], after[6]) and _same(after[6], c.own)


# ------------------------------------------------------------------------------------------------ 3: refusals
@gpu
def test_every_refusal_leaves_the_outputs_unwritten(cpm):
    import torch
    Z, Tc = 24, 24
    lo, hi, ex = [0.1, 0.2], [0.9, 0.8], [0.5, 1.0]
    w = np.array([[1.0, 1.0, 1.0], [0.0, 1.0, 0.5]])

    def refused(s, status, word, *, flags=IVP, weights=w, record=True, grad_dest=False, raw=None):
        bufs = [torch.full((4096 + 2 * Tc * Z * 2,), SENT, dtype=torch.int64, device="cuda") for _ in range(5)]
        torch.cuda.synchronize()
        ptr = [b.data_ptr() for b in bufs]
        with pytest.raises(cpm.CpmError) as e:
            if raw is not None:
                raw(ptr)
            else:
                s.expected_fit_dev(lo, hi, ex, weights, ptr[0] if record else 0, 0, bool(flags & IVP), bool(flags & DEST), ptr[1], ptr[2], ptr[3],
                                   ptr[4] if (flags & DEST or grad_dest) else 0)
        s.sync()
        assert e.value.status == status and word in str(e.value), str(e.value)
        for b in bufs:
            assert bool((b == SENT).all()), "a refused call wrote an output"

    from carparkingmaps_amd import _lib
    with _Ctx(cpm, Z, Tc, measured=False, tangent=False) as c:
        s = c.s
        L, h = s._L, s._h
        refused(s, ERR_STATE, "measured activity")
        s.set_measured_activity(c.m_act)
        refused(s, ERR_STATE, "measured parking")
        s.set_measured(c.m_park)
        refused(s, ERR_STATE, "tangent", flags=IVP | DEST)
        refused(s, ERR_ARG, "null record", record=False)
        refused(s, ERR_ARG, "not finite", weights=np.array([[1.0, np.nan, 1.0], [0.0, 1.0, 0.5]]))
        refused(s, ERR_ARG, "without CPM_FIT_DEST", grad_dest=True)
        import ctypes
        a = np.zeros(8)
        p = a.ctypes.data_as(ctypes.c_void_p)
        wv = np.ascontiguousarray(w).ctypes.data_as(ctypes.c_void_p)

        def call(B=2, p_min=p, weights=wv, flags=IVP):
            return lambda ptr: _lib.check(L.cpm_expected_fit_dev(h, B, p_min, p, p, None, flags, weights, ctypes.c_void_p(ptr[0]), ctypes.c_void_p(ptr[1]),
                                                                 ctypes.c_void_p(ptr[2]), ctypes.c_void_p(ptr[3]), None))
        refused(s, ERR_ARG, "outside 1..", raw=call(B=0))
        refused(s, ERR_ARG, "outside 1..", raw=call(B=65))
        refused(s, ERR_ARG, "null parameter", raw=call(p_min=None))
        refused(s, ERR_ARG, "null weights", raw=call(weights=None))
        refused(s, ERR_ARG, "unknown flag bits", raw=call(flags=IVP | 0x2))
        # a non-finite measured activity leaves what was installed
        bad = c.m_act.copy()
        bad[3] = np.inf
        with pytest.raises(cpm.CpmError) as e:
            s.set_measured_activity(bad)
        assert e.value.status == ERR_ARG
        good = _fit_dev(s, FLEETS[:2], IVP)
        s.set_measured_activity(c.m_act)
        assert _same(_fit_dev(s, FLEETS[:2], IVP)["record"], good["record"])
        s.set_measured_activity(None)
        refused(s, ERR_STATE, "measured activity")
    with cpm.Sampler(Z, Tc) as s:                                   # no datamatrix
        from test_expected_gpu import _tables
        p_drive, p_dest, _ = _tables(Z, Tc)
        s.set_p_dest(p_dest)
        refused(s, ERR_STATE, "datamatrix", weights=np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]))


# ------------------------------------------------------------------------------------------------ 4: the evaluator
def _evaluator(cpm, c):
    from carparkingmaps_amd import model_selection as ms
    return ms, ms.Evaluator(c.s, C=1, seed=1, measured_activity=c.m_act, measured_parking=c.m_park)


def _path_tol(Z, Tc, amp):
    """The sum of the two paths' bounds, relative to the magnitude sum M of a derivative's terms.  Host path: numpy's pairwise sums of
    at most T * Z terms, (log2(T Z) + 12) roundings with numpy's pow / log inside.  Device path: the header's chain-rule constant.  Both
    paths start from the same densities, but their cotangents differ by the order of the hour sums: the activity's min-max
    normalisation carries a relative rounding of the hour sums into (a - lo) / range amplified by amp = max(a) / range, and the adjoint
    is linear in the cotangent -- (32 + log2(Z)) roundings of either path's hour sums, three operations deep, both paths."""
    host = (np.log2(Tc * Z) + 12) * 2.0 ** -53
    cot = 2 * 3 * (32 + np.log2(Z)) * 2.0 ** -53 * amp
    return host + ref.chain_bound(Tc, Z) + cot


@gpu
@pytest.mark.parametrize("dest", [False, True])
def test_evaluator_expected_fit_against_expected_gradient_batch(cpm, dest):
    Z, Tc = 67, 24
    with _Ctx(cpm, Z, Tc) as c:
        ms, ev = _evaluator(cpm, c)
        pts = [ms.Point(e_drive=f[2], p_min=f[0], p_max=f[1], e_dest=E_DEST) for f in FLEETS[:5]]
        dens = ev.evaluate_expected_batch(pts, ivp=True)
        singles = {}
        for ob in ms.FIT_WEIGHT_KEYS:
            old = ev.expected_gradient_batch(pts, ob, ivp=True, dest=dest)
            new = ev.expected_fit(pts, {ob: 1.0}, ivp=True, dest=dest)
            singles[ob] = new
            s_tab = ev._s_table
            dw_sec = c.s.expected_trip_tangent()[0] if dest else None
            for o, n, pt, r in zip(old, new, pts, dens):
                assert set(n) >= {"value", "F", "d_p_min", "d_p_max", "d_e_drive", "traffic_activity"} and ("d_e_dest" in n) == dest
                hours = r["driving"].sum(axis=0)
                amp = hours.max() / np.ptp(hours) if ob == "activity_error" else 1.0
                tol = _path_tol(Z, Tc, amp)
                # the value is a mean of squares of terms of size <= 1 + |measured| <= 2 (min-max normalised): M = 4
                assert abs(n["value"] - o["value"]) <= tol * max(4.0, abs(o["value"])), (ob, n["value"], o["value"])
                assert n["value"] == n["F"] == n[ob]
                g = np.abs(o["grad_p_drive"])
                on = g != 0
                with np.errstate(all="ignore"):
                    se = np.where(on, np.power(s_tab, pt.e_drive), 0.0)
                    ln = np.where(on & (s_tab > 0), np.abs(np.log(np.where(s_tab > 0, s_tab, 1.0))), 0.0)
                mags = {"d_p_min": g.sum(), "d_p_max": g.sum(), "d_e_drive": (g * abs(pt.p_max - pt.p_min) * se * ln).sum()}
                if dest:
                    mags["d_e_dest"] = np.abs(o["grad_dest"]).sum()
                    if ob == "A_drive":
                        mags["d_e_dest"] += np.abs(r["driving"] * dw_sec).sum() / (Tc * 3600.0)
                for k, m in mags.items():
                    print(f"{ob} {k}: fit {n[k]:.15g} batch {o[k]:.15g} |diff| / (tol * M) {abs(n[k] - o[k]) / (tol * m) if m else 0.0:.3g}")
                    assert abs(n[k] - o[k]) <= tol * m, (ob, k, n[k], o[k], m)
        w = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}
        mixed = ev.expected_fit(pts, w, ivp=True, dest=dest)
        per_point = ev.expected_fit(pts, [w] * len(pts), ivp=True, dest=dest)
        for b in range(len(pts)):
            for k in ("F", "d_p_min", "d_p_max", "d_e_drive") + (("d_e_dest",) if dest else ()):
                parts = [w[ob] * singles[ob][b][k] for ob in ms.FIT_WEIGHT_KEYS]
                # (the adjoint is linear in the cotangent: the three runs' roundings, each within the bound above of its own magnitude,
                #  stay below 2^-30 of the parts at these shapes)
                assert abs(mixed[b][k] - sum(parts)) <= 2.0 ** -30 * sum(abs(p) for p in parts), (b, k, mixed[b][k], parts)
                assert mixed[b][k] == per_point[b][k]


@gpu
def test_evaluator_derivatives_against_central_differences_of_evaluate_expected(cpm):
    """Judged by the differences' own truncation error: the derivative from steps h and h / 2; their gap bounds the finer one's error."""
    Z, Tc = 67, 24
    with _Ctx(cpm, Z, Tc) as c:
        ms, ev = _evaluator(cpm, c)
        pt = ms.Point(e_drive=0.73, p_min=0.2, p_max=0.85, e_dest=E_DEST)
        w = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}
        got = ev.expected_fit([pt], w, ivp=True, dest=True)[0]

        def F(**kw):
            q = ms.Point(**{**dict(e_drive=pt.e_drive, p_min=pt.p_min, p_max=pt.p_max, e_dest=pt.e_dest), **kw})
            r = ev.evaluate_expected(q, ivp=True)
            return sum(w[k] * r[k] for k in w)

        base = F()
        assert abs(base - got["F"]) <= 1e-12 * abs(base)
        for name, key in (("p_min", "d_p_min"), ("p_max", "d_p_max"), ("e_drive", "d_e_drive"), ("e_dest", "d_e_dest")):
            x0 = getattr(pt, name)
            ds = [(F(**{name: x0 + h}) - F(**{name: x0 - h})) / (2 * h) for h in (2e-4, 1e-4)]
            err = abs(ds[0] - ds[1]) + 2.0 ** -53 * abs(base) / 1e-4 * 64 + 1e-9 * abs(ds[1])
            print(f"{key}: fit {got[key]:.12g} central difference {ds[1]:.12g} (gap {abs(ds[0] - ds[1]):.3g})")
            assert abs(got[key] - ds[1]) <= err, (key, got[key], ds, err)


@gpu
def test_refine_expected_descends_inside_the_bounds(cpm):
    Z, Tc = 67, 24
    with _Ctx(cpm, Z, Tc) as c:
        ms, ev = _evaluator(cpm, c)
        truth = ms.Point(e_drive=0.8, p_min=0.15, p_max=0.75, e_dest=E_DEST)
        r = ev.evaluate_expected(truth, ivp=True)
        ev = ms.Evaluator(c.s, C=1, seed=1, measured_activity=r["traffic_activity"], measured_parking=None)
        c.s.set_measured_activity(r["traffic_activity"])
        rng = np.random.default_rng(9)
        starts = [ms.Point(e_drive=truth.e_drive * (1 + 0.4 * rng.uniform(-1, 1)), p_min=truth.p_min + 0.1 * rng.uniform(-1, 1),
                           p_max=truth.p_max + 0.15 * rng.uniform(-1, 1), e_dest=E_DEST) for _ in range(5)]
        bounds = {"e_drive": (0.05, 4.0), "p_min": (0.0, 0.6), "p_max": (0.3, 1.0)}
        out = ms.refine_expected(ev, starts, {"activity_error": 1.0}, steps=10, bounds=bounds)
        assert len(out) == 5
        for k, o in enumerate(out):
            fs = [f for _, f in o["path"]]
            assert all(b <= a for a, b in zip(fs, fs[1:])), fs                     # F never increases along a path
            assert len(fs) <= 11
            for p, _ in o["path"]:
                assert bounds["e_drive"][0] <= p.e_drive <= bounds["e_drive"][1] and bounds["p_min"][0] <= p.p_min <= bounds["p_min"][1]
                assert bounds["p_max"][0] <= p.p_max <= bounds["p_max"][1] and p.p_min < p.p_max
            assert fs[-1] < fs[0], (k, fs)                                         # every start ends below its initial F
            assert len(o["gradient"]) == 3 and np.isfinite(o["gradient"]).all()
            print(f"start {k}: F {fs[0]:.3e} -> {fs[-1]:.3e} in {len(fs) - 1} accepted steps, {o['calls']} calls")
