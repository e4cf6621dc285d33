"""The batched adjoint of the expected densities (include/cpm_expected_grad_batch.h) on the GPU.  The main test is bit equality: fleet
b's slices of every output against the B = 1 device entries with fleet b's table installed and fleet b's cotangents.  Then the
outputs against the definition (the exact rational form within the header's bound, the numpy form within twice that), the device
entries between guard words, the same bits every time and in either order of batch sizes on one context, no trace in later calls, the
errors, and Evaluator.expected_gradient_batch against expected_gradient.

Every batch has distinct random p_drive tables and distinct signed cotangents (a seed per fleet), so a mix-up of fleets, passes or
strides shows.  Fleet 0's table carries the entries 0, 1, NaN, negative and above 1 (exactly 0 there); the last fleet of a batch of two
or more has an all-zero cotangent (its outputs are exactly 0).  The p_destin tables are those of tests/test_expected_gpu.py with a
zero row and a row whose total is below 1 planted at every size.

Shapes: T = 3.  Z = 2, 3, 5, 67 reach rows off a 16-byte boundary and a strip that is not full; 64, 127, 128, 129, 257 the edges of
the 128-origin strips; 1,031 several segments and more than one round of the unrolled loop.  B = 1 takes the B = 1 kernels, 2, 3, 5
and 8 every instantiation of the batched ones (3 and 5 with fleets that are computed and not stored), 9 and 17 a second and a third
pass of one fleet behind full ones."""
import functools

import numpy as np
import pytest

import expected_reference as R
import expected_grad_reference as G
import expected_grad_dest_reference as D
from test_expected_gpu import GUARD, SENT, SPECIAL, _pi0, _sampler, _tables
from test_expected_grad_gpu import _dev_call as _single, _same, _special
from test_expected_grad_dest_gpu import _dev_call as _single_dest, _tangent

gpu = pytest.mark.gpu
SEED = 20240611
ERR_ARG, ERR_STATE = -1, -3
TC = 3
ALL_Z = [2, 3, 5, 64, 67, 127, 128, 129, 257, 1031]
ALL_B = [1, 2, 3, 5, 8, 9, 17]
PAIRS = sorted({(Z, B) for Z in ALL_Z for B in (3, 9)} | {(Z, B) for Z in (129, 1031) for B in ALL_B})


@functools.lru_cache(maxsize=None)
def _dest_tables(Z, Tc):
    """(p_dest, row tables) -- computed once and shared; nobody writes to them.  A zero row in the middle hour and a row scaled by 0.7
    in every hour, whose residual goes to its last destination, at every Z"""
    p_dest = np.array(_tables(Z, Tc)[1], order="F")
    p_dest[Z - 1, :, (Tc - 1) // 2] = 0.0
    p_dest[0, :, :] *= 0.7
    p_dest.setflags(write=False)
    tables = R.row_tables(p_dest)
    assert (tables[0] == 0.0).any() and (tables[2] > 0.25).any()
    return p_dest, tables


def _fleet_tables(Z, Tc, B, seed=0):
    """(Z, Tc, B) F-order: random tables strictly inside (0, 1); fleet 0 with SPECIAL planted where _special says"""
    pd = np.asfortranarray(np.random.default_rng(1000 * Z + B + seed).uniform(0.02, 0.98, (Z, Tc, B)))
    k = min(Z, len(SPECIAL))
    pd[:k, 1 % Tc, 0] = SPECIAL[:k]
    return pd


def _fleet_cotangents(Z, Tc, B, seed=0):
    """g_park, g_drv (Z, Tc, B), g_next (Z, B), F-order: a seed per fleet; the last fleet of B >= 2 all zero"""
    gp, gd, gn = (np.zeros((Z, Tc, B), order="F"), np.zeros((Z, Tc, B), order="F"), np.zeros((Z, B), order="F"))
    for b in range(B):
        kind = "zero" if (B >= 2 and b == B - 1) else "random"
        gp[:, :, b], gd[:, :, b], gn[:, b] = G.signed_cotangents(Z, Tc, 31 * Z + 7 * b + seed, kind)
    return gp, gd, gn


def _batch_call(s, B, gp, gd, pi0, ivp, gn, want_pi0=True, dest=False):
    """the batched device entry between guard words on sentinel-filled outputs: every word written, none outside.  Returns
    grad_p_drive (Z, T, B), grad_pi0 (Z, B) or None, grad_dest (Z, T, B) or None"""
    import torch
    Z, Tc = s.Z, s.T
    cot = np.empty((B, 2, Tc, Z))
    for b in range(B):
        cot[b, 0], cot[b, 1] = gp[:, :, b].T, gd[:, :, b].T
    d_cot = torch.from_numpy(cot).cuda()
    outs = [torch.full((2 * GUARD + n,), SENT, dtype=torch.int64, device="cuda") for n in (B * Z * Tc, B * Z, B * Z * Tc)]
    d_pi0 = None if pi0 is None else torch.from_numpy(np.ascontiguousarray(pi0)).cuda()
    d_gn = None if gn is None else torch.from_numpy(np.ascontiguousarray(gn.T)).cuda()                # [B][Z]
    torch.cuda.synchronize()
    at = lambda x: x.data_ptr() + 8 * GUARD
    args = dict(d_pi0_ptr=0 if pi0 is None else d_pi0.data_ptr(), ivp=ivp, d_gnext_ptr=0 if gn is None else d_gn.data_ptr(),
                d_grad_pi0_ptr=at(outs[1]) if want_pi0 else 0)
    if dest:
        s.expected_grad_dest_batch_dev(d_cot.data_ptr(), at(outs[0]), at(outs[2]), **args)
    else:
        s.expected_grad_batch_dev(d_cot.data_ptr(), at(outs[0]), **args)
    s.sync()
    outs = [a.cpu().numpy() for a in outs]
    for a, written in zip(outs, (True, want_pi0, dest)):
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside an output"
        if written:
            assert not np.any(a[GUARD:-GUARD] == SENT), "a word of an output was not written"
        else:
            assert np.all(a == SENT), "an output that was not asked for was written"
    body = [a[GUARD:-GUARD].view(np.float64) for a in outs]
    return (body[0].reshape(B, Tc, Z).transpose(2, 1, 0), body[1].reshape(B, Z).T if want_pi0 else None,
            body[2].reshape(B, Tc, Z).transpose(2, 1, 0) if dest else None)


def _planted_zeros(Z, Tc, B, grad, gpi0, gdest):
    for z, t in _special(Z, Tc):                                       # fleet 0: clipped entries
        assert grad[z, t, 0] == 0.0
    if B >= 2:                                                         # the last fleet: an all-zero cotangent
        for a in (grad, gpi0, gdest):
            assert a is None or not a[..., B - 1].any()


# ------------------------------------------------------------------------------------------------ 1: the bits of the B = 1 calls
VARIANTS = [(False, False, True, False), (True, True, False, True), (False, True, True, True), (True, False, False, False)]


@gpu
@pytest.mark.parametrize("Z,B", PAIRS)
def test_fleet_b_carries_the_bits_of_the_single_call(cpm, Z, B):
    Tc = TC
    p_dest, tables = _dest_tables(Z, Tc)
    pd = _fleet_tables(Z, Tc, B)
    gp, gd, gn_all = _fleet_cotangents(Z, Tc, B)
    pi0 = _pi0(Z, "given")
    with _sampler(cpm, Z, Tc, pd[:, :, 0], p_dest) as s:
        s.set_p_dest_tangent(_tangent(p_dest, tables, Z + B))
        s.set_p_drive_batch(pd)
        got = {}
        for v in VARIANTS:                                             # (ivp, with G_next, with grad_pi0, dest)
            ivp, with_next, want_pi0, dest = v
            got[v] = _batch_call(s, B, gp, gd, pi0 if ivp else None, ivp, gn_all if with_next else None, want_pi0, dest)
            _planted_zeros(Z, Tc, B, *got[v])
        assert np.any(got[VARIANTS[1]][2] != 0.0)
        for b in range(B):
            s.set_p_drive(pd[:, :, b])
            g_p, g_d = np.asfortranarray(gp[:, :, b]), np.asfortranarray(gd[:, :, b])
            for v in VARIANTS:
                ivp, with_next, want_pi0, dest = v
                gn = np.ascontiguousarray(gn_all[:, b]) if with_next else None
                if dest:
                    grad, gpi0, gdest = _single_dest(s, g_p, g_d, pi0 if ivp else None, ivp, gn)
                else:
                    grad, gpi0 = _single(s, g_p, g_d, pi0 if ivp else None, ivp, gn)
                bgrad, bpi0, bdest = got[v]
                assert _same(bgrad[:, :, b], grad), (v, b)
                assert not want_pi0 or _same(bpi0[:, b], gpi0), (v, b)
                assert not dest or _same(bdest[:, :, b], gdest), (v, b)


# ------------------------------------------------------------------------------------------------ 2: against the definition
@gpu
@pytest.mark.parametrize("Z", [2, 3, 5, 67])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z):
    Tc, B = TC, 5
    p_dest, tables = _dest_tables(Z, Tc)
    pd = _fleet_tables(Z, Tc, B, 1)
    gp, gd, gn_all = _fleet_cotangents(Z, Tc, B, 1)
    dP = _tangent(p_dest, tables, Z)
    with _sampler(cpm, Z, Tc, pd[:, :, 0], p_dest) as s:
        s.set_p_dest_tangent(dP)
        s.set_p_drive_batch(pd)
        variants = [(R.IVP, "given", True)] + ([(0, "uniform", False)] if Z <= 5 else [])
        for flags, kind, with_next in variants:
            pi0 = _pi0(Z, kind)
            grad, gpi0, gdest = _batch_call(s, B, gp, gd, pi0, bool(flags), gn_all if with_next else None, True, True)
            _planted_zeros(Z, Tc, B, grad, gpi0, gdest)
            for b in range(B):
                gn = gn_all[:, b] if with_next else None
                args = (pd[:, :, b], p_dest, gp[:, :, b], gd[:, :, b], pi0, flags, gn, tables)
                egrad, epi0, bg, bp = G.exact_with_bounds(*args)
                edest, bd, _, _ = D.exact_adjoint_dest(args[0], p_dest, dP, *args[2:])
                for name, g, e, bound in (("grad_p_drive", grad[:, :, b], egrad, bg), ("grad_pi0", gpi0[:, b], epi0, bp),
                                          ("grad_dest", gdest[:, :, b], edest, bd)):
                    w, z = G.worst_ratio(g, e, bound)
                    print(f"Z={Z} B={B} fleet {b} flags={flags} pi0={kind} g_next={with_next}: {name} worst error / bound {w:.4f}")
                    assert z, "a word whose magnitude is 0 is not 0"
                    assert w <= 1.0, name


@gpu
@pytest.mark.parametrize("Z", [129, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc, B = TC, 9
    p_dest, tables = _dest_tables(Z, Tc)
    pd = _fleet_tables(Z, Tc, B, 2)
    gp, gd, gn_all = _fleet_cotangents(Z, Tc, B, 2)
    dP = _tangent(p_dest, tables, Z)
    with _sampler(cpm, Z, Tc, pd[:, :, 0], p_dest) as s:
        s.set_p_dest_tangent(dP)
        s.set_p_drive_batch(pd)
        for flags, kind, with_next in ((0, "uniform", False), (R.IVP, "given", True)):
            pi0 = _pi0(Z, kind)
            grad, gpi0, gdest = _batch_call(s, B, gp, gd, pi0, bool(flags), gn_all if with_next else None, True, True)
            _planted_zeros(Z, Tc, B, grad, gpi0, gdest)
            worst = {}
            for b in range(B):
                gn = gn_all[:, b] if with_next else None
                args = (gp[:, :, b], gd[:, :, b], pi0, flags, gn, tables)
                ndest, ngrad, npi0 = D.numpy_adjoint_dest(pd[:, :, b], p_dest, dP, *args)
                bd = D.numpy_adjoint_dest(pd[:, :, b], p_dest, dP, *args, bound_factor=2.0)[0]
                bg, bp = G.numpy_adjoint(pd[:, :, b], p_dest, *args, bound_factor=2.0)
                for name, g, want, tol in (("grad_p_drive", grad[:, :, b], ngrad, bg), ("grad_pi0", gpi0[:, b], npi0, bp),
                                           ("grad_dest", gdest[:, :, b], ndest, bd)):
                    assert np.all(g[tol == 0.0] == 0.0), (name, b)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ratio = np.where(tol != 0.0, np.abs(g - want) / tol, 0.0)
                    worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
                    assert np.all(np.isfinite(g)) and ratio.max() <= 1.0, (name, b)
            print(f"Z={Z} B={B} flags={flags}: worst error / (2 x bound) over the fleets: "
                  + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ 3: the device entries
@gpu
def test_same_bits_every_time_and_in_either_order_of_batch_sizes(cpm):
    """B = 9 after B = 3 on one context and the reverse: the workspace grows once and is laid out for the batch at hand"""
    Z, Tc = 129, TC
    p_dest, tables = _dest_tables(Z, Tc)
    dP = _tangent(p_dest, tables, 4)
    case = {B: (_fleet_tables(Z, Tc, B, 3), _fleet_cotangents(Z, Tc, B, 3)) for B in (3, 9)}
    seen = {}
    for order in ((3, 9, 3), (9, 3, 9)):
        with _sampler(cpm, Z, Tc, case[3][0][:, :, 0], p_dest) as s:
            s.set_p_dest_tangent(dP)
            for B in order:
                pd, (gp, gd, gn) = case[B]
                s.set_p_drive_batch(pd)
                for dest in (False, True):
                    for _ in range(2):
                        got = _batch_call(s, B, gp, gd, _pi0(Z, "given"), True, gn, True, dest)
                        first = seen.setdefault((B, dest), got)
                        assert all(a is None or _same(a, b) for a, b in zip(got, first)), (order, B, dest)
                blocking = s.expected_grad_batch(gp, gd, _pi0(Z, "given"), ivp=True, g_next=gn, dest=True)
                for key, a in zip(("grad_p_drive", "grad_pi0", "grad_dest"), seen[(B, True)]):
                    assert blocking[key].shape == a.shape and _same(blocking[key], a), key
                plain = s.expected_grad_batch(gp, gd, _pi0(Z, "given"), ivp=True, g_next=gn)
                assert set(plain) == {"grad_p_drive", "grad_pi0"} and _same(plain["grad_p_drive"], seen[(B, False)][0])
    assert np.any(seen[(9, True)][2][:, :, 0] != 0.0)


@gpu
def test_the_call_leaves_no_trace(cpm):
    import torch
    Z, Tc, cpz, B = 67, 24, 50, 5
    C = Z * cpz
    p_dest, tables = _dest_tables(Z, Tc)
    own = np.nan_to_num(_tables(Z, Tc)[0])
    pd = _fleet_tables(Z, Tc, B, 4)
    gp, gd, gn = _fleet_cotangents(Z, Tc, B, 4)
    g1 = G.signed_cotangents(Z, Tc, 4)
    with _sampler(cpm, Z, Tc, own, p_dest) as s:
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        s.set_p_dest_tangent(_tangent(p_dest, tables, 9))
        s.set_p_drive_batch(pd)

        def snapshot():
            out = torch.empty(B * s.expected_words(), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            s.expected_batch_dev(out.data_ptr(), 0, True)
            s.sync()
            return (out.cpu().numpy(),) + _single(s, g1[0], g1[1], _pi0(Z, "given"), True, g1[2]) + s.expected(want_next=True)

        before, step, snap = s.resample(SEED), s.last_step(), snapshot()
        for dest in (False, True):
            _batch_call(s, B, gp, gd, None, False, None, True, dest)
            _batch_call(s, B, gp, gd, _pi0(Z, "given"), True, gn, True, dest)
            s.expected_grad_batch(gp, gd, ivp=True, g_next=gn, dest=dest)
        assert s.last_step() == step
        for x, y in zip(snap, snapshot()):
            assert _same(x, y)
        assert _same(s.get_p_drive_batch(), pd) and _same(s.get_p_drive(), own)
        after = s.resample(SEED)
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step


# ------------------------------------------------------------------------------------------------ 4: errors
@gpu
def test_errors_leave_the_outputs_untouched(cpm, O):
    import torch
    Z, Tc, B = 24, TC, 3
    p_dest, tables = _dest_tables(Z, Tc)
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    pd = _fleet_tables(Z, Tc, B, 5)
    gp, gd, gn = _fleet_cotangents(Z, Tc, B, 5)
    gp[:, :, B - 1] = 0.25                                             # (every fleet's cotangent is finite and non-zero here)
    dP = _tangent(p_dest, tables, 1)
    cot = torch.zeros(B * 2 * Tc * Z, dtype=torch.float64, device="cuda")
    dev = [torch.full((B * Z * Tc,), SENT, dtype=torch.int64, device="cuda") for _ in range(3)]
    host = [np.full(B * Z * Tc, SENT, dtype=np.int64) for _ in range(3)]
    torch.cuda.synchronize()
    dp = [a.data_ptr() for a in dev]
    hp = [a.ctypes.data for a in host]
    vp = lambda v: v.ctypes.data

    def untouched():
        torch.cuda.synchronize()
        return all(bool((a == SENT).all()) for a in dev) and all(np.all(a == SENT) for a in host)

    with cpm.Sampler(Z, Tc) as s:
        L, h = s._L, s._h
        last = lambda: L.cpm_last_error().decode()
        calls = {
            "batch_dev": lambda flags=0, c=cot.data_ptr(), g=dp[0]: L.cpm_expected_grad_batch_dev(h, None, flags, c, None, g, dp[1]),
            "batch": lambda flags=0, a=vp(gp), b=vp(gd), g=hp[0]: L.cpm_expected_grad_batch(h, None, flags, a, b, vp(gn), g, hp[1]),
            "dest_dev": lambda flags=0, c=cot.data_ptr(), g=dp[0], d=dp[2]: L.cpm_expected_grad_dest_batch_dev(h, None, flags, c, None, g, dp[1], d),
            "dest": lambda flags=0, a=vp(gp), b=vp(gd), g=hp[0], d=hp[2]: L.cpm_expected_grad_dest_batch(h, None, flags, a, b, vp(gn), g, hp[1], d),
        }
        s.set_p_drive(pd[:, :, 0])
        s.set_p_dest(p_dest)
        s.set_p_dest_tangent(dP)
        for name, call in calls.items():                               # no batch tables
            assert call() == ERR_STATE and "no batch tables" in last(), name
        assert untouched()
        s.set_p_dest(p_dest)                                           # (drops the tangent)
        s.set_p_drive_batch(pd)
        for name in ("dest_dev", "dest"):                              # no tangent
            assert calls[name]() == ERR_STATE and "tangent" in last(), name
        assert untouched()
        s.set_datamatrix(dm, dist)
        s.build_p_dest(2, want=False)
        s.build_p_dest_tangent()
        assert calls["dest"]() == 0
        assert not np.any(host[0] == SENT) and not np.any(host[2] == SENT) and not np.any(host[1][:B * Z] == SENT)
        for a in host:
            a[:] = SENT
        s.build_p_dest(1.7, want=False)                                # a new table: the tangent went with the old one
        for name in ("dest_dev", "dest"):
            assert calls[name]() == ERR_STATE and "tangent" in last(), name
        assert untouched()
        s.build_p_dest_tangent()
        for name, call in calls.items():
            for flags in (2, 0x80000001):                              # unknown flag bits
                assert call(flags) == ERR_ARG and "flag" in last(), name
        # NULL cotangents and outputs
        assert calls["batch_dev"](c=None) == ERR_ARG and calls["batch_dev"](g=None) == ERR_ARG
        assert calls["dest_dev"](c=None) == ERR_ARG and calls["dest_dev"](g=None) == ERR_ARG and calls["dest_dev"](d=None) == ERR_ARG
        assert calls["batch"](a=None) == ERR_ARG and calls["batch"](b=None) == ERR_ARG and calls["batch"](g=None) == ERR_ARG
        assert calls["dest"](a=None) == ERR_ARG and calls["dest"](g=None) == ERR_ARG and calls["dest"](d=None) == ERR_ARG
        assert untouched()
        # a cotangent word of fleet 2 that is not finite, in the blocking forms
        for value in (np.nan, np.inf):
            bad = np.array(gd, order="F")
            bad[4, 1, 1] = value
            for name in ("batch", "dest"):
                assert calls[name](b=vp(bad)) == ERR_ARG, name
                assert "fleet 2, zone 5, hour 2" in last(), last()
            with pytest.raises(cpm.CpmError) as e:
                s.expected_grad_batch(gp, bad, dest=True)
            assert e.value.status == ERR_ARG and "fleet 2" in str(e.value)
        badn = np.array(gn, order="F")
        badn[6, 1] = np.nan
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad_batch(gp, gd, g_next=badn)
        assert e.value.status == ERR_ARG and "fleet 2, zone 7" in str(e.value)
        assert untouched()
        with pytest.raises(ValueError):
            s.expected_grad_batch(gp[:, :, :2], gd[:, :, :2])          # cotangents for another number of fleets
        assert np.all(np.isfinite(s.expected_grad_batch(gp, gd, g_next=gn, dest=True)["grad_dest"]))


# ------------------------------------------------------------------------------------------------ 5: end to end
@gpu
def test_evaluator_batch_gives_the_dicts_of_expected_gradient_bit_for_bit(cpm, O):
    from carparkingmaps_amd import model_selection as ms
    Z, Tc = 24, 24
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    rng = np.random.default_rng(5)
    m_act, m_park = rng.uniform(0, 1, Tc), rng.uniform(0, 1, (Z, Tc))
    pts = [ms.Point(0.6, 0.15, 0.8, 1.7), ms.Point(0.5, 0.1, 0.9, 1.7), ms.Point(1.3, 0.0, 1.0, 1.7), ms.Point(0.25, 0.2, 0.7, 1.7)]
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        ev = ms.Evaluator(s, C=1, seed=SEED, measured_activity=m_act, measured_parking=m_park)
        for ob in ("activity_error", "parking_error", "A_drive"):
            for dest in (True, False):
                batch = ev.expected_gradient_batch(pts, ob, dest=dest)
                assert len(batch) == len(pts)
                for pt, got in zip(pts, batch):
                    want = ev.expected_gradient(pt, ob, dest=dest)
                    assert set(got) == set(want) and (("d_e_dest" in got) == dest)
                    for k in want:
                        if k == "objective":
                            assert got[k] == want[k] == ob
                        else:
                            a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
                            assert a.shape == b.shape and _same(a, b), (ob, dest, k)
                assert np.any(batch[0]["grad_p_drive"] != 0.0)
        with pytest.raises(ValueError):
            ev.expected_gradient_batch(pts[:2] + [ms.Point(0.5, 0.1, 0.9, 2)], "A_drive")
