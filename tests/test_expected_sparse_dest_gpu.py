"""The e_dest direction from a compact tangent of p_destin (include/cpm_expected_sparse_dest.h) on the GPU.  Every comparison is
array_equal on int64 views against the dense call of a second, fresh context with the same tables and the same tangent: the contract
is bit equality.  Every context that relies on sparse tables asserts CPM_INFO_SPARSE_TABLES > 0 when it is made.

Upload route (CPM_OPT_SPARSE_UPLOAD, T = 3): the hand-made tables of expected_sparse_reference at Z = 403, 518, 1,031 and 1,089 (the
last segment EMPTY), and the walk tables of expected_sparse_dest_reference at Z = 1,031, whose rows hold 0, 1, 63, 64, 65, 255, 256, 257 and 309
cells, all cells in one segment, and a cell in every segment.  Dataset route: Z = 358 (and 403, 518 for the builder), T = 24.
Tables of Z = 2 and Z <= 65 never get compact rows (a row pack must be worth it: include/cpm.h), so at those sizes the sparse calls'
contract is the refusal, which is what the cases there assert -- whichever way the library decides, the case holds it to the contract
of the route it took."""
import ctypes
import functools

import numpy as np
import pytest

import expected_grad_dest_reference as D
import expected_grad_reference as G
import expected_reference as R
import expected_sparse_dest_reference as SD
import expected_sparse_reference as S
from test_expected_fit_gpu import FLEETS, _measured
from test_expected_sparse_grad_gpu import (ERR_ARG, ERR_STATE, ERR_TABLE, GUARD, SEED, TU, _body, _cots, _dataset, _datamatrix, _dev, _fleet_tables,
                                           _from_dataset, _grad_dev, _guarded, _ptr, _same, _upload)

gpu = pytest.mark.gpu
FIT_DEST = 0x100


def _info(s, cpm):
    from carparkingmaps_amd import _lib
    return s.get_info(cpm.CPM_INFO_P_DENSE), s.get_info(_lib.CPM_INFO_DEST_TANGENT_DENSE), s.get_info(_lib.CPM_INFO_DEST_TANGENT_COMPACT)


@functools.lru_cache(maxsize=None)
def _tangent(Z, walk=False, seed=1, density=None):
    """a signed tangent on the stored cells (p != 0) of the uploaded tables, rows summing to 0, +0 elsewhere: (Z, Z, T) F-order"""
    p = SD.walk_tables(Z, TU)[1] if walk else S.sparse_tables(Z, TU, density=density)[1]
    dP = np.zeros(p.shape, order="F")
    for t in range(TU):
        dP[:, :, t] = SD.signed_tangent_on_cells(np.ascontiguousarray(p[:, :, t]), (), 100 * seed + 7 * Z + t)[0]
    assert (dP < 0).any() and (dP > 0).any() and not dP[p == 0.0].any()
    dP.setflags(write=False)
    return dP


def _pair(cpm, Z, walk=False, dm=False, negative=False):
    """(sparse context with the compact tangent, fresh dense twin with the dense tangent): the same uploaded tables in both"""
    p = SD.walk_tables(Z, TU)[1] if walk else None
    dP = _tangent(Z, walk)
    s, d = _upload(cpm, Z, dm=dm, negative=negative, p_dest=p), _upload(cpm, Z, dm=dm, negative=negative, p_dest=p)
    s.set_p_dest_tangent(dP, sparse=True)
    d.set_p_dest_tangent(dP)
    assert _info(s, cpm)[1:] == (0, 1) and _info(d, cpm)[1:] == (1, 0)
    return s, d


def _gdest_dev(s, cot, pi0, ivp, gn, sparse, want_pi0=True, B=0):
    """expected_grad_dest[_batch]_dev between guard words -> int64 (grad [B][T][Z], grad_pi0 [B][Z], grad_dest [B][T][Z])"""
    import torch
    nb = max(B, 1)
    d_cot, d_pi0, d_gn = _dev(cot), _dev(pi0), _dev(gn)
    grad, gpi0, gdest = _guarded(nb * s.Z * s.T), _guarded(nb * s.Z), _guarded(nb * s.Z * s.T)
    torch.cuda.synchronize()
    call = s.expected_grad_dest_batch_dev if B else s.expected_grad_dest_dev
    call(d_cot.data_ptr(), grad.data_ptr() + 8 * GUARD, gdest.data_ptr() + 8 * GUARD, _ptr(d_pi0), ivp, _ptr(d_gn),
         gpi0.data_ptr() + 8 * GUARD if want_pi0 else 0, sparse=sparse)
    s.sync()
    return _body(grad).reshape(nb, s.T, s.Z), _body(gpi0, want_pi0).reshape(nb, s.Z), _body(gdest).reshape(nb, s.T, s.Z)


def _all_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1: the builder
def _ds_context(cpm, Z, e_dest=2):
    dm, dist = _dataset(Z, 24)
    s = cpm.Sampler(Z, 24)
    s.set_datamatrix(dm, dist)
    s.build_p_drive(0.1, 0.9, 0.5, want=False)
    s.build_p_dest(e_dest, want=False)
    assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0, "the table fell back to dense packs"
    return s


@gpu
@pytest.mark.parametrize("Z", [403, 518])
def test_builder_gives_the_bits_of_the_dense_builder_on_the_dataset_route(cpm, Z):
    with _ds_context(cpm, Z, 1.7) as s, _ds_context(cpm, Z, 1.7) as d:
        assert _info(s, cpm) == (0, 0, 0)
        s.build_p_dest_tangent(sparse=True)
        assert _info(s, cpm) == (0, 0, 1)
        got = s.get_p_dest_tangent(sparse=True)
        want = d.build_p_dest_tangent(want=True)
        assert _same(got, want) and got.any() and np.isfinite(got).all()
        assert not np.signbit(got[got == 0.0]).any()                       # +0.0 at p == 0 and off the stored cells
        assert _same(s.build_p_dest_tangent(want=True, sparse=True), want)  # the same bits a second time
        assert _info(s, cpm) == (0, 0, 1) and _info(d, cpm)[1:] == (1, 0)
        with pytest.raises(cpm.CpmError) as e:                             # the dense calls do not see the compact tangent
            s.get_p_dest_tangent()
        assert e.value.status == ERR_STATE
        s.build_p_dest(1.7, want=False)                                    # any install of tables drops it
        assert _info(s, cpm) == (0, 0, 0)
        with pytest.raises(cpm.CpmError) as e:
            s.get_p_dest_tangent(sparse=True)
        assert e.value.status == ERR_STATE and "cpm_build_p_dest_tangent_sparse" in str(e.value)
        s.build_p_dest_tangent(sparse=True)
        dm, dist = _dataset(Z, 24)
        s.set_datamatrix(dm, dist)                                         # a new datamatrix drops it, and the builder's precondition
        assert _info(s, cpm)[2] == 0
        with pytest.raises(cpm.CpmError) as e:
            s.build_p_dest_tangent(sparse=True)
        assert e.value.status == ERR_STATE
        s.build_p_dest(0, want=False)                                      # e_dest = 0: no tangent, as the dense builder
        with pytest.raises(cpm.CpmError) as e:
            s.build_p_dest_tangent(sparse=True)
        assert e.value.status == ERR_STATE and "e_dest" in str(e.value)
    with _upload(cpm, 403, dm=True) as s:                                  # uploaded tables: nothing to differentiate
        with pytest.raises(cpm.CpmError) as e:
            s.build_p_dest_tangent(sparse=True)
        assert e.value.status == ERR_STATE and _info(s, cpm)[1:] == (0, 0)


# ------------------------------------------------------------------------------------------------ 2: the setter
@gpu
def test_setter_round_trip_and_its_refusals(cpm):
    Z = 1031
    dP, other = _tangent(Z, True), _tangent(Z, True, seed=2)
    p = SD.walk_tables(Z, TU)[1]
    with _upload(cpm, Z, p_dest=p) as s:
        s.set_p_dest_tangent(dP, sparse=True)
        assert _same(s.get_p_dest_tangent(sparse=True), dP) and _info(s, cpm) == (1, 0, 1)
        bad = np.array(other, order="F")
        o, d, t = 5, int(np.nonzero(p[5, :, 1] == 0.0)[0][3]), 1
        bad[o, d, t] = -0.5                                                # one non-zero entry off the stored cells
        with pytest.raises(cpm.CpmError) as e:
            s.set_p_dest_tangent(bad, sparse=True)
        text = str(e.value)
        assert e.value.status == ERR_TABLE and f"hour {t + 1}, origin {o + 1}, destination {d + 1}" in text
        assert _same(s.get_p_dest_tangent(sparse=True), dP)                # the previous tangent is still installed
        bad = np.array(other, order="F")
        bad[7, 3, 2] = np.nan
        with pytest.raises(cpm.CpmError) as e:
            s.set_p_dest_tangent(bad, sparse=True)
        assert e.value.status == ERR_ARG and "finite" in str(e.value)
        assert _same(s.get_p_dest_tangent(sparse=True), dP)
        minus = np.array(other, order="F")
        minus[o, d, t] = -0.0                                              # -0.0 is zero
        s.set_p_dest_tangent(minus, sparse=True)
        assert _same(s.get_p_dest_tangent(sparse=True), other)
        s.set_p_dest(p)
        assert _info(s, cpm)[2] == 0


# ------------------------------------------------------------------------------------------------ 3: grad_dest, single call
def _single_cases(s, d, cpm):
    Z, Tc = s.Z, s.T
    cot, gn = _cots(Z, Tc, 1, Z)
    for ivp in (False, True):
        for pi0 in (None, S.pi0_with_zeros(Z)):
            for with_next in (False, True):
                for want_pi0 in (True, False):
                    g = gn if with_next else None
                    got = _gdest_dev(s, cot, pi0, ivp, g, True, want_pi0)
                    want = _gdest_dev(d, cot, pi0, ivp, g, False, want_pi0)
                    assert _all_equal(got, want), (Z, ivp, pi0 is None, with_next, want_pi0)
                    plain = _grad_dev(s, cot, pi0, ivp, g, True, want_pi0)         # cpm_expected_sparse_grad's bits
                    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])
        again = _gdest_dev(s, cot, None, ivp, gn, True)
        assert _all_equal(again, _gdest_dev(s, cot, None, ivp, gn, True)), "the same bits on a second call"
        assert again[2].view(np.float64).any() and np.isfinite(again[2].view(np.float64)).all()
        zero = _gdest_dev(s, np.zeros_like(cot), None, ivp, None, True)
        assert not zero[0].any() and not zero[1].any() and not zero[2].any()       # a zero cotangent: exact +0 everywhere
    return again


@gpu
@pytest.mark.parametrize("Z", [403, 518, 1031, 1089])
def test_single_grad_dest_gives_the_bits_of_the_dense_call_on_the_upload_route(cpm, Z):
    s, d = _pair(cpm, Z)
    with s, d:
        got = _single_cases(s, d, cpm)
        zero_rows = S.sparse_tables(Z, TU)[2]["zero"]
        assert not got[2][0][:TU - 1, zero_rows].any()                     # zero rows: exactly +0
        assert _info(s, cpm) == (1, 0, 1)                                  # (the uploaded array stays resident; no dense tangent)


@gpu
def test_rows_of_every_walk_length_give_the_bits_of_the_dense_call(cpm):
    Z = 1031                                                               # (rows of 309 cells keep their sparse packs at this size)
    p = SD.walk_tables(Z, TU)[1]
    counts = np.count_nonzero(p, axis=1)
    assert [int(counts[o, 0]) for o in SD.WALK_ROWS] == list(SD.WALK_ROWS.values())
    nseg = G.segments(Z)[0]
    seg_of = lambda o: {int(dd) // G.segments(Z)[1] for dd in np.nonzero(p[o, :, 0])[0]}
    assert len(seg_of(SD.WALK_ONE_SEGMENT)) == 1 and len(seg_of(SD.WALK_EVERY_SEGMENT)) == nseg
    s, d = _pair(cpm, Z, walk=True)
    with s, d:
        cot, gn = _cots(Z, TU, 9, 41)
        pi0 = S.pi0_with_zeros(Z)
        pi0[:11] = np.arange(1, 12) / 7.0                                  # the walk rows carry mass
        for ivp, g in ((False, gn[:1]), (True, None), (True, gn[:1])):
            got, want = _gdest_dev(s, cot[:1], pi0, ivp, g, True), _gdest_dev(d, cot[:1], pi0, ivp, g, False)
            assert _all_equal(got, want), (Z, ivp)
        gd = got[2][0].view(np.float64)
        assert not gd[:, 0].any() and gd[:, 2:11].any(axis=0).all()        # the empty row: +0; every other walk row takes part
        for B in (2, 3, 9):
            fleets = _fleet_tables(Z, TU, B)
            for c in (s, d):
                c.set_p_drive_batch(fleets)
            got, want = _gdest_dev(s, cot[:B], pi0, True, gn[:B], True, B=B), _gdest_dev(d, cot[:B], pi0, True, gn[:B], False, B=B)
            assert _all_equal(got, want), (Z, B)


@gpu
def test_single_grad_dest_on_the_dataset_route(cpm):
    with _from_dataset(cpm, 1.7) as s, _from_dataset(cpm, 1.7) as d:
        s.build_p_dest_tangent(sparse=True)
        d.build_p_dest_tangent()
        _single_cases(s, d, cpm)
        assert _info(s, cpm) == (0, 0, 1) and _info(d, cpm) == (1, 1, 0)


@gpu
@pytest.mark.parametrize("Z", [2, 65])
def test_small_tables_hold_the_contract_of_the_route_they_take(cpm, Z):
    """Z = 2 and Z <= 65: where the library gives such a table compact rows, grad_dest is held to the bound of
    include/cpm_expected_grad_dest.h against the exact (rational) reference and to the dense call's bits; where it does not, every
    sparse call is refused with CPM_ERR_STATE and the two routes named, before anything is written."""
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    dP = np.where(np.asarray(p_dest) != 0.0, D.signed_tangent(p_dest, 5 * Z), 0.0)
    gp, gd, gn = G.signed_cotangents(Z, TU, 7 * Z + TU, "random")
    with cpm.Sampler(Z, TU) as s:
        s.set_sparse_upload(True)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        if s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0:
            s.set_p_dest_tangent(dP, sparse=True)
            got = s.expected_grad_dest(gp, gd, ivp=True, g_next=gn, sparse=True)
            exact, bound, _, _ = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, R.IVP, gn)
            w, z = G.worst_ratio(got["grad_dest"], exact, bound)
            print(f"Z={Z}: grad_dest worst error / bound {w:.4f}")
            assert z and w <= 1.0
            s.set_p_dest_tangent(dP)
            want = s.expected_grad_dest(gp, gd, ivp=True, g_next=gn)
            assert all(_same(got[k], want[k]) for k in got)
        else:
            for call in (lambda: s.set_p_dest_tangent(dP, sparse=True), lambda: s.get_p_dest_tangent(sparse=True),
                         lambda: s.expected_grad_dest(gp, gd, sparse=True), lambda: s.build_p_dest_tangent(sparse=True)):
                with pytest.raises(cpm.CpmError) as e:
                    call()
                assert e.value.status == ERR_STATE
            assert "CPM_OPT_SPARSE_UPLOAD" in str(e.value) or "cpm_build_p_dest" in str(e.value)
            s.set_p_dest_tangent(dP)                                       # the dense route meets the bound at this size
            got = s.expected_grad_dest(gp, gd, ivp=True, g_next=gn)
            exact, bound, _, _ = D.exact_adjoint_dest(p_drive, p_dest, dP, gp, gd, None, R.IVP, gn)
            w, z = G.worst_ratio(got["grad_dest"], exact, bound)
            assert z and w <= 1.0


@gpu
def test_sparse_grad_dest_meets_twice_the_bound_against_the_numpy_form(cpm):
    """independently of any kernel here, at the smallest size that has compact rows: the numpy form of
    tests/expected_grad_dest_reference.py, held to twice the header's bound as tests/test_expected_grad_dest_gpu.py holds the dense call"""
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    dP = _tangent(Z)
    tables = R.row_tables(p_dest)
    with _upload(cpm, Z) as s:
        s.set_p_dest_tangent(dP, sparse=True)
        for flags, pi0, with_next in ((0, None, False), (R.IVP, S.pi0_with_zeros(Z) / S.pi0_with_zeros(Z).sum(), True)):
            gp, gd, gn = G.signed_cotangents(Z, TU, 7 * Z + TU, "random")
            gn = gn if with_next else None
            got = s.expected_grad_dest(gp, gd, pi0, ivp=bool(flags), g_next=gn, sparse=True)["grad_dest"]
            want, _, _ = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables)
            tol, _, _ = D.numpy_adjoint_dest(p_drive, p_dest, dP, gp, gd, pi0, flags, gn, tables, bound_factor=2.0)
            assert np.all(got[tol == 0.0] == 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(tol != 0.0, np.abs(got - want) / tol, 0.0)
            print(f"Z={Z} flags={flags}: grad_dest worst error / (2 x bound) {ratio.max():.4f}")
            assert np.all(np.isfinite(got)) and ratio.max() <= 1.0 and got.any()


# ------------------------------------------------------------------------------------------------ 4: batch
@gpu
@pytest.mark.parametrize("B", [1, 2, 7, 8, 9, 17])
def test_batched_grad_dest_against_the_dense_batch_and_the_single_sparse_call(cpm, B):
    Z = 403
    fleets = _fleet_tables(Z, TU, B)
    cot, gn = _cots(Z, TU, B, 200 + B)
    pi0 = S.pi0_with_zeros(Z)
    s, d = _pair(cpm, Z)
    with s, d:
        for c in (s, d):
            c.set_p_drive_batch(fleets)
        for ivp, g in ((False, gn), (True, None)):
            got = _gdest_dev(s, cot, pi0, ivp, g, True, B=B)
            want = _gdest_dev(d, cot, pi0, ivp, g, False, B=B)
            assert _all_equal(got, want), (B, ivp)
            for b in sorted({0, B // 2, B - 1}):
                s.set_p_drive(fleets[:, :, b])
                one = _gdest_dev(s, cot[b:b + 1], pi0, ivp, None if g is None else g[b:b + 1], True)
                assert all(np.array_equal(one[k][0], got[k][b]) for k in range(3)), (B, b, ivp)
        assert got[2].view(np.float64).any()
        a = s.expected_grad_batch(np.asfortranarray(cot[:, 0].transpose(2, 1, 0)), np.asfortranarray(cot[:, 1].transpose(2, 1, 0)), pi0, True,
                                  gn.T, dest=True, sparse=True, compact_tangent=True)
        b_ = d.expected_grad_batch(np.asfortranarray(cot[:, 0].transpose(2, 1, 0)), np.asfortranarray(cot[:, 1].transpose(2, 1, 0)), pi0, True,
                                   gn.T, dest=True)
        assert a.keys() == b_.keys() and all(_same(a[k], b_[k]) for k in a)


# ------------------------------------------------------------------------------------------------ 5: trip tangent
def _trip_tan_dev(s, sparse):
    import torch
    w = _guarded(2 * s.Z * s.T)
    torch.cuda.synchronize()
    s.expected_trip_tangent_dev(w.data_ptr() + 8 * GUARD, sparse=sparse)
    s.sync()
    return _body(w)


@gpu
@pytest.mark.parametrize("Z", [403, 1089])
def test_trip_tangent_gives_the_bits_of_the_dense_call(cpm, Z):
    dm, _ = _datamatrix(Z, TU, True)
    assert (dm[..., 0] < 0).any()                                          # a negative mean
    s, d = _pair(cpm, Z, dm=True, negative=True)
    with s, d:
        got = _trip_tan_dev(s, True)
        assert np.array_equal(got, _trip_tan_dev(d, False)) and got.view(np.float64).any() and np.isfinite(got.view(np.float64)).all()
        a, b = s.expected_trip_tangent(sparse=True), d.expected_trip_tangent()
        assert _same(a[0], b[0]) and _same(a[1], b[1])
        assert s.expected_trip_builds() == 0 and _info(s, cpm) == (1, 0, 1)
    with _upload(cpm, Z, dm=True, dist=False) as s:
        s.set_p_dest_tangent(_tangent(Z), sparse=True)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_trip_tangent(sparse=True)
        assert e.value.status == ERR_STATE and "distance matrix" in str(e.value)


# ------------------------------------------------------------------------------------------------ 6: fit
def _fit_dest_dev(s, fleets, ivp, sparse):
    import torch
    Z, Tc, B = s.Z, s.T, len(fleets)
    sizes = dict(record=B * s.fit_words(), expected=B * 2 * Tc * Z, cotangent=B * 2 * Tc * Z, grad_p_drive=B * Tc * Z, grad_dest=B * Tc * Z)
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    at = lambda k: bufs[k].data_ptr() + 8 * GUARD
    torch.cuda.synchronize()
    s.expected_fit_dev([f[0] for f in fleets], [f[1] for f in fleets], [f[2] for f in fleets], np.array([f[3] for f in fleets]), at("record"), 0,
                       ivp, True, at("expected"), at("cotangent"), at("grad_p_drive"), at("grad_dest"), sparse=sparse, compact_tangent=sparse)
    s.sync()
    return {k: _body(b) for k, b in bufs.items()}


@gpu
@pytest.mark.parametrize("route", ["dataset", "upload"])
def test_fit_with_dest_gives_the_bits_of_the_dense_fit(cpm, route):
    if route == "dataset":
        s, d = _from_dataset(cpm, 1.7), _from_dataset(cpm, 1.7)
        s.build_p_dest_tangent(sparse=True)
        d.build_p_dest_tangent()
    else:
        s, d = _pair(cpm, 403, dm=True)
        m_act, m_park = _measured(403, TU)
        for c in (s, d):
            c.set_measured_activity(m_act)
            c.set_measured(m_park)
    single = [(0.10, 0.90, 0.5, w) for w in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.7, 1.3, 2.1))]    # every objective weighed in turn
    with s, d:
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        for ivp in (False, True):
            for fleets in [[f] for f in single] + [FLEETS]:                # B = 1 and B = 9
                got, want = _fit_dest_dev(s, fleets, ivp, True), _fit_dest_dev(d, fleets, ivp, False)
                for k in got:
                    assert np.array_equal(got[k], want[k]), (route, ivp, len(fleets), fleets[0][3], k)
                rec = got["record"].view(np.float64).reshape(len(fleets), -1)
                assert np.isfinite(rec[:, 8]).all()                        # dF / d e_dest is there
        assert len(FLEETS) == 9
        args = ([f[0] for f in FLEETS], [f[1] for f in FLEETS], [f[2] for f in FLEETS], np.array([f[3] for f in FLEETS]))
        a = s.expected_fit(*args, dest=True, want=("expected", "cotangent", "grad_p_drive", "grad_dest"), sparse=True, compact_tangent=True)
        b = d.expected_fit(*args, dest=True, want=("expected", "cotangent", "grad_p_drive", "grad_dest"))
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
        assert _info(s, cpm) == ((0 if route == "dataset" else 1), 0, 1)
        # grad_dest without the flag stays CPM_ERR_ARG; without a compact tangent the flag is refused as before, the record untouched
        one = np.array([0.1]), np.array([0.9]), np.array([0.5]), np.array([1.0, 0.0, 0.0])
        rec, gd = np.zeros(s.fit_words()), np.zeros(s.Z * s.T)
        L, h = s._L, s._h
        assert L.cpm_expected_sparse_fit(h, 1, vp(one[0]), vp(one[1]), vp(one[2]), None, 0, vp(one[3]), vp(rec), None, None, None, vp(gd)) == ERR_ARG
        assert not rec.any()
        s.set_p_dest(S.sparse_tables(403, TU)[1]) if route == "upload" else s.build_p_dest(1.7, want=False)     # drops the tangent
        assert _info(s, cpm)[2] == 0
        rc = L.cpm_expected_sparse_fit(h, 1, vp(one[0]), vp(one[1]), vp(one[2]), None, FIT_DEST, vp(one[3]), vp(rec), None, None, None, None)
        text = L.cpm_last_error()
        assert rc == ERR_ARG and b"dense" in text and b"tangent" in text and not rec.any()
        assert b"cpm_build_p_dest_tangent_sparse" in text and b"cpm_set_p_dest_tangent_sparse" in text


# ------------------------------------------------------------------------------------------------ 7: residency
@gpu
def test_a_four_parameter_fit_on_the_dataset_route_holds_neither_dense_array(cpm):
    from carparkingmaps_amd import model_selection as M
    cot, gn = _cots(358, 24, 2, 9)
    gp, gd = np.asfortranarray(cot[0, 0].T), np.asfortranarray(cot[0, 1].T)
    gp2, gd2 = np.stack([gp, gp], axis=2), np.stack([gd, gd], axis=2)
    with _from_dataset(cpm, 1.7) as s:
        s.build_p_drive_batch([0.1, 0.2], [0.9, 0.8], [0.5, 1.0])
        steps = [("builder", lambda: s.build_p_dest_tangent(sparse=True)),
                 ("grad_dest", lambda: s.expected_grad_dest(gp, gd, ivp=True, g_next=gn[0], sparse=True)),
                 ("batch", lambda: s.expected_grad_batch(gp2, gd2, ivp=True, dest=True, sparse=True, compact_tangent=True)),
                 ("trip tangent", lambda: s.expected_trip_tangent(sparse=True)),
                 ("fit", lambda: s.expected_fit([0.1, 0.2], [0.9, 0.8], [0.5, 1.0], [1.0, 1.0, 1.0], ivp=True, dest=True, sparse=True,
                                                compact_tangent=True))]
        for name, call in steps:
            assert _info(s, cpm)[:2] == (0, 0), name
            call()
            assert _info(s, cpm)[:2] == (0, 0), f"{name} built a dense array"
        assert s.expected_trip_builds() == 0
    dm, dist = _dataset()
    m_act, m_park = _measured(358, 24)
    pts = [M.Point(0.5, 0.1, 0.9, 1.7), M.Point(0.7, 0.05, 0.8, 1.7)]
    w = {"activity_error": 1.0, "A_drive": 0.5}
    C, cpz = 3580, 10
    with cpm.Sampler(358, 24) as s, cpm.Sampler(358, 24) as fresh:
        for c in (s, fresh):
            c.set_datamatrix(dm, dist)
        ev = M.Evaluator(s, C, SEED, measured_activity=m_act, measured_parking=m_park, expected_sparse=True, expected_sparse_dest=True)
        out = M.refine_expected(ev, pts, w, steps=3, dest=True)
        assert len(out) == 2 and s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        assert _info(s, cpm) == (0, 0, 1), "refine_expected(dest=True) built a dense array"
        ev.expected_gradient(pts[0], "A_drive", dest=True)
        ev.expected_gradient_batch(pts, "A_drive", dest=True)
        assert _info(s, cpm) == (0, 0, 1)
        # a following resample and expected() return what a fresh context returns
        for c in (s, fresh):
            c.build_p_drive(0.1, 0.9, 0.5, want=False)
            c.build_p_dest(1.7, want=False)
            c.init_states(C, cpz)
        a, b = s.resample(SEED), fresh.resample(SEED)
        assert np.array_equal(a["parking"], b["parking"]) and np.array_equal(a["driving"], b["driving"])
        ea, eb = s.expected(ivp=True), fresh.expected(ivp=True)
        assert all(_same(x, y) for x, y in zip(ea, eb))


# ------------------------------------------------------------------------------------------------ 8: Evaluator
@gpu
def test_evaluator_with_a_compact_tangent_gives_the_default_evaluators_bits_and_meets_central_differences(cpm):
    from carparkingmaps_amd import model_selection as M
    dm, dist = _dataset()
    m_act, m_park = _measured(358, 24)
    pt = M.Point(e_drive=0.6, p_min=0.15, p_max=0.8, e_dest=1.5)
    pts = [pt, M.Point(0.7, 0.05, 0.8, 1.5)]
    objectives = ("activity_error", "parking_error", "A_drive")
    w = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}
    res = {}
    for compact in (True, False):
        with cpm.Sampler(358, 24) as s:
            s.set_datamatrix(dm, dist)
            ev = M.Evaluator(s, 3580, SEED, measured_activity=m_act, measured_parking=m_park, expected_sparse=compact, expected_sparse_dest=compact)
            out = [ev.expected_gradient(pt, ob, dest=True) for ob in objectives]
            out += ev.expected_gradient_batch(pts, "A_drive", dest=True)
            out += ev.expected_fit(pts, w, dest=True)
            assert _info(s, cpm) == ((0, 0, 1) if compact else (1, 1, 0))
            res[compact] = out
            if not compact:
                continue
            # d_e_dest against a central difference of evaluate_expected in e_dest, judged by its own truncation error
            base = ev.evaluate_expected(pt)
            on = G.inside(s.get_p_drive())
            arg = lambda r: (r["driving"].sum(axis=0).argmin(), r["driving"].sum(axis=0).argmax(), tuple(r["parking"].argmin(axis=1)),
                             tuple(r["parking"].argmax(axis=1)))
            fd = {ob: {} for ob in objectives}
            for h in (2.0 ** -10, 2.0 ** -11):
                vals = []
                for sgn in (1.0, -1.0):
                    r = ev.evaluate_expected(M.Point(pt.e_drive, pt.p_min, pt.p_max, pt.e_dest + sgn * h))
                    # the point is one where nothing clips and no argmin / argmax hour changes between the steps (at e_dest = 1.7 one
                    # of the 358 zones changes its hour of most parking inside the step)
                    assert np.array_equal(G.inside(s.get_p_drive()), on) and arg(r) == arg(base), h
                    vals.append(r)
                for ob in objectives:
                    fd[ob][h] = (vals[0][ob] - vals[1][ob]) / (2 * h)
            for ob, new in zip(objectives, out[:3]):
                dd, a, b = new["d_e_dest"], fd[ob][2.0 ** -10], fd[ob][2.0 ** -11]
                floor = 2.0 ** -30 * max(abs(new["d_" + name]) for name in ("p_min", "p_max", "e_drive", "e_dest"))
                tol = 4 * abs(a - b) + floor
                print(f"{ob} d/de_dest: adjoint {dd:.12e}, FD(h/2) {b:.12e}, |difference| / tolerance {abs(dd - b) / tol:.4f}")
                assert abs(dd - b) <= tol, ob
    for a, b in zip(res[True], res[False]):
        assert a.keys() == b.keys() and "d_e_dest" in a
        for k in a:
            if isinstance(a[k], str):
                assert a[k] == b[k]
            else:
                assert _same(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), k


# ------------------------------------------------------------------------------------------------ 9: refusals
@gpu
def test_refusals_come_before_anything_is_enqueued(cpm):
    import torch
    Z = 403
    gp, gd, gn = G.signed_cotangents(Z, TU, 3)
    gp2, gd2 = np.asfortranarray(np.stack([gp, gp], axis=2)), np.asfortranarray(np.stack([gd, gd], axis=2))
    dP = _tangent(Z)
    with _upload(cpm, Z, sparse=False, dm=True) as s:                       # dense tables: CPM_ERR_STATE, the two routes named
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        s.set_p_drive_batch(_fleet_tables(Z, TU, 2))
        s.set_p_dest_tangent(dP)
        for call in (lambda: s.set_p_dest_tangent(dP, sparse=True), lambda: s.get_p_dest_tangent(sparse=True),
                     lambda: s.expected_grad_dest(gp, gd, sparse=True), lambda: s.expected_trip_tangent(sparse=True),
                     lambda: s.expected_grad_batch(gp2, gd2, dest=True, sparse=True, compact_tangent=True)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "cpm_build_p_dest" in str(e.value) and "CPM_OPT_SPARSE_UPLOAD" in str(e.value)
        s.expected_grad_dest(gp, gd)                                        # (the dense calls are untouched by the refusals)
        assert _info(s, cpm)[1:] == (1, 0)
    with _upload(cpm, Z, dm=True) as s:                                     # compact rows, but no compact tangent
        s.set_p_drive_batch(_fleet_tables(Z, TU, 2))
        s.set_p_dest_tangent(dP)                                            # (a dense tangent does not count)
        for call in (lambda: s.get_p_dest_tangent(sparse=True), lambda: s.expected_grad_dest(gp, gd, sparse=True),
                     lambda: s.expected_trip_tangent(sparse=True),
                     lambda: s.expected_grad_batch(gp2, gd2, dest=True, sparse=True, compact_tangent=True)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "cpm_set_p_dest_tangent_sparse" in str(e.value) and "cpm_build_p_dest_tangent_sparse" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_fit(0.1, 0.9, 0.5, [0.0, 0.0, 1.0], dest=True, sparse=True, compact_tangent=True)
        assert e.value.status == ERR_ARG and "dense" in str(e.value)
        s.set_p_dest_tangent(dP, sparse=True)
        L, h = s._L, s._h
        buf = torch.zeros(4 * Z * TU, dtype=torch.float64, device="cuda")
        p = ctypes.c_void_p(buf.data_ptr())
        assert L.cpm_expected_sparse_grad_dest_dev(h, None, 0, None, None, p, None, p) == ERR_ARG         # NULL cotangent
        assert L.cpm_expected_sparse_grad_dest_dev(h, None, 0, p, None, None, None, p) == ERR_ARG         # NULL outputs
        assert L.cpm_expected_sparse_grad_dest_dev(h, None, 0, p, None, p, None, None) == ERR_ARG
        assert L.cpm_expected_sparse_grad_dest_dev(h, None, 2, p, None, p, None, p) == ERR_ARG            # unknown flag bits
        assert L.cpm_expected_sparse_grad_dest_batch_dev(h, None, 4, p, None, p, None, p) == ERR_ARG
        assert L.cpm_expected_sparse_grad_dest_batch_dev(h, None, 0, p, None, p, None, None) == ERR_ARG
        assert L.cpm_expected_sparse_trip_tangent_dev(h, None) == ERR_ARG
        assert L.cpm_set_p_dest_tangent_sparse(h, None) == ERR_ARG and L.cpm_get_p_dest_tangent_sparse(h, None) == ERR_ARG
        torch.cuda.synchronize()
        assert not buf.cpu().numpy().any()
        bad = np.array(gd)
        bad[3, 1] = np.inf
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad_dest(gp, bad, sparse=True)
        assert e.value.status == ERR_ARG and "finite" in str(e.value)
        assert _same(s.get_p_dest_tangent(sparse=True), dP)
