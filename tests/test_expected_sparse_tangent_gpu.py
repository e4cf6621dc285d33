"""The forward tangent from the compact rows of sparse tables (include/cpm_expected_sparse_tangent.h) on the GPU.  Every comparison is
array_equal on int64 views against the dense call of a second, fresh context with the same tables and the same tangent: the contract
is bit equality.  Every context that relies on sparse tables asserts CPM_INFO_SPARSE_TABLES > 0 when it is made (_upload, _from_dataset).

Upload route (CPM_OPT_SPARSE_UPLOAD, T = 3): the hand-made tables of expected_sparse_reference at Z = 403, 518, 1,031 and 1,089, and
the walk tables of expected_sparse_dest_reference at Z = 1,031 with one column densified to 300 cells beside the column of (nearly)
every origin: columns of one, two and more than two 256-cell chunks of the column walk.  Dataset route: Z = 358, T = 24."""
import ctypes
import functools

import numpy as np
import pytest

import expected_grad_reference as G
import expected_reference as R
import expected_sparse_dest_reference as SD
import expected_sparse_reference as S
import expected_tangent_reference as TG
from test_expected_fit_gpu import _measured
from test_expected_sparse_dest_gpu import _gdest_dev, _info, _pair, _tangent
from test_expected_sparse_grad_gpu import (ERR_ARG, ERR_STATE, ERR_TABLE, GUARD, SEED, SENT, TU, _body, _cots, _dataset, _dev, _from_dataset, _guarded, _ptr,
                                           _same, _upload)

gpu = pytest.mark.gpu
C4 = (0.0, 0.0, 0.0, 1.0)


def _directions(p_drive, K, seed):
    """K signed directions for the device entry: (d p_drive [K][T][Z], d pi_0 [K][Z]), C-order; NaN where p_drive is not strictly inside
    (0, 1) -- dq is exactly 0 there whatever the direction holds; direction 0 moves p_drive alone, direction 1 pi_0 alone"""
    Z, Tc = p_drive.shape
    rng = np.random.default_rng(seed)
    dpd, dpi0 = rng.uniform(-1.0, 1.0, (K, Tc, Z)), rng.uniform(-1.0, 1.0, (K, Z))
    dpi0[0] = 0.0
    if K > 1:
        dpd[1] = 0.0
    off = ~G.inside(np.asarray(p_drive)).T
    assert off.any()
    dpd[:, off] = np.nan
    return dpd, dpi0


class _Call:
    """expected_tangent_dev between guard words, the inputs uploaded once"""

    def __init__(self, dpd, dpi0, pi0=None):
        self.dpd, self.dpi0, self.pi0 = _dev(dpd), _dev(dpi0), _dev(pi0)

    def __call__(self, s, K, c, ivp, sparse, k0=0, want_next=True, want_primal=True):
        import torch
        Z, Tc = s.Z, s.T
        out, nxt, prim = _guarded(K * 2 * Z * Tc), _guarded(K * Z), _guarded(2 * Z * Tc)
        at = lambda b, on=True: b.data_ptr() + 8 * GUARD if on else 0
        torch.cuda.synchronize()
        s.expected_tangent_dev(K, at(out), 0 if self.dpd is None else self.dpd[k0:].data_ptr(), 0 if self.dpi0 is None else self.dpi0[k0:].data_ptr(),
                               c, _ptr(self.pi0), ivp, at(nxt, want_next), at(prim, want_primal), sparse=sparse)
        s.sync()
        return _body(out).reshape(K, 2, Tc, Z), _body(nxt, want_next).reshape(K, Z), _body(prim, want_primal)


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _f64(a):
    return a.view(np.float64)


# ------------------------------------------------------------------------------------------------ 1: the device entry, upload route
@gpu
@pytest.mark.parametrize("Z", [403, 518, 1031, 1089])
def test_dev_form_gives_the_bits_of_the_dense_twin_on_the_upload_route(cpm, Z):
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 4, 17 * Z)
    s, d = _pair(cpm, Z)
    with s, d:
        for pi0 in (None, S.pi0_with_zeros(Z)):
            call = _Call(dpd, dpi0, pi0)
            for ivp in (False, True):
                got, want = call(s, 4, C4, ivp, True), call(d, 4, C4, ivp, False)
                assert _equal(got, want), (Z, ivp, pi0 is None)
                assert np.isfinite(_f64(got[0])).all() and all(_f64(got[0])[k].any() for k in range(4))
                no_c = call(s, 4, None, ivp, True)
                assert _equal(no_c, call(d, 4, None, ivp, False))
                assert np.array_equal(no_c[0][:3], got[0][:3]) and not np.array_equal(no_c[0][3], got[0][3])     # u moves direction 4 alone
                assert np.array_equal(no_c[2], got[2])
        assert _info(s, cpm) == (1, 0, 1) and _info(d, cpm) == (1, 1, 0)       # (the uploaded array stays resident; no dense tangent)


# ------------------------------------------------------------------------------------------------ 2: the column walk's chunks
@functools.lru_cache(maxsize=None)
def _walk_case(Z=1031):
    """the walk tables with column Z // 2 densified to 300 cells, and a signed tangent on the stored cells"""
    _, p = SD.walk_tables(Z, TU)
    p = np.array(p, order="F")
    dcol = Z // 2
    for t in range(TU):
        rows = [o for o in range(20, Z) if 0.9 < p[o, :, t].sum() and p[o, dcol, t] == 0.0][:300 - int(np.count_nonzero(p[:, dcol, t]))]
        p[rows, :, t] *= 0.5
        p[rows, dcol, t] = 0.25
    dP = np.zeros(p.shape, order="F")
    for t in range(TU):
        dP[:, :, t] = SD.signed_tangent_on_cells(np.ascontiguousarray(p[:, :, t]), (), 900 + t)[0]
    for a in (p, dP):
        a.setflags(write=False)
    return p, dP


@gpu
def test_rows_and_columns_of_every_walk_length_give_the_bits_of_the_dense_call(cpm):
    Z = 1031
    p, dP = _walk_case(Z)
    rows = np.count_nonzero(p, axis=1)
    assert [int(rows[o, 0]) for o in SD.WALK_ROWS] == list(SD.WALK_ROWS.values())      # rows of 0, 1, 63, 64, 65, 255, 256, 257, 309 cells
    cols = np.count_nonzero(p[:, :, 0], axis=0)
    assert ((cols > 256) & (cols <= 512)).any() and (cols > 512).any() and ((cols > 0) & (cols < 256)).any()    # two, more, one chunk
    assert (p.sum(axis=1) <= 1.0).all()
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 4, 23)
    pi0 = S.pi0_with_zeros(Z)
    pi0[:11] = np.arange(1, 12) / 7.0                                      # the walk rows carry mass
    call = _Call(dpd, dpi0, pi0)
    with _upload(cpm, Z, p_dest=p) as s, _upload(cpm, Z, p_dest=p) as d:
        s.set_p_dest_tangent(dP, sparse=True)
        d.set_p_dest_tangent(dP)
        for ivp in (False, True):
            got, want = call(s, 4, C4, ivp, True), call(d, 4, C4, ivp, False)
            assert _equal(got, want), ivp
        assert _info(s, cpm)[1:] == (0, 1)


# ------------------------------------------------------------------------------------------------ 3: every instantiation and pass
@gpu
def test_every_K_gives_the_dense_bits_and_direction_k_does_not_depend_on_K(cpm):
    Z = 403
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 16, 5)
    c = np.zeros(16)
    c[[3, 5, 7, 9, 15]] = (1.0, -0.5, 2.0, 0.25, -1.5)                     # several directions share one u, in all three passes
    call = _Call(dpd, dpi0, S.pi0_with_zeros(Z))
    s, d = _pair(cpm, Z)
    with s, d:
        full = call(s, 16, c, True, True)
        assert _equal(full, call(d, 16, c, True, False))
        for K in (1, 3, 4, 7, 8, 15):                                      # NB = 2, 4, 5, 8; a partial pass; a second and a third pass
            got = call(s, K, c[:K], True, True)
            assert _equal(got, call(d, K, c[:K], True, False)), K
            assert np.array_equal(got[0], full[0][:K]) and np.array_equal(got[1], full[1][:K]) and np.array_equal(got[2], full[2]), K
        for k in range(16):                                                # alone: the bits it has among 16
            one = call(s, 1, c[k:k + 1], True, True, k0=k)
            assert np.array_equal(one[0][0], full[0][k]) and np.array_equal(one[1][0], full[1][k]), k
        for k in (3, 5, 7, 9, 15):                                         # ... and u takes part
            plain = call(s, 1, None, True, True, k0=k)
            assert not np.array_equal(plain[0][0], full[0][k]), k


# ------------------------------------------------------------------------------------------------ 4, 5: the primal; no tangent needed
@gpu
def test_primal_carries_expected_sparse_devs_bits_and_zero_c_dest_needs_no_tangent(cpm):
    import torch
    Z = 518
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 3, 9)
    pi0 = S.pi0_with_zeros(Z)
    call = _Call(dpd, dpi0, pi0)
    with _upload(cpm, Z) as s, _upload(cpm, Z) as d:
        assert _info(s, cpm)[1:] == (0, 0)
        for ivp in (False, True):
            for c in (None, np.zeros(3), np.array([0.0, -0.0, 0.0])):
                got = call(s, 3, c, ivp, True)
                assert _equal(got, call(d, 3, c, ivp, False)), ivp
            exp = _guarded(2 * Z * TU)
            torch.cuda.synchronize()
            s.expected_dev(exp.data_ptr() + 8 * GUARD, call.pi0.data_ptr(), ivp, sparse=True)
            s.sync()
            assert np.array_equal(_body(exp), got[2])
            only = call(s, 3, None, ivp, True, want_next=False, want_primal=False)                 # the optional outputs stay untouched
            assert np.array_equal(only[0], got[0])
        assert _info(s, cpm)[1:] == (0, 0)                                                         # neither tangent exists, none was built
        with pytest.raises(cpm.CpmError) as e:
            call(s, 3, np.array([0.0, 0.5, 0.0]), False, True)
        assert e.value.status == ERR_STATE and "cpm_set_p_dest_tangent_sparse" in str(e.value)


# ------------------------------------------------------------------------------------------------ 6: dataset route, Evaluator, LM
@gpu
def test_dataset_route_gives_the_dense_bits_and_holds_neither_dense_array(cpm):
    with _from_dataset(cpm, 1.7) as s, _from_dataset(cpm, 1.7) as d:
        s.build_p_dest_tangent(sparse=True)
        d.build_p_dest_tangent()
        tabs = s.build_p_drive_tangent(0.1, 0.9, 0.5)                      # (Z, T, 3): d / d (p_min, p_max, e_drive)
        assert _same(tabs, d.build_p_drive_tangent(0.1, 0.9, 0.5))
        dpd = np.zeros((4, s.T, s.Z))
        dpd[:3] = tabs.transpose(2, 1, 0)
        call = _Call(dpd, None, None)
        for ivp in (False, True):
            got, want = call(s, 4, C4, ivp, True), call(d, 4, C4, ivp, False)
            assert _equal(got, want), ivp
            assert all(_f64(got[0])[k].any() for k in range(4)) and np.isfinite(_f64(got[0])).all()
        a = s.expected_tangent(4, np.asfortranarray(dpd.transpose(2, 1, 0)), None, C4, None, True, want_next=True, want_expected=True, sparse=True)
        b = d.expected_tangent(4, np.asfortranarray(dpd.transpose(2, 1, 0)), None, C4, None, True, want_next=True, want_expected=True)
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
        assert np.array_equal(np.ascontiguousarray(a["d_parking"].transpose(2, 1, 0)).view(np.int64), got[0][:, 0])
        assert _info(s, cpm) == (0, 0, 1) and _info(d, cpm) == (1, 1, 0)


@gpu
def test_refine_expected_lm_runs_sparse_with_the_default_evaluators_path(cpm):
    from carparkingmaps_amd import model_selection as M
    dm, dist = _dataset()
    m_act, m_park = _measured(358, 24)
    pts = [M.Point(0.5, 0.1, 0.9, 1.7)]
    w = {"activity_error": 1.0, "parking_error": 1.0, "A_drive": 0.5}
    out, jac = {}, {}
    for sparse in (True, False):
        with cpm.Sampler(358, 24) as s:
            s.set_datamatrix(dm, dist)
            ev = M.Evaluator(s, 3580, SEED, measured_activity=m_act, measured_parking=m_park, expected_sparse=sparse, expected_sparse_dest=sparse,
                             expected_sparse_tangent=sparse)
            out[sparse] = M.refine_expected_lm(ev, pts, w, steps=3)
            if sparse:
                assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
                assert _info(s, cpm) == (0, 0, 0), "refine_expected_lm built a dense array"
            jac[sparse] = ev.expected_jacobian(pts[0], dest=True)
            assert _info(s, cpm) == ((0, 0, 1) if sparse else (1, 1, 0))
    a, b = out[True][0], out[False][0]
    assert a["calls"] == b["calls"] >= 2 and len(a["path"]) == len(b["path"]) >= 1
    for (pa, fa), (pb, fb) in zip(a["path"], b["path"]):                   # point for point, bit for bit
        assert _same(np.array([pa.e_drive, pa.p_min, pa.p_max, fa]), np.array([pb.e_drive, pb.p_min, pb.p_max, fb]))
    assert _same(np.array(a["gradient"]), np.array(b["gradient"])) and a["lam"] == b["lam"]
    assert jac[True].keys() == jac[False].keys() and all(_same(jac[True][k], jac[False][k]) for k in jac[True])
    assert jac[True]["d_parking"].shape == (4, 358, 24) and jac[True]["d_parking"][3].any()


# ------------------------------------------------------------------------------------------------ 7: independently of any kernel here
@gpu
def test_sparse_tangent_meets_twice_the_bound_against_the_numpy_tangent(cpm):
    """the numpy form of tests/expected_tangent_reference.py at the smallest size that has compact rows, held to twice the header's
    bound as tests/test_expected_tangent_gpu.py holds the dense call at Z >= 255; a word of magnitude 0 is exactly 0"""
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    dP = _tangent(Z)
    tables = R.row_tables(p_dest)
    d_pi0, d_pd = TG.directions(Z, TU, 3, 13 * Z + TU)
    c3 = np.array([0.0, -0.75, 1.5])
    with _upload(cpm, Z) as s:
        s.set_p_dest_tangent(dP, sparse=True)
        for flags, pi0 in ((0, S.pi0_with_zeros(Z) / S.pi0_with_zeros(Z).sum()), (R.IVP, None)):
            got = s.expected_tangent(3, d_pd, d_pi0, c3, pi0, bool(flags), want_next=True, sparse=True)
            coef = TG.bounds(Z, TU, flags)
            for k in range(3):
                args = (p_drive, p_dest, pi0, flags, d_pi0[:, k], d_pd[:, :, k], c3[k], dP, tables)
                want, mags = TG.numpy_tangent(*args), TG.numpy_tangent(*args, magnitude=True)
                for name, g, w_, m, cf in zip(("d_parking", "d_driving", "d_pi_next"),
                                              (got["d_parking"][:, :, k], got["d_driving"][:, :, k], got["d_pi_next"][:, k]), want, mags, coef):
                    tol = 2.0 * np.asarray(cf) * m
                    assert np.all(np.isfinite(g)) and np.all(g[m == 0.0] == 0.0)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ratio = np.where(tol != 0.0, np.abs(g - w_) / tol, np.where(g == w_, 0.0, np.inf))
                    print(f"Z={Z} flags={flags} k={k} {name}: worst error / (2 x bound) {ratio.max():.4f}")
                    assert ratio.max() <= 1.0


# ------------------------------------------------------------------------------------------------ 8: caches
@gpu
def test_a_new_tangent_and_new_tables_rebuild_the_transposed_tangent(cpm):
    Z = 403
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 3, 31)
    c = np.array([0.0, 0.0, 1.0])
    call = _Call(dpd, dpi0, None)
    s, d = _pair(cpm, Z)
    with s, d:
        first = call(s, 3, c, True, True)
        assert _equal(first, call(d, 3, c, True, False))
        other = _tangent(Z, seed=2)
        s.set_p_dest_tangent(other, sparse=True)                           # a second compact tangent: the new twin's bits
        d.set_p_dest_tangent(other)
        second = call(s, 3, c, True, True)
        assert _equal(second, call(d, 3, c, True, False)) and not np.array_equal(second[0][2], first[0][2])
        assert np.array_equal(second[0][:2], first[0][:2])
        dense_p = S.sparse_tables(Z, TU, density=0.1)[1]                   # new tables drop the tangent ...
        s.set_p_dest(dense_p)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0 and _info(s, cpm)[1:] == (0, 0)
        with pytest.raises(cpm.CpmError) as e:
            call(s, 3, c, True, True)
        assert e.value.status == ERR_STATE
        call(s, 3, None, True, True)                                       # (zero c_dest needs none)
        dP = _tangent(Z, density=0.1)                                      # ... and the next one is carried through the new cells
        s.set_p_dest_tangent(dP, sparse=True)
        with _upload(cpm, Z, density=0.1) as fresh:
            fresh.set_p_dest_tangent(dP)
            assert _equal(call(s, 3, c, True, True), call(fresh, 3, c, True, False))


# ------------------------------------------------------------------------------------------------ 9: no trace
@gpu
def test_the_same_bits_again_and_no_trace_in_later_calls(cpm):
    import torch
    Z, C, cpz = 403, 4030, 10
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 8, 41)
    c = np.zeros(8)
    c[[2, 7]] = (1.0, -2.0)
    call = _Call(dpd, dpi0, S.pi0_with_zeros(Z))
    cot, gn = _cots(Z, TU, 1, Z)
    s, _d = _pair(cpm, Z)
    with s, _d:
        s.init_states(C, cpz)

        def later():
            r = s.resample(SEED)
            exp = _guarded(2 * Z * TU)
            torch.cuda.synchronize()
            s.expected_dev(exp.data_ptr() + 8 * GUARD, 0, True, sparse=True)
            s.sync()
            return (r["parking"], r["driving"], _body(exp)) + _gdest_dev(s, cot, None, True, gn, True)

        before = later()
        got = call(s, 8, c, True, True)
        assert _equal(got, call(s, 8, c, True, True)), "the same bits on a second call"
        assert _equal(before, later())
        assert _info(s, cpm) == (1, 0, 1)


# ------------------------------------------------------------------------------------------------ 10: refusals
def _refused(L, h, fn, args, status, bufs):
    import torch
    assert fn(h, *args) == status, L.cpm_last_error()
    torch.cuda.synchronize()
    for b in bufs:
        assert np.all(b.cpu().numpy() == SENT), "a refused call wrote to an output"
    return L.cpm_last_error().decode()


@gpu
def test_refusals_come_before_anything_is_written(cpm):
    Z = 403
    dP = _tangent(Z)
    p_drive = S.sparse_tables(Z, TU)[0]
    dpd, dpi0 = _directions(p_drive, 2, 3)
    d_dpd, d_dpi0 = _dev(dpd), _dev(dpi0)
    out, nxt, prim = _guarded(17 * 2 * Z * TU), _guarded(17 * Z), _guarded(2 * Z * TU)
    bufs = (out, nxt, prim)
    vp = lambda b: ctypes.c_void_p(b.data_ptr() + 8 * GUARD)
    arr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)     # (the array as it lies: F-order where the ABI wants it)
    one = np.array([0.0, 1.0])
    dev = lambda K, flags, c, o=out: (K, None, flags, ctypes.c_void_p(d_dpi0.data_ptr()), ctypes.c_void_p(d_dpd.data_ptr()), arr(c),
                                      None if o is None else vp(o), vp(nxt), vp(prim))
    with _upload(cpm, Z, sparse=False) as s:                               # dense tables: the two routes named
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        s.set_p_dest_tangent(dP)
        text = _refused(s._L, s._h, s._L.cpm_expected_sparse_tangent_dev, dev(2, 0, one), ERR_STATE, bufs)
        assert "cpm_build_p_dest" in text and "CPM_OPT_SPARSE_UPLOAD" in text
        with pytest.raises(cpm.CpmError) as e:
            s.expected_tangent(2, None, None, None, sparse=True)
        assert e.value.status == ERR_STATE and "CPM_OPT_SPARSE_UPLOAD" in str(e.value)
        s.expected_tangent(2, None, None, one)                             # (the dense call is untouched by the refusals)
    with _upload(cpm, Z) as s:
        L, h, fn = s._L, s._h, s._L.cpm_expected_sparse_tangent_dev
        s.set_p_dest_tangent(dP)                                           # only a dense tangent: it does not count
        assert _info(s, cpm)[1:] == (1, 0)
        text = _refused(L, h, fn, dev(2, 0, one), ERR_STATE, bufs)
        assert "cpm_set_p_dest_tangent_sparse" in text and "cpm_build_p_dest_tangent_sparse" in text
        s.set_p_dest_tangent(dP, sparse=True)
        for K in (0, 17):
            assert "K = " in _refused(L, h, fn, dev(K, 0, None), ERR_ARG, bufs)
        _refused(L, h, fn, dev(2, 0, one, None), ERR_ARG, bufs)            # NULL output
        _refused(L, h, fn, dev(2, 2, one), ERR_ARG, bufs)                  # unknown flag bits
        for bad in (np.nan, np.inf):
            assert "finite" in _refused(L, h, fn, dev(2, 0, np.array([0.0, bad])), ERR_ARG, bufs)
        # the blocking form
        zt = np.zeros((Z, TU, 2), order="F")
        host = [np.full((Z, TU, 2), 7.0, order="F"), np.full((Z, TU, 2), 7.0, order="F"), np.full((Z, TU), 7.0, order="F")]
        blocking = L.cpm_expected_sparse_tangent

        def block(dpi0_h=None, dpd_h=None, park=None, drv=None, d_park=host[0], d_drv=host[1], c=one):
            rc = blocking(h, 2, None, 0, arr(dpi0_h), arr(dpd_h), arr(c), arr(d_park), arr(d_drv), None, arr(park), arr(drv))
            assert all((a == 7.0).all() for a in host), "a refused call wrote to an output"
            return rc, L.cpm_last_error().decode()

        bad = np.zeros((Z, 2), order="F")
        bad[5, 1] = np.nan
        rc, text = block(dpi0_h=bad)
        assert rc == ERR_ARG and "dpi0" in text and "finite" in text
        bad = np.array(zt)
        bad[7, 1, 0] = -np.inf
        rc, text = block(dpd_h=bad)
        assert rc == ERR_ARG and "dp_drive" in text and "finite" in text
        rc, text = block(park=host[2])
        assert rc == ERR_ARG and "go together" in text
        rc, text = block(drv=host[2])
        assert rc == ERR_ARG and "go together" in text
        rc, _ = block(d_drv=None)
        assert rc == ERR_ARG
        rc, _ = block(d_park=None)
        assert rc == ERR_ARG
        # a row total above 1: CPM_ERR_TABLE with the dense call's text, in front of the first copy
        p = np.array(S.sparse_tables(Z, TU)[1], order="F")
        p[2, :, 1] *= 2.5
        assert p[2, :, 1].sum() > 1.01
        s.set_p_dest(p)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        for _ in range(2):                                                 # (refused every time, not only when the check is first made)
            text = _refused(L, h, fn, dev(2, 0, None), ERR_TABLE, bufs)
            assert "hour 2, origin 3" in text
        rc, text2 = block(c=None)
        assert rc == ERR_TABLE and text2 == text
        with pytest.raises(cpm.CpmError) as e:                             # the dense call of the same tables: the same text
            s.expected_tangent(2, None, None, None)
        assert e.value.status == ERR_TABLE and str(e.value).endswith(text)


@gpu
@pytest.mark.parametrize("Z", [2, 65])
def test_small_tables_hold_the_contract_of_the_route_they_take(cpm, Z):
    """Z = 2 and Z <= 65: where the library gives such a table compact rows, the sparse tangent carries the dense call's bits; where it
    does not, the call is refused with CPM_ERR_STATE and the two routes named, before anything is written."""
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    dP = np.array(SD.signed_tangent_on_cells(np.ascontiguousarray(p_dest[:, :, 0]), (), Z)[0])
    dP = np.asfortranarray(np.stack([np.where(np.asarray(p_dest[:, :, t]) != 0.0, dP, 0.0) for t in range(TU)], axis=2))
    d_pi0, d_pd = TG.directions(Z, TU, 2, Z)
    c = np.array([0.0, 1.0])
    with cpm.Sampler(Z, TU) as s:
        s.set_sparse_upload(True)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        if s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0:
            s.set_p_dest_tangent(dP, sparse=True)
            got = s.expected_tangent(2, d_pd, d_pi0, c, None, True, want_next=True, want_expected=True, sparse=True)
            s.set_p_dest_tangent(dP)
            want = s.expected_tangent(2, d_pd, d_pi0, c, None, True, want_next=True, want_expected=True)
            assert all(_same(got[k], want[k]) for k in got)
        else:
            for cc in (None, c):
                with pytest.raises(cpm.CpmError) as e:
                    s.expected_tangent(2, d_pd, d_pi0, cc, None, True, sparse=True)
                assert e.value.status == ERR_STATE
                assert "CPM_OPT_SPARSE_UPLOAD" in str(e.value) and "cpm_build_p_dest" in str(e.value)
            s.set_p_dest_tangent(dP)                                       # the dense route is there at this size
            assert s.expected_tangent(2, d_pd, d_pi0, c, None, True)["d_parking"].any()
