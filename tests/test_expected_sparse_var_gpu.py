"""The seed variances of count and travel functionals from the compact rows (include/cpm_expected_sparse_var.h) on the GPU.  Every
comparison is array_equal on int64 views against the dense call of a second, fresh context with the same tables: the contract is bit
equality.  Every context that relies on sparse tables asserts CPM_INFO_SPARSE_TABLES > 0 when it is made.

Upload route (CPM_OPT_SPARSE_UPLOAD, the hand-made tables of expected_sparse_reference.sparse_tables, T = 3): Z = 403 (odd; 12 segments
of 34), 518 (even; 16 of 33), 1,031 (32 of 33, the last with 8 destinations), 1,089 (34 of 33, the last EMPTY); these rows hold 16 to 45
cells, one chunk of the row walk, so Z = 1,031 is also run at densities 0.1 and 0.3: rows of two and of more than four chunks.  Dataset
route: Z = 358, T = 24, density 0.06; its compact rows keep cells of weight 0.  K = 1, 3, 4, 5, 9 of the count pass (4 functionals a
pass) reaches every instantiation, a partial pass, and a second and a third pass; K = 1, 2, 3, 5 does the same for travel (2 a pass)."""
import ctypes

import numpy as np
import pytest

import expected_reference as R
import expected_linear_var_reference as LV
import expected_sparse_reference as S
import expected_travel_var_reference as TV
from test_expected_sparse_grad_gpu import LONG_ROWS, SEED, TU, UPLOAD_SIZES, _dataset, _from_dataset, _longest_row, _measured, _upload

gpu = pytest.mark.gpu
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4
KEYS = ("mean", "var", "zone_mean", "zone_var")
COMBOS = [(False, False, True), (True, True, True), (True, False, False), (False, True, False)]      # (ivp, start given, d_zone given)


def _guarded(words):
    import torch
    return torch.full((2 * GUARD + words,), SENT, dtype=torch.int64, device="cuda")


def _body(buf, what, written=True):
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), f"a store outside {what}"
    if written:
        assert not np.any(a[GUARD:-GUARD] == SENT), f"a word of {what} was not written"
    else:
        assert np.all(a == SENT), f"{what} was written"
    return a[GUARD:-GUARD]


def _w(Z):
    w = np.random.default_rng(Z).integers(0, 50, Z).astype(np.float64)
    w[Z // 2] = 0.0
    return w


def _dev_call(s, f, w, ivp, zone, sparse):
    """expected_linear_var_dev (f = (A, B)) or expected_travel_var_dev (f = (A, B, S, D)), each (Z, T, K), between guard words on
    sentinel-filled outputs.  -> int64 views: dict(out [K][2], zone [K][2][Z] or None)"""
    import torch
    K = f[0].shape[2]
    coeff = np.ascontiguousarray(np.stack([x.transpose(2, 1, 0) for x in f], axis=1))              # [K][2 or 4][T][Z]
    d_coeff = torch.from_numpy(coeff).cuda()
    out, zn = _guarded(2 * K), _guarded(2 * K * s.Z)
    d_w = None if w is None else torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    call = s.expected_linear_var_dev if len(f) == 2 else s.expected_travel_var_dev
    call(K, d_coeff.data_ptr(), out.data_ptr() + 8 * GUARD, 0 if w is None else d_w.data_ptr(), ivp, zn.data_ptr() + 8 * GUARD if zone else 0, sparse=sparse)
    s.sync()
    z = _body(zn, "d_zone", zone)                                      # (a NULL d_zone: not a word of the buffer is touched)
    return {"out": _body(out, "d_out").reshape(K, 2), "zone": z.reshape(K, 2, s.Z) if zone else None}


def _eq(a, b):
    if (a["zone"] is None) != (b["zone"] is None):
        return False
    return np.array_equal(a["out"], b["out"]) and (a["zone"] is None or np.array_equal(a["zone"], b["zone"]))


def _f64(x):
    return np.ascontiguousarray(x).view(np.float64)


def _vsec_dev(s, sparse):
    import torch
    buf = _guarded(s.Z * s.T)
    torch.cuda.synchronize()                                           # (the fill runs on torch's stream, the call on the context's)
    s.expected_trip_var_dev(buf.data_ptr() + 8 * GUARD, sparse=sparse)
    s.sync()
    return _body(buf, "d_v")


def _cut(f, a, b):
    return [np.asfortranarray(x[:, :, a:b]) for x in f]


def _compare(s, d, f, Ks, label):
    """the sparse call of s against the dense call of d for the first K functionals of f, every K of Ks, every combination; functional
    k of K against the K = 1 sparse call; the same bits on a repeated call"""
    w = _w(s.Z)
    for K in Ks:
        fk = _cut(f, 0, K)
        for ivp, start, zone in COMBOS:
            got = _dev_call(s, fk, w if start else None, ivp, zone, True)
            want = _dev_call(d, fk, w if start else None, ivp, zone, False)
            assert _eq(got, want), (label, K, ivp, start, zone)
            assert np.isfinite(_f64(got["out"])).all() and (_f64(got["out"])[:, 1] > 0).all(), (label, K)
        again = _dev_call(s, fk, w, True, True, True)
        assert _eq(again, _dev_call(s, fk, w, True, True, True)), "the same bits on a repeated call"
        for k in sorted({0, K // 2, K - 1}):
            one = _dev_call(s, _cut(f, k, k + 1), w, True, True, True)
            assert np.array_equal(one["out"][0], again["out"][k]) and np.array_equal(one["zone"][0], again["zone"][k]), (label, K, k)


# ------------------------------------------------------------------------------------------------ 1: the count functionals
@gpu
@pytest.mark.parametrize("Z", UPLOAD_SIZES)
def test_linear_var_gives_the_bits_of_the_dense_call_on_the_upload_route(cpm, Z):
    f = LV.signed_functionals(Z, TU, 9, 3 * Z)
    with _upload(cpm, Z) as s, _upload(cpm, Z) as d:
        _compare(s, d, f, (1, 3, 4, 5, 9), Z)
        a = s.expected_linear_var(f[0], f[1], start=_w(Z), ivp=True, per_zone=True, sparse=True)       # the blocking forms
        b = d.expected_linear_var(f[0], f[1], start=_w(Z), ivp=True, per_zone=True)
        assert all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in KEYS)
        dev = _dev_call(s, f, _w(Z), True, True, True)
        assert np.array_equal(_f64(dev["out"])[:, 0], a["mean"]) and np.array_equal(_f64(dev["zone"])[:, 1].T, a["zone_var"])
        plain = s.expected_linear_var(f[0][:, :, 2], f[1][:, :, 2], sparse=True)
        assert set(plain) == {"mean", "var"} and plain == d.expected_linear_var(f[0][:, :, 2], f[1][:, :, 2])


# ------------------------------------------------------------------------------------------------ 2: trip variance weights and travel
@gpu
@pytest.mark.parametrize("Z", UPLOAD_SIZES)
def test_trip_var_and_travel_var_give_the_bits_of_the_dense_calls_on_the_upload_route(cpm, Z):
    f = TV.signed_functionals(Z, TU, 5, 5 * Z)
    with _upload(cpm, Z, dm=True) as s, _upload(cpm, Z, dm=True) as d:
        v = _vsec_dev(s, True)
        assert np.array_equal(v, _vsec_dev(d, False)) and np.isfinite(_f64(v)).all() and (_f64(v) > 0).any()
        assert np.array_equal(s.expected_trip_var(sparse=True).view(np.int64), np.asfortranarray(_f64(v).reshape(TU, Z).T).view(np.int64))
        _compare(s, d, f, (1, 2, 3, 5), Z)
        zero = [f[0], f[1], np.zeros_like(f[2]), np.zeros_like(f[3])]                                   # S = D = 0: the sparse linear call's words
        for ivp, start, zone in COMBOS[:2]:
            w = _w(Z) if start else None
            assert _eq(_dev_call(s, zero, w, ivp, zone, True), _dev_call(s, zero[:2], w, ivp, zone, True)), (Z, ivp)
        a = s.expected_travel_var(*f, start=_w(Z), ivp=True, per_zone=True, sparse=True)                # the blocking forms
        b = d.expected_travel_var(*f, start=_w(Z), ivp=True, per_zone=True)
        assert all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in KEYS)
        a = s.expected_travel_var(f[0], f[1], None, f[3], sparse=True)                                  # a NULL trip array
        b = d.expected_travel_var(f[0], f[1], None, f[3])
        assert all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in ("mean", "var"))
        assert (s.expected_trip_var_builds(sparse=True), s.expected_trip_var_builds()) == (1, 0)
        assert (d.expected_trip_var_builds(sparse=True), d.expected_trip_var_builds()) == (0, 1)


# ------------------------------------------------------------------------------------------------ 3: long rows, and the dataset route
@gpu
@pytest.mark.parametrize("density,above,most", LONG_ROWS)
def test_rows_of_several_chunks_give_the_bits_of_the_dense_calls(cpm, density, above, most):
    Z = 1031
    longest, median = _longest_row(Z, density)
    assert above < median and above < longest <= most, (longest, median)    # the typical row, not only the longest, is past the edge
    lin, trav = LV.signed_functionals(Z, TU, 5, 41), TV.signed_functionals(Z, TU, 3, 43)
    with _upload(cpm, Z, dm=True, density=density) as s, _upload(cpm, Z, dm=True, density=density) as d:
        assert np.array_equal(_vsec_dev(s, True), _vsec_dev(d, False))
        w = _w(Z)
        for f in (lin, trav):
            for ivp, start, zone in COMBOS[:2]:
                got, want = _dev_call(s, f, w if start else None, ivp, zone, True), _dev_call(d, f, w if start else None, ivp, zone, False)
                assert _eq(got, want), (density, len(f), ivp)
            assert (_f64(got["out"])[:, 1] > 0).all()


@gpu
def test_every_call_on_the_dataset_route(cpm):
    lin, trav = LV.signed_functionals(358, 24, 9, 7), TV.signed_functionals(358, 24, 3, 9)
    with _from_dataset(cpm, measured=False) as s, _from_dataset(cpm, measured=False) as d:
        w = _w(358)
        assert np.array_equal(_vsec_dev(s, True), _vsec_dev(d, False))
        for f in (lin, trav):
            for ivp, start, zone in COMBOS[:2]:
                got, want = _dev_call(s, f, w if start else None, ivp, zone, True), _dev_call(d, f, w if start else None, ivp, zone, False)
                assert _eq(got, want), (len(f), ivp)
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0 and d.get_info(cpm.CPM_INFO_P_DENSE) == 1


# ------------------------------------------------------------------------------------------------ 4: independent of the dense kernels
@gpu
def test_sparse_linear_var_meets_twice_the_bound_against_the_numpy_form(cpm):
    Z, K = 403, 5
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    tables = R.row_tables(p_dest)
    A, B = LV.signed_functionals(Z, TU, K, Z)
    w = _w(Z)
    with _upload(cpm, Z) as s:
        for flags in (0, LV.IVP):
            got = s.expected_linear_var(A, B, start=w, ivp=bool(flags), per_zone=True, sparse=True)
            for k in (0, K - 1):
                want = LV.numpy_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables)
                mag = LV.numpy_lv(p_drive, p_dest, A[:, :, k], B[:, :, k], w, flags, tables, magnitude=True)
                bound = {key: 2.0 * np.asarray(v) for key, v in LV.bounds(Z, TU, flags, mag, w).items()}
                one = {"mean": got["mean"][k], "var": got["var"][k], "zone_mean": got["zone_mean"][:, k], "zone_var": got["zone_var"][:, k]}
                for key in KEYS:
                    g, e, b = np.atleast_1d(one[key]), np.atleast_1d(want[key]), np.atleast_1d(bound[key])
                    ratio = float(np.max(np.abs(g - e) / np.where(b > 0, b, 1.0)))
                    print(f"Z={Z} flags={flags} k={k}: {key} worst error / (2 x bound) {ratio:.4f}")
                    assert np.all(np.isfinite(g)) and np.all(np.abs(g - e) <= b), (key, flags, k, ratio)


# ------------------------------------------------------------------------------------------------ 5: the centring
@gpu
@pytest.mark.parametrize("Z", [403, 1089])
def test_a_functional_constant_over_the_zones_has_variance_exactly_zero(cpm, Z):
    hours = np.arange(1.0, TU + 1.0) * 0.3                             # (constant over the zones, not over the hours)
    A = np.stack([np.broadcast_to(c * hours[None, :], (Z, TU)) for c in (1.0, 1e6)], axis=2)
    A = np.asfortranarray(np.concatenate([A, A[:, :, :1]], axis=2))    # (the third: with a driving term, a check of the check)
    B = np.zeros((Z, TU, 3), order="F")
    B[:, :, 2] = 1.0
    w = _w(Z)
    with _upload(cpm, Z, dm=True) as s:
        for ivp in (False, True):
            for f in ((A, B), (A, B, np.zeros_like(A), np.zeros_like(A))):
                got = _dev_call(s, f, w, ivp, True, True)
                out, zone = _f64(got["out"]), _f64(got["zone"])
                assert out[0, 1] == 0.0 and out[1, 1] == 0.0 and not zone[:2, 1].any(), (Z, ivp, len(f))
                assert out[2, 1] > 0.0
                assert abs(out[0, 0] - hours.sum() * w.sum()) <= 1e-9 * hours.sum() * w.sum()


# ------------------------------------------------------------------------------------------------ 6: residency
def _every_sparse_call(s):
    Z, Tc = s.Z, s.T
    lin, trav = LV.signed_functionals(Z, Tc, 5, 1), TV.signed_functionals(Z, Tc, 3, 2)
    w = _w(Z)
    _dev_call(s, lin, w, True, True, True)
    _dev_call(s, trav, None, False, False, True)
    _vsec_dev(s, True)
    s.expected_linear_var(lin[0], lin[1], start=w, sparse=True)
    s.expected_trip_var(sparse=True)
    s.expected_travel_var(*trav, ivp=True, sparse=True)
    assert s.expected_trip_var_builds(sparse=True) == 1 and s.expected_trip_var_builds() == 0


@gpu
def test_no_sparse_variance_call_expands_the_dense_array(cpm):
    from carparkingmaps_amd import model_selection as M
    dm, dist = _dataset()
    m_act, m_park = _measured(358, 24)
    pt = M.Point(0.5, 0.1, 0.9, 2)
    res = {}
    for sparse in (True, False):
        with cpm.Sampler(358, 24) as s:
            s.set_datamatrix(dm, dist)
            ev = M.Evaluator(s, 3580, SEED, measured_activity=m_act, measured_parking=m_park, expected_sparse=sparse)
            ev._install(pt)
            assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0 and s.get_info(cpm.CPM_INFO_P_DENSE) == 0
            if sparse:
                _every_sparse_call(s)
                assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0, "a sparse variance call expanded the dense array"
            res[sparse] = ev.expected_noise(pt, travel=True)
            assert s.get_info(cpm.CPM_INFO_P_DENSE) == (0 if sparse else 1), "expected_noise under expected_sparse expanded the dense array"
    a, b = res[True], res[False]                                       # ... and the Evaluator's noise is the default Evaluator's, bit for bit
    assert a.keys() == b.keys() == {"activity", "activity_error_std", "parking_error_std", "A_drive"}
    assert all(np.array_equal(a["activity"][k].view(np.int64), b["activity"][k].view(np.int64)) for k in ("mean", "var"))
    assert a["activity_error_std"] == b["activity_error_std"] and a["parking_error_std"] == b["parking_error_std"] and a["A_drive"] == b["A_drive"]
    assert a["A_drive"]["seconds_std"] > 0 and a["activity_error_std"] > 0


# ------------------------------------------------------------------------------------------------ 7: the caches follow their inputs
@gpu
def test_sparse_trip_variance_weights_follow_new_tables_datamatrix_and_distances(cpm):
    dm, dist = _dataset()
    trav = TV.signed_functionals(358, 24, 2, 4)
    with _from_dataset(cpm, 2, measured=False) as s:
        first = _vsec_dev(s, True)
        assert np.array_equal(first, _vsec_dev(s, True)) and s.expected_trip_var_builds(sparse=True) == 1      # cached
        s.build_p_dest(1.5, want=False)                                # another e_dest
        got = _vsec_dev(s, True)
        with _from_dataset(cpm, 1.5, measured=False) as d:
            assert np.array_equal(got, _vsec_dev(d, False))
        assert not np.array_equal(got, first) and s.expected_trip_var_builds(sparse=True) == 2
        dist2 = np.asfortranarray(np.array(dist) * 1.25)               # new distances: v_sec keeps its words, the cache is rebuilt, travel moves
        before = _dev_call(s, trav, None, True, True, True)
        s.set_distance(dist2)
        assert np.array_equal(_vsec_dev(s, True), got) and s.expected_trip_var_builds(sparse=True) == 3
        after = _dev_call(s, trav, None, True, True, True)
        with _from_dataset(cpm, 1.5, measured=False) as d:
            d.set_distance(dist2)
            assert _eq(after, _dev_call(d, trav, None, True, True, False))
        assert not _eq(before, after)
        dm2 = np.array(dm, order="F")                                  # a new datamatrix (the tables go with it: built again)
        dm2[..., 1] *= 1.5
        s.set_datamatrix(dm2, dist2)
        s.build_p_dest(1.5, want=False)
        got2 = _vsec_dev(s, True)
        with cpm.Sampler(358, 24) as d:
            d.set_datamatrix(dm2, dist2)
            d.build_p_drive(0.1, 0.9, 0.5, want=False)
            d.build_p_dest(1.5, want=False)
            assert np.array_equal(got2, _vsec_dev(d, False))
        assert not np.array_equal(got2, got) and s.expected_trip_var_builds(sparse=True) == 4
        assert s.expected_trip_var_builds() == 0 and s.expected_trip_builds() == 0 and s.get_info(cpm.CPM_INFO_P_DENSE) == 0
    Z = 403
    _, p_b, _ = S.sparse_tables(Z, TU, seed=8)
    with _upload(cpm, Z, dm=True) as s:
        a = _vsec_dev(s, True)
        s.set_p_dest(p_b)                                              # another uploaded table
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        b = _vsec_dev(s, True)
        with _upload(cpm, Z, dm=True, p_dest=p_b) as d:
            assert np.array_equal(b, _vsec_dev(d, False))
        assert not np.array_equal(a, b) and s.expected_trip_var_builds(sparse=True) == 2 and s.expected_trip_var_builds() == 0
        dense = _vsec_dev(s, False)                                    # a dense build in between moves its own counter alone
        assert np.array_equal(dense, b) and (s.expected_trip_var_builds(sparse=True), s.expected_trip_var_builds()) == (2, 1)


# ------------------------------------------------------------------------------------------------ 8: no trace
@gpu
def test_sparse_calls_leave_no_trace_in_a_later_dense_call_or_resample(cpm, O):
    Z, cpz = 403, 50
    C = Z * cpz
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SEED, zone0)
    lin, trav = LV.signed_functionals(Z, TU, 5, 1), TV.signed_functionals(Z, TU, 3, 2)
    w = _w(Z)
    with _upload(cpm, Z, dm=True) as s, _upload(cpm, Z, dm=True) as d:
        s.init_states(C, cpz)
        _dev_call(s, lin, w, True, True, True)
        _dev_call(s, trav, w, False, True, True)
        assert np.array_equal(s.solve_ivp(SEED), ref["zone0"])
        s.expected_travel_var(*trav, sparse=True)
        r = s.resample(SEED)
        assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])
        step = s.last_step()
        s.expected_linear_var(lin[0], lin[1], start=w, ivp=True, sparse=True)
        s.expected_trip_var(sparse=True)
        assert s.last_step() == step
        for f in (lin, trav):                                          # the dense calls of the context that made sparse calls, and of one that never did
            for ivp in (False, True):
                assert _eq(_dev_call(s, f, w, ivp, True, False), _dev_call(d, f, w, ivp, True, False))
        assert np.array_equal(_vsec_dev(s, False), _vsec_dev(d, False))
        pairs = [(s.expected(ivp=True), d.expected(ivp=True)), (s.expected_trip(), d.expected_trip()),
                 (tuple(s.expected_var(ivp=True).values()), tuple(d.expected_var(ivp=True).values()))]
        for here, never in pairs:
            assert all(np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)) for a, b in zip(here, never))
        for f in (lin, trav):                                          # ... and a dense call changes nothing a later sparse call returns
            assert _eq(_dev_call(s, f, w, True, True, True), _dev_call(d, f, w, True, True, True))
        assert s.expected_trip_var_builds() == d.expected_trip_var_builds() == 1


# ------------------------------------------------------------------------------------------------ 9: refusals
@gpu
def test_refusals(cpm):
    import torch
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    lin, trav = LV.signed_functionals(Z, TU, 2, 9), TV.signed_functionals(Z, TU, 2, 10)
    calls = lambda s: (lambda: s.expected_linear_var(*lin, sparse=True), lambda: s.expected_travel_var(*trav, sparse=True),
                       lambda: s.expected_trip_var(sparse=True))
    with _upload(cpm, Z, sparse=False, dm=True) as s:                   # dense tables: CPM_ERR_STATE, the two routes named
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        buf = torch.zeros(8 * Z * TU, dtype=torch.float64, device="cuda")
        dev = (lambda: s.expected_linear_var_dev(1, buf.data_ptr(), buf.data_ptr(), sparse=True),
               lambda: s.expected_travel_var_dev(1, buf.data_ptr(), buf.data_ptr(), sparse=True),
               lambda: s.expected_trip_var_dev(buf.data_ptr(), sparse=True))
        for call in calls(s) + dev:
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "cpm_build_p_dest" in str(e.value) and "CPM_OPT_SPARSE_UPLOAD" in str(e.value)
        assert not buf.cpu().numpy().any()
        assert np.all(np.isfinite(s.expected_linear_var(*lin)["var"]))  # (the dense calls are untouched by the refusals)
        assert s.expected_trip_var_builds(sparse=True) == 0
    with cpm.Sampler(Z, TU) as s:                                      # the refusals of the dense namesakes, in their order
        s.set_sparse_upload(True)
        for call in calls(s)[:2]:
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "p_drive" in str(e.value)
        s.set_p_drive(p_drive)
        for call in calls(s):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        s.set_p_dest(p_dest)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        for call in calls(s)[1:]:
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "datamatrix" in str(e.value)
        assert np.all(np.isfinite(s.expected_linear_var(*lin, sparse=True)["var"]))     # (the counts need neither)
    with _upload(cpm, Z, dm=True, dist=False) as s:                    # sparse tables and a datamatrix, but no distance matrix
        for call in calls(s)[1:]:
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "distance matrix" in str(e.value)
    with _upload(cpm, Z, dm=True) as s:
        L, h = s._L, s._h
        buf = torch.zeros(16 * Z * TU, dtype=torch.float64, device="cuda")
        p = ctypes.c_void_p(buf.data_ptr())
        host = np.zeros(4 * Z * TU)
        vp = host.ctypes.data_as(ctypes.c_void_p)
        for fn in (L.cpm_expected_sparse_linear_var_dev, L.cpm_expected_sparse_travel_var_dev):
            assert fn(h, None, 0, 1, None, p, None) == ERR_ARG and b"d_coeff" in L.cpm_last_error()
            assert fn(h, None, 0, 1, p, None, None) == ERR_ARG and b"d_out" in L.cpm_last_error()
            for K in (0, -1, 65):
                assert fn(h, None, 0, K, p, p, None) == ERR_ARG and b"K = " in L.cpm_last_error()
            for flags in (2, 0x100, 0x80000001):
                assert fn(h, None, flags, 1, p, p, None) == ERR_ARG and b"flag" in L.cpm_last_error()
            assert fn(None, None, 0, 1, p, p, None) == ERR_ARG
        assert L.cpm_expected_sparse_trip_var_dev(h, None) == ERR_ARG and L.cpm_expected_sparse_trip_var(h, None) == ERR_ARG
        assert L.cpm_expected_sparse_trip_var_builds(None) == ERR_ARG
        assert L.cpm_expected_sparse_linear_var(h, None, 0, 1, None, vp, vp, vp, None, None) == ERR_ARG
        assert L.cpm_expected_sparse_linear_var(h, None, 0, 1, vp, vp, None, vp, None, None) == ERR_ARG
        assert L.cpm_expected_sparse_travel_var(h, None, 0, 1, vp, None, None, None, vp, vp, None, None) == ERR_ARG
        assert L.cpm_expected_sparse_travel_var(h, None, 0, 1, vp, vp, None, None, vp, None, None, None) == ERR_ARG
        for K in (0, 65):
            assert L.cpm_expected_sparse_linear_var(h, None, 0, K, vp, vp, vp, vp, None, None) == ERR_ARG
            assert L.cpm_expected_sparse_travel_var(h, None, 0, K, vp, vp, None, None, vp, vp, None, None) == ERR_ARG
        assert not buf.cpu().numpy().any() and not host.any()
        for bad in (np.nan, np.inf, -1e-9):
            w = np.ones(Z)
            w[3] = bad
            for call in (lambda: s.expected_linear_var(*lin, start=w, sparse=True), lambda: s.expected_travel_var(*trav, start=w, sparse=True)):
                with pytest.raises(cpm.CpmError) as e:
                    call()
                assert e.value.status == ERR_ARG and "zone 4" in str(e.value)
        for bad in (np.nan, np.inf, -np.inf):
            for which in range(4):
                c = [x.copy(order="F") for x in trav]
                c[which][6, 2, 1] = bad
                with pytest.raises(cpm.CpmError) as e:
                    s.expected_travel_var(*c, sparse=True)
                assert e.value.status == ERR_ARG and "functional 2, zone 7, hour 3" in str(e.value)
                if which < 2:
                    with pytest.raises(cpm.CpmError) as e:
                        s.expected_linear_var(*c[:2], sparse=True)
                    assert e.value.status == ERR_ARG and "functional 2, zone 7, hour 3" in str(e.value)
        big = np.array(p_dest)
        big[2, :, 1] *= 2.5                                            # a row total above 1: the dense call's text
        s.set_p_dest(big)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        for call in calls(s):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_TABLE and "hour 2, origin 3" in str(e.value)
        text = str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_trip_var()
        assert e.value.status == ERR_TABLE and str(e.value) == text


# ------------------------------------------------------------------------------------------------ 10: Python
@gpu
def test_noise_helpers_with_sparse_give_their_dense_forms(cpm):
    from carparkingmaps_amd import model_selection as M
    Z = 518
    m_act, m_park = _measured(Z, TU)
    start = np.full(Z, 10.0)
    with _upload(cpm, Z, dm=True) as s, _upload(cpm, Z, dm=True) as d:
        for ivp in (False, True):
            a, b = M.activity_noise(s, start, ivp=ivp, sparse=True), M.activity_noise(d, start, ivp=ivp)
            assert all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in ("mean", "var")) and (a["var"] > 0).all()
            dens = d.expected(None, ivp=ivp)
            assert M.objective_noise(s, dens, 10 * Z, start, m_act, m_park, ivp=ivp, sparse=True) == M.objective_noise(d, dens, 10 * Z, start, m_act, m_park, ivp=ivp)
            a, b = M.travel_noise(s, start, ivp=ivp, sparse=True), M.travel_noise(d, start, ivp=ivp)
            assert a == b and a["seconds_std"] > 0 and a["km_std"] > 0
        assert s.expected_trip_var_builds() == 0 and d.expected_trip_var_builds(sparse=True) == 0
