"""The adjoint, the trip weights, the travel product and the fit from the compact rows (include/cpm_expected_sparse_grad.h) on the GPU.
Every comparison is array_equal on int64 views against the dense call of a second, fresh context with the same tables: the contract is
bit equality.  Every context that relies on sparse tables asserts CPM_INFO_SPARSE_TABLES > 0 when it is made.

Upload route (CPM_OPT_SPARSE_UPLOAD, the hand-made tables of expected_sparse_reference.sparse_tables, T = 3): Z = 403 (4 strips, 12
segments of 34), 518 (16 segments of 33), 1,031 (32 segments of 33, the last with 8 destinations), 1,089 (34 segments of 33, the last
EMPTY); these rows hold 16 to 45 cells, one chunk of the kernels' row walk, so Z = 1,031 is also run at densities 0.1 and 0.3: rows of 104
and 309 cells in the median, two and more than four chunks.  Dataset route: Z = 358, T = 24, density 0.06 as tests/test_expected_sparse_gpu.py uses; its compact rows keep cells of weight 0."""
import ctypes
import functools

import numpy as np
import pytest

import expected_grad_reference as G
import expected_reference as R
import expected_sparse_reference as S
from test_expected_fit_gpu import FLEETS, _measured

gpu = pytest.mark.gpu
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4
TU = 3
SEED = 20240611
UPLOAD_SIZES = [403, 518, 1031, 1089]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _datamatrix(Z, Tc, negative=False):
    """a datamatrix and distances for the uploaded tables: finite everywhere; negative: some means below 0 at stored cells"""
    from oracle import oracle as O
    O.build()
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.3)
    dm, dist = np.array(dm, order="F"), np.array(dist, order="F")
    if negative:
        _, p_dest, _ = S.sparse_tables(Z, Tc)
        o, d, t = np.nonzero(p_dest)
        pick = slice(0, len(o), 7)
        dm[o[pick], d[pick], t[pick], 0] = -25.0
    assert np.isfinite(dm).all() and np.isfinite(dist).all()         # the precondition of the sparse trip weights
    for a in (dm, dist):
        a.setflags(write=False)
    return dm, dist


def _upload(cpm, Z, sparse=True, dm=False, negative=False, p_dest=None, density=None, dist=True):
    """dm: with a datamatrix; dist=False: without its distance matrix; density: of sparse_tables (None: its default, rows of 16 to 45 cells)"""
    p_drive, p, _ = S.sparse_tables(Z, TU, density=density)
    s = cpm.Sampler(Z, TU)
    s.set_sparse_upload(sparse)
    if dm:
        matrix, km = _datamatrix(Z, TU, negative)
        s.set_datamatrix(matrix, km if dist else None)
    s.set_p_drive(p_drive)
    s.set_p_dest(p if p_dest is None else p_dest)
    if sparse:
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0, "the table fell back to dense packs"
    return s


@functools.lru_cache(maxsize=None)
def _dataset(Z=358, Tc=24):
    from oracle import oracle as O
    O.build()
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.06)
    assert np.isfinite(dm).all() and np.isfinite(dist).all()
    for a in (dm, dist):
        a.setflags(write=False)
    return dm, dist


def _from_dataset(cpm, e_dest=2, measured=True):
    dm, dist = _dataset()
    s = cpm.Sampler(358, 24)
    s.set_datamatrix(dm, dist)
    s.build_p_drive(0.1, 0.9, 0.5, want=False)
    s.build_p_dest(e_dest, want=False)
    assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0, "the table fell back to dense packs"
    if measured:
        m_act, m_park = _measured(358, 24)
        s.set_measured_activity(m_act)
        s.set_measured(m_park)
    return s


def _guarded(n):
    import torch
    return torch.full((2 * GUARD + n,), SENT, dtype=torch.int64, device="cuda")


def _body(buf, written=True):
    a = buf.cpu().numpy()
    assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
    if written:
        assert not np.any(a[GUARD:-GUARD] == SENT), "a word of the output was not written"
    else:
        assert np.all(a == SENT)
    return a[GUARD:-GUARD]


def _dev(t):
    import torch
    return None if t is None else torch.from_numpy(np.ascontiguousarray(t)).cuda()


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _grad_dev(s, cot, pi0, ivp, gn, sparse, want_pi0=True, B=0):
    """expected_grad[_batch]_dev between guard words.  cot: (B, 2, T, Z) C-order; gn: (B, Z).  -> int64 (grad [B][T][Z], grad_pi0 [B][Z])"""
    import torch
    nb = max(B, 1)
    d_cot, d_pi0, d_gn = _dev(cot), _dev(pi0), _dev(gn)
    grad, gpi0 = _guarded(nb * s.Z * s.T), _guarded(nb * s.Z)
    torch.cuda.synchronize()
    call = s.expected_grad_batch_dev if B else s.expected_grad_dev
    call(d_cot.data_ptr(), grad.data_ptr() + 8 * GUARD, _ptr(d_pi0), ivp, _ptr(d_gn), gpi0.data_ptr() + 8 * GUARD if want_pi0 else 0, sparse=sparse)
    s.sync()
    return _body(grad).reshape(nb, s.T, s.Z), _body(gpi0, want_pi0).reshape(nb, s.Z)


def _cots(Z, Tc, B, seed):
    """distinct cotangents per fleet with negative entries and exact zeros: (B, 2, T, Z), and G_next (B, Z)"""
    rng = np.random.default_rng(seed)
    cot = rng.normal(0.0, 1.0, (B, 2, Tc, Z))
    cot[rng.random(cot.shape) < 0.1] = 0.0
    gn = rng.normal(0.0, 1.0, (B, Z))
    assert (cot < 0).any() and (cot == 0).any()
    return cot, gn


def _fleet_tables(Z, Tc, B):
    f = np.asfortranarray(np.random.default_rng(B).uniform(0.0, 1.0, (Z, Tc, B)))
    f[:5, 1, 0] = [np.nan, -0.1, 0.0, 1.0, 1.5]                      # clipped entries: grad_p_drive exactly 0
    return f


# ------------------------------------------------------------------------------------------------ 1: adjoint, single call
def _single_cases(s, d, cpm):
    Z, Tc = s.Z, s.T
    cot, gn = _cots(Z, Tc, 1, Z)
    for ivp in (False, True):
        for pi0 in (None, S.pi0_with_zeros(Z)):
            for with_next in (False, True):
                for want_pi0 in (True, False):
                    g = gn if with_next else None
                    got = _grad_dev(s, cot, pi0, ivp, g, True, want_pi0)
                    want = _grad_dev(d, cot, pi0, ivp, g, False, want_pi0)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (Z, ivp, pi0 is None, with_next, want_pi0)
        again = _grad_dev(s, cot, None, ivp, gn, True)
        assert all(np.array_equal(a, b) for a, b in zip(again, _grad_dev(s, cot, None, ivp, gn, True))), "the same bits on a second call"
        assert again[0].view(np.float64).any() and np.isfinite(again[0].view(np.float64)).all()
        zero = _grad_dev(s, np.zeros_like(cot), None, ivp, None, True)
        assert not zero[0].any() and not zero[1].any()               # a zero cotangent: exact +0 everywhere
    return got


@gpu
@pytest.mark.parametrize("Z", UPLOAD_SIZES)
def test_single_adjoint_gives_the_bits_of_the_dense_call_on_the_upload_route(cpm, Z):
    with _upload(cpm, Z) as s, _upload(cpm, Z) as d:
        p_drive = np.array(S.sparse_tables(Z, TU)[0])
        p_drive[:5, 1] = [np.nan, -0.1, 0.0, 1.0, 1.5]
        for c in (s, d):
            c.set_p_drive(p_drive)
        _single_cases(s, d, cpm)
        cot, gn = _cots(Z, TU, 1, Z)
        grad, _ = _grad_dev(s, cot, None, True, gn, True)
        assert not grad[0, 1, :5].any()                              # clipped p_drive entries: exactly 0
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 1                 # (the uploaded array stays resident)


@gpu
def test_single_adjoint_gives_the_bits_of_the_dense_call_on_the_dataset_route(cpm):
    with _from_dataset(cpm) as s, _from_dataset(cpm) as d:
        _single_cases(s, d, cpm)
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0 and d.get_info(cpm.CPM_INFO_P_DENSE) == 1


# ------------------------------------------------------------------------------------------------ 2: adjoint, batched
@gpu
@pytest.mark.parametrize("B", [1, 2, 3, 5, 9, 17])
def test_batched_adjoint_against_the_dense_batch_and_the_single_sparse_call(cpm, B):
    Z = 403
    fleets = _fleet_tables(Z, TU, B)
    cot, gn = _cots(Z, TU, B, 100 + B)
    pi0 = S.pi0_with_zeros(Z)
    with _upload(cpm, Z) as s, _upload(cpm, Z) as d:
        for c in (s, d):
            c.set_p_drive_batch(fleets)
        for ivp, g in ((False, gn), (True, None), (True, gn)):
            got = _grad_dev(s, cot, pi0, ivp, g, True, B=B)
            want = _grad_dev(d, cot, pi0, ivp, g, False, B=B)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (B, ivp)
            for b in range(B):
                s.set_p_drive(fleets[:, :, b])
                one = _grad_dev(s, cot[b:b + 1], pi0, ivp, None if g is None else g[b:b + 1], True)
                assert np.array_equal(one[0][0], got[0][b]) and np.array_equal(one[1][0], got[1][b]), (B, b, ivp)
        assert not got[0][0, 1, :5].any()


@gpu
def test_batched_adjoint_on_the_dataset_route_and_an_empty_trailing_segment(cpm):
    B = 9
    with _from_dataset(cpm) as s, _from_dataset(cpm) as d:
        for c in (s, d):
            c.build_p_drive_batch([f[0] for f in FLEETS], [f[1] for f in FLEETS], [f[2] for f in FLEETS])
        cot, gn = _cots(358, 24, B, 77)
        got, want = _grad_dev(s, cot, None, True, gn, True, B=B), _grad_dev(d, cot, None, True, gn, False, B=B)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0
    Z, B = 1089, 3
    fleets = _fleet_tables(Z, TU, B)
    cot, gn = _cots(Z, TU, B, 5)
    with _upload(cpm, Z) as s, _upload(cpm, Z) as d:
        for c in (s, d):
            c.set_p_drive_batch(fleets)
        got, want = _grad_dev(s, cot, None, False, gn, True, B=B), _grad_dev(d, cot, None, False, gn, False, B=B)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# rows of more than one chunk of 64 cells, as Melbourne's shape has them (205 cells on average): the accumulators carried from chunk to
# chunk, a segment's run that continues at the head of the next chunk, the chunks loaded ahead, and past 256 cells those loaded in turn
LONG_ROWS = [(0.1, 64, 256), (0.3, 256, 512)]      # (density of sparse_tables at Z = 1,031, longest row above, and at most)


def _longest_row(Z, density):
    _, p_dest, _ = S.sparse_tables(Z, TU, density=density)
    counts = np.count_nonzero(p_dest, axis=1)                         # (Z origins, T): the stored cells of every row
    return int(counts.max()), float(np.median(counts))


@gpu
@pytest.mark.parametrize("density,above,most", LONG_ROWS)
def test_rows_of_several_chunks_give_the_bits_of_the_dense_calls(cpm, density, above, most):
    Z = 1031
    longest, median = _longest_row(Z, density)
    assert above < median and above < longest <= most, (longest, median)    # the typical row, not only the longest, is past the edge
    cot, gn = _cots(Z, TU, 9, 31)
    pi0 = S.pi0_with_zeros(Z)
    with _upload(cpm, Z, dm=True, density=density) as s, _upload(cpm, Z, dm=True, density=density) as d:
        for ivp, g in ((False, gn[:1]), (True, None)):
            got, want = _grad_dev(s, cot[:1], pi0, ivp, g, True), _grad_dev(d, cot[:1], pi0, ivp, g, False)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (density, ivp)
            assert got[0].view(np.float64).any()
        for B in (2, 3, 9):                                           # every batched instantiation, and a pass of one behind a pass of eight
            fleets = _fleet_tables(Z, TU, B)
            for c in (s, d):
                c.set_p_drive_batch(fleets)
            got, want = _grad_dev(s, cot[:B], pi0, True, gn[:B], True, B=B), _grad_dev(d, cot[:B], pi0, True, gn[:B], False, B=B)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (density, B)
        s.set_p_drive(fleets[:, :, 8])                                # fleet 8 of the batch of nine against the single sparse call
        one = _grad_dev(s, cot[8:9], pi0, True, gn[8:9], True)
        assert np.array_equal(one[0][0], got[0][8]) and np.array_equal(one[1][0], got[1][8])
        w = _trip_dev(s, True)
        assert np.array_equal(w, _trip_dev(d, False)) and np.isfinite(w.view(np.float64)).all()
        tr, tr_d = _travel_dev(s, True, 9), _travel_dev(d, False, 9)
        assert np.array_equal(tr[0], tr_d[0]) and np.array_equal(tr[1], tr_d[1])
        assert s.expected_trip_builds() == 0


# ------------------------------------------------------------------------------------------------ 3: an independent check
@gpu
def test_sparse_adjoint_meets_twice_the_bound_against_the_numpy_form(cpm):
    """the bound tests/test_expected_grad_gpu.py applies to the dense call at sizes the exact form is too slow for: twice the header's"""
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    tables = R.row_tables(p_dest)
    with _upload(cpm, Z) as s:
        for flags, pi0, with_next in ((0, None, False), (R.IVP, S.pi0_with_zeros(Z) / S.pi0_with_zeros(Z).sum(), True)):
            gp, gd, gn = G.signed_cotangents(Z, TU, 7 * Z + TU, "random")
            gn = gn if with_next else None
            got = s.expected_grad(gp, gd, pi0, ivp=bool(flags), g_next=gn, sparse=True)
            ngrad, npi0 = G.numpy_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables)
            bg, bp = G.numpy_adjoint(p_drive, p_dest, gp, gd, pi0, flags, gn, tables, bound_factor=2.0)
            for name, g, want, tol in (("grad_p_drive", got["grad_p_drive"], ngrad, bg), ("grad_pi0", got["grad_pi0"], npi0, bp)):
                assert np.all(g[tol == 0.0] == 0.0), name
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(tol != 0.0, np.abs(g - want) / tol, 0.0)
                print(f"Z={Z} flags={flags}: {name} worst error / (2 x bound) {ratio.max():.4f}")
                assert np.all(np.isfinite(g)) and ratio.max() <= 1.0, name


# ------------------------------------------------------------------------------------------------ 4: trip weights and travel
def _trip_dev(s, sparse):
    import torch
    w = _guarded(2 * s.Z * s.T)
    torch.cuda.synchronize()
    s.expected_trip_dev(w.data_ptr() + 8 * GUARD, sparse=sparse)
    s.sync()
    return _body(w)


def _travel_dev(s, sparse, B=0, ivp=True):
    import torch
    nb = max(B, 1)
    exp = torch.empty(nb * s.expected_words(), dtype=torch.float64, device="cuda")
    trav, tot = _guarded(nb * 2 * s.Z * s.T), _guarded(2 * nb)
    torch.cuda.synchronize()
    (s.expected_batch_dev if B else s.expected_dev)(exp.data_ptr(), 0, ivp, sparse=sparse)
    s.expected_travel_dev(exp.data_ptr(), nb, trav.data_ptr() + 8 * GUARD, tot.data_ptr() + 8 * GUARD, sparse=sparse)
    s.sync()
    return _body(trav), _body(tot)


@gpu
@pytest.mark.parametrize("Z,negative", [(403, False), (403, True), (518, False), (1031, False), (1089, False)])
def test_trip_weights_and_travel_give_the_bits_of_the_dense_calls_on_the_upload_route(cpm, Z, negative):
    dm, dist = _datamatrix(Z, TU, negative)
    assert np.isfinite(dm).all() and np.isfinite(dist).all() and bool((dm[..., 0] < 0).any()) == negative
    fleets = _fleet_tables(Z, TU, 3)
    with _upload(cpm, Z, dm=True, negative=negative) as s, _upload(cpm, Z, dm=True, negative=negative) as d:
        builds = s.expected_trip_builds()
        w = _trip_dev(s, True)
        assert np.array_equal(w, _trip_dev(d, False))
        assert np.isfinite(w.view(np.float64)).all() and w.view(np.float64).any()
        for c in (s, d):
            c.set_p_drive_batch(fleets)
        for B in (0, 3):
            got, want = _travel_dev(s, True, B), _travel_dev(d, False, B)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (Z, B)
        a, b = s.expected_travel(S.pi0_with_zeros(Z), ivp=False, sparse=True), d.expected_travel(S.pi0_with_zeros(Z), ivp=False)
        assert all(_same(a[k], b[k]) for k in a)
        assert s.expected_trip_builds() == builds == 0 and d.expected_trip_builds() == 1      # the counter counts dense builds only


@gpu
def test_trip_weights_and_travel_on_the_dataset_route(cpm):
    with _from_dataset(cpm) as s, _from_dataset(cpm) as d:
        assert np.array_equal(_trip_dev(s, True), _trip_dev(d, False))
        got, want = _travel_dev(s, True), _travel_dev(d, False)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0 and s.expected_trip_builds() == 0


# ------------------------------------------------------------------------------------------------ 5: fit
def _fit_dev(s, fleets, ivp, sparse, pi0=None):
    import torch
    Z, Tc, B = s.Z, s.T, len(fleets)
    bufs = {k: _guarded(n) for k, n in dict(record=B * s.fit_words(), expected=B * 2 * Tc * Z, cotangent=B * 2 * Tc * Z, grad_p_drive=B * Tc * Z).items()}
    at = lambda k: bufs[k].data_ptr() + 8 * GUARD
    d_pi0 = _dev(pi0)
    torch.cuda.synchronize()
    s.expected_fit_dev([f[0] for f in fleets], [f[1] for f in fleets], [f[2] for f in fleets], np.array([f[3] for f in fleets]), at("record"), _ptr(d_pi0),
                       ivp, False, at("expected"), at("cotangent"), at("grad_p_drive"), 0, sparse=sparse)
    s.sync()
    return {k: _body(b) for k, b in bufs.items()}


@gpu
@pytest.mark.parametrize("route", ["dataset", "upload"])
def test_fit_gives_the_bits_of_the_dense_fit(cpm, route):
    if route == "dataset":
        make = lambda: _from_dataset(cpm)
    else:
        def make():
            s = _upload(cpm, 403, dm=True)
            m_act, m_park = _measured(403, TU)
            s.set_measured_activity(m_act)
            s.set_measured(m_park)
            return s
    single = [(0.10, 0.90, 0.5, w) for w in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.7, 1.3, 2.1))]    # every objective weighed in turn
    with make() as s, make() as d:
        for ivp in (False, True):
            for fleets in [[f] for f in single] + [FLEETS]:
                got, want = _fit_dev(s, fleets, ivp, True), _fit_dev(d, fleets, ivp, False)
                for k in got:
                    assert np.array_equal(got[k], want[k]), (route, ivp, len(fleets), fleets[0][3], k)
        pi0 = S.pi0_with_zeros(s.Z)
        got, want = _fit_dev(s, FLEETS[:3], True, True, pi0), _fit_dev(d, FLEETS[:3], True, False, pi0)
        assert all(np.array_equal(got[k], want[k]) for k in got)
        a = s.expected_fit([f[0] for f in FLEETS], [f[1] for f in FLEETS], [f[2] for f in FLEETS], np.array([f[3] for f in FLEETS]),
                           want=("expected", "cotangent", "grad_p_drive"), sparse=True)
        b = d.expected_fit([f[0] for f in FLEETS], [f[1] for f in FLEETS], [f[2] for f in FLEETS], np.array([f[3] for f in FLEETS]),
                           want=("expected", "cotangent", "grad_p_drive"))
        assert a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
        if route == "dataset":
            assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0
        # CPM_FIT_DEST is refused, by the library itself
        L, h = s._L, s._h
        one = np.array([0.1]), np.array([0.9]), np.array([0.5]), np.array([1.0, 0.0, 0.0])
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        rec = np.zeros(s.fit_words())
        rc = L.cpm_expected_sparse_fit(h, 1, vp(one[0]), vp(one[1]), vp(one[2]), None, 0x100, vp(one[3]), vp(rec), None, None, None, None)
        assert rc == ERR_ARG and b"dense" in L.cpm_last_error() and b"tangent" in L.cpm_last_error() and not rec.any()
        rc = L.cpm_expected_sparse_fit(h, 1, vp(one[0]), vp(one[1]), vp(one[2]), None, 0, vp(one[3]), vp(rec), None, None, None, vp(rec))
        assert rc == ERR_ARG                                          # grad_dest without CPM_FIT_DEST, as the namesake


# ------------------------------------------------------------------------------------------------ 6: residency
@gpu
def test_no_sparse_call_expands_the_dense_array_on_the_dataset_route(cpm):
    from carparkingmaps_amd import model_selection as M
    cot, gn = _cots(358, 24, 2, 9)
    gp, gd = np.asfortranarray(cot[0, 0].T), np.asfortranarray(cot[0, 1].T)
    with _from_dataset(cpm) as s:
        dense = lambda: s.get_info(cpm.CPM_INFO_P_DENSE)
        s.build_p_drive_batch([0.1, 0.2], [0.9, 0.8], [0.5, 1.0])
        steps = [("grad", lambda: s.expected_grad(gp, gd, ivp=True, g_next=gn[0], sparse=True)),
                 ("grad batch", lambda: s.expected_grad_batch(np.stack([gp, gp], axis=2), np.stack([gd, gd], axis=2), ivp=True, sparse=True)),
                 ("trip", lambda: s.expected_trip(sparse=True)),
                 ("travel", lambda: (s.expected_travel(sparse=True), s.expected_travel_batch(sparse=True))),
                 ("fit", lambda: s.expected_fit([0.1, 0.2], [0.9, 0.8], [0.5, 1.0], [1.0, 1.0, 1.0], ivp=True, sparse=True))]
        for name, call in steps:
            assert dense() == 0, name
            call()
            assert dense() == 0, f"{name} expanded the dense array"
        assert s.expected_trip_builds() == 0
    dm, dist = _dataset()
    m_act, m_park = _measured(358, 24)
    pts = [M.Point(0.5, 0.1, 0.9, 2), M.Point(0.7, 0.05, 0.8, 2)]
    with cpm.Sampler(358, 24) as s:
        s.set_datamatrix(dm, dist)
        ev = M.Evaluator(s, 3580, SEED, measured_activity=m_act, measured_parking=m_park, expected_sparse=True)
        dense = lambda: s.get_info(cpm.CPM_INFO_P_DENSE)
        ev.evaluate_expected(pts[0])                                   # (fails on the parent without touching a new symbol)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0 and dense() == 0, "evaluate_expected expanded the dense array"
        ev.evaluate_expected_batch(pts)
        assert dense() == 0
        for objective in ("activity_error", "parking_error", "A_drive"):
            ev.expected_gradient(pts[0], objective)
            assert dense() == 0, objective
        ev.expected_gradient_batch(pts, "A_drive")
        assert dense() == 0
        ev.expected_fit(pts, {"activity_error": 1.0, "parking_error": 1.0, "A_drive": 1.0})
        assert dense() == 0
        out = M.refine_expected(ev, pts, {"activity_error": 1.0, "A_drive": 0.5}, steps=3)
        assert dense() == 0 and len(out) == 2, "refine_expected expanded the dense array"
    with _upload(cpm, 403, dm=True) as s:                              # the upload route keeps its array
        s.expected_trip(sparse=True)
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 1


# ------------------------------------------------------------------------------------------------ 7: the caches follow their inputs
@gpu
def test_sparse_trip_weights_follow_new_tables_datamatrix_and_distances(cpm):
    dm, dist = _dataset()
    with _from_dataset(cpm, 2) as s:
        first = _trip_dev(s, True)
        s.build_p_dest(1.5, want=False)                                # another e_dest
        got = _trip_dev(s, True)
        with _from_dataset(cpm, 1.5) as d:
            assert np.array_equal(got, _trip_dev(d, False))
        assert not np.array_equal(got, first)
        dist2 = np.asfortranarray(np.array(dist) * 1.25)               # new distances
        s.set_distance(dist2)
        got = _trip_dev(s, True)
        with _from_dataset(cpm, 1.5) as d:
            d.set_distance(dist2)
            assert np.array_equal(got, _trip_dev(d, False))
        dm2 = np.array(dm, order="F")                                  # a new datamatrix (the tables go with it: built again)
        dm2[..., 0] *= 1.5
        for c in (s,):
            c.set_datamatrix(dm2, dist2)
            c.build_p_dest(1.5, want=False)
        got2 = _trip_dev(s, True)
        with cpm.Sampler(358, 24) as d:
            d.set_datamatrix(dm2, dist2)
            d.build_p_drive(0.1, 0.9, 0.5, want=False)
            d.build_p_dest(1.5, want=False)
            assert np.array_equal(got2, _trip_dev(d, False))
        assert not np.array_equal(got2, got)
        assert s.expected_trip_builds() == 0 and s.get_info(cpm.CPM_INFO_P_DENSE) == 0
    Z = 403
    _, p_b, _ = S.sparse_tables(Z, TU, seed=8)
    with _upload(cpm, Z, dm=True) as s:
        a = _trip_dev(s, True)
        s.set_p_dest(p_b)                                              # another uploaded table
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        b = _trip_dev(s, True)
        with _upload(cpm, Z, dm=True, p_dest=p_b) as d:
            assert np.array_equal(b, _trip_dev(d, False))
        assert not np.array_equal(a, b) and s.expected_trip_builds() == 0


# ------------------------------------------------------------------------------------------------ 8: no trace
@gpu
def test_sparse_calls_leave_no_trace_in_any_later_call(cpm, O):
    Z, cpz = 403, 50
    C = Z * cpz
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SEED, zone0)
    cot, gn = _cots(Z, TU, 3, 1)
    gp, gd = np.asfortranarray(cot[0, 0].T), np.asfortranarray(cot[0, 1].T)
    gp3, gd3 = np.asfortranarray(cot[:, 0].transpose(2, 1, 0)), np.asfortranarray(cot[:, 1].transpose(2, 1, 0))
    m_act, m_park = _measured(Z, TU)
    fit = lambda c, **kw: c.expected_fit([f[0] for f in FLEETS[:3]], [f[1] for f in FLEETS[:3]], [f[2] for f in FLEETS[:3]],
                                         np.array([f[3] for f in FLEETS[:3]]), ivp=True, want=("expected", "cotangent", "grad_p_drive"), **kw)
    with _upload(cpm, Z, dm=True) as s, _upload(cpm, Z, dm=True) as d:
        for c in (s, d):
            c.set_measured_activity(m_act)
            c.set_measured(m_park)
            c.set_p_drive_batch(_fleet_tables(Z, TU, 3))
        s.init_states(C, cpz)
        s.expected_grad(gp, gd, ivp=True, g_next=gn[0], sparse=True)
        s.expected_grad_batch(gp3, gd3, sparse=True)
        s.expected_trip(sparse=True)
        s.expected_travel(sparse=True)
        s.expected_travel_batch(ivp=True, sparse=True)
        assert np.array_equal(s.solve_ivp(SEED), ref["zone0"])
        s.expected_grad(gp, gd, sparse=True)
        r = s.resample(SEED)
        assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])
        step = s.last_step()
        fit(s, sparse=True)
        s.expected_grad_batch(gp3, gd3, ivp=True, sparse=True)
        assert s.last_step() == step
        for c in (s, d):                                               # (the fit installs its points as the batch tables: the same in both)
            c.set_p_drive_batch(_fleet_tables(Z, TU, 3))
        pi0 = S.pi0_with_zeros(Z)
        pairs = [(s.expected(pi0, ivp=True, want_next=True), d.expected(pi0, ivp=True, want_next=True)),
                 (tuple(s.expected_grad(gp, gd, pi0, ivp=True, g_next=gn[0]).values()), tuple(d.expected_grad(gp, gd, pi0, ivp=True, g_next=gn[0]).values())),
                 (tuple(s.expected_grad_batch(gp3, gd3).values()), tuple(d.expected_grad_batch(gp3, gd3).values())),
                 (s.expected_trip(), d.expected_trip())]
        for here, never in pairs:
            assert all(_same(a, b) for a, b in zip(here, never))
        here, never = fit(s), fit(d)
        assert here.keys() == never.keys() and all(_same(here[k], never[k]) for k in here)
        assert s.expected_trip_builds() == d.expected_trip_builds() == 1


# ------------------------------------------------------------------------------------------------ 9: refusals
@gpu
def test_refusals(cpm):
    import torch
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    gp, gd, gn = G.signed_cotangents(Z, TU, 3)
    gp3, gd3 = np.asfortranarray(np.stack([gp, gp], axis=2)), np.asfortranarray(np.stack([gd, gd], axis=2))
    fit = lambda c: c.expected_fit(0.1, 0.9, 0.5, [0.0, 0.0, 1.0], sparse=True)
    with _upload(cpm, Z, sparse=False, dm=True) as s:                   # dense tables: CPM_ERR_STATE, the two routes named
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        s.set_p_drive_batch(_fleet_tables(Z, TU, 2))
        for call in (lambda: s.expected_grad(gp, gd, sparse=True), lambda: s.expected_grad_batch(gp3, gd3, sparse=True),
                     lambda: s.expected_trip(sparse=True), lambda: s.expected_travel(sparse=True), lambda: s.expected_travel_batch(sparse=True),
                     lambda: fit(s)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "cpm_build_p_dest" in str(e.value) and "CPM_OPT_SPARSE_UPLOAD" in str(e.value)
        s.expected_grad(gp, gd)                                        # (the dense calls are untouched by the refusals)
        assert s.expected_trip_builds() == 0
    with _upload(cpm, Z) as s:                                         # sparse tables, but no batch tables, datamatrix or distances
        for call in (lambda: s.expected_grad_batch(gp3, gd3, sparse=True), lambda: s.expected_travel_batch(sparse=True)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "batch" in str(e.value)
        for call in (lambda: s.expected_trip(sparse=True), lambda: s.expected_travel(sparse=True), lambda: fit(s)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "datamatrix" in str(e.value)
    with _upload(cpm, Z, dm=True, dist=False) as s:                    # sparse tables and a datamatrix, but no distance matrix
        for call in (lambda: s.expected_trip(sparse=True), lambda: s.expected_travel(sparse=True), lambda: fit(s)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE and "distance matrix" in str(e.value)
        s.set_p_drive_batch(_fleet_tables(Z, TU, 2))
        with pytest.raises(cpm.CpmError) as e:
            s.expected_travel_batch(sparse=True)
        assert e.value.status == ERR_STATE and "distance matrix" in str(e.value)
        s.expected_grad(gp, gd, sparse=True)                           # (the adjoint needs neither)
    with _upload(cpm, Z) as s:
        L, h = s._L, s._h
        buf = torch.zeros(4 * Z * TU, dtype=torch.float64, device="cuda")
        p = ctypes.c_void_p(buf.data_ptr())
        assert L.cpm_expected_sparse_grad_dev(h, None, 0, None, None, p, None) == ERR_ARG            # NULL cotangent
        assert L.cpm_expected_sparse_grad_dev(h, None, 0, p, None, None, None) == ERR_ARG            # NULL output
        assert L.cpm_expected_sparse_grad_dev(h, None, 2, p, None, p, None) == ERR_ARG               # unknown flag bits
        assert L.cpm_expected_sparse_grad_batch_dev(h, None, 4, p, None, p, None) == ERR_ARG
        assert L.cpm_expected_sparse_trip_dev(h, None) == ERR_ARG
        assert L.cpm_expected_sparse_travel_dev(h, p, 1, None, None) == ERR_ARG
        assert L.cpm_expected_sparse_travel_dev(h, p, 0, p, None) == ERR_ARG
        assert not buf.cpu().numpy().any()
        bad = np.array(gd)
        bad[3, 1] = np.inf
        for call in (lambda: s.expected_grad(gp, bad, sparse=True), lambda: s.expected_grad(gp, gd, g_next=np.full(Z, np.nan), sparse=True)):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_ARG and "finite" in str(e.value)
        s.set_p_drive_batch(_fleet_tables(Z, TU, 2))
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad_batch(gp3, np.asfortranarray(np.stack([gd, bad], axis=2)), sparse=True)
        assert e.value.status == ERR_ARG and "fleet 2" in str(e.value)
        big = np.array(p_dest)
        big[2, :, 1] *= 2.5                                            # a row total above 1: the dense call's text
        s.set_p_dest(big)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad(gp, gd, sparse=True)
        assert e.value.status == ERR_TABLE and "hour 2, origin 3" in str(e.value)
        text = str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_grad(gp, gd)
        assert e.value.status == ERR_TABLE and str(e.value) == text


# ------------------------------------------------------------------------------------------------ 10: Python
@gpu
def test_sampler_keywords_against_their_dense_forms(cpm):
    Z = 518
    cot, gn = _cots(Z, TU, 3, 4)
    gp, gd = np.asfortranarray(cot[0, 0].T), np.asfortranarray(cot[0, 1].T)
    gp3, gd3 = np.asfortranarray(cot[:, 0].transpose(2, 1, 0)), np.asfortranarray(cot[:, 1].transpose(2, 1, 0))
    pi0 = S.pi0_with_zeros(Z)
    m_act, m_park = _measured(Z, TU)
    with _upload(cpm, Z, dm=True) as s, _upload(cpm, Z, dm=True) as d:
        for c in (s, d):
            c.set_p_drive_batch(_fleet_tables(Z, TU, 3))
            c.set_measured_activity(m_act)
            c.set_measured(m_park)
        for ivp in (False, True):
            a, b = s.expected_grad(gp, gd, pi0, ivp, gn[0], sparse=True), d.expected_grad(gp, gd, pi0, ivp, gn[0])
            assert all(_same(a[k], b[k]) for k in a)
            a, b = s.expected_grad_batch(gp3, gd3, pi0, ivp, gn.T, sparse=True), d.expected_grad_batch(gp3, gd3, pi0, ivp, gn.T)
            assert all(_same(a[k], b[k]) for k in a)
            a, b = s.expected_travel(pi0, ivp, sparse=True), d.expected_travel(pi0, ivp)
            assert all(_same(a[k], b[k]) for k in a)
            a, b = s.expected_travel_batch(pi0, ivp, sparse=True), d.expected_travel_batch(pi0, ivp)
            assert all(_same(a[k], b[k]) for k in a)
        assert all(_same(x, y) for x, y in zip(s.expected_trip(sparse=True), d.expected_trip()))
        with pytest.raises(ValueError):
            s.expected_grad_batch(gp3, gd3, dest=True, sparse=True)


@gpu
def test_evaluator_with_expected_sparse_gives_the_default_evaluators_gradients_and_fit_bit_for_bit(cpm):
    from carparkingmaps_amd import model_selection as M
    dm, dist = _dataset()
    m_act, m_park = _measured(358, 24)
    pts = [M.Point(0.5, 0.1, 0.9, 2), M.Point(0.7, 0.05, 0.8, 2), M.Point(0.4, 0.2, 0.95, 2)]
    w = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}
    res = {}
    for sparse in (True, False):
        with cpm.Sampler(358, 24) as s:
            s.set_datamatrix(dm, dist)
            ev = M.Evaluator(s, 3580, SEED, measured_activity=m_act, measured_parking=m_park, expected_sparse=sparse)
            out = [ev.expected_gradient(pts[0], k) for k in ("activity_error", "parking_error", "A_drive")]
            out += ev.expected_gradient_batch(pts, "A_drive") + ev.expected_gradient_batch(pts, "parking_error")
            out += ev.expected_fit(pts, w)
            assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0 and s.get_info(cpm.CPM_INFO_P_DENSE) == (0 if sparse else 1)
            res[sparse] = out
    for a, b in zip(res[True], res[False]):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(a[k], str):
                assert a[k] == b[k]
            else:
                assert _same(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), k
