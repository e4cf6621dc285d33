"""The expected densities straight from sparse tables (include/cpm_expected_sparse.h) on the GPU.  Every comparison is array_equal
against the dense call (include/cpm_expected.h) on a second, fresh context with the same tables: the contract is bit equality.  Every
test first asserts CPM_INFO_SPARSE_TABLES > 0, so a table that fell back to dense packs fails loudly.

Upload route (CPM_OPT_SPARSE_UPLOAD, the hand-made tables of expected_sparse_reference.sparse_tables, T = 3 so that both alignments of
an odd Z's rows occur at every destination): Z = 403 (odd, below one lane wrap), 518 (even, just past the wrap at 512 origins), 1,031
(odd, two wraps, Z % 4 = 3: the last workgroup is partial).  All three qualify for sparse packs under the 60 % rule (rows of 16 to 45
cells: the sparse pack is the 256-word minimum against 516, 708 and 1,348 dense words).  Dataset route: Z = 358, T = 24, density 0.06 as
tests/test_expected_gpu.py uses; its compact rows keep cells of weight 0."""
import functools

import numpy as np
import pytest

import expected_sparse_reference as S

gpu = pytest.mark.gpu
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_ARG, ERR_STATE, ERR_TABLE = -1, -3, -4
TU = 3
SEED = 20240611


def _upload(cpm, Z, Tc, p_drive, p_dest, sparse=True):
    s = cpm.Sampler(Z, Tc)
    s.set_sparse_upload(sparse)
    s.set_p_drive(p_drive)
    s.set_p_dest(p_dest)
    if sparse:
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0, "the table fell back to dense packs"
    return s


@functools.lru_cache(maxsize=None)
def _dataset(Z=358, Tc=24):
    from oracle import oracle as O
    O.build()
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.06)
    for a in (dm, dist):
        a.setflags(write=False)
    return dm, dist


def _from_dataset(cpm, e_dest=2, Z=358, Tc=24):
    dm, dist = _dataset(Z, Tc)
    s = cpm.Sampler(Z, Tc)
    s.set_datamatrix(dm, dist)
    s.build_p_drive(0.1, 0.9, 0.5, want=False)
    s.build_p_dest(e_dest, want=False)
    assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0, "the table fell back to dense packs"
    return s


def _dev_call(s, pi0, ivp, sparse, want_next=True, batch=0):
    """expected[_batch]_dev between guard words on sentinel-filled outputs: every word written, none outside.  -> (out [B][2][T][Z], next)"""
    import torch
    Z, Tc, B = s.Z, s.T, max(batch, 1)
    out = torch.full((2 * GUARD + B * s.expected_words(),), SENT, dtype=torch.int64, device="cuda")
    nxt = torch.full((2 * GUARD + Z,), SENT, dtype=torch.int64, device="cuda")
    d_pi0 = None if pi0 is None else torch.from_numpy(np.ascontiguousarray(pi0)).cuda()
    torch.cuda.synchronize()
    p0 = 0 if pi0 is None else d_pi0.data_ptr()
    if batch:
        s.expected_batch_dev(out.data_ptr() + 8 * GUARD, p0, ivp, sparse=sparse)
    else:
        s.expected_dev(out.data_ptr() + 8 * GUARD, p0, ivp, nxt.data_ptr() + 8 * GUARD if want_next else 0, sparse=sparse)
    s.sync()
    out, nxt = out.cpu().numpy(), nxt.cpu().numpy()
    for a in (out, nxt):
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
    body = out[GUARD:-GUARD]
    assert not np.any(body == SENT), "a word of d_out was not written"
    if want_next and not batch:
        assert not np.any(nxt[GUARD:-GUARD] == SENT)
    else:
        assert np.all(nxt == SENT)
    return body.reshape(B, 2, Tc, Z), nxt[GUARD:-GUARD]           # (int64 views of the f64 words: equality is bit equality)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _sane(out):
    park = out.view(np.float64)[:, 0]
    assert np.all(np.isfinite(park)) and np.all(park >= 0.0) and park.sum() > 0.0


# ------------------------------------------------------------------------------------------------ 1: upload route
@gpu
@pytest.mark.parametrize("Z", [403, 518, 1031])
def test_upload_route_gives_the_bits_of_the_dense_call(cpm, Z):
    p_drive, p_dest, info = S.sparse_tables(Z, TU)
    assert (p_dest[:, info["full"], TU - 1] > 0).all() and not p_dest[:, info["empty"], :].any()
    assert not p_dest[info["zero"], :, 0].any() and (p_dest[info["half"]].sum(axis=1) < 0.75).all()
    with _upload(cpm, Z, TU, p_drive, p_dest) as s, _upload(cpm, Z, TU, p_drive, p_dest) as d:
        for pi0 in (None, S.pi0_with_zeros(Z)):
            for ivp in (False, True):
                got = _dev_call(s, pi0, ivp, True)
                want = _dev_call(d, pi0, ivp, False)
                assert _same(got, want), (Z, pi0 is None, ivp)
                _sane(got[0])
                assert _same(_dev_call(s, pi0, ivp, True), got), "repeated calls give the same bits"
                assert _same((_dev_call(s, pi0, ivp, True, want_next=False)[0],), (got[0],))
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0 and d.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0


# ------------------------------------------------------------------------------------------------ 2: dataset route
@gpu
def test_dataset_route_never_expands_the_dense_array(cpm):
    with _from_dataset(cpm) as s, _from_dataset(cpm) as d:
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0
        first = _dev_call(s, None, True, True)
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0, "the sparse call expanded the dense array"
        _sane(first[0])
        want = _dev_call(d, None, True, False)                      # a fresh context's dense call
        assert d.get_info(cpm.CPM_INFO_P_DENSE) == 1
        assert _same(first, want)
        dense_here = _dev_call(s, None, True, False)                # the dense call on the same context
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 1
        assert _same(dense_here, first)
        assert _same(_dev_call(s, None, True, True), first)         # and the sparse call again
        pi0 = S.pi0_with_zeros(s.Z)
        assert _same(_dev_call(s, pi0, False, True), _dev_call(d, pi0, False, False))


@gpu
def test_info_p_dense_on_dense_and_uploaded_tables(cpm):
    Z = 67
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    with cpm.Sampler(Z, TU) as s:
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0                # no tables yet
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0 and s.get_info(cpm.CPM_INFO_P_DENSE) == 1
    p_drive, p_dest, _ = S.sparse_tables(403, TU)
    with _upload(cpm, 403, TU, p_drive, p_dest) as s:
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 1                # (the uploaded array stays resident)


# ------------------------------------------------------------------------------------------------ 3: batch
@gpu
@pytest.mark.parametrize("B", [1, 2, 3, 5, 8, 9, 17])
def test_fleet_b_of_a_sparse_batch_is_the_single_sparse_call_and_the_dense_batch(cpm, B):
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    fleets = np.asfortranarray(np.random.default_rng(B).uniform(0.0, 1.0, (Z, TU, B)))
    fleets[:5, 1, 0] = [np.nan, -0.1, 0.0, 1.0, 1.5]
    pi0 = S.pi0_with_zeros(Z)
    with _upload(cpm, Z, TU, p_drive, p_dest) as s, _upload(cpm, Z, TU, p_drive, p_dest) as d:
        for c in (s, d):
            c.set_p_drive_batch(fleets)
        for ivp in (False, True):
            got, _ = _dev_call(s, pi0, ivp, True, batch=B)
            want, _ = _dev_call(d, pi0, ivp, False, batch=B)
            assert np.array_equal(got, want), (B, ivp)
            for b in range(B):
                s.set_p_drive(fleets[:, :, b])
                one, _ = _dev_call(s, pi0, ivp, True)
                assert np.array_equal(one[0], got[b]), (B, b, ivp)


# ------------------------------------------------------------------------------------------------ 4: the per-table arrays
@gpu
@pytest.mark.parametrize("route", ["upload", "dataset"])
def test_per_table_arrays_are_word_for_word_those_of_the_dense_builder(cpm, route):
    if route == "upload":
        p_drive, p_dest, info = S.sparse_tables(1031, TU)
        make = lambda: _upload(cpm, 1031, TU, p_drive, p_dest)
    else:
        make = lambda: _from_dataset(cpm)
    with make() as s, make() as d:
        sparse = s.expected_sparse_aux(True)
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == (1 if route == "upload" else 0)
        dense = d.expected_sparse_aux(False)
        for name, a, b in zip(("ell", "r", "start", "list"), sparse, dense):
            assert np.array_equal(a.view(np.int32 if a.dtype == np.int32 else np.int64), b.view(np.int32 if b.dtype == np.int32 else np.int64)), name
        ell, r, start, lst = sparse
        Z = s.Z
        assert ell.min() >= 0 and ell.max() <= Z and (ell != Z - 1).mean() > 0.5      # rows end early: lists all over the destinations
        assert (start[:, 0] == 0).all() and (np.diff(start, axis=1) >= 0).all()
        assert all(sorted(lst[t]) == list(range(Z)) for t in range(s.T))
        if route == "upload":
            assert (ell[:TU - 1, info["zero"]] == Z).all() and (r[:, info["half"]] > 0.25).all()
        both = s.expected_sparse_aux(False)                             # the dense builder on the same context: the same words again
        assert all(np.array_equal(a, b) for a, b in zip(both[:1] + both[2:], dense[:1] + dense[2:])) and np.array_equal(both[1].view(np.int64), dense[1].view(np.int64))


# ------------------------------------------------------------------------------------------------ 5: no trace
@gpu
def test_sparse_calls_leave_no_trace_in_a_later_resample_or_dense_call(cpm, O):
    Z, cpz = 403, 50
    C = Z * cpz
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SEED, zone0)
    with _upload(cpm, Z, TU, p_drive, p_dest) as s, _upload(cpm, Z, TU, p_drive, p_dest) as d:
        s.init_states(C, cpz)
        s.set_p_drive_batch(np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (Z, TU, 3))))
        s.expected(sparse=True)
        s.expected(ivp=True, sparse=True)
        s.expected_batch(sparse=True)
        assert np.array_equal(s.solve_ivp(SEED), ref["zone0"])
        s.expected(sparse=True)
        r = s.resample(SEED)
        assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])
        step = s.last_step()
        s.expected(sparse=True)
        assert s.last_step() == step
        here = s.expected(S.pi0_with_zeros(Z), ivp=True, want_next=True)
        never = d.expected(S.pi0_with_zeros(Z), ivp=True, want_next=True)           # a context that never made a sparse call
        assert all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(here, never))


# ------------------------------------------------------------------------------------------------ 6: the cache follows the tables
@gpu
def test_sparse_call_follows_a_new_table(cpm):
    pi0 = S.pi0_with_zeros(358)
    with _from_dataset(cpm, 2) as s:
        first = _dev_call(s, pi0, False, True)
        s.build_p_dest(1.5, want=False)                                  # another e_dest
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        got = _dev_call(s, pi0, False, True)
        assert s.get_info(cpm.CPM_INFO_P_DENSE) == 0
        with _from_dataset(cpm, 1.5) as d:
            assert _same(got, _dev_call(d, pi0, False, False))
        assert not _same(got, first)
        s.refresh_tables()
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        assert _same(_dev_call(s, pi0, False, True), got)
    Z = 403
    p_drive, p_a, _ = S.sparse_tables(Z, TU)
    _, p_b, _ = S.sparse_tables(Z, TU, seed=8)
    pi0 = S.pi0_with_zeros(Z)
    with _upload(cpm, Z, TU, p_drive, p_a) as s:
        a = _dev_call(s, pi0, True, True)
        s.set_p_dest(p_b)                                                # another table
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        b = _dev_call(s, pi0, True, True)
        with _upload(cpm, Z, TU, p_drive, p_b) as d:
            assert _same(b, _dev_call(d, pi0, True, False))
        assert not _same(a, b)
        s.refresh_tables()
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        assert _same(_dev_call(s, pi0, True, True), b)


# ------------------------------------------------------------------------------------------------ 7: refusals
@gpu
def test_refusals(cpm):
    import ctypes
    import torch
    Z = 403
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    with cpm.Sampler(Z, TU) as s:                                        # dense tables
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        with pytest.raises(cpm.CpmError) as e:
            s.expected(sparse=True)
        assert e.value.status == ERR_STATE and "cpm_build_p_dest" in str(e.value) and "CPM_OPT_SPARSE_UPLOAD" in str(e.value)
        s.expected()                                                     # (the dense call is untouched by the refusal)
    with cpm.Sampler(Z, TU) as s:                                        # no tables at all, then no p_dest
        s.set_sparse_upload(True)
        for call in (s.expected, s.expected_batch):
            with pytest.raises(cpm.CpmError) as e:
                call(sparse=True)
            assert e.value.status == ERR_STATE
        s.set_p_drive(p_drive)
        with pytest.raises(cpm.CpmError) as e:
            s.expected(sparse=True)
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        s.set_p_dest(p_dest)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        with pytest.raises(cpm.CpmError) as e:                           # no batch tables
            s.expected_batch(sparse=True)
        assert e.value.status == ERR_STATE and "batch" in str(e.value)
        out = torch.zeros(s.expected_words(), dtype=torch.float64, device="cuda")
        L, h = s._L, s._h
        assert L.cpm_expected_sparse_dev(h, None, 2, ctypes.c_void_p(out.data_ptr()), None) == ERR_ARG      # unknown flag bits
        assert L.cpm_expected_sparse_dev(h, None, 0, None, None) == ERR_ARG                                   # NULL d_out
        assert L.cpm_expected_sparse_batch_dev(h, None, 0, None) == ERR_ARG
        assert L.cpm_expected_sparse_batch_dev(h, None, 4, ctypes.c_void_p(out.data_ptr())) == ERR_ARG
        big = np.array(p_dest)
        big[2, :, 1] *= 2.5                                              # (a residual row or not: its total is above 1 now)
        assert big[2, :, 1].sum() > 1.01
        s.set_p_dest(big)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        for _ in range(2):                                               # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected(sparse=True)
            assert e.value.status == ERR_TABLE and "hour 2, origin 3" in str(e.value)
        sparse_text = str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected()
        assert e.value.status == ERR_TABLE and str(e.value) == sparse_text
        s.set_p_dest(p_dest)
        park, _ = s.expected(sparse=True)
        assert np.all(np.isfinite(park))
        bad = np.full(Z, 1.0 / Z)
        bad[3] = np.nan
        with pytest.raises(cpm.CpmError) as e:
            s.expected(bad, sparse=True)
        assert e.value.status == ERR_ARG


# ------------------------------------------------------------------------------------------------ 8: Python
@gpu
def test_sampler_keywords_against_their_dense_forms(cpm):
    Z = 518
    p_drive, p_dest, _ = S.sparse_tables(Z, TU)
    fleets = np.asfortranarray(np.random.default_rng(5).uniform(0.0, 1.0, (Z, TU, 3)))
    pi0 = S.pi0_with_zeros(Z)
    bits = lambda arrays: [np.asarray(a).view(np.int64) for a in arrays]
    with _upload(cpm, Z, TU, p_drive, p_dest) as s, _upload(cpm, Z, TU, p_drive, p_dest) as d:
        for c in (s, d):
            c.set_p_drive_batch(fleets)
        for ivp in (False, True):
            assert _same(bits(s.expected(pi0, ivp, want_next=True, sparse=True)), bits(d.expected(pi0, ivp, want_next=True)))
            assert _same(bits(s.expected_batch(pi0, ivp, sparse=True)), bits(d.expected_batch(pi0, ivp)))
        assert _same(bits(s.expected(sparse=True)), bits(d.expected()))


@gpu
def test_evaluator_with_expected_sparse_gives_the_default_evaluators_results_bit_for_bit(cpm):
    from carparkingmaps_amd import model_selection as M
    dm, dist = _dataset()
    pts = [M.Point(0.5, 0.1, 0.9, 2), M.Point(0.7, 0.05, 0.8, 2), M.Point(0.4, 0.2, 0.95, 2)]
    res = {}
    for sparse in (True, False):
        with cpm.Sampler(358, 24) as s:
            s.set_datamatrix(dm, dist)
            ev = M.Evaluator(s, 358 * 10, SEED, expected_sparse=sparse)
            one = ev.evaluate_expected(pts[0])
            assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
            res[sparse] = [one] + ev.evaluate_expected_batch(pts)
    for a, b in zip(res[True], res[False]):
        assert a.keys() == b.keys()
        for k in a:
            x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
            assert np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64)), k
