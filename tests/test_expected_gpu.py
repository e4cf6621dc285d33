"""Expected parking and driving densities by Markov propagation (include/cpm_expected.h) on the GPU: the device against the exact
(rational) form of the definition within h * (Z + 8) * 2^-52, against the numpy form within twice that at the sizes the exact form is
too slow for, on uploaded, dataset-built and skewed tables; the same bits every time and fleet b of a batch bit for bit the single
call; the device sampler's counts within the 5.5 sigma cap; the errors, and no trace in a later resample.

Shapes: Z = 2, 5, 67 reach rows off a 16-byte boundary (odd Z) and a last tile of rows that is not full; Z = 192 has fewer pairs than
a workgroup has lanes, Z = 513 more, Z = 1,031 more than one round of the unrolled loop (2 x 256 pairs)."""
import functools

import numpy as np
import pytest

import expected_reference as R

gpu = pytest.mark.gpu
T = 24
SEED = 20240611
CAP = 5.5
GUARD = 16
SENT = 0x5A5A5A5A5A5A5A5A                    # as f64: 2.9e130, not a value the kernels write
ERR_STATE, ERR_TABLE = -3, -4
SPECIAL = [np.nan, -0.1, 0.0, 1.0, 1.5]      # p_drive entries the Bernoulli maps to 0, 0, 0, 1, 1


@functools.lru_cache(maxsize=None)
def _tables(Z, Tc, kind="modified"):
    """(p_drive, p_dest, row tables) -- computed once and shared; nobody writes to them"""
    from oracle import oracle as O
    O.build()
    if kind == "skewed":
        p_drive, p_dest = O.synth_p_drive(Z, Tc, 11), O.synth_p_dest_dense(Z, Tc, 11, skew_q=3)
    else:
        p_drive, p_dest = R.modified_tables(O, Z, Tc)
    k = min(Z, len(SPECIAL))
    p_drive[:k, 1 % Tc] = SPECIAL[:k]
    for a in (p_drive, p_dest):
        a.setflags(write=False)
    return p_drive, p_dest, R.row_tables(p_dest)


def _pi0(Z, kind):
    if kind == "uniform":
        return None
    if kind == "unit":
        e = np.zeros(Z)
        e[Z // 2] = 1.0
        return e
    return np.random.default_rng(Z).uniform(0.0, 2.0, Z)


def _sampler(cpm, Z, Tc, p_drive, p_dest):
    s = cpm.Sampler(Z, Tc)
    s.set_p_drive(p_drive)
    s.set_p_dest(p_dest)
    return s


def _tols(Z, Tc, flags):
    h = R.operators_behind(Tc, flags)
    return h, np.array([R.bound(Z, k) for k in h])[None, :], np.array([R.bound_driving(Z, k) for k in h])[None, :]


def _dev_call(s, pi0, ivp, want_next=True):
    """expected_dev between guard words on sentinel-filled outputs: every word written, none outside"""
    import torch
    Z, Tc = s.Z, s.T
    out = torch.full((2 * GUARD + s.expected_words(),), SENT, dtype=torch.int64, device="cuda")
    nxt = torch.full((2 * GUARD + Z,), SENT, dtype=torch.int64, device="cuda")
    d_pi0 = None if pi0 is None else torch.from_numpy(np.ascontiguousarray(pi0)).cuda()
    torch.cuda.synchronize()
    s.expected_dev(out.data_ptr() + 8 * GUARD, 0 if pi0 is None else d_pi0.data_ptr(), ivp, nxt.data_ptr() + 8 * GUARD if want_next else 0)
    s.sync()
    out, nxt = out.cpu().numpy(), nxt.cpu().numpy()
    for a in (out, nxt):
        assert np.all(a[:GUARD] == SENT) and np.all(a[-GUARD:] == SENT), "a store outside the output"
    body = out[GUARD:-GUARD]
    assert not np.any(body == SENT), "a word of d_out was not written"
    both = body.view(np.float64).reshape(2, Tc, Z)
    if want_next:
        assert not np.any(nxt[GUARD:-GUARD] == SENT)
    else:
        assert np.all(nxt == SENT)
    return both[0].T, both[1].T, nxt[GUARD:-GUARD].view(np.float64)


# ------------------------------------------------------------------------------------------------ 1: against the references
@gpu
@pytest.mark.parametrize("Tc", [1, 2, 24])
@pytest.mark.parametrize("Z", [2, 5, 67])
def test_device_meets_the_bound_against_the_exact_form(cpm, Z, Tc):
    p_drive, p_dest, tables = _tables(Z, Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        variants = ((0, "uniform"), (R.IVP, "given"), (0, "unit"), (R.IVP, "uniform"))
        for flags, kind in variants[:2] if Z * Tc > 1000 else variants:   # (the exact form of 47 operators at Z = 67 takes a second)
            pi0 = _pi0(Z, kind)
            park, drv, nxt = s.expected(pi0, ivp=bool(flags), want_next=True)
            epark, edrv, enxt = R.exact_expected(p_drive, p_dest, pi0, flags, tables)
            h, tp, td = _tols(Z, Tc, flags)
            wp, zp = R.worst_ratio(park, epark, tp)
            wd, zd = R.worst_ratio(drv, edrv, td)
            wn, zn = R.worst_ratio(nxt, enxt, R.bound(Z, h[-1] + 1))
            print(f"Z={Z} T={Tc} flags={flags} pi0={kind}: worst error / bound: parking {wp:.3f}, driving {wd:.3f}, pi_next {wn:.3f}")
            assert zp and zd and zn, "a word whose exact value is 0 is not 0"
            assert wp <= 1.0 and wd <= 1.0 and wn <= 1.0
            dpark, ddrv, dnxt = _dev_call(s, pi0, bool(flags))          # the asynchronous entry: the same bits
            assert np.array_equal(dpark, park) and np.array_equal(ddrv, drv) and np.array_equal(dnxt, nxt)
        _dev_call(s, None, False, want_next=False)


def _against_numpy(s, p_drive, p_dest, tables, what):
    Z, Tc = p_drive.shape
    for flags, kind in ((0, "uniform"), (R.IVP, "given")):
        pi0 = _pi0(Z, kind)
        park, drv, nxt = s.expected(pi0, ivp=bool(flags), want_next=True)
        npark, ndrv, nnxt = R.numpy_expected(p_drive, p_dest, pi0, flags, tables)
        h, tp, td = _tols(Z, Tc, flags)
        for name, got, want, tol in (("parking", park, npark, 2 * tp), ("driving", drv, ndrv, 2 * td), ("pi_next", nxt, nnxt, 2 * R.bound(Z, h[-1] + 1))):
            assert np.all(got[want == 0.0] == 0.0), name
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(want != 0.0, np.abs(got - want) / (tol * np.abs(want)), 0.0)
            ratio = np.where((tol == 0.0) & (got != want), np.inf, np.nan_to_num(ratio))
            print(f"{what} Z={Z} T={Tc} flags={flags}: {name} worst error / (2 x bound) {ratio.max():.3f}")
            assert ratio.max() <= 1.0, name


@gpu
@pytest.mark.parametrize("Z", [192, 513, 1031])
def test_device_meets_twice_the_bound_against_the_numpy_form(cpm, Z):
    Tc = 3
    p_drive, p_dest, tables = _tables(Z, Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        _against_numpy(s, p_drive, p_dest, tables, "uploaded")


@gpu
def test_skewed_tables(cpm):
    Z, Tc = 67, 24
    p_drive, p_dest, tables = _tables(Z, Tc, "skewed")
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        park, drv = s.expected()
        epark, edrv, _ = R.exact_expected(p_drive, p_dest, None, 0, tables)
        _, tp, td = _tols(Z, Tc, 0)
        (wp, zp), (wd, zd) = R.worst_ratio(park, epark, tp), R.worst_ratio(drv, edrv, td)
        print(f"skewed Z={Z}: worst error / bound: parking {wp:.3f}, driving {wd:.3f}")
        assert zp and zd and wp <= 1.0 and wd <= 1.0


@gpu
def test_tables_built_from_a_datamatrix_go_through_the_dense_array(cpm, O):
    """sparse row packs: the product reads the dense array that ensure_dense_p expands them to"""
    Z, Tc = 358, 24                                                 # (the compact-row route takes T = 24 only)
    dm, dist = O.synth_datamatrix(Z, Tc, 11, density=0.06)
    with cpm.Sampler(Z, Tc) as s:
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        s.build_p_dest(2, want=False)
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0       # (words of a sparse row pack; 0: dense packs)
        first = s.expected()                                       # (before anything else asked for the dense array)
        p_dest = s.build_p_dest(2, want=True)                      # the same tables again, and their array for the references
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0       # (words of a sparse row pack; 0: dense packs)
        tables = R.row_tables(p_dest)
        assert (tables[1] != Z - 1).mean() > 0.5                   # sparse rows end early: the residual lists lie all over the destinations
        _against_numpy(s, p_drive, p_dest, tables, "dataset")
        again = s.expected()
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


@gpu
@pytest.mark.parametrize("Z", [5, 67])
def test_pi_next_fed_back_is_a_two_day_evaluation(cpm, Z):
    Tc = 2
    p_drive, p_dest, tables = _tables(Z, Tc)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        _, _, nxt = s.expected(want_next=True)
        park2, drv2, nxt2 = s.expected(nxt, want_next=True)
        _, _, e1 = R.exact_expected(p_drive, p_dest, None, 0, tables)
        epark, edrv, e2 = R.exact_expected(p_drive, p_dest, e1, 0, tables)
        h = [Tc + t for t in range(Tc)]
        wp, zp = R.worst_ratio(park2, epark, np.array([R.bound(Z, k) for k in h])[None, :])
        wd, zd = R.worst_ratio(drv2, edrv, np.array([R.bound_driving(Z, k) for k in h])[None, :])
        wn, zn = R.worst_ratio(nxt2, e2, R.bound(Z, 2 * Tc))
        print(f"Z={Z}: day two, worst error / bound: parking {wp:.3f}, driving {wd:.3f}, pi_next {wn:.3f}")
        assert zp and zd and zn and wp <= 1.0 and wd <= 1.0 and wn <= 1.0


# ------------------------------------------------------------------------------------------------ 2: determinism and the batch contract
@gpu
@pytest.mark.parametrize("Z,Tc", [(67, 24), (513, 3)])
@pytest.mark.parametrize("B", [1, 3, 8, 9, 64])
def test_fleet_b_of_a_batch_gives_the_bits_of_the_single_call(cpm, Z, Tc, B):
    p_drive, p_dest, _ = _tables(Z, Tc)
    rng = np.random.default_rng(100 * B + Z)
    p_drives = np.asfortranarray(rng.uniform(0.0, 1.0, (Z, Tc, B)))
    p_drives[:, :, 0] = p_drive                                     # (the special entries ride along in fleet 0)
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_drive_batch(p_drives)
        for ivp in (False, True):
            park, drv = s.expected_batch(ivp=ivp)
            park2, drv2 = s.expected_batch(ivp=ivp)
            assert park.shape == drv.shape == (Z, Tc, B)
            assert np.array_equal(park, park2) and np.array_equal(drv, drv2)
            for b in range(B):
                s.set_p_drive(p_drives[:, :, b])
                one_p, one_d = s.expected(ivp=ivp)
                assert np.array_equal(one_p, park[:, :, b]) and np.array_equal(one_d, drv[:, :, b]), (b, ivp)
                if b == 0:
                    again_p, again_d = s.expected(ivp=ivp)
                    assert np.array_equal(one_p, again_p) and np.array_equal(one_d, again_d)
        same = np.asfortranarray(np.repeat(p_drives[:, :, :1], B, axis=2))
        s.set_p_drive_batch(same)
        park, drv = s.expected_batch(pi0=_pi0(Z, "given"))
        for b in range(1, B):
            assert np.array_equal(park[:, :, b], park[:, :, 0]) and np.array_equal(drv[:, :, b], drv[:, :, 0])


@gpu
def test_batch_dev_entry_writes_every_word_and_nothing_else(cpm):
    import torch
    Z, Tc, B = 67, 24, 9
    p_drive, p_dest, _ = _tables(Z, Tc)
    p_drives = np.asfortranarray(np.random.default_rng(3).uniform(0.0, 1.0, (Z, Tc, B)))
    with _sampler(cpm, Z, Tc, p_drive, p_dest) as s:
        s.set_p_drive_batch(p_drives)
        park, drv = s.expected_batch()
        out = torch.full((2 * GUARD + B * s.expected_words(),), SENT, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.expected_batch_dev(out.data_ptr() + 8 * GUARD)
        s.sync()
        out = out.cpu().numpy()
        assert np.all(out[:GUARD] == SENT) and np.all(out[-GUARD:] == SENT) and not np.any(out[GUARD:-GUARD] == SENT)
        got = out[GUARD:-GUARD].view(np.float64).reshape(B, 2, Tc, Z)
        for b in range(B):
            assert np.array_equal(got[b, 0].T, park[:, :, b]) and np.array_equal(got[b, 1].T, drv[:, :, b])


# ------------------------------------------------------------------------------------------------ 3: the sampler on the device
@gpu
@pytest.mark.parametrize("ivp", [False, True])
def test_device_sampler_lies_within_the_cap_of_the_device_expectation(cpm, ivp):
    Z, cpz = 67, 2000
    C = Z * cpz
    from oracle import oracle as O
    p_drive, p_dest = R.modified_tables(O, Z, T)
    with _sampler(cpm, Z, T, p_drive, p_dest) as s:
        s.init_states(C, cpz)
        if ivp:
            s.solve_ivp(SEED, want=False)
        r = s.resample(SEED)
        park, drv = s.expected(ivp=ivp)
    zp = np.abs(r["parking"] / C - park) / np.maximum(np.sqrt(park * (1 - park) / C), 1e-12)
    zd = np.abs(r["driving"] - C * drv) / np.maximum(np.sqrt(C * drv * (1 - drv)), 1e-12)
    print(f"ivp={ivp}: parking {zp.max():.2f} sigma, driving {zd.max():.2f} sigma")
    assert zp.max() < CAP and zd.max() < CAP
    if not ivp:
        assert np.array_equal(r["parking"][:, 0] / C, park[:, 0])


# ------------------------------------------------------------------------------------------------ 4: errors and side effects
@gpu
def test_row_total_above_one_and_missing_tables(cpm):
    Z, Tc = 24, 24
    p_drive, p_dest, _ = _tables(Z, Tc)
    big = np.array(p_dest)
    big[2, :, 4] *= 1.25
    with cpm.Sampler(Z, Tc) as s:
        for call in (s.expected, s.expected_batch):
            with pytest.raises(cpm.CpmError) as e:
                call()
            assert e.value.status == ERR_STATE
        s.set_p_drive(p_drive)
        with pytest.raises(cpm.CpmError) as e:
            s.expected()
        assert e.value.status == ERR_STATE and "p_dest" in str(e.value)
        s.set_p_dest(big)
        for _ in range(2):                                          # (refused every time, not only when the check is first made)
            with pytest.raises(cpm.CpmError) as e:
                s.expected()
            assert e.value.status == ERR_TABLE and "hour 5, origin 3" in str(e.value)
        with pytest.raises(cpm.CpmError) as e:
            s.expected_batch()
        assert e.value.status == ERR_STATE
        s.set_p_dest(p_dest)                                        # a table change rebuilds the per-table arrays
        park, _ = s.expected()
        assert np.all(np.isfinite(park))
        for bad in (np.nan, np.inf, -1e-9):
            pi0 = np.full(Z, 1.0 / Z)
            pi0[3] = bad
            with pytest.raises(cpm.CpmError) as e:
                s.expected(pi0)
            assert e.value.status == -1


@gpu
def test_expected_leaves_no_trace_in_a_later_resample(cpm):
    Z, cpz = 67, 200
    C = Z * cpz
    p_drive, p_dest, _ = _tables(Z, T)
    with _sampler(cpm, Z, T, np.nan_to_num(p_drive), p_dest) as s:
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        before, step = s.resample(SEED), s.last_step()
        s.set_p_drive_batch(np.asfortranarray(np.random.default_rng(1).uniform(0, 1, (Z, T, 3))))
        s.expected()
        s.expected(ivp=True)
        s.expected_batch()
        assert s.last_step() == step
        after = s.resample(SEED)
        assert np.array_equal(before["parking"], after["parking"]) and np.array_equal(before["driving"], after["driving"])
        assert s.last_step() == step
