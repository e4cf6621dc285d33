"""The compact-row dataset route (csrc/cpm_dataset.h: k_ds_cells, k_ds_sort, k_ds_pdrive, k_ds_pdest, k_ds_dense_p) and the host logic
that chooses between it and the dense builders (ensure_dataset, build_p_dest_sparse, ensure_travel_tables, ensure_pdrive_mean in
csrc/cpm_api.hip) on the hand-made datamatrices of tests/dataset_edges.py: rows of 0, 1, 63 / 64 / 65, 127 / 128 / 129 and 511 / 512 /
513 cells, kept cells of weight 0 at both ends of a row, a row whose cells total 0, cells without a standard deviation, a pair constant
over the day, and one context taken through sparse -> dense -> sparse -> error -> sparse.

Expected values: the CPU oracle's createpdrive / createpdestin / fast_run on the same datamatrix, computed once per fixture and left
unchanged; for createpdestin's rows in addition a rational-arithmetic evaluation (dataset_edges.pdest_row_exact) with a bound derived
from the rounding model, which the oracle itself is held to first, in a test that needs no GPU.  The device's p_drive is compared with
the oracle's at the suite's 4e-16; the reference runs use the oracle's p_drive (a draw would have to fall between two thresholds 2^-53
apart for that to matter).

GPU tests A .. E are marked `gpu`; the fixture and reference checks in front of them run without one.  The step records that
`pinned` reads are printed (pytest -s): the family is pinned, the repeats of a context's first steps are reported, not fixed."""
import time
import types

import numpy as np
import pytest

import dataset_edges as E
import side_reference as S
from conftest import SIM_SEED
from dataset_edges import _probe_k53, _ref_categorical
from product_form import pinned

gpu = pytest.mark.gpu
INFO_SPARSE = 6      # CPM_INFO_SPARSE_TABLES
ERR_TABLE = -4       # CPM_ERR_TABLE
Z, T, CPZ = 358, 24, 40
WORDS_129 = 276      # pack_row_words of a 129-cell longest row: 36 guide words + 160 high words + 80 words of u16 destinations
CAP_Z, CAP_CPZ = 1158, 8
WORDS_512 = 884      # ... of a 512-cell one: 68 + 544 + 272

# the rows every table check looks at, 0-based (origin, hour): every planted row, the D1 row and its neighbour, an empty row, the last origin,
# the rows that end in a cell of weight 0
PROBED = ([(0, 0), (1, 3)] + [(o, E.ROW_HOUR) for o in E.ROW_LENGTHS] + [(4, E.ROW_HOUR_2), (7, E.ROW_HOUR_2), (8, 7), (8, 8), (9, 9), (9, 10),
          (10, 6), (11, 5), (200, 12), (Z - 1, 0)] + [(14, t) for t in range(12)] + [(14, 15)])
FEW = [(7, E.ROW_HOUR), (8, 7), (9, 9), (E.WIDE_ORIGIN, E.WIDE_HOUR), (200, 12)]


def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _case(O, dm, dist, cpz, p_min=0.1, e_dest=2):
    """the oracle's tables and day on one datamatrix, read-only"""
    Zc, Tc = dm.shape[0], dm.shape[2]
    C = Zc * cpz
    p_drive = O.createpdrive(dm, dist, Zc, Tc, p_min, 0.9, 0.5)
    p_dest = O.createpdestin(dm, Zc, Tc, e_dest)
    ref = None
    if not np.isnan(p_dest).any():
        ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), datamatrix=dm, dist=dist)
    for a in (dm, dist, p_drive, p_dest):
        a.setflags(write=False)
    return types.SimpleNamespace(dm=dm, dist=dist, Z=Zc, T=Tc, cpz=cpz, C=C, p_drive=p_drive, p_dest=p_dest, ref=ref)


@pytest.fixture(scope="module")
def edge(O):
    dm, dist = E.edge_datamatrix(O, Z, T)
    c = _case(O, dm, dist, CPZ)
    c.exact = {rc: E.pdest_row_exact(dm, *rc) for rc in PROBED}
    return c


@pytest.fixture(scope="module")
def wide(O, edge):
    return _case(O, E.wide_variant(edge.dm), edge.dist, CPZ)


@pytest.fixture(scope="module")
def edge_p3(O, edge):
    """the edge matrix under build_p_drive(0.3, 0.9, 0.5): p_drive of the D1 row (9, 9) is p_min, so cars drive out of it"""
    c = _case(O, edge.dm, edge.dist, CPZ, p_min=0.3)
    c.faithful = S.reference(O, c.p_drive, c.p_dest, Z, CPZ, T, SIM_SEED, dm=edge.dm, dist=edge.dist)
    return c


# ------------------------------------------------------------------------------------------------ without a GPU
def test_the_edge_fixture_holds_what_it_plants(O, edge):
    dm = edge.dm
    L = E.row_lengths(dm)
    assert L.max() == 129 and L[16:].max() < 63                       # the planted rows are the long ones
    assert not L[0].any() and not L[[12, 13, 15]].any()                     # empty origins
    assert L[1, 3] == 1 and dm[1, Z - 1, 3, 0] > 0
    for o, n in E.ROW_LENGTHS.items():
        assert L[o, E.ROW_HOUR] == n and L[o, E.ROW_HOUR_2] == n, o
        assert (dm[o, list(E.MUST) + [Z - 1], E.ROW_HOUR, 0] > 0).all(), o
        w = edge.p_dest[o, :, E.ROW_HOUR]
        assert (w != 0).sum() == n and len(np.unique(w[w != 0])) > n // 3, o      # weights that vary (x = 1 in the hour of the maximum)
    assert (L[1:12] > 0).all()                                        # every planted origin holds data in every hour ...
    assert not np.isnan(edge.p_drive).any() and (edge.p_drive[1:12] >= 0.1).all() and not edge.p_drive[0].any()   # ... and drives
    # pairs populated all day: kept cells of weight 0, at both ends of row (8, 7)
    assert ((dm[8, :, :, 0] != 0).sum(axis=1) == T).sum() == 40 and ((dm[9, :, :, 0] != 0).sum(axis=1) == T).sum() == 12
    k = np.flatnonzero(E.kept_cells(dm)[8, :, 7])
    assert len(k) == 40 and L[8, 7] == 40
    assert edge.p_dest[8, k[0], 7] == 0 and edge.p_dest[8, k[-1], 7] == 0 and dm[8, k[0], 7, 0] > 0 and dm[8, k[-1], 7, 0] > 0
    assert 0 < (edge.p_dest[8, k, 7] == 0).sum() < 40 and edge.p_dest[8, :, 7].sum() > 0.99
    # twelve rows that begin and end with a kept cell of weight 0; some total less than 1, so that a draw can lie above the total
    below = []
    for t in range(12):
        k = np.flatnonzero(E.kept_cells(dm)[14, :, t])
        assert len(k) == 22 and k[0] == 0 and k[-1] == Z - 1 and edge.p_dest[14, 0, t] == 0 and edge.p_dest[14, Z - 1, t] == 0, t
        if edge.p_dest[14, :, t].cumsum()[-1] < 1.0 - 2.0 ** -53:
            below.append(t)
    assert below, "no row of origin 14 totals less than 1"
    print(f"rows (14, t) that total less than 1 - 2^-53: t = {below}")
    assert edge.p_dest[14, 0, 15] > 0 and edge.p_dest[14, Z - 1, 15] > 0
    # the D1 row: 12 kept cells, total 0
    assert L[9, 9] == 12 and not edge.p_dest[9, :, 9].any() and (dm[9, :, 9, 0] > 0).sum() == 12
    assert (edge.p_dest[9, :, 10] != 0).sum() == 12
    # standard deviations: none on the 30 cells of row (10, 6) and on 5 % of the background; one without a mean
    m, sd = dm[..., 0], dm[..., 1]
    assert L[10, 6] == 30 and ((m[10, :, 6] != 0) & (sd[10, :, 6] == 0)).sum() == 30
    cells = int((m[16:] != 0).sum())
    n_sd0 = int(((m != 0) & (sd == 0)).sum())
    assert abs(n_sd0 - 30 - 0.05 * cells) < 6 * np.sqrt(0.05 * 0.95 * cells), (n_sd0, cells)   # (Binomial(cells, 0.05): six sigma)
    assert ((m == 0) & (sd != 0)).sum() == 1 and m[11, 13, 5] == 0 and sd[11, 13, 5] == 5.0 and L[11, 5] == 10
    assert not np.isnan(edge.p_dest).any()
    print(f"cells of the background {cells}, cells without a standard deviation {n_sd0}")


def test_the_variants_and_the_cap_fixture(O, edge, wide):
    w = wide.dm
    Lw = E.row_lengths(w)
    assert Lw.max() == 200 and Lw[E.WIDE_ORIGIN, E.WIDE_HOUR] == 200 and (Lw[E.WIDE_ORIGIN] > 0).all()
    others = np.arange(Z) != E.WIDE_ORIGIN
    assert np.array_equal(w[others], edge.dm[others])
    # the day on the wide matrix is another day: origin 12 drives, out of its 200-cell row too, so tables left over from the other
    # datamatrix cannot pass for this one's (nor the other way round)
    assert np.array_equal(wide.p_drive[others], edge.p_drive[others]) and (wide.p_drive[E.WIDE_ORIGIN] >= 0.1).all() and not edge.p_drive[E.WIDE_ORIGIN].any()
    assert wide.ref["driving"][E.WIDE_ORIGIN].sum() > 100 and edge.ref["driving"][E.WIDE_ORIGIN].sum() == 0
    assert wide.ref["driving"][E.WIDE_ORIGIN, E.WIDE_HOUR] >= 8
    assert wide.ref["sum_tt_q16"] != edge.ref["sum_tt_q16"] and not np.array_equal(wide.ref["parking"], edge.ref["parking"])
    # the constant pair sits on an origin that drives, in front of most of its cells: its p_drive differs from the edge matrix's
    n = E.nan_variant(edge.dm)
    o, j = E.nan_pair(edge.dm)
    assert o == E.NAN_ORIGIN and 0 < j < np.flatnonzero(edge.dm[o, :, 0, 0])[2] and not edge.dm[o, j].any()
    nan_drive = O.createpdrive(n, edge.dist, Z, T, 0.1, 0.9, 0.5)
    assert np.array_equal(np.flatnonzero((nan_drive != edge.p_drive).any(axis=1)), [o]) and edge.ref["driving"][o].sum() > 100
    assert E.row_lengths(n).max() == 129
    p = O.createpdestin(n, Z, T, 2)
    assert np.isnan(p).any() and not np.isnan(p[np.arange(Z) != E.NAN_ORIGIN]).any()
    for longest in (512, 513):
        dm, _ = E.cap_datamatrix(O, CAP_Z, T, longest)
        L = E.row_lengths(dm)
        (o1, t1), (o2, t2) = E.cap_rows(CAP_Z)
        assert L[o1, t1] == 511 and L[o2, t2] == longest and L.max() == longest
        assert sorted(L.ravel())[-5] < 64                             # (two rows and their twins: everything else is background)
        del dm


def test_the_reference_run_draws_from_the_d1_row(O, edge_p3):
    c = edge_p3
    assert c.p_drive[9, 9] == 0.3                                     # every pair at its minimum: (ms - min) / (max - min) = 0
    assert c.ref["driving"][9, 9] >= 8
    f = c.faithful
    assert np.array_equal(f["parking"], c.ref["parking"]) and np.array_equal(f["driving"], c.ref["driving"]) and f["sum_tt_q16"] == c.ref["sum_tt_q16"]
    assert f["flows"][9, 9, 9] == c.ref["driving"][9, 9] and f["flows"][9, 9].sum() == f["flows"][9, 9, 9]   # D1: they stay, and count as driving


def test_the_oracle_stays_within_the_exact_bound(O, edge):
    worst = {rc: E.check_row_exact(edge.p_dest[rc[0], :, rc[1]], edge.exact[rc], rc) for rc in PROBED}
    print("largest relative error of the oracle's rows, in units of the bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) > 0                                    # (the rows are not trivially exact: the bound is at work)
    # the check bites: an entry just beyond the bound of its 129-cell row ((n + 14) 2^-53, the row's own error is 0.03 of that: an
    # error of (n + 20) 2^-53 is out, one of (n + 8) 2^-53 is in), and a weight where the exact row has none
    rc = (7, E.ROW_HOUR)
    j = int(np.flatnonzero(edge.p_dest[rc[0], :, rc[1]])[3])
    for ulps, out in ((129 + 20, True), (129 + 8, False)):
        row = edge.p_dest[rc[0], :, rc[1]].copy()
        row[j] = float(edge.exact[rc][j] * (1 + ulps * E.U))
        assert abs(row[j] / float(edge.exact[rc][j]) - 1) > 100 * 2.0 ** -53
        if out:
            with pytest.raises(AssertionError):
                E.check_row_exact(row, edge.exact[rc], rc)
        else:
            E.check_row_exact(row, edge.exact[rc], rc)
    row = edge.p_dest[8, :, 7].copy()
    row[int(np.flatnonzero(E.kept_cells(edge.dm)[8, :, 7])[0])] = 5e-324
    with pytest.raises(AssertionError):
        E.check_row_exact(row, edge.exact[(8, 7)], (8, 7))


# ------------------------------------------------------------------------------------------------ helpers of the GPU tests
def _probe_rows(s, p_dest, rows, rng):
    """get_cdf_row and debug_categorical on, below and above every breakpoint of the rows (0-based) against the oracle's p_destin"""
    total_exact = 0
    for (o, t) in rows:
        cdf = np.cumsum(p_dest[o, :, t])
        k53 = _probe_k53(cdf, rng)
        got, n_exact = s.debug_categorical(o + 1, t + 1, k53)
        assert np.array_equal(got, _ref_categorical(cdf, k53)), (o, t)
        assert np.array_equal(s.get_cdf_row(o + 1, t + 1), cdf), (o, t)
        total_exact += n_exact
    return total_exact


def _run(s, kernel, case, label, ref=None, travel=True):
    """IVP and a (travel) resample of the case's fleet under `kernel` against the oracle's day"""
    ref = case.ref if ref is None else ref
    s.set_kernel(kernel)
    s.init_states(case.C, case.cpz)
    with pinned(s, kernel, repeats=None) as ivp:
        zone0 = s.solve_ivp(SIM_SEED)
    assert np.array_equal(zone0, ref["zone0"]), label
    with pinned(s, kernel, repeats=None) as step:
        r = s.resample(SIM_SEED, travel=travel)
    print(f"{label}, kernel {kernel}: ivp {ivp} resample {step}")
    assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"]), label
    if travel:
        assert r["sum_tt_q16"] == ref["sum_tt_q16"], label
    return r


def _build(s, case, words, label, e_dest=2):
    """both tables from the context's datamatrix against the oracle's, and the info word"""
    p_drive = s.build_p_drive(0.1, 0.9, 0.5)
    np.testing.assert_allclose(p_drive, case.p_drive, rtol=4e-16, atol=0, equal_nan=True, err_msg=label)
    p_dest = s.build_p_dest(e_dest)
    assert s.get_info(INFO_SPARSE) == words, label
    assert np.array_equal(p_dest, case.p_dest), label
    return p_drive, p_dest


@pytest.fixture(scope="module")
def device_edge(cpm, edge):
    """the device's (p_drive, p_dest) of the edge matrix on the sparse route, from a context of their own, read-only"""
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(edge.dm, edge.dist)
        tables = _build(s, edge, WORDS_129, "edge tables")
    for a in tables:
        a.setflags(write=False)
    return tables


# ------------------------------------------------------------------------------------------------ A: edge rows on the sparse route
@gpu
def test_a_edge_rows_on_the_sparse_route(cpm, O, edge, device_edge):
    rng = np.random.default_rng(6)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(edge.dm, edge.dist)
        p_drive, p_dest = _build(s, edge, WORDS_129, "A")
        assert np.array_equal(p_dest, device_edge[1]) and _same(p_drive, device_edge[0])     # (the same bits from every context)
        worst = max(E.check_row_exact(p_dest[o, :, t], edge.exact[(o, t)], (o, t)) for (o, t) in PROBED)
        s.build_p_dest(2, want=False)                        # (no dense array this time: the tables alone)
        n_exact = _probe_rows(s, edge.p_dest, PROBED, rng)
        print(f"A: largest error against the exact rows {worst:.3f} of the bound; {n_exact} probes decided by the walk over the row's cells")
        for kernel in (0, 1, 2, 5):
            _run(s, kernel, edge, "A")
        assert s.get_info(INFO_SPARSE) == WORDS_129
        # a Float64 exponent: pow() on the device against libm's, its own day
        p_half = s.build_p_dest(0.5)
        assert s.get_info(INFO_SPARSE) == WORDS_129
        np.testing.assert_allclose(p_half, O.createpdestin(edge.dm, Z, T, 0.5), rtol=1e-12, atol=0)
        assert not p_half[9, :, 9].any() and p_half[8, :, 7].sum() > 0.99
        ref = O.fast_run(edge.p_drive, O.build_cdf(p_half), edge.C, SIM_SEED, _zone0(edge.C, CPZ), datamatrix=edge.dm, dist=edge.dist)
        _run(s, 5, edge, "A, e_dest = 0.5", ref)
        _probe_rows(s, p_half, [(7, E.ROW_HOUR), (8, 7), (9, 9)], rng)


# ------------------------------------------------------------------------------------------------ B: the D1 row
@gpu
def test_b_the_d1_row_on_the_sparse_pack(cpm, O, edge_p3):
    """Row (9, 9) holds 12 cells whose weights are all 0: a row that is neither empty nor drawable.  The oracle's D1 policy
    (src/resampling.jl:35-36: destination = origin, counted as driving) must hold on the sparse pack too."""
    c = edge_p3
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(c.dm, c.dist)
        p_drive = s.build_p_drive(0.3, 0.9, 0.5)
        np.testing.assert_allclose(p_drive, c.p_drive, rtol=4e-16, atol=0, equal_nan=True)
        assert p_drive[9, 9] == 0.3
        s.build_p_dest(2, want=False)
        assert s.get_info(INFO_SPARSE) == WORDS_129
        for kernel in (5, 0):
            r = _run(s, kernel, c, "B", travel=False)
            assert r["driving"][9, 9] == c.ref["driving"][9, 9] >= 8
        with pinned(s, 0, repeats=None):
            r = s.resample(SIM_SEED, flows=True)
        S.check("flows", r, c.faithful, where="B")
        assert r["flows"][9, 9, 9] == c.ref["driving"][9, 9] and r["flows"][9, 9].sum() == r["flows"][9, 9, 9]


# ------------------------------------------------------------------------------------------------ C: the two routes agree
@gpu
def test_c_the_dense_route_agrees_with_the_sparse_one(cpm, O, edge, wide, device_edge):
    """200 cells in one row of origin 12 send the whole dataset to the dense builders (420 pack words against 60 % of 484).  Every
    other origin's tables must be the sparse route's, bit for bit, and the day -- origin 12 drives, 18 cars out of the 200-cell row --
    the oracle's on this matrix, which is not the edge matrix's day."""
    a_drive, a_dest = device_edge
    rng = np.random.default_rng(7)
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(wide.dm, wide.dist)
        p_drive, p_dest = _build(s, wide, 0, "C")
        others = np.arange(Z) != E.WIDE_ORIGIN
        assert np.array_equal(p_dest[others], a_dest[others]) and _same(p_drive[others], a_drive[others])
        assert (p_dest[E.WIDE_ORIGIN, :, E.WIDE_HOUR] != 0).sum() == E.WIDE_CELLS and not a_dest[E.WIDE_ORIGIN].any()
        _probe_rows(s, wide.p_dest, FEW + [(1, 3), (2, E.ROW_HOUR), (10, 6)], rng)
        _run(s, 0, wide, "C")
        assert s.get_info(INFO_SPARSE) == 0


# ------------------------------------------------------------------------------------------------ D: one context through the routes
@gpu
def test_d_one_context_through_the_routes(cpm, O, edge, wide):
    """What a stale ds_valid / ds_ok / tt_valid / tts_valid / tts_fixed / sparse_tables / pdrive_mean_valid would break: every step is
    checked against the reference of ITS datamatrix and exponent.  (Step 2: x^0 = 1 for every pair with data, so createpdestin gives
    1 / (pairs with data) along a row and nothing on an origin without data -- the oracle's table, not 1 / Z.)"""
    rng = np.random.default_rng(8)
    nan_dm = E.nan_variant(edge.dm)
    nan_drive = O.createpdrive(nan_dm, edge.dist, Z, T, 0.1, 0.9, 0.5)
    flat = _case(O, edge.dm, edge.dist, CPZ, e_dest=0)
    pairs = (edge.dm[..., 0].max(axis=2) > 0).sum(axis=1)
    assert flat.p_dest[20, :, 3].max() == 1.0 / pairs[20] and not flat.p_dest[0].any()

    def check(s, case, words, label, p_dest):
        assert s.get_info(INFO_SPARSE) == words, label
        np.testing.assert_allclose(s.get_p_drive(), case.p_drive, rtol=4e-16, atol=0, equal_nan=True, err_msg=label)
        if p_dest is not None:
            assert np.array_equal(p_dest, case.p_dest), label
        _probe_rows(s, case.p_dest, FEW, rng)
        _run(s, 0, case, label)
        assert s.get_info(INFO_SPARSE) == words, label

    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(edge.dm, edge.dist)
        _, first = _build(s, edge, WORDS_129, "D1")
        check(s, edge, WORDS_129, "D1 sparse", first)
        check(s, flat, 0, "D2 e_dest = 0, dense", s.build_p_dest(0))
        again = s.build_p_dest(2)
        assert np.array_equal(again, first)
        check(s, edge, WORDS_129, "D3 sparse again", again)
        s.set_datamatrix(wide.dm)                            # (the distance matrix stays)
        _, p = _build(s, wide, 0, "D4")
        check(s, wide, 0, "D4 wide, dense", p)
        s.refresh_tables()
        check(s, wide, 0, "D5 refreshed", None)
        s.set_datamatrix(edge.dm)
        _, p = _build(s, edge, WORDS_129, "D6")
        assert np.array_equal(p, first)
        check(s, edge, WORDS_129, "D6 sparse after dense", p)
        s.set_datamatrix(nan_dm)
        np.testing.assert_allclose(s.build_p_drive(0.1, 0.9, 0.5), nan_drive, rtol=4e-16, atol=0, equal_nan=True)
        with pytest.raises(cpm.CpmError) as e:
            s.build_p_dest(2)
        assert e.value.status == ERR_TABLE
        with pytest.raises(cpm.CpmError):                    # (the context is left without a table)
            s.resample(SIM_SEED, travel=True)
        s.set_datamatrix(edge.dm)
        _, p = _build(s, edge, WORDS_129, "D8")
        assert np.array_equal(p, first)
        check(s, edge, WORDS_129, "D8 sparse after the error", p)
        s.refresh_tables()
        check(s, edge, WORDS_129, "D8 refreshed", None)


# ------------------------------------------------------------------------------------------------ E: the cap
@gpu
def test_e_a_row_of_exactly_the_capacity_and_one_beyond(cpm, O):
    """512 cells = kDsCap: every LDS array of the per-row kernels is full and the sparse pack (884 words) just passes the 60 % rule at
    Z = 1,158 (8,840 <= 8,856).  513 cells: the sweep counts the row, stores 512 of it and flags the dataset, which takes the dense
    builders; its travel rows come from build_sparse_travel_rows.  The oracle's share of the time is printed apart from the device's."""
    rng = np.random.default_rng(9)
    rows = E.cap_rows(CAP_Z)
    near = [(rows[0][0], (rows[0][1] + 12) % T), (rows[1][0], (rows[1][1] + 12) % T), (rows[0][0], 0), (CAP_Z - 1, T - 1)]
    t_cpu = t_dev = 0.0
    with cpm.Sampler(CAP_Z, T) as s:
        for longest, words in ((512, WORDS_512), (513, 0)):
            t0 = time.perf_counter()
            dm, dist = E.cap_datamatrix(O, CAP_Z, T, longest)
            case = _case(O, dm, dist, CAP_CPZ)
            exact = {rc: E.pdest_row_exact(dm, *rc) for rc in rows}
            for rc in rows:
                E.check_row_exact(case.p_dest[rc[0], :, rc[1]], exact[rc], rc)        # (the oracle first)
            t_cpu += time.perf_counter() - t0
            t0 = time.perf_counter()
            s.set_datamatrix(dm, dist)
            p_drive, p_dest = _build(s, case, words, f"E {longest}")
            assert (p_dest[rows[1][0], :, rows[1][1]] != 0).sum() == longest
            worst = max(E.check_row_exact(p_dest[o, :, t], exact[(o, t)], (o, t)) for (o, t) in rows)
            del p_dest
            n_exact = _probe_rows(s, case.p_dest, rows + near, rng)
            _run(s, 5, case, f"E {longest}")
            assert s.get_info(INFO_SPARSE) == words
            t_dev += time.perf_counter() - t0
            drivers = [int(case.ref['driving'][o, t]) for (o, t) in rows]
            assert min(drivers) >= 24                                                   # (the travel rows of the long rows are sampled)
            print(f"E {longest}: drivers out of the long rows {drivers}, "
                  f"error against the exact rows {worst:.3f} of the bound, {n_exact} probes decided by the walk")
            del dm, dist, case
    print(f"E: oracle and fixtures {t_cpu:.2f} s, device calls and comparisons {t_dev:.2f} s")
