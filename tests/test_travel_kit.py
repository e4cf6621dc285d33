"""The truncated-normal travel-time sampler on every branch of its f64 kit (csrc/cpm_rng.h: det_log, det_sqrt, det_erf, ppnd,
ppnd_tail, truncnormal_mass, truncnormal_draw, q16): the only floating-point arithmetic on the hot path that must agree bit for bit
between CPU and GPU.

Three links.  Without a GPU: the oracle's kit against mpmath at 50 digits on the probes of tests/travel_ladder.py, and the census of
the fixtures (which branches their trips and probes execute: a condition on the inputs).  On the GPU, bit for bit and without a
tolerance: the device's functions against the oracle's through the two diagnostic entries (cpm_debug_f64_kit, cpm_debug_travel_draw),
which also reach what no resample draws (u = 0, |u - 1/2| within 1e-11 of 1/2, the lower clamp), and every place the draw is compiled
at -- the per-car kernels, the three travel tables of the grouped path (CPM_INFO_TRAVEL_TABLE 1, 2, 3) and the batched resample -- on
datamatrices whose standard deviations run down the ladder of travel_ladder.RUNGS.

One launch site is out of reach of a small test: the grouped path runs its travel kernel hour by hour only when the runs of all T
hours exceed 24 GiB (GroupedWork::ensure_history); every test here, like every other test of the suite, takes the one launch over
the kept runs.  And nothing reaches the upper clamp of truncnormal_draw (travel_ladder.py says why)."""
import functools
import math
import types

import numpy as np
import pytest

import dataset_edges as E
import travel_ladder as TL
from conftest import SIM_SEED, TABLE_SEED
from product_form import CAR, GROUPED, pinned

gpu = pytest.mark.gpu

Z, T, CPZ = 40, 24, 50
KERNELS = [pytest.param(0, id="auto"), pytest.param(1, id="car"), pytest.param(2, id="zone_lds"), pytest.param(5, id="zone_grouped")]
INFO_TRAVEL_TABLE = 12
MIN_RUNG_TRIPS = 100

# The oracle's worst relative error against mpmath's inverse CDF on the drawn trips of the ladder day whose cell has mass < 1 - 1e-9
# (test_oracle_draws_against_mpmath_on_the_ladder_trips measures it and fails when it grows): 3.25e-16 was measured, on 13,844 trips
# (one and a half units in the last place of a double just above a power of two).  The per-car GPU test allows twice this figure.
ORACLE_WORST_DRAW = 3.3e-16


def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ------------------------------------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def ladder_day(O):
    """The ladder fixture (Z = 40, T = 24, 50 cars per zone), the oracle's tables and both of its days on it, read-only: the
    faithful three-pass form with every car's matrices (`state`, `trans`) and the fast twin (`ref`)."""
    C = Z * CPZ
    dm, dist, idx = TL.ladder_datamatrix(O, Z, T, TABLE_SEED, 0.3)
    p_drive = O.createpdrive(dm, dist, Z, T, 0.1, 0.9, 0.5)
    p_dest = O.createpdestin(dm, Z, T, 2)
    st, tr = O.initializestates(C, CPZ, T)
    init = O.solveinitialvalueproblem(st, tr, p_drive, p_dest, C, Z, SIM_SEED)
    st, tr = O.initializestates(C, CPZ, T)
    st[:, 0] = init
    O.resampling(st, tr, C, Z, p_drive, p_dest, dm, dist, SIM_SEED)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, CPZ), want_state=True, datamatrix=dm, dist=dist)
    _freeze(dm, dist, idx, p_drive, p_dest, init, st, tr, ref["parking"], ref["driving"], ref["state"], ref["zone0"])
    return types.SimpleNamespace(C=C, dm=dm, dist=dist, idx=idx, p_drive=p_drive, p_dest=p_dest, init=init, state=st, trans=tr, ref=ref)


@functools.lru_cache(maxsize=None)
def draw_reference(O):
    """The probe product of cpm_debug_travel_draw (travel_ladder.draw_probes), the oracle's answers and its census, read-only"""
    k, m, s, spans = TL.draw_probes(O)
    draw, mass, q16 = TL.orc_draw(O, k, m, s)
    census = {name: int(hit.sum()) for name, hit in TL.draw_census(O, k, m, s).items()}
    _freeze(k, m, s, draw, mass, q16)
    return types.SimpleNamespace(k=k, mean=m, sd=s, spans=spans, draw=draw, mass=mass, q16=q16, census=census)


def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def mp_isf(mp, r, steps=3):
    """z with 1 - Phi(z) = erfc(z / sqrt 2) / 2 = r for 0 < r <= 1/2, at mpmath's working precision: Newton's iteration on mpmath's
    erfc from scipy's double-precision answer.  The start is good to 1e-13 at worst (r is rounded to a double for it), each step
    squares the error, and `steps` are taken (two already leave 1e-50)."""
    from scipy import special
    r = mp.mpf(r)
    z = mp.mpf(-float(special.ndtri(float(r))))
    root2, root2pi = mp.sqrt(2), mp.sqrt(2 * mp.pi)
    for _ in range(steps):
        z = z + (mp.erfc(z / root2) / 2 - r) * root2pi * mp.exp(z * z / 2)
    return z


@functools.lru_cache(maxsize=None)
def ladder_trips_mpmath(O):
    """The drawn trips of the faithful ladder day whose cell has mass < 1 - 1e-9 (no cancellation in 1/2 - |q|), and mpmath's draw for
    each: x = mu + sigma Phi^-1(1/2 + (u - 1/2) E), E = erf(mu / (10 sigma sqrt 2)), from the cell's two doubles and the trip's
    uniform O.uniforms(seed, car, T - 1 + hour, 1) in 50-digit arithmetic, rounded to a double at the end."""
    mp = _mp()
    day = ladder_day(O)
    car, hour, o, d = TL.trips_of_trans(day.state, day.trans)
    mean, sd = day.dm[o, d, hour, 0], day.dm[o, d, hour, 1]
    s1 = TL.sigma_of(mean, sd)
    mass = TL.orc(O, "truncnormal_mass", mean, s1)
    keep = (o != d) & (s1 > 0) & (mass > 0) & (mass < 1 - 1e-9)
    car, hour, mean, s1 = car[keep], hour[keep], mean[keep], s1[keep]
    u = TL.trip_uniforms(O, SIM_SEED, car, hour, T)
    root2, half = mp.sqrt(2), mp.mpf(0.5)
    want = np.empty(len(car))
    for i, (m_, s_, u_) in enumerate(zip(mean.tolist(), s1.tolist(), u.tolist())):
        m_, s_ = mp.mpf(m_), mp.mpf(s_)
        q = (mp.mpf(u_) - half) * mp.erf(m_ / (10 * s_ * root2))
        z = mp.mpf(0) if q == 0 else mp.sign(q) * mp_isf(mp, half - abs(q), steps=2)
        want[i] = float(m_ + s_ * z)
    _freeze(car, hour, want)
    return types.SimpleNamespace(car=car, hour=hour, want=want)


def _worst_rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _rungs_visited(idx, state, label):
    """at least MIN_RUNG_TRIPS trips on cells of every rung, from the reference's per-car record: a condition on the fixture"""
    n = TL.rung_trips(idx, TL.trips_of_state(state))
    assert (n >= MIN_RUNG_TRIPS).all(), (label, dict(zip(TL.RUNGS, n.tolist())))
    return n


# ------------------------------------------------------------------------------------------------ without a GPU
def test_ladder_day_reaches_every_class(O):
    """The faithful day on the ladder fixture makes at least 1,000 trips in each of the nine classes: inside a zone, sigma <= 0,
    mass 0, the four branches of erf, the central rational of ppnd and its tail; and both of the oracle's forms agree on it."""
    day = ladder_day(O)
    got = TL.census(O, day.dm, TL.trips_of_trans(day.state, day.trans), seed=SIM_SEED, T=T)
    print(got)
    assert set(got) == set(TL.CLASSES)
    assert all(n >= 1000 for n in got.values()), got
    assert np.array_equal(day.ref["state"], day.state) and day.ref["sum_tt_q16"] == O.sum_travel_time_q16(day.trans)
    assert (TL.rung_trips(day.idx, TL.trips_of_trans(day.state, day.trans)) >= 1000).all()
    _rungs_visited(day.idx, day.ref["state"], "ladder day")


def test_oracle_kit_against_mpmath(O):
    """orc_erf, orc_log, orc_sqrt, orc_ppnd and orc_exp_neg against mpmath at 50 digits on the probes the GPU test compares bit for
    bit, under the bounds of test_truncated_normal_kit_against_scipy: erf 3e-16 absolute, ln and sqrt 5e-16 relative, ppnd 2e-15 x
    max(1, |want|) conditioned on r = 1/2 - |q| (exact in a double for |q| >= 1/4, and mpmath subtracts exactly below), exp_neg as in
    test_exp_neg_accuracy.  Measured here: 1.7e-16, 2.3e-16, 1.7e-16, 6.1e-16.  No probe needed a wider bound."""
    mp = _mp()
    L = O.lib()
    P = TL.kit_probes()
    worst = dict(erf=0.0, log=0.0, sqrt=0.0, ppnd=0.0)
    for x in P["erf"].tolist():
        got = L.orc_erf(x)
        if math.isnan(x) or x < 0:
            assert got == 0.0, x                                   # (the statement `if (!(x >= 0.0)) return 0.0`)
            continue
        err = float(abs(mp.mpf(got) - mp.erf(mp.mpf(x))))
        assert err <= 3e-16, (x, err)
        worst["erf"] = max(worst["erf"], err)
    assert L.orc_erf(6.0) == 1.0 and L.orc_erf(1e300) == 1.0
    for name, fn in (("log", mp.log), ("sqrt", mp.sqrt)):
        for x in P[name].tolist():
            got, want = getattr(L, "orc_" + name)(x), fn(mp.mpf(x))
            if want == 0:
                assert got == 0.0, (name, x)                       # ln 1
                continue
            err = float(abs((mp.mpf(got) - want) / want))
            assert err <= 5e-16, (name, x, err)
            worst[name] = max(worst[name], err)
    half = mp.mpf(0.5)
    for q in P["ppnd"].tolist():
        got = L.orc_ppnd(q)
        assert L.orc_ppnd(-q) == -got, q                           # odd, exactly
        if q < 0:
            continue                                               # (the mirror image: checked by the line above)
        if q == 0.5:
            assert got == 9.0                                      # r = 0: the val = 9 exit
            continue
        want = mp.mpf(0) if q == 0 else mp_isf(mp, half - mp.mpf(q))
        err = float(abs(mp.mpf(got) - want) / max(1, abs(want)))
        assert err <= 2e-15, (q, err)
        worst["ppnd"] = max(worst["ppnd"], err)
    for y in P["exp_neg"].tolist():
        got, want = L.orc_exp_neg(y), mp.exp(-mp.mpf(y))
        if y > 745.0:
            assert got == 0.0, y
        else:
            assert abs(mp.mpf(got) - want) <= 4e-16 * want + mp.mpf(5e-324), y
    print(worst)


def test_draw_probes_reach_every_branch(O):
    """The probe product of cpm_debug_travel_draw, on the oracle: its census shows every branch -- both rationals of the tail, the
    val = 9 exit and the lower clamp among them, which no resample reaches --, every draw lies in its window and the draws of a cell
    do not decrease with k.  The pinned oddity: where the mass rounds to exactly 1.0, u = 0 gives mu - 9 sigma, which for
    sigma < mu / 90 lies INSIDE the window, not at its edge (probability 2^-53 per draw)."""
    ref = draw_reference(O)
    print(ref.census)
    for name in ("sigma_le_0", "mass_0", "erf_1", "erf_2", "erf_3", "erf_4", "central", "tail_r_le_5", "tail_r_gt_5", "val_9", "clamp_lo"):
        assert ref.census[name] >= 20, (name, ref.census)
    assert ref.census["clamp_hi"] == 0                            # (unreachable: travel_ladder.py)
    _window_and_order(ref, ref.draw)
    L = O.lib()
    assert L.orc_truncnormal_mass(961.0, 0.961) == 1.0
    assert L.orc_truncnormal_draw(0.0, 961.0, 0.961, 1.0) == 961.0 + 0.961 * -9.0 == 952.351 > 0.9 * 961.0
    below, at = TL.mass_one_edge(O, 961.0)                        # sigma ~ mu / 83: mu - 9 sigma is below the window, the clamp takes it
    assert L.orc_truncnormal_mass(961.0, at) == 1.0 > L.orc_truncnormal_mass(961.0, below) and 961.0 / 85 < at < 961.0 / 80
    assert L.orc_truncnormal_draw(0.0, 961.0, at, 1.0) == 0.9 * 961.0


def _window_and_order(ref, draw):
    assert ((draw >= 0.9 * ref.mean) & (draw <= 1.1 * ref.mean)).all()
    for a, b in ref.spans:
        assert (np.diff(draw[a:b]) >= 0).all(), (ref.mean[a], ref.sd[a])
    # (each span holds ONE cell and its k ascending: travel_ladder.draw_probes)
    assert all((np.diff(ref.k[a:b].astype(np.int64)) > 0).all() and len(set(ref.sd[a:b])) == 1 for a, b in ref.spans)


def test_oracle_draws_against_mpmath_on_the_ladder_trips(O):
    """The oracle's travel-time column against mpmath's inverse CDF on the ladder day's drawn trips with mass < 1 - 1e-9: the measured
    worst relative error must not exceed ORACLE_WORST_DRAW, the figure the per-car GPU test doubles for its bound."""
    day, trips = ladder_day(O), ladder_trips_mpmath(O)
    assert len(trips.car) >= 10000
    worst = _worst_rel(day.trans[trips.car, trips.hour, 2], trips.want)
    print(f"oracle against mpmath on {len(trips.car)} trips: worst relative error {worst:.3e}")
    assert worst <= ORACLE_WORST_DRAW


# ------------------------------------------------------------------------------------------------ on the GPU
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@gpu
def test_device_kit_equals_the_oracle_bit_for_bit(cpm, O):
    """cpm_debug_f64_kit against orc_log, orc_sqrt, orc_erf, orc_ppnd and orc_exp_neg on travel_ladder.kit_probes, compared as 64-bit
    integers (so -0.0 and NaN payloads count)."""
    P = TL.kit_probes()
    with cpm.Sampler(8, 24) as s:
        for name in ("log", "sqrt", "erf", "ppnd", "exp_neg"):
            want = TL.orc_exp_neg(O, P[name]) if name == "exp_neg" else TL.orc(O, name, P[name])
            got = s.debug_f64_kit(name, P[name])
            differ = np.flatnonzero(_bits(got) != _bits(want))
            assert differ.size == 0, (name, [(float(P[name][i]), float(got[i]), float(want[i])) for i in differ[:5]])
        with pytest.raises(cpm.CpmError):
            s.debug_f64_kit(5, P["erf"])
        assert s.debug_f64_kit("erf", np.zeros(0)).shape == (0,)


@gpu
def test_device_draw_equals_the_oracle_on_every_branch(cpm, O):
    """cpm_debug_travel_draw against orc_truncnormal_mass, orc_truncnormal_draw and llrint(x * 65536) on the probe product: bit for
    bit, every draw in its window, non-decreasing in k per cell.  Census asserted (taken on the CPU from the oracle): sigma <= 0,
    mass 0, the four branches of erf, central, both rationals of the tail, the val = 9 exit, the lower clamp."""
    ref = draw_reference(O)
    for name in ("sigma_le_0", "mass_0", "erf_1", "erf_2", "erf_3", "erf_4", "central", "tail_r_le_5", "tail_r_gt_5", "val_9", "clamp_lo"):
        assert ref.census[name] >= 20, (name, ref.census)
    with cpm.Sampler(8, 24) as s:
        draw, mass, q16 = s.debug_travel_draw(ref.k, ref.mean, ref.sd)
        pinned_draw = s.debug_travel_draw([0], [961.0], [0.961])
        assert s.debug_travel_draw([], [], [])[0].shape == (0,)
    for got, want, what in ((mass, ref.mass, "mass"), (draw, ref.draw, "draw")):
        differ = np.flatnonzero(_bits(got) != _bits(want))
        assert differ.size == 0, (what, [(int(ref.k[i]), float(ref.mean[i]), float(ref.sd[i]), float(got[i]), float(want[i])) for i in differ[:5]])
    assert np.array_equal(q16, ref.q16)
    _window_and_order(ref, draw)
    assert pinned_draw[0][0] == 952.351 and pinned_draw[1][0] == 1.0 and pinned_draw[2][0] == round(952.351 * 65536)


@gpu
def test_per_car_matrices_on_the_ladder(cpm, O):
    """The per-car kernels (family CAR pinned, state and transition matrices wanted) on the ladder fixture: all four transition
    columns and the time sum equal O.resampling.  Independently of the oracle's kit, the travel-time column against mpmath's inverse
    CDF on the trips with mass < 1 - 1e-9, within twice the oracle's own measured worst (ORACLE_WORST_DRAW)."""
    day, trips = ladder_day(O), ladder_trips_mpmath(O)
    with cpm.Sampler(Z, T) as s:
        s.set_p_drive(day.p_drive)
        s.set_p_dest(day.p_dest)
        s.set_datamatrix(day.dm, day.dist)
        s.init_states(day.C, CPZ)
        with pinned(s, 0):
            assert np.array_equal(s.solve_ivp(SIM_SEED), day.init)
        with pinned(s, 0, family=CAR):
            r = s.resample(SIM_SEED, travel=True, want_state=True, want_trans=True)
    assert np.array_equal(r["state"], day.state)
    for col in range(4):
        assert np.array_equal(_bits(r["trans"][:, :, col]), _bits(day.trans[:, :, col])), col
    assert r["sum_tt_q16"] == O.sum_travel_time_q16(day.trans)
    worst = _worst_rel(r["trans"][trips.car, trips.hour, 2], trips.want)
    print(f"device against mpmath on {len(trips.car)} trips: worst relative error {worst:.3e}")
    assert worst <= 2 * ORACLE_WORST_DRAW


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_sums_on_the_ladder_in_every_family(cpm, O, kernel):
    """Parking, driving and the time sum of every kernel family on the ladder fixture equal O.fast_run; the grouped family (AUTO
    picks it at 50 cars per zone) draws from the sparse travel rows (CPM_INFO_TRAVEL_TABLE 2), in the one launch over the kept runs
    of all hours.  At least 100 trips on cells of every rung."""
    day = ladder_day(O)
    _rungs_visited(day.idx, day.ref["state"], "ladder day")
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(kernel)
        s.set_p_drive(day.p_drive)
        s.set_p_dest(day.p_dest)
        s.set_datamatrix(day.dm, day.dist)
        s.init_states(day.C, CPZ)
        assert s.get_info(INFO_TRAVEL_TABLE) == 0
        with pinned(s, kernel):
            assert np.array_equal(s.solve_ivp(SIM_SEED), day.ref["zone0"])
        with pinned(s, kernel):
            r = s.resample(SIM_SEED, travel=True)
        assert s.get_info(INFO_TRAVEL_TABLE) == (2 if kernel in (0, GROUPED) else 0)
    assert np.array_equal(r["parking"], day.ref["parking"])
    assert np.array_equal(r["driving"], day.ref["driving"])
    assert r["sum_tt_q16"] == day.ref["sum_tt_q16"]


@gpu
def test_compact_row_route_on_the_ladder(cpm, O):
    """dataset_edges.edge_datamatrix (Z = 358) with the ladder on its standard deviations -- the planted cells without one and the
    cell with a standard deviation and no mean stay --, tables built on the device, 30 cars per zone, grouped family: the travel
    kernel reads the travel rows of the compact dataset (CPM_INFO_TRAVEL_TABLE 1, written by k_ds_sort) and the sums equal the
    oracle's on the tables the device built.  At least 100 trips on cells of every rung."""
    Ze, cpz = 358, 30
    C = Ze * cpz
    dm, dist = E.edge_datamatrix(O, Ze, T)
    sd0 = (dm[..., 0] != 0) & (dm[..., 1] == 0)
    idx = TL.ladder_sd(dm, TL.LADDER_SEED, keep_sd0=True)
    assert (dm[..., 1][sd0] == 0).all() and sd0.sum() > 1000 and dm[11, 13, 5, 0] == 0.0 and dm[11, 13, 5, 1] == 5.0
    with cpm.Sampler(Ze, T) as s:
        s.set_kernel(GROUPED)
        s.set_datamatrix(dm, dist)
        p_drive = s.build_p_drive(0.1, 0.9, 0.5)
        p_dest = s.build_p_dest(2)
        assert s.get_info(INFO_TRAVEL_TABLE) == 1
        assert np.array_equal(p_dest, O.createpdestin(dm, Ze, T, 2))
        np.testing.assert_allclose(p_drive, O.createpdrive(dm, dist, Ze, T, 0.1, 0.9, 0.5), rtol=4e-16, atol=0, equal_nan=True)
        ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), want_state=True, datamatrix=dm, dist=dist)
        _rungs_visited(idx, ref["state"], "edge matrix")
        s.init_states(C, cpz)
        with pinned(s, GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, GROUPED, repeats=None):
            r = s.resample(SIM_SEED, travel=True)
        assert s.get_info(INFO_TRAVEL_TABLE) == 1
    assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])
    assert r["sum_tt_q16"] == ref["sum_tt_q16"]


@gpu
def test_dense_gather_route_on_the_ladder(cpm, O):
    """Z = 1,408, T = 2, density 0.3 and one origin's hour-0 row fully populated: its 1,407 cells are more than the
    (32,768 - 352) / 24 = 1,350 that fit the travel kernel's LDS next to the row's bitmap words, so the grouped path builds the dense
    table and gathers from it (CPM_INFO_TRAVEL_TABLE 3: k_build_travel_table, k_grouped_travel<false>, which computes the window's
    mass per driver).  Ladder standard deviations, 40 cars per zone; the sums equal the oracle's.  At least 100 trips per rung."""
    Zd, Td, cpz, full = 1408, 2, 40, 700
    C = Zd * cpz
    dm, dist = O.synth_datamatrix(Zd, Td, TABLE_SEED + 5, density=0.3)
    rng = np.random.default_rng(TL.LADDER_SEED + 6)
    others = np.setdiff1d(np.arange(Zd), [full])
    dm[full, others, 0, 0] = 300.0 + 2100.0 * rng.random(len(others))
    idx = TL.ladder_sd(dm, TL.LADDER_SEED + 5)
    assert (dm[full, :, 0, 0] != 0).sum() == 1407
    dm = np.asfortranarray(dm)
    p_drive = O.createpdrive(dm, dist, Zd, Td, 0.1, 0.9, 0.5)
    p_dest = O.createpdestin(dm, Zd, Td, 2)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), want_state=True, datamatrix=dm, dist=dist)
    _rungs_visited(idx, ref["state"], "dense gather")
    with cpm.Sampler(Zd, Td) as s:
        s.set_kernel(GROUPED)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.set_datamatrix(dm, dist)
        s.init_states(C, cpz)
        with pinned(s, GROUPED, repeats=None):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with pinned(s, GROUPED, repeats=None):
            r = s.resample(SIM_SEED, travel=True)
        assert s.get_info(INFO_TRAVEL_TABLE) == 3
    assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])
    assert r["sum_tt_q16"] == ref["sum_tt_q16"]


@gpu
def test_batched_resample_on_the_ladder(cpm, O):
    """Two fleets (their own p_drive and seed) on the ladder fixture with travel times, through the batched kernels: each fleet's
    counts and time sum equal its own single resample and the oracle's.  At least 100 trips per rung in each fleet."""
    day = ladder_day(O)
    tables = np.asfortranarray(np.stack([day.p_drive, O.createpdrive(day.dm, day.dist, Z, T, 0.3, 0.8, 1.0)], axis=2))
    seeds = np.array([SIM_SEED, SIM_SEED + 1], dtype=np.uint64)
    cdf = O.build_cdf(day.p_dest)
    refs = [O.fast_run(np.asfortranarray(tables[:, :, b]), cdf, day.C, int(seeds[b]), _zone0(day.C, CPZ), do_ivp=False, want_state=True,
                       datamatrix=day.dm, dist=day.dist) for b in range(2)]
    for b in range(2):
        _rungs_visited(day.idx, refs[b]["state"], f"fleet {b}")
    with cpm.Sampler(Z, T) as s:
        s.set_datamatrix(day.dm, day.dist)
        s.set_p_drive(day.p_drive)
        s.set_p_dest(day.p_dest)
        s.init_states(day.C, CPZ)
        s.set_p_drive_batch(tables)
        r = s.resample_batch(seeds, travel=True)
        rec = (s.get_info(cpm.CPM_INFO_LAST_KERNEL), s.get_info(cpm.CPM_INFO_LAST_FORM), s.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS))
        assert rec == (GROUPED, cpm.CPM_FORM_BATCH, 2), rec
        assert s.get_info(INFO_TRAVEL_TABLE) == 2
        singles = []
        for b in range(2):
            s.set_p_drive(np.asfortranarray(tables[:, :, b]))
            singles.append(s.resample(int(seeds[b]), travel=True))
    for b in range(2):
        for one in (singles[b], refs[b]):
            assert np.array_equal(r["parking"][:, :, b], one["parking"]) and np.array_equal(r["driving"][:, :, b], one["driving"]), b
            assert int(r["sum_tt_q16"][b]) == one["sum_tt_q16"], b
