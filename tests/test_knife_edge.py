"""Every form of the hour on draws that land exactly on a table edge (tests/knife_edge.py builds the days).

The reference compares with `<=` twice per car and hour (src/resampling.jl:15, :40); the tree compiles the first comparison in at least
nine places and the second in about as many.  A planted day puts hundreds of Bernoulli draws exactly on p_drive or one step (2^-53) above
it, and thousands of categorical draws exactly on a CDF breakpoint, one step behind one, exactly on a row total below 1 or one step
above it.  What each planted car must do follows from the reference's comparison and the construction alone.

CPU (not marked `gpu`): the C oracle in its fast and its faithful form and the plain Python restatement agree with every plant and
with the builder's stepper on every state; three mutants of the stepper (`<` in either comparison, the categorical on the high 32 bits
alone) change the parking counts of every day -- the evidence that the days can fail.
GPU: integer equality only.  Every arm is wrapped in `pinned`, so that it runs the form it names: the three kernel families and AUTO,
the grouped forms (CPM_OPT_FUSED 5, 0, 1, 3, 6, 8), both forms of hour T, sparse row packs of an uploaded table, cpm_debug_categorical,
the batched resample, the IVP -- counts against the oracle, and every plant read back from the per-car record of resample(paths=True),
which does not rest on the oracle.  The same on 4,000 cars whose global ids straddle 2^32 (Philox counter word c1 is car >> 32)."""
import numpy as np
import pytest

import knife_edge as K
import py_restatement as PY
from conftest import SIM_SEED
from product_form import CAR, GROUPED, MODE_FORM, ZONE_LDS, pinned

gpu = pytest.mark.gpu
AUTO = 0
INFO_SPARSE = 6      # CPM_INFO_SPARSE_TABLES
INFO_LAST_HOUR = 11  # CPM_INFO_LAST_HOUR
BIT = np.uint32(0x80000000)
MASK = np.uint32(0x7FFFFFFF)

SHAPES = {"z97": (97, 24, 40), "z403": (403, 6, 40)}       # Z no multiple of 32; the shape of tests/test_sparse_upload.py that qualifies for sparse packs, T != 24
TINY = (24, 6, 12)                                         # the plain Python restatement's day (floors waived)
# 4,000 cars across 2^32: init_states(97 * 2^27, 2^27, car_begin, 4000, car_stride)
BIG_CPZ = 1 << 27
BIG_N = 4000
BIG = {"stride1": ((1 << 32) - 2000, 1), "stride3": ((1 << 32) - 6001, 3)}
BIG_MAX_CAR = (1 << 32) + 6000                             # the bound the two ranges imply

_DAYS, _REFS = {}, {}
_NAMES = ["z97", "z403", "tiny", "stride1", "stride3"]


def _table_seed(name, kind):
    return 2 * _NAMES.index(name) + (kind == "ivp") + 1         # (a seed that misses a plant floor is changed here; the floor stays)


def _day(O, name, kind):
    """The planted day of a named case, built once and shared read-only."""
    key = (name, kind)
    if key in _DAYS:
        return _DAYS[key]
    ivp_scale = lambda T: (T - 1) / T if kind == "ivp" else 1.0
    if name in SHAPES:
        Z, T, cpz = SHAPES[name]
        n = Z * cpz
        day = K.build_day(O, Z, T, np.arange(n) // cpz + 1, np.arange(n), SIM_SEED, kind, table_seed=_table_seed(name, kind), floor_scale=ivp_scale(T))
        day["cpz"] = cpz
    elif name == "tiny":
        Z, T, cpz = TINY
        n = Z * cpz
        day = K.build_day(O, Z, T, np.arange(n) // cpz + 1, np.arange(n), SIM_SEED, kind, table_seed=_table_seed(name, kind), floor_scale=None)
        day["cpz"] = cpz
    else:
        Z, T, _ = SHAPES["z97"]
        begin, stride = BIG[name]
        cars = np.uint64(begin) + np.uint64(stride) * np.arange(BIG_N, dtype=np.uint64)
        if kind == "resample":
            zone0 = np.arange(BIG_N) % Z + 1                                           # dealt round-robin over the zones
        else:
            zone0 = (cars // np.uint64(BIG_CPZ)).astype(np.int64) + 1                  # where init_states puts them
            assert set(zone0.tolist()) == {32, 33}
        # (the floors of Z x 40 cars, scaled to 4,000 cars -- and to the T - 1 hours of an IVP)
        day = K.build_day(O, Z, T, zone0, cars, SIM_SEED, kind, table_seed=_table_seed(name, kind), floor_scale=BIG_N / (Z * 40) * ivp_scale(T), max_car=BIG_MAX_CAR)
        planted = np.array([int(cars[c]) for _, c, _, _ in day["plants"]])
        assert (planted < 1 << 32).sum() > 1000 and (planted >= 1 << 32).sum() > 1000
        day.update(cpz=BIG_CPZ, car_begin=begin, car_stride=stride)
    print(f"planted day {name} / {kind}: {day['counts']}")
    _DAYS[key] = day
    return day


def _ref(O, name, kind):
    """The oracle's fast run of a day (shared read-only): a resample day without an IVP, an IVP day with it (zone0: the post-IVP zones)."""
    key = (name, kind)
    if key not in _REFS:
        d = _day(O, name, kind)
        r = O.fast_run(d["p_drive"], O.build_cdf(d["p_dest"]), d["n"], d["seed"], d["zone0"], car_offset=d.get("car_begin", 0),
                       car_stride=d.get("car_stride", 1), do_ivp=kind == "ivp", want_state=True)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REFS[key] = r
    return _REFS[key]


def _faithful(O, d):
    """state and transition matrix of the faithful oracle (contiguous cars only: it takes an offset, no stride)"""
    assert d.get("car_stride", 1) == 1
    st, tr = O.initializestates(d["n"], d["cpz"], d["T"], car_offset=d.get("car_begin", 0))
    st[:, 0] = d["zone0"]
    if d["kind"] == "ivp":
        O.solveinitialvalueproblem(st, tr, d["p_drive"], d["p_dest"], d["n"], d["Z"], d["seed"], car_offset=d.get("car_begin", 0))
    else:
        O.resampling(st, tr, d["n"], d["Z"], d["p_drive"], d["p_dest"], None, None, d["seed"], car_offset=d.get("car_begin", 0))
    return st, tr


def _no_bad(bad, where):
    assert not bad, f"{where}: {len(bad)} plants do not hold; (hour, car, kind, expected, drove, destination) {bad[:8]}"


# ================================================================================================ CPU
ALL_DAYS = [(n, k) for n in ("z97", "z403") for k in ("resample", "ivp")]


@pytest.mark.parametrize("name,kind", ALL_DAYS + [("stride1", "resample"), ("stride1", "ivp")])
def test_both_forms_of_the_c_oracle_agree_with_every_plant_and_the_stepper(O, name, kind):
    d = _day(O, name, kind)
    T, hours = d["T"], d["hours"]
    mine = K.run(d)
    _no_bad(K.plants_hold(d, mine["drove"], mine["dest"] - 1), "stepper")
    st, tr = _faithful(O, d)
    assert np.array_equal(st, mine["state"])
    assert np.array_equal(tr[:, :hours, 0] == 1, mine["drove"]) and np.array_equal(tr[:, :hours, 1].astype(np.int64), mine["dest"])
    _no_bad(K.plants_hold(d, tr[:, :hours, 0] == 1, tr[:, :hours, 1].astype(np.int64) - 1), "faithful oracle")
    r = _ref(O, name, kind)
    if kind == "ivp":
        assert np.array_equal(r["zone0"], mine["state"][:, T - 1])
    else:
        assert np.array_equal(r["state"], mine["state"])
        assert np.array_equal(r["parking"], mine["parking"]) and np.array_equal(r["driving"], mine["driving"])
        # the fast form keeps no transitions: a planted destination of an applied hour is the car's next state
        for t, c, k, e in d["plants"]:
            if k not in (K.DRIVES, K.STAYS) and t + 1 < T:
                assert r["state"][c, t + 1] - 1 == e, (t, c, k, e)


def test_the_strided_fleet_across_2_32_in_the_fast_oracle(O):
    """(the faithful form takes no stride: the fast one and the stepper)"""
    for kind in ("resample", "ivp"):
        d, r = _day(O, "stride3", kind), _ref(O, "stride3", kind)
        mine = K.run(d)
        _no_bad(K.plants_hold(d, mine["drove"], mine["dest"] - 1), "stepper")
        if kind == "ivp":
            assert np.array_equal(r["zone0"], mine["state"][:, d["T"] - 1])
        else:
            assert np.array_equal(r["state"], mine["state"]) and np.array_equal(r["driving"], mine["driving"])


def test_the_plain_python_restatement_agrees_with_every_plant_and_the_stepper(O):
    d = _day(O, "tiny", "resample")
    Z, T, n = d["Z"], d["T"], d["n"]
    assert min(d["counts"].values()) >= 10, d["counts"]           # (floors waived, every kind still present)
    st, tr = O.initializestates(n, d["cpz"], T)
    assert np.array_equal(st[:, 0], d["zone0"])
    PY.resampling(st, tr, d["p_drive"], d["p_dest"], n, Z, T, lambda i, t: O.uniforms(d["seed"], i - 1, T - 1 + t - 1, 0))
    mine = K.run(d)
    assert np.array_equal(st, mine["state"]) and np.array_equal(tr[:, :, 0] == 1, mine["drove"])
    assert np.array_equal(tr[:, :, 1].astype(np.int64), mine["dest"])
    _no_bad(K.plants_hold(d, tr[:, :, 0] == 1, tr[:, :, 1].astype(np.int64) - 1), "py_restatement")
    pk, dr = PY.histogram(Z, T, st, tr, n)
    assert np.array_equal(pk.astype(np.int64), mine["parking"]) and np.array_equal(dr.astype(np.int64), mine["driving"])


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_a_wrong_comparison_changes_the_parking_counts_of_every_day(O, mutant):
    for name, kind in ALL_DAYS + [("tiny", "resample")] + [(n, k) for n in BIG for k in ("resample", "ivp")]:
        d = _day(O, name, kind)
        good, wrong = K.run(d), K.run(d, mutant)
        changed = int((good["parking"] != wrong["parking"]).sum())
        print(f"{mutant}: {name} / {kind}: {changed} parking counts change, {len(K.plants_hold(d, wrong['drove'], wrong['dest'] - 1))} plants fail")
        assert changed > 0, (name, kind)
        assert K.plants_hold(d, wrong["drove"], wrong["dest"] - 1), (name, kind)


# ================================================================================================ GPU
def _sampler(cpm, d, sparse=False):
    s = cpm.Sampler(d["Z"], d["T"])
    if sparse:
        s.set_sparse_upload(True)
    s.set_p_drive(d["p_drive"])
    s.set_p_dest(d["p_dest"])
    assert (s.get_info(INFO_SPARSE) > 0) == sparse
    return s


def _start(s, d):
    """the day's cars in the day's start state (a resample day: installed with set_state; an IVP day: init_states' own)"""
    if "car_begin" in d:
        s.init_states(d["Z"] * BIG_CPZ, BIG_CPZ, car_begin=d["car_begin"], car_count=d["n"], car_stride=d["car_stride"])
    else:
        s.init_states(d["n"], d["cpz"])
    if d["kind"] == "resample":
        s.set_state(d["zone0"])
    assert np.array_equal(s.get_state(), d["zone0"])


def _same_counts(r, ref, where):
    assert np.array_equal(r["parking"], ref["parking"]), f"{where}: parking"
    assert np.array_equal(r["driving"], ref["driving"]), f"{where}: driving"


def _check_paths(d, r, where):
    """every plant, read back from the per-car record (which does not rest on the oracle)"""
    p = r["paths"]
    assert p.shape == (d["T"], d["n"])
    _no_bad(K.plants_hold(d, ((p & BIT) != 0).T, (p & MASK).astype(np.int64).T), where)


def _paths_step(s, d, ref, kernel, where, **pin):
    with pinned(s, kernel, repeats=None, **pin) as rec:
        r = s.resample(d["seed"], paths=True)
    _same_counts(r, ref, where)
    _check_paths(d, r, where)
    return rec


@gpu
@pytest.mark.parametrize("kernel", [CAR, ZONE_LDS, GROUPED, AUTO], ids=["car", "zone_lds", "grouped", "auto"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_families_on_the_resample_day(cpm, O, name, kernel):
    d, ref = _day(O, name, "resample"), _ref(O, name, "resample")
    with _sampler(cpm, d) as s:
        s.set_kernel(kernel)
        _start(s, d)
        rec = _paths_step(s, d, ref, kernel, f"{name} kernel {kernel}")
        assert rec["kernel"] == (GROUPED if kernel == AUTO else kernel), rec      # (40 cars per zone: AUTO resolves to the grouped family)
        with pinned(s, kernel, repeats=None):                                     # the plain resample: hour T in its default form
            _same_counts(s.resample(d["seed"]), ref, f"{name} kernel {kernel}, plain")


@gpu
@pytest.mark.parametrize("mode", [5, 0, 1, 3, 6, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_grouped_forms_on_the_resample_day(cpm, O, name, mode):
    d, ref = _day(O, name, "resample"), _ref(O, name, "resample")
    with _sampler(cpm, d) as s:
        s.set_kernel(GROUPED)
        s.set_fused(mode)
        _start(s, d)
        if mode != 5:
            assert s.get_info(cpm.CPM_INFO_FUSED) == MODE_FORM[mode], f"fused mode {mode} has no instantiation at Z = {d['Z']}"
        rec = _paths_step(s, d, ref, GROUPED, f"{name} fused {mode}", fused=mode)
        print(f"{name} fused mode {mode}: {rec}")
        with pinned(s, GROUPED, fused=mode, repeats=None):
            _same_counts(s.resample(d["seed"]), ref, f"{name} fused {mode}, plain")


def _last_column_bernoulli_plants(d, ref):
    """Bernoulli plants of column T that discriminate, judged from the ORACLE's state: the car stands in a zone whose p_drive is its own
    draw (it drives) or one step below it (it must not)"""
    T = d["T"]
    n = 0
    for t, c, k, _ in d["plants"]:
        if t == T - 1 and k in (K.DRIVES, K.STAYS):
            edge = int(d["m_drive"][ref["state"][c, T - 1] - 1, T - 1])
            n += edge == int(d["kb"][c, T - 1]) - (k == K.STAYS)
    return n


@gpu
@pytest.mark.parametrize("count_only", [False, True], ids=["plain", "count_only"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_both_forms_of_hour_T(cpm, O, name, count_only):
    d, ref = _day(O, name, "resample"), _ref(O, name, "resample")
    T = d["T"]
    assert _last_column_bernoulli_plants(d, ref) >= 20
    with _sampler(cpm, d) as s:
        s.set_kernel(GROUPED)
        s.set_last_hour(count_only)
        _start(s, d)
        with pinned(s, GROUPED, repeats=None):
            r = s.resample(d["seed"])
        assert s.get_info(INFO_LAST_HOUR) == int(count_only)
        assert np.array_equal(r["driving"][:, T - 1], ref["driving"][:, T - 1]), "driving counts of hour T"
        _same_counts(r, ref, f"{name} last hour {count_only}")


@gpu
@pytest.mark.parametrize("mode", [5, 1, 6])
def test_sparse_row_packs_of_the_uploaded_table(cpm, O, mode):
    d, ref = _day(O, "z403", "resample"), _ref(O, "z403", "resample")
    with _sampler(cpm, d, sparse=True) as s:
        s.set_kernel(GROUPED)
        s.set_fused(mode)
        _start(s, d)
        if mode != 5:
            assert s.get_info(cpm.CPM_INFO_FUSED) == MODE_FORM[mode]
        _paths_step(s, d, ref, GROUPED, f"sparse fused {mode}", fused=mode)
        for count_only in (True, False):
            s.set_last_hour(count_only)
            with pinned(s, GROUPED, fused=mode, repeats=None):
                _same_counts(s.resample(d["seed"]), ref, f"sparse fused {mode}, plain, count-only {count_only}")
        assert s.get_info(INFO_SPARSE) > 0


@gpu
@pytest.mark.parametrize("name,sparse", [("z97", False), ("z403", False), ("z403", True)], ids=["z97", "z403", "z403_sparse"])
def test_debug_categorical_on_planted_rows(cpm, O, name, sparse):
    d = _day(O, name, "resample")
    state = K.run(d)["state"]
    rows = {}
    for t, c, k, e in d["plants"]:
        if k not in (K.DRIVES, K.STAYS):
            rows.setdefault((t, int(state[c, t])), []).append((int(d["kc"][c, t]), e))
    keys = sorted(rows)
    keys = [keys[i] for i in np.linspace(0, len(keys) - 1, 10).astype(int)]
    total_exact = 0
    with _sampler(cpm, d, sparse=sparse) as s:
        for t, z in keys:
            kc = np.array([k for k, _ in rows[t, z]], dtype=np.int64)
            planted = np.array([e for _, e in rows[t, z]], dtype=np.int64)
            probes = np.concatenate([kc, kc - 1, kc + 1])
            got, n_exact = s.debug_categorical(z, t + 1, probes.astype(np.uint64))
            assert np.array_equal(got[:kc.shape[0]] - 1, planted), (t, z)                       # by construction
            assert np.array_equal(got - 1, K.categorical(d["m_dest"][z - 1, :, t], probes)), (t, z)
            total_exact += n_exact
    assert total_exact > 0


@gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_batched_resample_with_every_edge_moved_the_other_way(cpm, O, name):
    d, ref = _day(O, name, "resample"), _ref(O, name, "resample")
    flipped = K.flipped_p_drive(d)
    tables = np.asfortranarray(np.stack([d["p_drive"], flipped, d["p_drive"]], axis=2))
    seeds = np.array([d["seed"], d["seed"], d["seed"] + 1], dtype=np.uint64)
    cdf = O.build_cdf(d["p_dest"])
    refs = [ref] + [O.fast_run(np.asfortranarray(tables[:, :, b]), cdf, d["n"], int(seeds[b]), d["zone0"], do_ivp=False) for b in (1, 2)]
    # fleet 1 in the first hour, where the fleets still stand alike: every planted zone drives one car less, or one more
    for t, c, k, _ in d["plants"]:
        if t == 0 and k in (K.DRIVES, K.STAYS):
            z = d["zone0"][c] - 1
            assert refs[1]["driving"][z, 0] - ref["driving"][z, 0] == (-1 if k == K.DRIVES else 1)
    with _sampler(cpm, d) as s:
        _start(s, d)
        s.set_p_drive_batch(tables)
        r = s.resample_batch(seeds)
        rec = dict(kernel=s.get_info(cpm.CPM_INFO_LAST_KERNEL), form=s.get_info(cpm.CPM_INFO_LAST_FORM), fleets=s.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS))
        assert rec == dict(kernel=GROUPED, form=cpm.CPM_FORM_BATCH, fleets=3), rec
    for b in range(3):
        assert np.array_equal(r["parking"][:, :, b], refs[b]["parking"]), f"fleet {b}: parking"
        assert np.array_equal(r["driving"][:, :, b], refs[b]["driving"]), f"fleet {b}: driving"


@gpu
@pytest.mark.parametrize("kernel", [CAR, ZONE_LDS, GROUPED], ids=["car", "zone_lds", "grouped"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_ivp_day(cpm, O, name, kernel):
    d, ref = _day(O, name, "ivp"), _ref(O, name, "ivp")
    hours = d["hours"]
    _, tr = _faithful(O, d)                                  # every plant holds in the faithful oracle's transition matrix of this IVP
    _no_bad(K.plants_hold(d, tr[:, :hours, 0] == 1, tr[:, :hours, 1].astype(np.int64) - 1), "faithful oracle")
    with _sampler(cpm, d) as s:
        s.set_kernel(kernel)
        _start(s, d)
        with pinned(s, kernel, repeats=None):
            got = s.solve_ivp(d["seed"])
        assert np.array_equal(got, ref["zone0"])


# ------------------------------------------------------------------------------------------------ car ids across 2^32
@gpu
@pytest.mark.parametrize("arm", ["car", "zone_lds", "grouped", "fused0", "fused1"])
@pytest.mark.parametrize("name", list(BIG))
def test_car_ids_across_2_32_on_the_resample_day(cpm, O, name, arm):
    d, ref = _day(O, name, "resample"), _ref(O, name, "resample")
    kernel = {"car": CAR, "zone_lds": ZONE_LDS}.get(arm, GROUPED)
    mode = {"fused0": 0, "fused1": 1}.get(arm, 5)
    with _sampler(cpm, d) as s:
        s.set_kernel(kernel)
        s.set_fused(mode)
        _start(s, d)
        if mode == 1:
            assert s.get_info(cpm.CPM_INFO_FUSED) == 1
        _paths_step(s, d, ref, kernel, f"{name} {arm}", fused=mode)
        if arm.startswith("fused"):
            for count_only in (False, True):
                s.set_last_hour(count_only)
                with pinned(s, kernel, fused=mode, repeats=None):
                    _same_counts(s.resample(d["seed"]), ref, f"{name} {arm}, count-only {count_only}")
                assert s.get_info(INFO_LAST_HOUR) == int(count_only)


@gpu
@pytest.mark.parametrize("kernel", [CAR, GROUPED], ids=["car", "grouped"])
@pytest.mark.parametrize("name", list(BIG))
def test_car_ids_across_2_32_on_the_ivp_day(cpm, O, name, kernel):
    """All the cars start in zones 32 and 33: buckets of 2,000 cars, which may grow the regions (repeats not checked)."""
    d, ref = _day(O, name, "ivp"), _ref(O, name, "ivp")
    with _sampler(cpm, d) as s:
        s.set_kernel(kernel)
        _start(s, d)
        with pinned(s, kernel, repeats=None):
            got = s.solve_ivp(d["seed"])
        assert np.array_equal(got, ref["zone0"])
