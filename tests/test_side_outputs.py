"""The side outputs of the fused resample -- dense and CSR flows, stays / parked, the per-car record and its expansion -- where the
per-feature suites (test_flows.py, test_flows_csr.py, test_stays.py, test_paths.py) do not go:

  A  heavy buckets: runs filled by k_grouped_sample AND k_grouped_sample_heavy (CPM_INFO_PARTS > 1), one-launch forms off;
  B  the random small problems of test_gpu_parity.py::test_randomized_small_configurations (T = 1, 2, 5, one car per zone, NaN / 0 / 1
     in p_drive, all-zero and single-destination rows, unreachable zones), every output instead of the counts alone;
  C  one context asked a fixed sequence of steps of every kind, so that every kind follows every other one;
  D  contiguous shards whose begin is off a zone boundary and whose size is no multiple of 4;
  E  a one-launch hour that bails out: the output returned is that of the repeated attempt.

Expected values come from tests/side_reference.py (the faithful oracle recipe, every output derived from its matrices in numpy);
every comparison is exact.  GPU tests are marked `gpu` and wrap every step in `pinned`; the host-only tests run without a GPU."""
import numpy as np
import pytest

import side_reference as R
from conftest import SIM_SEED, TABLE_SEED
from product_form import CAR, GROUPED, MODE_FORM, at_least, pinned
from test_paths import _HAND, _HAND_FLOWS, _HAND_PATHS
from test_stays import _HAND_PARKED, _HAND_STAYS

gpu = pytest.mark.gpu
T24 = 24


# ------------------------------------------------------------------------------------------------ one step of any kind
def _counts_of_dev(s, d_counts):
    """the count tensor of a device-resident step (parking | driving | sum_tt_q16 | status): the status word is clean"""
    Z, T = s.Z, s.T
    c = d_counts.cpu().numpy()
    assert c[-1] == 0, f"status word {c[-1]}"
    return dict(parking=np.asfortranarray(c[:Z * T].reshape(T, Z).T), driving=np.asfortranarray(c[Z * T:2 * Z * T].reshape(T, Z).T),
                sum_tt_q16=int(c[2 * Z * T]))


def _step(s, kind, seed, ref, travel=False, dev=False):
    """One resample of `kind` (side_reference.KINDS) on context s: the blocking call or, dev=True, the device-resident form into
    torch tensors pre-filled with -1 (paths: resample_paths_dev + paths_expand_dev, so the result carries state and trans too)."""
    Z, T, n = s.Z, s.T, s.car_count
    if not dev:
        if kind == "compat":
            r = s.resample(seed, travel=travel, want_state=True, want_trans=True)
        else:
            kw = {"plain": {}, "travel": {}, "flows": dict(flows=True), "csr": dict(flows="csr"), "stays": dict(stays=True), "paths": dict(paths=True)}[kind]
            r = s.resample(seed, travel=travel, **kw)
        r["travel"] = travel
        return r
    import torch
    new = lambda shape, dtype, fill=-1: torch.full(shape, fill, dtype=dtype, device="cuda")
    d_counts = new((s.counts_words(),), torch.int64)
    if kind == "stays":
        d_stays, d_parked = new((T * Z * T,), torch.int32), new((Z * T,), torch.int32)
        torch.cuda.synchronize()
        s.resample_stays_dev(seed, d_counts.data_ptr(), d_stays.data_ptr(), d_parked.data_ptr(), travel=travel)
        s.sync()
        r = _counts_of_dev(s, d_counts)
        r.update(stays=d_stays.cpu().numpy().reshape(T, Z, T), parked=d_parked.cpu().numpy().reshape(Z, T))
    elif kind == "paths":
        d_paths, d_state, d_trans = new((T * n,), torch.int32), new((T, n), torch.int64), new((4, T, n), torch.float64, -1.0)
        torch.cuda.synchronize()
        s.resample_paths_dev(seed, d_counts.data_ptr(), d_paths.data_ptr(), travel=travel)
        s.paths_expand_dev(seed, d_paths.data_ptr(), d_state.data_ptr(), d_trans.data_ptr(), travel=travel)
        s.sync()
        r = _counts_of_dev(s, d_counts)
        r.update(paths=np.ascontiguousarray(d_paths.cpu().numpy().view(np.uint32).reshape(T, n)), state=d_state.cpu().numpy().T,
                 trans=d_trans.cpu().numpy().transpose(2, 1, 0))
    elif kind == "csr":
        nnz, GUARD, PAD = int(ref["flows_csr"]["row_ptr"][-1]), -7, 64
        d_row_ptr = new((T * Z + 1,), torch.int64)
        d_dest, d_count = new((nnz + PAD,), torch.int32, GUARD), new((nnz + PAD,), torch.int32, GUARD)
        torch.cuda.synchronize()
        s.resample_flows_csr_dev(seed, d_counts.data_ptr(), d_row_ptr.data_ptr(), d_dest.data_ptr(), d_count.data_ptr(), nnz, travel=travel)
        s.sync()
        r = _counts_of_dev(s, d_counts)
        dest, count = d_dest.cpu().numpy(), d_count.cpu().numpy()
        assert (dest[nnz:] == GUARD).all() and (count[nnz:] == GUARD).all()            # nothing stored at or behind cap
        r.update(flows_csr=dict(row_ptr=d_row_ptr.cpu().numpy(), dest=dest[:nnz].copy(), count=count[:nnz].copy(), shape=(T, Z, Z)))
    else:
        raise ValueError(f"no device-resident form of {kind!r} here")
    r["travel"] = travel
    return r


def _check_step(kind, r, ref, dev=False, where=None, cars=slice(None)):
    R.check(kind, r, ref, cars, where)
    if r["travel"]:
        R.check("travel", r, ref, cars, where)
    if dev and kind == "paths":
        R.check("compat", r, ref, cars, where)


def _sampler(cpm, ref, dm=None, dist=None, kernel=None):
    s = cpm.Sampler(ref["Z"], ref["T"])
    if dm is not None:
        s.set_datamatrix(dm, dist)
    s.set_p_drive(ref["p_drive"])
    s.set_p_dest(ref["p_dest"])
    if kernel is not None:
        s.set_kernel(kernel)
    return s


_REFS = {}


def _shared(key, make):
    """a reference computed once and shared, unchanged (side_reference.reference returns read-only arrays)"""
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _synth_ref(O, Z, cpz, T, seed, skew_q=0, density=None):
    def make():
        dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=density) if density else (None, None)
        ref = R.reference(O, O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED, skew_q=skew_q), Z, cpz, T, seed, ivp_seed=SIM_SEED,
                          dm=dm, dist=dist)
        ref.update(dm=dm, dist=dist)
        return ref
    return _shared(("synth", Z, cpz, T, seed, skew_q, density), make)


# ------------------------------------------------------------------------------------------------ A: heavy buckets
HEAVY = (128, 160, 2)          # Z, cars per zone, skew_q


@gpu
def test_every_side_output_of_heavy_buckets(cpm, O):
    """Z = 128 x 160 cars per zone on Zipf-Mandelbrot destinations (skew_q = 2): the largest bucket is about 20 x the mean, 12 workgroups'
    slots, so the runs the side-output kernels read are filled by both sampler kernels and the one-launch forms are off.  After an IVP
    and a plain resample every kind runs without a repeat, with and without travel times, CPM_INFO_PARTS >= 2, hour T in its
    run-producing form (CPM_INFO_LAST_HOUR 0).  Then two fresh contexts whose very first step is a paths / a stays resample: it meets
    the heavy buckets, outgrows its regions and returns the output of the attempt that counted."""
    Z, cpz, q = HEAVY
    ref = _synth_ref(O, Z, cpz, T24, SIM_SEED, skew_q=q, density=0.9)
    print(f"heavy: largest bucket {int(ref['parking'].max())} = {ref['parking'].max() / cpz:.1f} x the mean, "
          f"{int((ref['parking'] > 1024).sum(axis=0).max())} buckets above 1,024 in one hour, in {int((ref['parking'] > 1024).any(axis=0).sum())} hours")
    assert ref["parking"].max() > 5 * 256 and ref["parking"].max() < 32 * cpz
    # one origin sends more than the 128 entries of a pass to ONE destination, hour T included: runs of several passes, whatever the grouping
    assert ref["flows"].max() > 4 * 128 and ref["flows"][T24 - 1].max() > 128
    with _sampler(cpm, ref, ref["dm"], ref["dist"], kernel=5) as s:
        s.init_states(Z * cpz, cpz)
        with pinned(s, 5, repeats=None, parts=at_least(2)) as step:
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        print(f"heavy: the IVP ended on {step}")
        with pinned(s, 5, repeats=None, parts=at_least(2)) as step:
            _check_step("plain", _step(s, "plain", SIM_SEED, ref), ref)
        print(f"heavy: the first resample ended on {step}")
        for travel in (False, True):
            for kind, kept in (("flows", False), ("flows", True), ("csr", False), ("stays", False), ("paths", False)):
                s.set_flows_kept(kept)
                with pinned(s, 5, repeats=0, parts=at_least(2)):
                    r = _step(s, kind, SIM_SEED, ref, travel=travel)
                assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 0, (kind, kept, travel)
                _check_step(kind, r, ref, where=(kept, travel))
        with pinned(s, 5, repeats=0, parts=at_least(2)) as step:
            r = _step(s, "paths", SIM_SEED, ref, travel=True, dev=True)
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 0
        _check_step("paths", r, ref, dev=True)
        print(f"heavy: cap_mult {step['cap_mult']}, parts {step['parts']} at the end")
    for kind in ("paths", "stays"):
        with _sampler(cpm, ref, ref["dm"], ref["dist"], kernel=5) as s:
            s.init_states(Z * cpz, cpz)
            s.set_state(ref["zone0"])
            with pinned(s, 5, family=GROUPED, repeats=at_least(1), parts=at_least(2)) as step:
                r = _step(s, kind, SIM_SEED, ref)
            print(f"heavy: a first {kind} resample ended on {step}")
            _check_step(kind, r, ref)


# ------------------------------------------------------------------------------------------------ B: random small problems
def _tiny_tables():
    """Z = 3, one car per zone, T = 2: n = 3 < 4 cars.  Zone 1 always sends its car to zone 2; zone 2 drives half the time, to zone 1 or
    3; zone 3 keeps its car in hour 0 (p_drive 0) and has an all-zero p_dest row in hour 1 (a trip inside the zone)."""
    p_drive = np.asfortranarray([[1.0, 1.0], [0.5, 0.5], [0.0, 1.0]])
    p_dest = np.zeros((3, 3, 2), order="F")
    p_dest[0, 1, :] = 1.0
    p_dest[1, 0, :] = 0.5
    p_dest[1, 2, :] = 0.5
    return dict(Z=3, T=2, cpz=1, p_drive=p_drive, p_dest=p_dest)


# (seed of side_reference.random_tables, T override, cars-per-zone override); the drawn seeds hold T = 24 only at 7 cars per zone
SMALL_CASES = [(seed, None, None) for seed in range(24)] + [(13, 24, 120), (17, 24, 40), (1, 7, 41), ("tiny", None, None)]
_TABLES = {}


def _small_tables(case):
    if case not in _TABLES:
        _TABLES[case] = _tiny_tables() if case[0] == "tiny" else R.random_tables(*case)
    return _TABLES[case]


def _case_id(case):
    return "-".join(str(v) for v in case if v is not None)


def test_the_small_cases_cover_the_shapes_they_are_there_for():
    shapes = [_small_tables(case) for case in SMALL_CASES]
    for want_T in (1, 2, 5, 7):
        assert any(sh["T"] == want_T for sh in shapes), want_T
    assert any(sh["T"] == 24 and sh["cpz"] >= 40 for sh in shapes)
    assert any(sh["cpz"] == 1 for sh in shapes)
    assert any(sh["Z"] * sh["cpz"] < 4 for sh in shapes)
    assert any((4 * sh["Z"] * sh["cpz"]) % 16 != 0 for sh in shapes)
    assert any(np.isnan(sh["p_drive"]).any() for sh in shapes)
    assert any((sh["p_dest"].sum(axis=1) == 0).any() for sh in shapes)              # all-zero rows
    assert any((sh["p_dest"].sum(axis=(0, 2)) == 0).any() for sh in shapes)         # a zone nobody reaches
    # the generator is the one of test_gpu_parity.py: the shapes of seeds 0 .. 23 as drawn there
    drawn = [_small_tables((seed, None, None)) for seed in range(24)]
    assert sorted(seed for seed, sh in enumerate(drawn) if sh["cpz"] == 1) == [4, 11, 12, 18, 19]
    assert [seed for seed, sh in enumerate(drawn) if sh["T"] == 1] == [3, 4, 5, 7, 8, 9, 10, 16, 19, 22]
    assert [sum(sh["T"] == t for sh in drawn) for t in (1, 2, 5, 24)] == [10, 8, 4, 2]
    assert [(seed, sh["cpz"]) for seed, sh in enumerate(drawn) if sh["T"] == 24] == [(13, 7), (17, 7)]     # (hence the overrides)
    assert [seed for seed, sh in enumerate(drawn) if not np.isnan(sh["p_drive"]).any()] == [5, 7, 9]


@gpu
@pytest.mark.parametrize("case", SMALL_CASES, ids=_case_id)
def test_every_side_output_of_randomized_small_configurations(cpm, O, case):
    """Kernel 5 and AUTO, each on one context: the IVP, a plain resample (either may grow the regions), then flows, CSR flows, stays,
    paths and the device-resident paths with their expansion, none of which repeats anything."""
    sh = _small_tables(case)
    Z, T, cpz = sh["Z"], sh["T"], sh["cpz"]
    seed = SIM_SEED + (case[0] if isinstance(case[0], int) else 99)
    ref = _shared(("small", case), lambda: R.reference(O, sh["p_drive"], sh["p_dest"], Z, cpz, T, seed))
    if isinstance(case[0], int):
        assert (ref["flows"][:, np.arange(Z), np.arange(Z)] > 0).any()              # trips inside a zone occur
    told = []
    for kernel in (5, 0):
        with _sampler(cpm, ref, kernel=kernel) as s:
            s.init_states(Z * cpz, cpz)
            with pinned(s, kernel, repeats=None) as ivp:
                assert np.array_equal(s.solve_ivp(seed), ref["zone0"]), (kernel, Z, T, cpz)
            with pinned(s, kernel, repeats=None) as first:
                _check_step("plain", _step(s, "plain", seed, ref), ref, where=(kernel, Z, T, cpz))
            for kind, dev in (("flows", False), ("csr", False), ("stays", False), ("paths", False), ("paths", True)):
                with pinned(s, kernel, repeats=0):
                    r = _step(s, kind, seed, ref, dev=dev)
                _check_step(kind, r, ref, dev=dev, where=(kernel, Z, T, cpz, dev))
            told.append(f"kernel {kernel}: ivp {ivp['kernel']}/{ivp['form']} resample {first['kernel']}/{first['form']} repeats {first['repeats']}")
    print(f"case {_case_id(case)} Z={Z} T={T} cpz={cpz}: " + "; ".join(told))


# ------------------------------------------------------------------------------------------------ C: a mixed sequence on one context
CORE = ("plain", "flows", "csr", "stays", "paths", "compat")
FUSED_MODES = (5, 0, 1, 3, 6)
SMALL, BIG = 40, 120            # cars per zone of the two fleets of the sequence (Z = 67)


def _euler(kinds):
    """an Eulerian circuit of the complete directed graph on `kinds` (Hierholzer): every ordered pair of distinct kinds is one edge"""
    out = {a: [b for b in kinds if b != a] for a in kinds}
    stack, circuit = [kinds[0]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop(0))
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def _sequence():
    """The steps of test C, in order: dicts of kind (CORE or "batch"), k (seed SIM_SEED + k), travel, dev, fused, kept, last_hour, cpz
    and fresh (the first step after the fleet changed).  The circuit gives every ordered pair of kinds; what is put in between keeps the
    pairs around it: a batch after a step X is followed by X again, and the block of the two fleet changes -- paths, stays on the large
    fleet, stays, paths back on the small one -- stands behind a paths step."""
    kinds = _euler(CORE)
    steps = []
    changed = False
    # where the extras go (the host-only test below holds what they must keep): the fleet changes behind the first paths step of the
    # circuit's second third, so that steps of every kind run before, between (on the large fleet) and after them; one batch in
    # the first third, on regions only the IVP and a few steps have touched, and one in the last, behind both fleet changes
    for i, kind in enumerate(kinds):
        steps.append(dict(kind=kind, cpz=SMALL))
        if kind == "paths" and not changed and i >= 10:
            steps += [dict(kind="paths", cpz=BIG, fresh=True), dict(kind="stays", cpz=BIG), dict(kind="stays", cpz=SMALL, fresh=True),
                      dict(kind="paths", cpz=SMALL)]
            changed = True
        elif i in (5, 21):
            steps += [dict(kind="batch", cpz=SMALL), dict(kind=kind, cpz=SMALL)]
    seen = {}
    for i, st in enumerate(steps):
        kind = st["kind"]
        seen[kind] = seen.get(kind, 0) + 1
        st.setdefault("fresh", False)
        st.update(i=i, k=i % 3, travel=(i % 4 == 1 and kind != "batch"), fused=FUSED_MODES[(i // 2) % 5], kept=(i // 3) % 2 == 1, last_hour=(i // 5) % 2 == 0)
        # every second stays / paths / csr step takes the device-resident form (which cannot repair: never right after a fleet change)
        st["dev"] = kind in ("stays", "paths", "csr") and seen[kind] % 2 == 0 and st["cpz"] == SMALL and not st["fresh"]
    return steps


def test_the_sequence_holds_every_ordered_pair_of_kinds_and_every_variant_twice():
    steps = _sequence()
    kinds = [st["kind"] for st in steps]
    pairs = {(a, b) for a, b in zip(kinds, kinds[1:]) if a in CORE and b in CORE and a != b}
    assert pairs == {(a, b) for a in CORE for b in CORE if a != b} and len(pairs) == 30 and len(steps) >= 31
    assert all(a["k"] != b["k"] for a, b in zip(steps, steps[1:]))                     # consecutive steps: different seeds
    assert sum(st["travel"] for st in steps) >= 2 and kinds.count("batch") >= 2
    for kind in ("stays", "paths", "csr"):
        assert sum(st["dev"] for st in steps if st["kind"] == kind) >= 2, kind
    for mode in FUSED_MODES:
        assert sum(st["fused"] == mode for st in steps) >= 2, mode
    for key in ("kept", "last_hour"):
        assert sum(st[key] for st in steps) >= 2 and sum(not st[key] for st in steps) >= 2, key
    # after a csr step another kind runs before the next csr step
    assert all(not (a["kind"] == "csr" and b["kind"] == "csr") for a, b in zip(steps, steps[1:]))
    # the fleet changes twice: to the large fleet (paths, stays), and back (stays, paths)
    change = [i for i, st in enumerate(steps) if st["fresh"]]
    assert len(change) == 2 and change[1] == change[0] + 2
    a = change[0]
    assert [(st["kind"], st["cpz"]) for st in steps[a:a + 4]] == [("paths", BIG), ("stays", BIG), ("stays", SMALL), ("paths", SMALL)]
    assert all(st["cpz"] == SMALL for st in steps[:a] + steps[a + 4:])
    assert not any(st["dev"] for st in steps if st["fresh"])


@gpu
def test_a_step_does_not_depend_on_the_step_before_it(cpm, O):
    """Z = 67, T = 24, AUTO (the grouped family), one context for the whole sequence of `_sequence`: every step against the reference of
    its seed, pinned without a repeat (but the first after a fleet change), and the state left as it was."""
    Z, T = 67, T24
    steps = _sequence()
    ref_of = lambda cpz, k: _synth_ref(O, Z, cpz, T, SIM_SEED + k, density=0.9)
    base = ref_of(SMALL, 0)
    skipped, ran = set(), {mode: 0 for mode in FUSED_MODES}
    with _sampler(cpm, base, base["dm"], base["dist"]) as s:
        s.init_states(Z * SMALL, SMALL)
        with pinned(s, 0, family=GROUPED):
            assert np.array_equal(s.solve_ivp(SIM_SEED), base["zone0"])
        s.set_p_drive_batch(np.stack([base["p_drive"], base["p_drive"]], axis=2))
        cpz = SMALL
        for st in steps:
            kind, where = st["kind"], str(st)
            if st["cpz"] != cpz:
                cpz = st["cpz"]
                s.init_states(Z * cpz, cpz)
                s.set_state(ref_of(cpz, 0)["zone0"])
            ref = ref_of(cpz, st["k"])
            mode = st["fused"]
            s.set_fused(mode)
            if mode not in (5, 0) and s.get_info(cpm.CPM_INFO_FUSED) != MODE_FORM[mode]:    # (as tests/test_stays.py: no instantiation at this shape)
                skipped.add(mode)
                mode = 5
                s.set_fused(5)
            ran[mode] += 1
            s.set_flows_kept(st["kept"])
            s.set_last_hour(st["last_hour"])
            if kind == "batch":
                before = s.last_step()
                rb = s.resample_batch((SIM_SEED, SIM_SEED + 1), travel=st["travel"])
                after = s.last_step()
                assert (after["kernel"], after["form"], after["batch_fleets"]) == (GROUPED, cpm.CPM_FORM_BATCH, 2), (where, after)
                assert after["repeats"] == before["repeats"] and after["bailouts"] == before["bailouts"], (where, before, after)
                for b in (0, 1):
                    one = dict(parking=np.asfortranarray(rb["parking"][:, :, b]), driving=np.asfortranarray(rb["driving"][:, :, b]))
                    R.check("plain", one, ref_of(cpz, b), where=(where, b))
            else:
                family = CAR if kind == "compat" else GROUPED
                with pinned(s, 0, family=family, fused=mode, repeats=None if st["fresh"] else 0) as rec:
                    r = _step(s, kind, SIM_SEED + st["k"], ref, travel=st["travel"], dev=st["dev"])
                if st["fresh"]:
                    print(f"step {st['i']}: first {kind} step of {cpz} cars per zone ended on {rec}")
                _check_step(kind, r, ref, dev=st["dev"], where=where)
            assert np.array_equal(s.get_state(), ref["zone0"]), where              # a resample leaves the state unchanged
    print(f"sequence of {len(steps)} steps; fused modes without an instantiation at Z = {Z}: {sorted(skipped) or 'none'}")
    assert all(ran[mode] >= 2 for mode in FUSED_MODES if mode not in skipped), ran
    # at this fixed shape every forced mode has a form (fused_shape_ok of csrc/cpm_grouped.h: 4 zones per group, a row pack of one
    # round of a workgroup's loads; T >= 3 for the day launch), so a skip here would take a mode out of the sequence unnoticed
    assert not skipped, skipped


# ------------------------------------------------------------------------------------------------ D: contiguous shards
SHARDS = ((0, 2679), (2679, 2683), (5362, 2678))            # (car_begin, car_count) of Z = 67 x 120 = 8,040 cars


def test_the_shards_tile_the_fleet_off_every_boundary():
    cpz = BIG
    assert SHARDS[0][0] == 0 and sum(n for _, n in SHARDS) == 67 * cpz
    for (b0, n0), (b1, _) in zip(SHARDS, SHARDS[1:]):
        assert b0 + n0 == b1
    assert all(n % 4 != 0 and n >= 32 * 67 for _, n in SHARDS) and all(b % cpz != 0 for b, _ in SHARDS[1:])


@gpu
def test_contiguous_shards_are_column_sets_and_sum_to_the_whole_fleet(cpm, O):
    """Three contiguous shards of Z = 67 x 120 under kernel 5: a shard starts with three times its mean bucket in a third of the
    zones.  Its IVP and its record are the shard's columns of the whole fleet's; flows, CSR flows (densified), stays, parked and the
    counts of the three shards sum to the whole fleet's."""
    Z, cpz, T = 67, BIG, T24
    C = Z * cpz
    ref = _synth_ref(O, Z, cpz, T, SIM_SEED, density=0.9)
    total = {k: np.zeros_like(ref[k], dtype=np.int64) for k in ("parking", "driving", "flows", "stays", "parked")}
    total["csr"] = np.zeros_like(ref["flows"], dtype=np.int64)
    for begin, count in SHARDS:
        cars = slice(begin, begin + count)
        with _sampler(cpm, ref, kernel=5) as s:
            s.init_states(C, cpz, begin, count)
            assert s.car_count == count
            with pinned(s, 5, repeats=None) as step:
                assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"][cars]), begin
            print(f"shard [{begin}, {begin + count}): the IVP ended on {step}")
            with pinned(s, 5, repeats=None) as step:
                plain = _step(s, "plain", SIM_SEED, ref)
            print(f"shard [{begin}, {begin + count}): the first resample ended on {step}")
            R.check("plain", plain, ref, cars, begin)
            out = {}
            for kind in ("paths", "flows", "csr", "stays"):
                with pinned(s, 5, repeats=0):
                    out[kind] = _step(s, kind, SIM_SEED, ref)
                _check_step(kind, out[kind], ref, where=begin, cars=cars)
                assert np.array_equal(out[kind]["parking"], plain["parking"]) and np.array_equal(out[kind]["driving"], plain["driving"]), (begin, kind)
            # the shard against the oracle's matrices of its cars alone
            mine = R.derive(ref["state"][cars], ref["trans"][cars], Z)
            assert np.array_equal(plain["parking"], mine["parking"]) and np.array_equal(plain["driving"], mine["driving"]), begin
            assert np.array_equal(out["flows"]["flows"], mine["flows"]), begin
            assert np.array_equal(out["stays"]["stays"], mine["stays"]) and np.array_equal(out["stays"]["parked"], mine["parked"]), begin
            for k in ("row_ptr", "dest", "count"):
                assert np.array_equal(out["csr"]["flows_csr"][k], mine["flows_csr"][k]), (begin, k)
            total["parking"] += plain["parking"]
            total["driving"] += plain["driving"]
            total["flows"] += out["flows"]["flows"]
            total["csr"] += cpm.flows_csr_to_dense(out["csr"]["flows_csr"])
            total["stays"] += out["stays"]["stays"]
            total["parked"] += out["stays"]["parked"]
    for k in ("parking", "driving", "flows", "stays", "parked"):
        assert np.array_equal(total[k], ref[k]), k
    assert np.array_equal(total["csr"], ref["flows"])


# ------------------------------------------------------------------------------------------------ E: a one-launch hour that bails out
@gpu
@pytest.mark.parametrize("mode", [2, 4, 7])
def test_a_bailed_out_step_returns_the_output_of_the_repeated_attempt(cpm, O, mode):
    """Z = 192 x 120, kernel 5, CPM_OPT_FUSED 2 / 4 / 7: the blocks of the one-launch form give up at once, the blocking call repeats
    the step with two launches per hour (at least one repeat, exactly one bail-out counted) and returns that attempt's output."""
    Z, cpz, T = 192, 120, T24
    ref = _synth_ref(O, Z, cpz, T, SIM_SEED)
    with _sampler(cpm, ref, kernel=5) as s:
        s.set_fused(mode)
        s.init_states(Z * cpz, cpz)
        if s.get_info(cpm.CPM_INFO_FUSED) != MODE_FORM[mode]:
            print(f"Z = {Z}: no instantiation for fused mode {mode} (CPM_INFO_FUSED {s.get_info(cpm.CPM_INFO_FUSED)})")
            assert mode != 2
            return
        for kind in ("flows", "csr", "stays", "paths"):
            s.set_fused(mode)
            s.init_states(Z * cpz, cpz)
            s.set_state(ref["zone0"])
            assert s.get_info(cpm.CPM_INFO_FUSED) == MODE_FORM[mode], kind
            repeats0, bailouts0 = s.get_info(cpm.CPM_INFO_STEPS_REPEATED), s.get_info(cpm.CPM_INFO_FUSED_BAILOUTS)
            with pinned(s, 5, fused=mode, form=0, repeats=None, bailouts=None):
                r = _step(s, kind, SIM_SEED, ref)
            _check_step(kind, r, ref, where=(mode, kind))
            assert s.get_info(cpm.CPM_INFO_STEPS_REPEATED) - repeats0 >= 1, (mode, kind)
            assert s.get_info(cpm.CPM_INFO_FUSED_BAILOUTS) - bailouts0 == 1, (mode, kind)


# ------------------------------------------------------------------------------------------------ host only: the reference itself
def _hand_matrices():
    st = np.array([c[0] for c in _HAND], dtype=np.int64)
    tr = np.zeros((10, 4, 4), dtype=np.float64)
    for i, (zones, drove, dests) in enumerate(_HAND):
        it = iter(dests)
        for t in range(4):
            tr[i, t, 0] = drove[t]
            tr[i, t, 1] = next(it) if drove[t] else zones[t]
    return st, tr


def test_the_reference_on_ten_cars_written_out_by_hand(cpm):
    st, tr = _hand_matrices()
    got = R.derive(st, tr, 3)
    assert got["paths"].dtype == np.uint32 and np.array_equal(got["paths"], np.array(_HAND_PATHS, dtype=np.uint32))
    flows, stays, parked = np.zeros((4, 3, 3), dtype=np.int32), np.zeros((4, 3, 4), dtype=np.int32), np.zeros((3, 4), dtype=np.int32)
    for table, cells in ((flows, _HAND_FLOWS), (stays, _HAND_STAYS), (parked, _HAND_PARKED)):
        for k, v in cells.items():
            table[k] = v
    for k, want in (("flows", flows), ("stays", stays), ("parked", parked)):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want), k
    assert np.array_equal(got["parking"], [[5, 2, 4, 6], [3, 5, 3, 4], [2, 3, 3, 0]])      # (counted off _HAND's zones, hour by hour)
    assert np.array_equal(got["driving"], flows.sum(axis=2).T) and got["driving"].sum() == 14
    # the CSR restatement: canonical, and back to the dense tensor through the product's own helper
    csr = got["flows_csr"]
    R.check_csr_canonical(csr, 4, 3)
    assert csr["row_ptr"].tolist() == [0, 2, 2, 3, 3, 6, 7, 7, 7, 9, 10, 11, 11] and csr["dest"].tolist() == [1, 2, 2, 0, 1, 2, 0, 0, 1, 1, 2]
    assert csr["count"].tolist() == [2, 1, 1, 1, 1, 1, 1, 2, 1, 2, 1]
    back = cpm.flows_csr_to_dense(csr)
    assert back.dtype == np.int32 and np.array_equal(back, flows)
    # and `check` itself tells a wrong word, a wrong cell and an unsorted row from the right ones
    ref = dict(got, Z=3, T=4, state=st, trans=tr)
    good = dict(parking=np.asfortranarray(got["parking"]), driving=np.asfortranarray(got["driving"]), travel=False)
    R.check("paths", dict(good, paths=got["paths"].copy()), ref)
    R.check("paths", dict(good, paths=got["paths"][:, 2:7].copy()), ref, cars=slice(2, 7))
    R.check("stays", dict(good, stays=stays, parked=parked), ref)
    R.check("flows", dict(good, flows=flows), ref)
    R.check("csr", dict(good, flows_csr=csr), ref)
    R.check("compat", dict(good, state=st, trans=tr), ref)
    wrong = got["paths"].copy()
    wrong[3, 9] ^= 1
    bad_stays = stays.copy()
    bad_stays[1, 1, 0], bad_stays[1, 1, 1] = 2, 1                                           # (the row sum is still driving[1, 1])
    swapped = dict(csr, dest=csr["dest"].copy())
    swapped["dest"][[0, 1]] = swapped["dest"][[1, 0]]
    for kind, r in (("paths", dict(good, paths=wrong)), ("stays", dict(good, stays=bad_stays, parked=parked)), ("csr", dict(good, flows_csr=swapped)),
                    ("flows", dict(good, flows=np.asfortranarray(flows))), ("plain", dict(good, parking=good["parking"] + 1))):
        with pytest.raises(AssertionError):
            R.check(kind, r, ref)
