"""The narrow twin of the one-launch hour (csrc/cpm_narrow.h, k_grouped_hour_narrow) on the GPU: counts against the oracle and against
the wide kernel, bit for bit, with the form of every step pinned (tests/product_form.py: the grouped family, the one-launch hour as
asked, regions of 4 x the mean, one workgroup per zone, no bail-out, no repeat -- a step that left a status bit behind is repeated
and fails the pin) and what was streamed read back from CPM_INFO_NARROW_PACK."""
import numpy as np
import pytest

import test_knife_edge as KE
from conftest import SIM_SEED, TABLE_SEED
from product_form import GROUPED, at_least, pinned
from test_narrow_pack import HOUR_NQ, narrow_words, need, rung_of, wide_words

gpu = pytest.mark.gpu


def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


def _pin(s, **kw):
    return pinned(s, GROUPED, fused=1, cap_mult=4, parts=1, **kw)


def _same(r, ref, where=""):
    assert np.array_equal(r["parking"], ref["parking"]), f"{where}: parking"
    assert np.array_equal(r["driving"], ref["driving"]), f"{where}: driving"


def _sampler(cpm, Z, T):
    s = cpm.Sampler(Z, T)
    s.set_kernel(GROUPED)
    s.set_fused(1)
    return s


@gpu
def test_narrow_against_wide_against_the_oracle(cpm, O):
    """option 1, 0, 1 in one context: the same counts three times, narrow packs streamed in the first and the third step only, and
    the tie counter moving in those two only (about 17 undecided draws per resample here: 0 has probability below 1e-7)"""
    Z, T, cpz = 192, 24, 120
    C = Z * cpz
    p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz))
    with _sampler(cpm, Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with _pin(s):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        assert s.narrow_pack() == 1
        got, ties = [], [s.narrow_ties()]
        for on in (1, 0, 1):
            s.set_narrow_pack(on)
            with _pin(s):
                r = s.resample(SIM_SEED)
            assert s.narrow_pack() == on
            _same(r, ref, f"narrow pack {on}")
            got.append(r)
            ties.append(s.narrow_ties())
        for r in got[1:]:
            _same(r, got[0], "narrow against wide")
        print("narrow ties after the IVP and each resample:", ties)
        assert ties[0] > 0 and ties[1] > ties[0] and ties[2] == ties[1] and ties[3] > ties[2], ties


@gpu
@pytest.mark.parametrize("name,kind", [("z97", "resample"), ("z403", "resample"), ("z97", "ivp")])
def test_the_narrow_twin_on_the_edge_draws(cpm, O, name, kind):
    """the planted days of tests/test_knife_edge.py (draws exactly on a table edge or one step beside it): every plant read back from
    the per-car record, counts against the oracle"""
    d, ref = KE._day(O, name, kind), KE._ref(O, name, kind)
    with KE._sampler(cpm, d) as s:
        s.set_kernel(GROUPED)
        s.set_fused(1)
        KE._start(s, d)
        if kind == "ivp":
            with _pin(s):
                assert np.array_equal(s.solve_ivp(d["seed"]), ref["zone0"])
        else:
            with _pin(s):
                r = s.resample(d["seed"], paths=True)
            _same(r, ref, name)
            KE._check_paths(d, r, name)
        assert s.narrow_pack() == 1


def _edge_zs():
    """Z of rungs 1 .. 3 of the hour's ladder behind which the narrow twin issues another number of LDS-DMA instructions than at Z - 1,
    and behind which the narrow pack NEEDS another number (inside a rung the twin then repeats its last chunk): the smallest of each"""
    issued = {}
    for Z in range(2, 8193):
        issued.setdefault(rung_of(need(wide_words(Z))), []).append(need(narrow_words(Z)))
    issued = {r: max(v) for r, v in issued.items()}
    in_rungs = [Z for Z in range(3, 8193) if rung_of(need(wide_words(Z))) in HOUR_NQ[:3]]
    a = next(Z for Z in in_rungs if issued[rung_of(need(wide_words(Z)))] != issued[rung_of(need(wide_words(Z - 1)))])
    b = next(Z for Z in in_rungs if need(narrow_words(Z)) != need(narrow_words(Z - 1)))
    return sorted({a - 1, a, b - 1, b})


def test_the_rung_edges_found_on_the_cpu():
    assert _edge_zs() == [833, 834, 1473, 1474]


@gpu
@pytest.mark.parametrize("Z", [833, 834, 1473, 1474])
def test_rung_edges(cpm, O, Z):
    T, cpz = 3, 32
    C = Z * cpz
    p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)
    assert p_dest.nbytes < 100e6
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz))
    with _sampler(cpm, Z, T) as s:
        s.synth_tables(TABLE_SEED)
        s.init_states(C, cpz)
        with _pin(s):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        with _pin(s):
            r = s.resample(SIM_SEED)
        assert s.narrow_pack() == 1
        _same(r, ref, f"Z = {Z}")


def _sparse_table(Z, T, rng, density=0.06):
    w = rng.random((Z, Z, T))
    w[rng.random((Z, Z, T)) >= density] = 0.0
    tot = w.sum(axis=1, keepdims=True)
    return np.asfortranarray(np.divide(w, tot, out=np.zeros_like(w), where=tot > 0))


@gpu
def test_table_life_cycle_in_one_context(cpm, O):
    """synth_tables, set_p_dest of another dense table, refresh_tables, a sparse install, dense again: the narrow packs follow every
    dense install (a stale pack would give the counts of the table before) and are not streamed on sparse tables"""
    Z, T, cpz = 403, 6, 40
    C = Z * cpz
    p_drive = O.synth_p_drive(Z, T, TABLE_SEED)
    tables = {"synth": O.synth_p_dest_dense(Z, T, TABLE_SEED), "other": O.synth_p_dest_dense(Z, T, TABLE_SEED + 1),
              "sparse": _sparse_table(Z, T, np.random.default_rng(5))}
    refs = {k: O.fast_run(p_drive, O.build_cdf(p), C, SIM_SEED, _zone0(C, cpz), do_ivp=False) for k, p in tables.items()}
    assert not np.array_equal(refs["synth"]["parking"], refs["other"]["parking"])

    def step(s, key, narrow):
        with _pin(s):
            r = s.resample(SIM_SEED)
        assert s.narrow_pack() == narrow, key
        _same(r, refs[key], key)

    with _sampler(cpm, Z, T) as s:
        s.synth_tables(TABLE_SEED)
        s.init_states(C, cpz)
        step(s, "synth", 1)
        s.set_p_dest(tables["other"])
        step(s, "other", 1)
        s.refresh_tables()
        step(s, "other", 1)
        s.set_sparse_upload(True)
        s.set_p_dest(tables["sparse"])
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) > 0
        step(s, "sparse", 0)
        s.set_sparse_upload(False)
        s.set_p_dest(tables["synth"])
        assert s.get_info(cpm.CPM_INFO_SPARSE_TABLES) == 0
        step(s, "synth", 1)


@gpu
def test_a_one_launch_hour_that_gives_up(cpm, O):
    """CPM_OPT_FUSED = 2 (the placing blocks give up at once) with the narrow pack on: the step is repeated on two launches per hour
    with wide packs, and its counts are the oracle's"""
    Z, T, cpz = 130, 6, 300
    C = Z * cpz
    p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), do_ivp=False)
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(GROUPED)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        s.set_fused(2)
        s.set_narrow_pack(True)
        with pinned(s, GROUPED, fused=2, form=0, repeats=at_least(1), bailouts=1, cap_mult=4, parts=1):
            r = s.resample(SIM_SEED)
        assert s.narrow_pack() == 0
        _same(r, ref, "after the bail-out")


@gpu
def test_ivp_then_resample_with_travel_times(cpm, O):
    Z, T, cpz = 67, 24, 41
    C = Z * cpz
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.3)
    p_drive = O.createpdrive(dm, dist, Z, T, 0.1, 0.9, 0.5)
    p_dest = O.createpdestin(dm, Z, T, 2)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, _zone0(C, cpz), datamatrix=dm, dist=dist)
    with _sampler(cpm, Z, T) as s:
        s.set_narrow_pack(True)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.set_datamatrix(dm, dist)
        s.init_states(C, cpz)
        with _pin(s):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"])
        assert s.narrow_pack() == 1
        with _pin(s):
            r = s.resample(SIM_SEED, travel=True)
        assert s.narrow_pack() == 1
        _same(r, ref, "travel resample")
        assert r["sum_tt_q16"] == ref["sum_tt_q16"]
