"""The narrow hour with its waves' drivers compacted before the search (csrc/cpm_narrow.h, "dense drivers"; cpm_grouped.h, first_pass)
on the GPU: parking and driving counts against the oracle and against the same context on wide packs -- the wide k_grouped_hour is not
compacted -- bit for bit, with the form of every step pinned (tests/product_form.py) and what was streamed read back from
CPM_INFO_NARROW_PACK.  The planted shapes hold more than 700 cars per zone, where the hour runs six cars per lane; the random small
shapes run the twin's one-car form, which compacts too (K' is 0 or 1 there)."""
import functools

import numpy as np
import pytest

from conftest import SIM_SEED, TABLE_SEED
from carparkingmaps_amd._lib import CPM_CELL_HOUR
from product_form import GROUPED, pinned

gpu = pytest.mark.gpu

# hour 1's planted buckets: waves of every K from 1 to 6 (256 threads x 6 cars), a dense slot exactly full and one car more (64, 65: one
# wave; 256, 257 and 1,536, 1,537: a workgroup's slots exactly full and one car more), and the walk beyond the register-resident cars
SIZES = (1, 63, 64, 65, 256, 257, 1535, 1536, 1537, 2000)
P_CLASSES = (1.0, 0.0, 0.5)  # hour 1's p_drive of a planted zone: K' = K, K' = 0, about half
FILL, FILL_CARS = 6, 1000    # zones that only lift the mean above 700 cars per zone (six cars per lane)
HEAVY = 4 * 4 * 256          # a bucket is heavy above this (kHeavy x the slots of a four-car workgroup, cpm_grouped.h)


def _pin(s):
    return pinned(s, GROUPED, fused=1, cap_mult=4, parts=1)


def _same(r, ref, where):
    assert np.array_equal(r["parking"], ref["parking"]), f"{where}: parking"
    assert np.array_equal(r["driving"], ref["driving"]), f"{where}: driving"


def _sampler(cpm, Z, T):
    s = cpm.Sampler(Z, T)
    s.set_kernel(GROUPED)
    s.set_fused(1)
    return s


def _cell(rec):
    """(kind, CPT, NQ rung) of the sampler launch of the step's applied hours (include/cpm.h, CPM_INFO_CELL_APPLIED)"""
    w = rec["cells"]["applied"]
    return w & 255, (w >> 8) & 255, (w >> 16) & 255


def _narrow_then_wide(s, ref, where, cpt, **kw):
    """one resample on narrow packs, one on wide packs in the same context: both the oracle's counts, both the one-launch hour with
    `cpt` cars per lane (the twin writes the wide kernel's record word)"""
    got = []
    for on in (1, 0):
        s.set_narrow_pack(on)
        with _pin(s) as rec:
            r = s.resample(SIM_SEED, **kw)
        assert s.narrow_pack() == on, where
        assert _cell(rec)[:2] == (CPM_CELL_HOUR, cpt), f"{where}: launched {_cell(rec)}"
        _same(r, ref, f"{where}, narrow pack {on}")
        got.append(r)
    _same(got[0], got[1], f"{where}, narrow against wide")
    return got


@functools.lru_cache(maxsize=None)
def _planted(O):
    sizes = [n for _ in P_CLASSES for n in SIZES] + [FILL_CARS] * FILL
    Z, T = len(sizes), 3
    zone0 = np.repeat(np.arange(1, Z + 1, dtype=np.int64), sizes)
    C = len(zone0)
    p_drive = np.full((Z, T), 0.5, order="F")
    for k, p in enumerate(P_CLASSES):
        p_drive[k * len(SIZES):(k + 1) * len(SIZES), 0] = p
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, zone0, do_ivp=False)
    return dict(Z=Z, T=T, C=C, sizes=np.array(sizes), zone0=zone0, p_drive=p_drive, p_dest=p_dest, ref=ref)


def test_the_planted_sizes_occur_in_the_oracle(O):
    """from the oracle's own counts: hour 1 holds the planted buckets, zones of p_drive 1 / 0 drive all / none of them, the mean
    bucket asks for six cars per lane, and no bucket of any hour is heavy or leaves a region of 4 x the mean"""
    d = _planted(O)
    park, drive, n = d["ref"]["parking"], d["ref"]["driving"], len(SIZES)
    assert np.array_equal(park[:, 0], d["sizes"])
    assert np.array_equal(drive[:n, 0], SIZES) and not drive[n:2 * n, 0].any()
    half = drive[2 * n:3 * n, 0]
    assert (half[4:] > 0).all() and (half[4:] < np.array(SIZES[4:])).all()
    mean = d["C"] // d["Z"]
    assert mean > 700, mean                      # grouped_cpt_wide: six cars per lane (the GPU case reads the CPT from the launch record)
    assert 1537 > 6 * 256 and 2000 > 6 * 256     # the walk beyond the register-resident cars
    assert park.max() <= HEAVY and park.max() <= 4 * mean
    assert (park.sum(axis=0) == d["C"]).all()


@gpu
def test_planted_bucket_sizes(cpm, O):
    d = _planted(O)
    with _sampler(cpm, d["Z"], d["T"]) as s:
        s.set_p_drive(d["p_drive"])
        s.set_p_dest(d["p_dest"])
        s.init_states(d["C"], -(-d["C"] // d["Z"]))
        s.set_state(d["zone0"])
        _narrow_then_wide(s, d["ref"], "planted sizes", 6)


@gpu
def test_an_hour_of_drivers_only_and_one_of_stayers_only(cpm, O):
    """hour 2: every car of every zone drives (K' = K in every wave; about 800 cars per zone fill four of a wave's six slots -- the
    scratch is at its capacity in the planted zones of 1,536 and 1,537 cars with p_drive 1); hour 3: none does (K' = 0)"""
    Z, T, cpz = 32, 4, 800
    C = Z * cpz
    p_drive = np.full((Z, T), 0.5, order="F")
    p_drive[:, 1], p_drive[:, 2] = 1.0, 0.0
    p_dest = O.synth_p_dest_dense(Z, T, TABLE_SEED)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, zone0, do_ivp=False)
    assert np.array_equal(ref["driving"][:, 1], ref["parking"][:, 1]) and not ref["driving"][:, 2].any()
    assert np.array_equal(ref["parking"][:, 3], ref["parking"][:, 2]) and ref["parking"].max() <= HEAVY
    with _sampler(cpm, Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        _narrow_then_wide(s, ref, "all drive, none drives", 6)


@gpu
def test_zone_hours_without_a_destination(cpm, O):
    """p_destin rows that are all zero: the zone's drivers stay home and are counted in `driving`"""
    Z, T, cpz = 32, 3, 800
    C = Z * cpz
    p_drive = np.full((Z, T), 0.5, order="F")
    p_dest = np.array(O.synth_p_dest_dense(Z, T, TABLE_SEED))
    zero = [(3, 0), (17, 0), (17, 1), (30, 1)]
    for o, t in zero:
        p_dest[o, :, t] = 0.0
    p_dest = np.asfortranarray(p_dest)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, zone0, do_ivp=False, want_state=True)
    for o, t in zero:
        assert ref["driving"][o, t] > 0
        here = ref["state"][:, t] == o + 1
        assert (ref["state"][here, t + 1] == o + 1).all() if t + 1 < T else True
    with _sampler(cpm, Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        _narrow_then_wide(s, ref, "zero rows", 6)


@gpu
@pytest.mark.parametrize("Z,cpz", [(192, 120), (67, 40)])
def test_random_small_shapes(cpm, O, Z, cpz):
    T = 24
    C = Z * cpz
    p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, zone0)
    with _sampler(cpm, Z, T) as s:
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        for on in (1, 0):
            s.set_narrow_pack(on)
            s.init_states(C, cpz)
            with _pin(s):
                assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"]), f"IVP state, narrow pack {on}"
            assert s.narrow_pack() == on
            with _pin(s) as rec:
                r = s.resample(SIM_SEED)
            assert s.narrow_pack() == on
            assert _cell(rec)[:2] == (CPM_CELL_HOUR, 1), _cell(rec)
            _same(r, ref, f"Z = {Z}, narrow pack {on}")
