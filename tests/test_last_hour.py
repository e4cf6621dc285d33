"""Hour T of a grouped resample, counts only (CPM_OPT_LAST_HOUR, csrc/cpm_count.h): k_grouped_count / k_batch_count leave behind what
the plain form of the sampler leaves apart from the destinations nobody reads -- bucket sizes, Bernoulli successes, the overflow bit,
the heavy-bucket words the context sizes its next step from -- bit for bit, under either value of the option, against the oracle, on
shards, in the batched resample and next to the profiling record.  CPM_INFO_LAST_HOUR tells what was launched."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SIM_SEED

from product_form import pinned

GROUPED = 5  # CPM_KERNEL_ZONE_GROUPED

# the all-stayers buckets of hour 2: around the wave (64), the workgroup (256), four and six workgroups' worth of slots (1,024 / 1,536:
# a round of the count kernel, the widest plain sampler) and one past two of them
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2049]
ZERO_ROW_ZONES = (7, 13)  # p_drive 1 and an all-zero p_dest row at hour 2 (buckets of 257 and 1,536 cars when everybody stays)


def _bucket_state(Z, cpz):
    """zone (1-based) of every car: the zones' sizes are SIZES, then pads of about 2,100 cars that make C = Z * cpz"""
    C = Z * cpz
    pads = Z - len(SIZES)
    rest = C - sum(SIZES)
    sizes = SIZES + [rest // pads + (1 if k < rest % pads else 0) for k in range(pads)]
    assert sum(sizes) == C and max(sizes) < 4 * cpz
    return np.repeat(np.arange(1, Z + 1, dtype=np.int64), sizes), np.array(sizes)


def _hour2_tables(Z, first):
    """p_drive[:, 0] = first; hour 2 cycles through the edge probabilities; uniform rows, two all-zero rows at hour 2"""
    cycle = [0.0, 1.0, 0.5, 2.0 ** -53, 1.0 - 2.0 ** -53, 0.3]
    p_drive = np.zeros((Z, 2), order="F")
    p_drive[:, 0] = first
    p_drive[:, 1] = [cycle[z % 6] for z in range(Z)]
    p_dest = np.full((Z, Z, 2), 1.0 / Z, order="F")
    for z in ZERO_ROW_ZONES:
        assert p_drive[z, 1] == 1.0
        p_dest[z, :, 1] = 0.0
    return p_drive, p_dest


@pytest.mark.gpu
@pytest.mark.parametrize("first", [0.0, 1.0, 0.5], ids=["stayers", "arrivals", "mixed"])
def test_bucket_shapes_equal_the_oracle_and_the_plain_form(cpm, O, first):
    import torch
    from carparkingmaps_amd.distributed import split_counts
    Z, T, cpz = 32, 2, 1450
    C = Z * cpz
    state, sizes = _bucket_state(Z, cpz)
    p_drive, p_dest = _hour2_tables(Z, first)
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, state, do_ivp=False)
    tensors = {}
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(GROUPED)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        s.set_state(state)
        for option in (1, 0):
            s.set_last_hour(bool(option))
            with pinned(s, GROUPED):
                r = s.resample(SIM_SEED)
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == option
            assert np.array_equal(r["parking"], ref["parking"]), f"option {option}: parking"
            assert np.array_equal(r["driving"], ref["driving"]), f"option {option}: driving"
            counts = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda:0")
            with pinned(s, GROUPED):
                s.resample_dev(SIM_SEED, counts.data_ptr())
            s.sync()
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == option
            tensors[option] = counts.cpu().numpy()
            pk, dr, _ = split_counts(counts, Z, T)
            assert np.array_equal(pk, ref["parking"]) and np.array_equal(dr, ref["driving"]), f"option {option}: device tensor"
    assert np.array_equal(tensors[1], tensors[0]) and tensors[1][-1] == 0  # (the status word is the last one)
    if first == 0.0:
        assert np.array_equal(ref["parking"][:, 1], sizes)  # sizes exactly as set
    for z in ZERO_ROW_ZONES:  # a zero row does not keep a car from driving: only its destination would have been its origin
        assert ref["driving"][z, 1] == ref["parking"][z, 1] and tensors[1][T * Z + Z + z] == ref["parking"][z, 1]
    assert (ref["driving"][0::6, 1] == 0).all() and np.array_equal(ref["driving"][1::6, 1], ref["parking"][1::6, 1])


def _heavy_case(O):
    Z, T, cpz = 8, 2, 1300
    C = Z * cpz
    p_drive = np.zeros((Z, T), order="F")
    p_drive[1:5, 0] = 1.0     # hour 1: the cars of zones 1 to 4 all drive ...
    p_drive[:, 1] = 0.4
    p_dest = np.full((Z, Z, T), 1.0 / Z, order="F")
    p_dest[:, :, 0] = 0.0
    p_dest[:, 1, 0] = 1.0     # ... to zone 1
    zone0 = np.arange(C, dtype=np.int64) // cpz + 1
    ref = O.fast_run(p_drive, O.build_cdf(p_dest), C, SIM_SEED, zone0, do_ivp=False)
    assert ref["parking"][1, 1] == 4 * cpz == 5200  # above 4 x 1,024 slots, and the whole bucket region (4 x the mean)
    return Z, T, cpz, C, p_drive, p_dest, ref


@pytest.mark.gpu
def test_a_heavy_bucket_first_seen_in_hour_T_sizes_the_next_step_alike(cpm, O):
    Z, T, cpz, C, p_drive, p_dest, ref = _heavy_case(O)
    parts = {}
    for option in (1, 0):
        with cpm.Sampler(Z, T) as s:  # fresh contexts: no heavy bucket seen
            s.set_kernel(GROUPED)
            s.set_last_hour(bool(option))
            s.set_p_drive(p_drive)
            s.set_p_dest(p_dest)
            s.init_states(C, cpz)
            assert s.get_info(cpm.CPM_INFO_PARTS) == 1
            with pinned(s, GROUPED):
                r = s.resample(SIM_SEED)
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == option
            assert np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"]), f"option {option}"
            parts[option] = s.get_info(cpm.CPM_INFO_PARTS)
    assert parts[1] == parts[0] and parts[1] > 1, parts


@pytest.mark.gpu
def test_two_strided_shards_add_up_to_the_single_run(cpm, O):
    Z, T, cpz = 37, 4, 200
    C = Z * cpz
    p_drive, p_dest = O.synth_p_drive(Z, T, 77), O.synth_p_dest_dense(Z, T, 77)
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(GROUPED)
        s.set_p_drive(p_drive)
        s.set_p_dest(p_dest)
        s.init_states(C, cpz)
        with pinned(s, GROUPED):
            whole = s.resample(SIM_SEED)
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 1
    pk, dr = np.zeros((Z, T), dtype=np.int64), np.zeros((Z, T), dtype=np.int64)
    for begin in (0, 1):
        with cpm.Sampler(Z, T) as s:
            s.set_kernel(GROUPED)
            s.set_p_drive(p_drive)
            s.set_p_dest(p_dest)
            s.init_states(C, cpz, car_begin=begin, car_stride=2)
            with pinned(s, GROUPED):
                r = s.resample(SIM_SEED)
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 1
            pk += r["parking"]
            dr += r["driving"]
    assert np.array_equal(pk, whole["parking"]) and np.array_equal(dr, whole["driving"])


@pytest.mark.gpu
def test_batch_fleets_equal_their_single_resamples_under_both_options(cpm, O):
    Z, T, cpz, B = 64, 3, 300, 3
    C = Z * cpz
    rng = np.random.default_rng(5)
    tables = np.asfortranarray(np.stack([O.synth_p_drive(Z, T, 78), rng.uniform(0, 1, (Z, T)), np.ones((Z, T))], axis=2))
    seeds = np.array([SIM_SEED, SIM_SEED, SIM_SEED + 1], dtype=np.uint64)
    got = {}
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(GROUPED)
        s.set_p_drive(np.asfortranarray(tables[:, :, 0]))
        s.set_p_dest(O.synth_p_dest_dense(Z, T, 78))
        s.init_states(C, cpz)
        s.set_p_drive_batch(tables)
        for option in (1, 0):
            s.set_last_hour(bool(option))
            got[option] = s.resample_batch(seeds)
            assert s.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS) == B and s.get_info(cpm.CPM_INFO_LAST_FORM) == cpm.CPM_FORM_BATCH
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == option
        s.set_last_hour(True)
        for b in range(B):
            s.set_p_drive(np.asfortranarray(tables[:, :, b]))
            with pinned(s, GROUPED):
                one = s.resample(int(seeds[b]))
            assert np.array_equal(got[1]["parking"][:, :, b], one["parking"]), f"fleet {b}: parking"
            assert np.array_equal(got[1]["driving"][:, :, b], one["driving"]), f"fleet {b}: driving"
    for key in ("parking", "driving", "sum_tt_q16"):
        assert np.array_equal(got[1][key], got[0][key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("option", [1, 0])
def test_every_sampler_launch_hands_its_event_pair_back(cpm, O, option):
    """bench.py counts T sampler-profiled launches per step and drops hour T's by index: the count-only launch takes the armed pair."""
    import torch
    Z, T, cpz = 64, 5, 300
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(GROUPED)
        s.set_last_hour(bool(option))
        s.set_p_drive(O.synth_p_drive(Z, T, 79))
        s.set_p_dest(O.synth_p_dest_dense(Z, T, 79))
        s.init_states(Z * cpz, cpz)
        counts = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda:0")
        s.set_profile(True, stride=1, kernel=0)
        for _ in range(2):
            s.resample_dev(SIM_SEED, counts.data_ptr())
        s.sync()
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == option
        ms = s.last_kernel_ms()
        s.set_profile(False)
    assert len(ms) == 2 * T, ms
    assert all(v > 0 for v in ms), ms
    assert int(counts[-1].item()) == 0


@pytest.mark.gpu
def test_the_other_forms_of_hour_T_are_left_alone(cpm, O):
    Z, T, cpz = 64, 4, 300
    dm, dist = O.synth_datamatrix(Z, T, 80, density=0.3)
    with cpm.Sampler(Z, T) as s:
        s.set_kernel(GROUPED)
        s.set_datamatrix(dm, dist)
        s.set_p_drive(O.synth_p_drive(Z, T, 80))
        s.set_p_dest(O.synth_p_dest_dense(Z, T, 80))
        s.init_states(Z * cpz, cpz)
        s.resample(SIM_SEED)
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 1
        for kw in (dict(travel=True), dict(flows=True), dict(stays=True)):
            s.resample(SIM_SEED, **kw)
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 0, kw
        for mode in (3, 6):
            s.set_fused(mode)
            with pinned(s, GROUPED, fused=mode):  # (the form ran: placing first / all hours in one launch keep their plain hour T)
                s.resample(SIM_SEED)
            assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 0, f"fused mode {mode} (form {s.get_info(cpm.CPM_INFO_LAST_FORM)})"
        s.set_fused(5)
        s.resample(SIM_SEED)
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 1
        s.solve_ivp(SIM_SEED)
        assert s.get_info(cpm.CPM_INFO_LAST_HOUR) == 0  # (an IVP has no hour T)


@pytest.mark.gpu
def test_the_option_takes_0_and_1_only(cpm):
    """(with a context, which needs a device: the host test below can only reach the null-context error)"""
    from carparkingmaps_amd import _lib
    with cpm.Sampler(8, 2) as s:
        for bad in (-1, 2, 8):
            assert s._L.cpm_set_option(s._h, _lib.CPM_OPT_LAST_HOUR, bad) == -1  # CPM_ERR_ARG
            assert b"last hour" in s._L.cpm_last_error()
        for ok in (0, 1):
            assert s._L.cpm_set_option(s._h, _lib.CPM_OPT_LAST_HOUR, ok) == 0


def test_constants_match_the_header_and_the_option_checks_its_value(cpm):
    from carparkingmaps_amd import _lib
    header = open(os.path.join(ROOT, "include", "cpm.h")).read()
    assert int(re.search(r"#define\s+CPM_OPT_LAST_HOUR\s+(\d+)", header).group(1)) == _lib.CPM_OPT_LAST_HOUR == 8
    assert int(re.search(r"#define\s+CPM_INFO_LAST_HOUR\s+(\d+)", header).group(1)) == _lib.CPM_INFO_LAST_HOUR == cpm.CPM_INFO_LAST_HOUR
    others = {k: int(v) for k, v in re.findall(r"#define\s+(CPM_(?:OPT|INFO)_\w+)\s+(\d+)", header)}
    assert [k for k, v in others.items() if k.startswith("CPM_OPT_") and v == 8] == ["CPM_OPT_LAST_HOUR"]
    assert [k for k, v in others.items() if k.startswith("CPM_INFO_") and v == _lib.CPM_INFO_LAST_HOUR] == ["CPM_INFO_LAST_HOUR"]
    L = _lib.load()
    for value in (0, 1, 2, -1):  # (no device, no context: an argument error before the value is looked at)
        assert L.cpm_set_option(None, _lib.CPM_OPT_LAST_HOUR, value) == -1
    # the value check itself, in the library's source: anything but 0 and 1 is CPM_ERR_ARG
    api = open(os.path.join(ROOT, "carparkingmaps_amd", "csrc", "cpm_api.hip")).read()
    case = api[api.index("case CPM_OPT_LAST_HOUR:"):]
    case = case[:case.index("return CPM_OK;")]
    assert re.search(r"if \(value != 0 && value != 1\) return fail\(CPM_ERR_ARG", case)
