#!/usr/bin/env python3
"""The batched resample (include/cpm_batch.h) against the single path on one GPU (development tool; bench.py is the contract bench).

Headline shape (cpm_synth_tables, Z = 4,096 x 1,000 cars per zone, no travel times), B in {1, 2, 4, 8, 16}: ms per fleet of
pipelined resample_batch_dev steps, of cpm_resample_dev one at a time on the same box, and of two contexts in flight -- the three in
interleaved blocks.  Every fleet of one batch step is checked against the single path (same state, its table, its seed).  Then the
Melbourne-shaped tables x 1,000 with travel times.  Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import carparkingmaps_amd as cpm
import _synth

ap = argparse.ArgumentParser()
ap.add_argument("--zones", type=int, default=4096)
ap.add_argument("--cpz", type=int, default=1000)
ap.add_argument("--batches", default="1,2,4,8,16")
ap.add_argument("--fleets", type=int, default=32, help="fleet-steps per timed block (each mode runs about as many resamples)")
ap.add_argument("--blocks", type=int, default=3, help="interleaved blocks per mode")
ap.add_argument("--mel-zones", type=int, default=2357)
ap.add_argument("--mel-batch", type=int, default=8)
ap.add_argument("--skip-mel", action="store_true")
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E


def timed(fn, n_steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def batch_bytes(s, nf):
    """algorithmic HBM bytes of one hour's batched sampler launch over nf fleets: the packs (and row totals) once per sub-batch of the
    launch, thresholds, car ids in and out and counts once per fleet (the terms of cpm_algorithmic_bytes_per_hour; the sub-batch
    rule of batch_per_wg in csrc/cpm_batch.h)"""
    Z, n = s.Z, s.car_count
    single = s.algorithmic_bytes_per_hour()
    fleet = Z * 8 + n * 8 + 2 * Z * 8
    pack = single - fleet
    per_cu = max(1, min(6, (160 * 1024) // ((pack - Z * 8) // Z + 4240)))
    slots = per_cu * cpm.device_info(0)["cu_count"]
    F = max(1, min(nf, Z * nf // (2 * slots)))
    nsub = -(-nf // F)
    return nsub * pack + nf * fleet, single


def run_shape(name, Z, cpz, batches, travel, setup):
    C = Z * cpz
    streams = [torch.cuda.Stream() for _ in range(3)]
    ctx = [cpm.Sampler(Z, T, stream=st) for st in streams]   # 0: batch + single one at a time; 1, 2: two contexts in flight
    for s in ctx:
        setup(s)
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
    s0 = ctx[0]
    base = s0.get_p_drive()
    rng = np.random.default_rng(4)
    nw = s0.counts_words()
    Bmax = max(batches)
    tables = np.asfortranarray(np.stack([np.clip(base * rng.uniform(0.5, 1.1), 0, 1) for _ in range(Bmax)], axis=2))
    d_batch = [torch.zeros(Bmax * nw, dtype=torch.int64, device="cuda") for _ in range(2)]
    d_one = [torch.zeros(nw, dtype=torch.int64, device="cuda") for _ in range(2)]
    # check: every fleet of one batch step of each size against the single path
    checked = {}
    for B in batches:
        s0.set_p_drive_batch(tables[:, :, :B])
        r = s0.resample_batch(SEED, travel=travel)
        ok = s0.get_info(cpm.CPM_INFO_LAST_BATCH_FLEETS) == B
        for b in range(B):
            s0.set_p_drive(np.asfortranarray(tables[:, :, b]))
            one = s0.resample(SEED, travel=travel)
            ok = ok and np.array_equal(r["parking"][:, :, b], one["parking"]) and np.array_equal(r["driving"][:, :, b], one["driving"]) \
                and int(r["sum_tt_q16"][b]) == one["sum_tt_q16"]
        checked[B] = bool(ok)
        print(f"{name}: B = {B} fleets equal their single resamples: {ok}", flush=True)
    s0.set_p_drive(base)
    flags = dict(travel=travel)

    def single_mode(k):
        for i in range(k):
            s0.resample_dev(SEED, d_one[i & 1].data_ptr(), **flags)

    def two_mode(k):
        for i in range(k):
            ctx[1 + (i & 1)].resample_dev(SEED, d_one[i & 1].data_ptr(), **flags)

    res = {}
    per_mode = {"single": [], "two_contexts": []}
    per_batch = {B: [] for B in batches}
    for blk in range(args.blocks + 1):                     # (block 0: warm-up, not recorded)
        for B in batches:
            s0.set_p_drive_batch(tables[:, :, :B])
            steps = max(2, args.fleets // B)
            dt = timed(lambda: [s0.resample_batch_dev(SEED, d_batch[i & 1].data_ptr(), **flags) for i in range(steps)], 1)
            if blk:
                per_batch[B].append(1e3 * dt / (steps * B))
            st = d_batch[(steps - 1) & 1][:B * nw].view(B, nw)[:, -1]
            if int(st.abs().sum()) != 0:
                print(f"{name}: B = {B}: status words set", flush=True)
        k = args.fleets
        dt1 = timed(lambda: single_mode(k), 1)
        dt2 = timed(lambda: two_mode(k), 1)
        if blk:
            per_mode["single"].append(1e3 * dt1 / k)
            per_mode["two_contexts"].append(1e3 * dt2 / k)
        print(f"{name}: block {blk}: " + ", ".join(f"B{B} {per_batch[B][-1]:.3f}" for B in batches if per_batch[B]) +
              (f", single {per_mode['single'][-1]:.3f}, two contexts {per_mode['two_contexts'][-1]:.3f} ms per fleet" if blk else " (warm-up)"), flush=True)
    res["ms_per_fleet_batch"] = {str(B): round(float(np.median(v)), 4) for B, v in per_batch.items()}
    res["ms_per_fleet_single"] = round(float(np.median(per_mode["single"])), 4)
    res["ms_per_fleet_two_contexts"] = round(float(np.median(per_mode["two_contexts"])), 4)
    res["blocks"] = {"batch": {str(B): [round(x, 4) for x in v] for B, v in per_batch.items()},
                     "single": [round(x, 4) for x in per_mode["single"]], "two_contexts": [round(x, 4) for x in per_mode["two_contexts"]]}
    res["checked_against_single"] = checked
    res["sampler_bytes_per_hour"] = {str(B): batch_bytes(s0, B)[0] for B in batches}
    res["single_sampler_bytes_per_hour"] = batch_bytes(s0, 1)[1]
    res.update(Z=Z, cpz=cpz, travel=travel)
    for s in ctx:
        s.close()
    return res


def headline(s):
    s.synth_tables(TSEED)


out = {"device": cpm.device_info(0)["name"]}
out["headline"] = run_shape("headline", args.zones, args.cpz, [int(b) for b in args.batches.split(",")], False, headline)
if not args.skip_mel:
    dm, dist = _synth.datamatrix(args.mel_zones, T)

    def melbourne(s):
        s.set_datamatrix(dm, dist)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)

    out["melbourne_travel"] = run_shape("melbourne", args.mel_zones, 1000, [1, args.mel_batch], True, melbourne)
print(json.dumps(out), flush=True)
