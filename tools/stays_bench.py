#!/usr/bin/env python3
"""What the parking stays cost (include/cpm_stays.h, csrc/cpm_stays.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096 x 1,000 cars per zone, cpm_synth_tables) and Melbourne's (Z = 2,357, cpm_synth_datamatrix at density
0.0868: sparse packs) x 1,000 and x 100.  Arms, ONE process, one context each, the same seeds:
  A   resample_dev: the step without stays (what bench.py times as ms_per_step)
  B   resample_stays_dev: the same step with k_grouped_stays behind every hour's launches and the `parked` pass at the end
in interleaved blocks of pipelined steps between two synchronisations (block 0 a warm-up, the median of the others), and
  C   once, not interleaved: what the library offered for the same arrays before -- the blocking resample(want_state=True,
      want_trans=True) plus a host loop over the hours -- whose arrays must equal arm B's.
Reported per shape: ms per resample of every arm, B - A in all and in microseconds per hour, the bytes of the per-car side array, and
B / C.  Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carparkingmaps_amd as cpm

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="headline,melbourne_x1000,melbourne_x100")
ap.add_argument("--steps", type=int, default=100, help="resamples per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--no-compat", action="store_true", help="skip arm C")
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
SHAPES = {"headline": (4096, 1000, False), "melbourne_x1000": (2357, 1000, True), "melbourne_x100": (2357, 100, True)}
ARMS = ("A", "B")


def make(Z, cpz, dataset):
    s = cpm.Sampler(Z, T)
    if dataset:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)
    else:
        s.synth_tables(TSEED)
    s.init_states(Z * cpz, cpz)
    s.solve_ivp(SEED, want=False)
    return s


def host_stays(state, trans, Z):
    """the host loop of the compat route: the definition of include/cpm_stays.h over the state / transition matrices"""
    n = state.shape[0]
    since = np.zeros(n, dtype=np.int64)
    stays = np.zeros((T, Z, T), dtype=np.int32)
    for t in range(T):
        drove = trans[:, t, 0] == 1
        cell = ((state[drove, t] - 1) * T + (t - since[drove])).astype(np.int64)
        stays[t] = np.bincount(cell, minlength=Z * T).reshape(Z, T)
        since[drove] = t + 1
    still = since < T
    parked = np.bincount((state[still, T - 1] - 1) * T + since[still], minlength=Z * T).reshape(Z, T).astype(np.int32)
    return stays, parked


out = {"device": cpm.device_info(0)["name"], "T": T, "steps_per_block": args.steps, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, cpz, dataset = SHAPES[name]
    ctx = {a: make(Z, cpz, dataset) for a in ARMS}
    d_counts = [torch.zeros(ctx["A"].counts_words(), dtype=torch.int64, device="cuda") for _ in range(2)]
    d_stays = torch.zeros(T * Z * T, dtype=torch.int32, device="cuda")
    d_parked = torch.zeros(Z * T, dtype=torch.int32, device="cuda")
    res = {"Z": Z, "cars_per_zone": cpz, "sparse_pack_words": ctx["A"].get_info(cpm.CPM_INFO_SPARSE_TABLES),
           "side_array_bytes": 4 * Z * cpz, "stays_bytes": 4 * T * Z * T, "parked_bytes": 4 * Z * T}
    blocking = {}
    for a, s in ctx.items():
        blocking[a] = s.resample(SEED, stays=(a == "B"))
        res[a] = {"step": s.last_step()}
    b = blocking["B"]
    res["counts_equal_in_both_arms"] = bool(np.array_equal(b["parking"], blocking["A"]["parking"]) and np.array_equal(b["driving"], blocking["A"]["driving"]))
    res["identities_hold"] = bool(np.array_equal(b["stays"].sum(axis=2, dtype=np.int64).T, b["driving"]) and
                                  np.array_equal(b["parked"].sum(axis=1, dtype=np.int64), b["parking"][:, T - 1] - b["driving"][:, T - 1]))
    res["drivers_per_resample"] = int(b["driving"].sum())
    res["open_stays"] = int(b["parked"].sum())
    per = {a: [] for a in ARMS}
    for blk in range(args.blocks + 1):                       # (block 0: warm-up, not recorded)
        for a, s in ctx.items():
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                if a == "A":
                    s.resample_dev(SEED, d_counts[i & 1].data_ptr())
                else:
                    s.resample_stays_dev(SEED, d_counts[i & 1].data_ptr(), d_stays.data_ptr(), d_parked.data_ptr())
            s.sync()
            dt = time.perf_counter() - t0
            if int(d_counts[(args.steps - 1) & 1][-1]) != 0:
                print(f"{name} {a}: status word set", flush=True)
            if blk:
                per[a].append(1e3 * dt / args.steps)
        if blk:
            print(f"{name} block {blk}: " + ", ".join(f"{a} {per[a][-1]:.4f}" for a in ARMS) + " ms per resample", flush=True)
    for a in ARMS:
        res[a]["step_after_timed_blocks"] = ctx[a].last_step()
        res[a]["ms_per_resample"] = round(float(np.median(per[a])), 4)
        res[a]["ms_per_resample_blocks"] = [round(x, 4) for x in per[a]]
    extra = res["B"]["ms_per_resample"] - res["A"]["ms_per_resample"]
    res["B"]["ms_over_A"] = round(extra, 4)
    res["B"]["us_per_hour_over_A"] = round(1e3 * extra / T, 2)
    res["B"]["device_arrays_equal_blocking"] = bool(np.array_equal(d_stays.cpu().numpy().reshape(T, Z, T), b["stays"]) and
                                                    np.array_equal(d_parked.cpu().numpy().reshape(Z, T), b["parked"]))
    if not args.no_compat:
        s = ctx["A"]
        walls = []
        for _ in range(2):                                   # (the first call allocates the per-car records: the second is reported)
            s.sync()
            t0 = time.perf_counter()
            r = s.resample(SEED, want_state=True, want_trans=True)
            t1 = time.perf_counter()
            stays_c, parked_c = host_stays(r["state"], r["trans"], Z)
            t2 = time.perf_counter()
            walls.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
            del r
        res["C"] = {"resample_with_matrices_ms": round(walls[-1][0], 1), "host_loop_ms": round(walls[-1][1], 1), "ms": round(sum(walls[-1]), 1),
                    "arrays_equal_arm_B": bool(np.array_equal(stays_c, b["stays"]) and np.array_equal(parked_c, b["parked"]))}
        # B as a user sees it next to C: the blocking call, the copies to the host included
        sB = ctx["B"]
        sB.sync()
        t0 = time.perf_counter()
        sB.resample(SEED, stays=True)
        res["B"]["blocking_with_host_copy_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        res["B_over_C_device_resident"] = round(res["B"]["ms_per_resample"] / res["C"]["ms"], 6)
        res["B_over_C_blocking"] = round(res["B"]["blocking_with_host_copy_ms"] / res["C"]["ms"], 5)
    out["shapes"][name] = res
    print(f"{name}: {json.dumps(res)}", flush=True)
    for s in ctx.values():
        s.close()
    del d_counts, d_stays, d_parked, blocking
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
