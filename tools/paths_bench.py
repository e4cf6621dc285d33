#!/usr/bin/env python3
"""What the per-car day record costs (include/cpm_paths.h, csrc/cpm_paths.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096 x 1,000 cars per zone, cpm_synth_tables) and Melbourne's (Z = 2,357, cpm_synth_datamatrix at density
0.0868: sparse packs) x 1,000 and x 100.  Arms, ONE process, one context each, the same seeds:
  A   resample_dev: the step without the record (what bench.py times as ms_per_step)
  B   resample_paths_dev on the grouped family: k_paths_carry + k_grouped_paths behind every hour's launches
  C   resample_paths_dev under set_kernel(CPM_KERNEL_CAR): the record from the per-car kernels (their d_rec, copied)
in interleaved blocks of pipelined steps between two synchronisations (block 0 a warm-up, the median of the others).  Once per shape,
not interleaved: the wall time of the blocking resample(want_state=True, want_trans=True), and that of arm B's step +
paths_expand_dev into device tensors, whose every array is compared with the blocking call's.
Reported per shape: ms per resample of every arm and their blocks, B - A in microseconds per hour, the bytes of the record, and whether
B lies below C by more than the largest max - min of any arm's blocks.  Prints one JSON line (plus progress lines).  Per-kernel
durations: run this under rocprofv3 --kernel-trace --stats with --blocks 1 --no-compat, in a run of its own."""
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
ap.add_argument("--steps", type=int, default=50, help="resamples per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--no-compat", action="store_true", help="skip the once-per-shape comparison with the blocking matrices")
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
SHAPES = {"headline": (4096, 1000, False), "melbourne_x1000": (2357, 1000, True), "melbourne_x100": (2357, 100, True)}
ARMS = ("A", "B", "C")


def make(Z, cpz, dataset, kernel):
    s = cpm.Sampler(Z, T)
    if dataset:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)
    else:
        s.synth_tables(TSEED)
    s.init_states(Z * cpz, cpz)
    s.solve_ivp(SEED, want=False)
    s.set_kernel(kernel)
    return s


out = {"device": cpm.device_info(0)["name"], "T": T, "steps_per_block": args.steps, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, cpz, dataset = SHAPES[name]
    n = Z * cpz
    ctx = {a: make(Z, cpz, dataset, cpm.CPM_KERNEL_CAR if a == "C" else cpm.CPM_KERNEL_AUTO) for a in ARMS}
    d_counts = [torch.zeros(ctx["A"].counts_words(), dtype=torch.int64, device="cuda") for _ in range(2)]
    d_paths = {a: torch.zeros(T * n, dtype=torch.int32, device="cuda") for a in ("B", "C")}
    res = {"Z": Z, "cars_per_zone": cpz, "sparse_pack_words": ctx["A"].get_info(cpm.CPM_INFO_SPARSE_TABLES), "record_bytes": 4 * T * n}
    blocking = {}
    for a, s in ctx.items():                                  # (the blocking call first: it repairs what the shape outgrows)
        blocking[a] = s.resample(SEED, paths=(a != "A"))
        res[a] = {"step": s.last_step()}
    res["counts_equal_in_all_arms"] = bool(all(np.array_equal(blocking[a][k], blocking["A"][k]) for a in ("B", "C") for k in ("parking", "driving")))
    res["records_equal_B_C"] = bool(np.array_equal(blocking["B"]["paths"], blocking["C"]["paths"]))
    res["drivers_per_resample"] = int(blocking["A"]["driving"].sum())

    def step(a, s, i):
        if a == "A":
            s.resample_dev(SEED, d_counts[i & 1].data_ptr())
        else:
            s.resample_paths_dev(SEED, d_counts[i & 1].data_ptr(), d_paths[a].data_ptr())

    per = {a: [] for a in ARMS}
    for blk in range(args.blocks + 1):                       # (block 0: warm-up, not recorded)
        for a, s in ctx.items():
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                step(a, s, i)
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
        res[a]["blocks_max_minus_min"] = round(max(per[a]) - min(per[a]), 4)
    extra = res["B"]["ms_per_resample"] - res["A"]["ms_per_resample"]
    res["B"]["ms_over_A"] = round(extra, 4)
    res["B"]["us_per_hour_over_A"] = round(1e3 * extra / T, 2)
    spread = max(res[a]["blocks_max_minus_min"] for a in ARMS)
    res["largest_block_spread_ms"] = spread
    res["C_minus_B_ms"] = round(res["C"]["ms_per_resample"] - res["B"]["ms_per_resample"], 4)
    res["B_below_C_by_more_than_the_spread"] = bool(res["C_minus_B_ms"] > spread)
    for a in ("B", "C"):
        res[a]["device_record_equals_blocking"] = bool(np.array_equal(d_paths[a].cpu().numpy().view(np.uint32).reshape(T, n), blocking[a]["paths"]))
    if not args.no_compat:
        s = ctx["A"]
        walls = []
        for _ in range(2):                                   # (the first call allocates the per-car records: the second is reported)
            s.sync()
            t0 = time.perf_counter()
            r = s.resample(SEED, want_state=True, want_trans=True)
            walls.append(1e3 * (time.perf_counter() - t0))
        res["compat"] = {"resample_with_matrices_ms": round(walls[-1], 1)}
        sB = ctx["B"]
        d_state = torch.zeros((T, n), dtype=torch.int64, device="cuda")
        d_trans = torch.zeros((4, T, n), dtype=torch.float64, device="cuda")
        walls = []
        for _ in range(2):
            sB.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sB.resample_paths_dev(SEED, d_counts[0].data_ptr(), d_paths["B"].data_ptr())
            sB.paths_expand_dev(SEED, d_paths["B"].data_ptr(), d_state.data_ptr(), d_trans.data_ptr())
            sB.sync()
            walls.append(1e3 * (time.perf_counter() - t0))
        res["B"]["step_plus_expand_dev_ms"] = round(walls[-1], 3)
        res["B"]["expanded_state_equals_compat"] = bool(np.array_equal(d_state.cpu().numpy().T, r["state"]))
        res["B"]["expanded_trans_equals_compat"] = bool(all(np.array_equal(d_trans[k].cpu().numpy().T, r["trans"][:, :, k]) for k in range(4)))
        res["B_plus_expand_over_compat"] = round(res["B"]["step_plus_expand_dev_ms"] / res["compat"]["resample_with_matrices_ms"], 6)
        del r, d_state, d_trans
    out["shapes"][name] = res
    print(f"{name}: {json.dumps(res)}", flush=True)
    for s in ctx.values():
        s.close()
    del d_counts, d_paths, blocking
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
