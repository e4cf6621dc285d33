#!/usr/bin/env python3
"""What the hourly OD trip counts cost (include/cpm_flows.h, csrc/cpm_flows.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096 x 1,000 cars per zone, cpm_synth_tables) and Melbourne's (Z = 2,357, cpm_synth_datamatrix at density
0.0868: sparse packs) x 1,000 and x 100.  Arms, ONE process, one context each, the same seeds:
  A        resample_dev: the step without flows (what bench.py times as ms_per_step)
  B_hour   resample_flows_dev, the OD kernel behind every hour's launches (CPM_OPT_FLOWS_KEPT 0)
  B_kept   resample_flows_dev, one launch of the OD kernel over the kept runs of all hours (CPM_OPT_FLOWS_KEPT 1)
in interleaved blocks of pipelined steps between two synchronisations (block 0 a warm-up, the median of the others), and
  C        once, not interleaved: what the library offered for the same tensor before -- the blocking resample(want_state=True,
           want_trans=True) plus a host histogram per hour -- whose flows must equal arm B's.
Reported per shape: ms per resample of every arm, B - A next to the OD kernel's algorithmic bytes (T * Z^2 * 4 written, 4 per driver and
the run lengths read) and the share of the 8 TB/s peak that makes, and B / C.  Prints one JSON line (plus progress lines)."""
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
HBM_PEAK = 8.0e12
SHAPES = {"headline": (4096, 1000, False), "melbourne_x1000": (2357, 1000, True), "melbourne_x100": (2357, 100, True)}
ARMS = ("A", "B_hour", "B_kept")


def make(Z, cpz, dataset, kept):
    s = cpm.Sampler(Z, T)
    if dataset:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)
    else:
        s.synth_tables(TSEED)
    s.set_flows_kept(kept)
    s.init_states(Z * cpz, cpz)
    s.solve_ivp(SEED, want=False)
    return s


out = {"device": cpm.device_info(0)["name"], "T": T, "steps_per_block": args.steps, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, cpz, dataset = SHAPES[name]
    ctx = {"A": make(Z, cpz, dataset, False), "B_hour": make(Z, cpz, dataset, False), "B_kept": make(Z, cpz, dataset, True)}
    d_counts = [torch.zeros(ctx["A"].counts_words(), dtype=torch.int64, device="cuda") for _ in range(2)]
    d_flows = torch.zeros(ctx["A"].flows_words(), dtype=torch.int32, device="cuda")
    res = {"Z": Z, "cars_per_zone": cpz, "sparse_pack_words": ctx["A"].get_info(cpm.CPM_INFO_SPARSE_TABLES)}
    blocking = {}
    for a, s in ctx.items():
        blocking[a] = s.resample(SEED, flows=(a != "A"))
        res[a] = {"step": s.last_step()}
    same = all(np.array_equal(blocking[a]["parking"], blocking["A"]["parking"]) and np.array_equal(blocking[a]["driving"], blocking["A"]["driving"])
               for a in ARMS) and np.array_equal(blocking["B_hour"]["flows"], blocking["B_kept"]["flows"])
    res["counts_and_flows_equal_in_all_arms"] = bool(same)
    drivers = int(blocking["A"]["driving"].sum())
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
                    s.resample_flows_dev(SEED, d_counts[i & 1].data_ptr(), d_flows.data_ptr())
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
    # the OD kernel's algorithmic bytes per resample: every cell written once, every driver's run entry and every run length read once
    alg = T * Z * Z * 4 + 4 * drivers + T * Z * 32 * 4
    res["drivers_per_resample"] = drivers
    res["od_kernel_algorithmic_bytes"] = alg
    for a in ("B_hour", "B_kept"):
        extra = res[a]["ms_per_resample"] - res["A"]["ms_per_resample"]
        res[a]["ms_over_A"] = round(extra, 4)
        res[a]["algorithmic_TBs"] = round(alg / (extra * 1e-3) / 1e12, 3) if extra > 0 else None
        res[a]["share_of_8TBs_peak"] = round(alg / (extra * 1e-3) / HBM_PEAK, 4) if extra > 0 else None
    if not args.no_compat:
        s = ctx["A"]
        walls = []
        for _ in range(2):                                   # (the first call allocates the per-car records: the second is reported)
            s.sync()
            t0 = time.perf_counter()
            r = s.resample(SEED, want_state=True, want_trans=True)
            t1 = time.perf_counter()
            flows_c = np.empty((T, Z, Z), dtype=np.int32)
            for t in range(T):
                drove = r["trans"][:, t, 0] == 1
                o, d = r["state"][drove, t] - 1, r["trans"][drove, t, 1].astype(np.int64) - 1
                flows_c[t] = np.bincount(o * Z + d, minlength=Z * Z).reshape(Z, Z)
            t2 = time.perf_counter()
            walls.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
            del r
        res["C"] = {"resample_with_matrices_ms": round(walls[-1][0], 1), "host_histogram_ms": round(walls[-1][1], 1),
                    "ms": round(sum(walls[-1]), 1), "flows_equal_arm_B": bool(np.array_equal(flows_c, blocking["B_hour"]["flows"]))}
        # B as a user sees it next to C: the blocking call, the copy of the tensor to the host included
        sB = ctx["B_hour"]
        sB.sync()
        t0 = time.perf_counter()
        sB.resample(SEED, flows=True)
        res["B_hour"]["blocking_with_host_copy_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["B_over_C_device_resident"] = round(res["B_hour"]["ms_per_resample"] / res["C"]["ms"], 6)
        res["B_over_C_blocking"] = round(res["B_hour"]["blocking_with_host_copy_ms"] / res["C"]["ms"], 5)
        del flows_c
    out["shapes"][name] = res
    print(f"{name}: {json.dumps(res)}", flush=True)
    for s in ctx.values():
        s.close()
    del d_counts, d_flows, blocking
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
