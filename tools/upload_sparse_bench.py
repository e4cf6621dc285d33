#!/usr/bin/env python3
"""An uploaded p_destin with and without sparse row packs (CPM_OPT_SPARSE_UPLOAD, csrc/cpm_upload.h) against the tables the device
builds itself (development tool; bench.py is the contract bench).

Melbourne's shape (Z = 2,357, cpm_synth_datamatrix at density 0.0868), x 100 and x 1,000 cars per zone, three arms in ONE process on
the same seeds:
  built   tables built on the device (build_p_dest: sparse packs from the dataset's compact rows)
  dense   that p_destin read back and uploaded with the option off (dense packs: what every upload got before the option)
  sparse  uploaded with the option on
Per arm: ms per resample (pipelined cpm_resample_dev steps between two synchronisations; the arms in interleaved blocks, block 0 a
warm-up, the median of the others), CPM_INFO_SPARSE_TABLES and the step record of a blocking resample, whose counts must be the
same in all three; for the uploads the wall time of set_p_dest (median of --uploads calls), for `sparse` the durations of its two
kernels (hipEvents of the dispatches, CPM_PROFILE_UPLOAD).  Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carparkingmaps_amd as cpm
from carparkingmaps_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--zones", type=int, default=2357)
ap.add_argument("--cpz", default="100,1000")
ap.add_argument("--density", type=float, default=0.0868)
ap.add_argument("--steps", type=int, default=200, help="resamples per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--uploads", type=int, default=3, help="timed set_p_dest calls per upload arm")
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
Z = args.zones
ARMS = ("built", "dense", "sparse")


def upload(s, p_dest, sparse):
    """wall time of set_p_dest (the call synchronises), median of a few; for the sparse route its two kernels' durations too"""
    s.set_sparse_upload(sparse)
    walls, kernels = [], []
    for _ in range(args.uploads + 1):                        # (the first call allocates: not recorded)
        if sparse:
            s.set_profile(True, kernel=_lib.CPM_PROFILE_UPLOAD)
        s.sync()
        t0 = time.perf_counter()
        s.set_p_dest(p_dest)
        walls.append(1e3 * (time.perf_counter() - t0))
        if sparse:
            kernels.append(s.last_kernel_ms())
            s.set_profile(False)
    rec = {"set_p_dest_wall_ms": round(float(np.median(walls[1:])), 3), "set_p_dest_wall_ms_all": [round(w, 3) for w in walls[1:]]}
    if sparse:
        k = np.array([m for m in kernels[1:] if len(m) == 2])
        if len(k):
            rec["k_up_compact_ms"] = round(float(np.median(k[:, 0])), 4)
            rec["k_up_pack_ms"] = round(float(np.median(k[:, 1])), 4)
    return rec


out = {"device": cpm.device_info(0)["name"], "Z": Z, "T": T, "density": args.density, "steps_per_block": args.steps, "blocks": args.blocks, "shapes": {}}
ctx = {a: cpm.Sampler(Z, T) for a in ARMS}
for s in ctx.values():
    s.synth_datamatrix(TSEED, args.density)
p_drive = ctx["built"].build_p_drive(0.1, 0.9, 0.5)
p_dest = ctx["built"].build_p_dest(2)
out["row_cells_max"] = int((p_dest != 0).sum(axis=1).max())
out["nonzero_share"] = round(float((p_dest != 0).mean()), 5)
arm_rec = {a: {} for a in ARMS}
for a in ("dense", "sparse"):
    ctx[a].set_p_drive(p_drive)
    arm_rec[a].update(upload(ctx[a], p_dest, a == "sparse"))
    print(f"{a}: {arm_rec[a]}", flush=True)
del p_dest
d_counts = [torch.zeros(ctx["built"].counts_words(), dtype=torch.int64, device="cuda") for _ in range(2)]

for cpz in [int(x) for x in args.cpz.split(",")]:
    C = Z * cpz
    res = {a: dict(arm_rec[a]) for a in ARMS}
    counts = {}
    for a, s in ctx.items():
        s.init_states(C, cpz)
        s.solve_ivp(SEED, want=False)
        counts[a] = s.resample(SEED)
        res[a]["sparse_pack_words"] = s.get_info(_lib.CPM_INFO_SPARSE_TABLES)
        res[a]["step"] = s.last_step()
        res[a]["sampler_bytes_per_hour"] = s.algorithmic_bytes_per_hour()
    agree = all(np.array_equal(counts[a]["parking"], counts["built"]["parking"]) and np.array_equal(counts[a]["driving"], counts["built"]["driving"])
                for a in ARMS)
    per = {a: [] for a in ARMS}
    for blk in range(args.blocks + 1):                       # (block 0: warm-up, not recorded)
        for a, s in ctx.items():
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                s.resample_dev(SEED, d_counts[i & 1].data_ptr())
            s.sync()
            dt = time.perf_counter() - t0
            if int(d_counts[(args.steps - 1) & 1][-1]) != 0:
                print(f"x{cpz} {a}: status word set", flush=True)
            if blk:
                per[a].append(1e3 * dt / args.steps)
        if blk:
            print(f"x{cpz} block {blk}: " + ", ".join(f"{a} {per[a][-1]:.4f}" for a in ARMS) + " ms per resample", flush=True)
    for a in ARMS:
        res[a]["step_after_timed_blocks"] = ctx[a].last_step()
        res[a]["ms_per_resample"] = round(float(np.median(per[a])), 4)
        res[a]["ms_per_resample_blocks"] = [round(x, 4) for x in per[a]]
    res["counts_equal_in_all_arms"] = bool(agree)
    res["sparse_over_dense"] = round(res["sparse"]["ms_per_resample"] / res["dense"]["ms_per_resample"], 4)
    res["sparse_over_built"] = round(res["sparse"]["ms_per_resample"] / res["built"]["ms_per_resample"], 4)
    out["shapes"][f"x{cpz}"] = res
for s in ctx.values():
    s.close()
print(json.dumps(out), flush=True)
