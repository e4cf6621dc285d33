#!/usr/bin/env python3
"""What the OD trip counts cost as compressed sparse rows (include/cpm_flows_csr.h, csrc/cpm_flows_csr.h; development tool modelled on
tools/flows_bench.py, whose shapes it uses; bench.py is the contract bench).

Arms, ONE process, one context each, the same seeds, in interleaved blocks of pipelined steps between two synchronisations (block 0
a warm-up, the median of the others):
  A        resample_dev: the step without flows
  B        resample_flows_dev in its default form: the dense tensor, the yardstick
  C_hour   resample_flows_csr_dev, count / scan / fill behind every hour's launches (CPM_OPT_FLOWS_KEPT 0)
  C_kept   resample_flows_csr_dev, one count / scan / fill over the kept runs of all hours (CPM_OPT_FLOWS_KEPT 1)
Reported per shape: nnz and the share of non-zero cells, bytes written per arm, ms per resample, B - A and C - A, and once per shape
the blocking wall time of resample(flows=True) against resample(flows="csr") (the median of --wall-reps calls after a first one that
allocates), whose arrays must equal np.nonzero of the dense tensor.  Prints one JSON line (plus progress lines)."""
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
ap.add_argument("--wall-reps", type=int, default=3, help="blocking calls per form whose median wall time is reported")
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
SHAPES = {"headline": (4096, 1000, False), "melbourne_x1000": (2357, 1000, True), "melbourne_x100": (2357, 100, True)}
ARMS = ("A", "B", "C_hour", "C_kept")


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


def wall(s, **kw):
    ms = []
    for _ in range(args.wall_reps + 1):                      # (the first call allocates: not reported)
        s.sync()
        t0 = time.perf_counter()
        r = s.resample(SEED, **kw)
        ms.append(1e3 * (time.perf_counter() - t0))
    return r, round(float(np.median(ms[1:])), 2)


out = {"device": cpm.device_info(0)["name"], "T": T, "steps_per_block": args.steps, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, cpz, dataset = SHAPES[name]
    ctx = {a: make(Z, cpz, dataset, a == "C_kept") for a in ARMS}
    res = {"Z": Z, "cars_per_zone": cpz, "sparse_pack_words": ctx["A"].get_info(cpm.CPM_INFO_SPARSE_TABLES)}
    # the blocking calls first: they grow what has to grow, give nnz, and are the wall-time comparison
    plain = ctx["A"].resample(SEED)
    dense, dense_ms = wall(ctx["B"], flows=True)
    csr = {}
    for a in ("C_hour", "C_kept"):
        r, ms = wall(ctx[a], flows="csr")
        csr[a] = r
        res[a] = {"blocking_ms": ms}
    res["B"] = {"blocking_ms": dense_ms}
    res["A"] = {}
    c = csr["C_hour"]["flows_csr"]
    nnz = int(c["row_ptr"][-1])
    flat = dense["flows"].reshape(T * Z, Z)
    rows, cols = np.nonzero(flat)
    ok = (nnz == rows.size and np.array_equal(np.diff(c["row_ptr"]), np.bincount(rows, minlength=T * Z)) and np.array_equal(c["dest"], cols)
          and np.array_equal(c["count"], flat[rows, cols]))
    k = csr["C_kept"]["flows_csr"]
    ok = ok and np.array_equal(k["row_ptr"], c["row_ptr"]) and np.array_equal(k["dest"], c["dest"]) and np.array_equal(k["count"], c["count"])
    ok = ok and all(np.array_equal(r["parking"], plain["parking"]) and np.array_equal(r["driving"], plain["driving"]) for r in (dense, *csr.values()))
    res["csr_equals_nonzero_of_dense_and_counts_equal_in_all_arms"] = bool(ok)
    res["nnz"] = nnz
    res["share_of_cells_non_zero"] = round(nnz / (T * Z * Z), 5)
    res["drivers_per_resample"] = int(plain["driving"].sum())
    res["A"]["bytes_written"] = 0
    res["B"]["bytes_written"] = T * Z * Z * 4
    for a in ("C_hour", "C_kept"):
        res[a]["bytes_written"] = nnz * 8 + (T * Z + 1) * 8 * 2          # entries; row_ptr written by the count and again by the scan
    res["blocking_dense_over_csr"] = round(dense_ms / res["C_hour"]["blocking_ms"], 2)
    del dense, csr, flat, rows, cols, c, k
    for a, s in ctx.items():
        res[a]["step"] = s.last_step()
    d_counts = [torch.zeros(ctx["A"].counts_words(), dtype=torch.int64, device="cuda") for _ in range(2)]
    d_flows = torch.zeros(ctx["A"].flows_words(), dtype=torch.int32, device="cuda")
    d_row_ptr = torch.zeros(T * Z + 1, dtype=torch.int64, device="cuda")
    d_dest = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    per = {a: [] for a in ARMS}
    for blk in range(args.blocks + 1):                       # (block 0: warm-up, not recorded)
        for a, s in ctx.items():
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                if a == "A":
                    s.resample_dev(SEED, d_counts[i & 1].data_ptr())
                elif a == "B":
                    s.resample_flows_dev(SEED, d_counts[i & 1].data_ptr(), d_flows.data_ptr())
                else:
                    s.resample_flows_csr_dev(SEED, d_counts[i & 1].data_ptr(), d_row_ptr.data_ptr(), d_dest.data_ptr(), d_count.data_ptr(), nnz)
            s.sync()
            dt = time.perf_counter() - t0
            if int(d_counts[(args.steps - 1) & 1][-1]) != 0:
                print(f"{name} {a}: status word set", flush=True)
            if a.startswith("C") and int(d_row_ptr[-1]) != nnz:
                print(f"{name} {a}: row_ptr ends on {int(d_row_ptr[-1])}, expected {nnz}", flush=True)
            if blk:
                per[a].append(1e3 * dt / args.steps)
        if blk:
            print(f"{name} block {blk}: " + ", ".join(f"{a} {per[a][-1]:.4f}" for a in ARMS) + " ms per resample", flush=True)
    for a in ARMS:
        res[a]["step_after_timed_blocks"] = ctx[a].last_step()
        res[a]["ms_per_resample"] = round(float(np.median(per[a])), 4)
        res[a]["ms_per_resample_blocks"] = [round(x, 4) for x in per[a]]
    for a in ("B", "C_hour", "C_kept"):
        res[a]["ms_over_A"] = round(res[a]["ms_per_resample"] - res["A"]["ms_per_resample"], 4)
    out["shapes"][name] = res
    print(f"{name}: {json.dumps(res)}", flush=True)
    for s in ctx.values():
        s.close()
    del d_counts, d_flows, d_row_ptr, d_dest, d_count
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
