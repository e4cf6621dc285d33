#!/usr/bin/env python3
"""What the expected densities cost (include/cpm_expected.h, csrc/cpm_expected.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096, cpm_synth_tables), Melbourne's Z = 2,357 with dense tables (cpm_synth_tables) and with tables built
from a datamatrix (cpm_synth_datamatrix at density 0.0868: sparse row packs, so the product reads the array ensure_dense_p expands).
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others):
  E     expected_dev: T operators
  EI    expected_dev with the IVP: 2T - 1 operators
  B<n>  expected_batch_dev over n = 1, 2, 4, 8, 16 fleets
  R     one resample_dev of 1,000 cars per zone, for scale
Reported per arm: ms per call, microseconds per operator, the bytes an operator reads of p (Z * Z * 8 per pass of at most eight
fleets) and the TB/s that is.  Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carparkingmaps_amd as cpm

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="headline,melbourne_dense,melbourne_dataset")
ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--cpz", type=int, default=1000)
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
SHAPES = {"headline": (4096, False), "melbourne_dense": (2357, False), "melbourne_dataset": (2357, True)}
FLEETS = (1, 2, 4, 8, 16)
PASS = 8  # fleets of one pass over p (kExpMaxNB)

out = {"device": cpm.device_info(0)["name"], "T": T, "calls_per_block": args.calls, "blocks": args.blocks, "cars_per_zone": args.cpz, "shapes": {}}
for name in args.shapes.split(","):
    Z, dataset = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        if dataset:
            s.synth_datamatrix(TSEED)
            s.build_p_drive(0.1, 0.9, 0.5, want=False)
            s.build_p_dest(2, want=False)
        else:
            s.synth_tables(TSEED)
        s.init_states(Z * args.cpz, args.cpz)
        s.solve_ivp(SEED, want=False)
        d_out = torch.empty(max(FLEETS) * s.expected_words(), dtype=torch.float64, device="cuda")
        d_counts = torch.empty(s.counts_words(), dtype=torch.int64, device="cuda")
        rng = np.random.default_rng(1)
        tables = {B: np.asfortranarray(rng.uniform(0.05, 0.95, (Z, T, B))) for B in FLEETS}
        torch.cuda.synchronize()
        s.expected_dev(d_out.data_ptr())          # (builds the per-table arrays: once, not timed)
        s.sync()
        arms = {"E": (lambda: s.expected_dev(d_out.data_ptr()), T, 1),
                "EI": (lambda: s.expected_dev(d_out.data_ptr(), ivp=True), 2 * T - 1, 1),
                "R": (lambda: s.resample_dev(SEED, d_counts.data_ptr()), T, 0)}
        for B in FLEETS:
            arms[f"B{B}"] = (lambda: s.expected_batch_dev(d_out.data_ptr()), T, -(-B // PASS))
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, (fn, _, _) in arms.items():
                if k[0] == "B":
                    s.set_p_drive_batch(tables[int(k[1:])])
                n = args.calls if k != "R" else max(2, args.calls // 4)
                s.sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                s.sync()
                if block:
                    ms[k].append((time.perf_counter() - t0) / n * 1e3)
        res = {"Z": Z, "sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "bytes_per_pass": Z * Z * 8, "arms": {}}
        for k, (_, ops, passes) in arms.items():
            m = statistics.median(ms[k])
            a = {"ms": round(m, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "us_per_operator": round(m * 1e3 / ops, 2)}
            if passes:
                a["bytes_per_operator"] = passes * Z * Z * 8
                a["TBps"] = round(ops * passes * Z * Z * 8 / (m * 1e-3) / 1e12, 3)
            res["arms"][k] = a
        res["B8_over_B1"] = round(res["arms"]["B8"]["ms"] / res["arms"]["B1"]["ms"], 3)
        res["E_over_R"] = round(res["arms"]["E"]["ms"] / res["arms"]["R"]["ms"], 3)
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
print(json.dumps(out))
