#!/usr/bin/env python3
"""What the adjoint of the expected densities costs (include/cpm_expected_grad.h, csrc/cpm_expected_grad.h; development tool, bench.py
is the contract bench).

Shapes: those of tools/expected_bench.py -- the headline (Z = 4,096, cpm_synth_tables), Melbourne's Z = 2,357 with dense tables and with
tables built from a datamatrix (sparse row packs, so the products read the array ensure_dense_p expands).
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others):
  E     expected_dev: T forward operators
  EI    expected_dev with the IVP: 2T - 1 forward operators
  G     expected_grad_dev: T - 1 forward operators, T backward operators of which T - 1 read p (the last one has mu = 0)
  GI    expected_grad_dev with the IVP and G_next: 2T - 2 forward operators, 2T - 1 backward operators
  R     one resample_dev of 1,000 cars per zone, for scale
Reported per arm: ms per call and, for the gradient arms, the ms left for the backward pass when the forward operators are charged at
the E / EI rate, microseconds per backward operator that reads p, and the TB/s of p that is.  Prints one JSON line (plus progress
lines).  --calls 3 --blocks 1 under a kernel trace gives the per-kernel times."""
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
        rng = np.random.default_rng(1)
        d_out = torch.empty(s.expected_words(), dtype=torch.float64, device="cuda")
        d_cot = torch.from_numpy(rng.uniform(-1.0, 1.0, s.expected_words())).cuda()
        d_gnext = torch.from_numpy(rng.uniform(-1.0, 1.0, Z)).cuda()
        d_grad = torch.empty(Z * T, dtype=torch.float64, device="cuda")
        d_gpi0 = torch.empty(Z, dtype=torch.float64, device="cuda")
        d_counts = torch.empty(s.counts_words(), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.expected_dev(d_out.data_ptr())          # (builds the per-table arrays: once, not timed)
        s.expected_grad_dev(d_cot.data_ptr(), d_grad.data_ptr())   # (and the workspace)
        s.sync()
        # (name: call, forward operators, backward operators that read p)
        arms = {"E": (lambda: s.expected_dev(d_out.data_ptr()), T, 0),
                "EI": (lambda: s.expected_dev(d_out.data_ptr(), ivp=True), 2 * T - 1, 0),
                "G": (lambda: s.expected_grad_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_grad_pi0_ptr=d_gpi0.data_ptr()), T - 1, T - 1),
                "GI": (lambda: s.expected_grad_dev(d_cot.data_ptr(), d_grad.data_ptr(), ivp=True, d_gnext_ptr=d_gnext.data_ptr(),
                                                   d_grad_pi0_ptr=d_gpi0.data_ptr()), 2 * T - 2, 2 * T - 1),
                "R": (lambda: s.resample_dev(SEED, d_counts.data_ptr()), 0, 0)}
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, (fn, _, _) in arms.items():
                n = args.calls if k != "R" else max(2, args.calls // 4)
                s.sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                s.sync()
                if block:
                    ms[k].append((time.perf_counter() - t0) / n * 1e3)
        res = {"Z": Z, "sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "bytes_per_operator": Z * Z * 8, "arms": {}}
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, (_, fwd, bwd) in arms.items():
            a = {"ms": round(med[k], 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4)}
            if fwd and not bwd:
                a["us_per_operator"] = round(med[k] * 1e3 / fwd, 2)
                a["TBps"] = round(fwd * Z * Z * 8 / (med[k] * 1e-3) / 1e12, 3)
            if bwd:
                base = "E" if k == "G" else "EI"
                fwd_ms = med[base] / arms[base][1] * fwd       # the forward operators at the forward arm's rate
                a["forward_ms_at_the_forward_rate"] = round(fwd_ms, 4)
                a["backward_ms"] = round(med[k] - fwd_ms, 4)
                a["us_per_backward_operator"] = round((med[k] - fwd_ms) * 1e3 / bwd, 2)
                a["backward_TBps"] = round(bwd * Z * Z * 8 / ((med[k] - fwd_ms) * 1e-3) / 1e12, 3)
                a["over_forward"] = round(med[k] / med[base], 3)
            res["arms"][k] = a
        res["G_over_R"] = round(med["G"] / med["R"], 3)
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
print(json.dumps(out))
