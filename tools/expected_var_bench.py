#!/usr/bin/env python3
"""What the exact variances cost (include/cpm_expected_var.h, csrc/cpm_expected_var.h; development tool, bench.py is the contract
bench).

Shapes: the headline (Z = 4,096) and Melbourne's Z = 2,357, dense tables (cpm_synth_tables), T = 24.  Arms, ONE process and one
context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up, the median of the
others):
  V     expected_var_dev: T - 1 products P <- P * M_t, T reduction passes
  VI    expected_var_dev with the IVP: 2T - 2 products, T reduction passes
  MM    torch.matmul of two f64 Z x Z device tensors, T - 1 of them per "call": the yardstick on the same box
Reported per arm: ms per call, ms per product and f64 TFLOP/s (2 Z^3 flop per product over the WHOLE call: the reduction passes and
the identity are inside the time, so the product kernel itself is no slower than the figure), and V's and VI's time per product over
MM's (the aim: at most 2).  Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import carparkingmaps_amd as cpm

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="headline,melbourne")
ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=3, help="interleaved blocks per arm (plus one warm-up block)")
args = ap.parse_args()
T, TSEED = 24, 0x5EED7AB1E
SHAPES = {"headline": 4096, "melbourne": 2357}

out = {"device": cpm.device_info(0)["name"], "T": T, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(TSEED)
        d_out = torch.empty(s.expected_var_words(), dtype=torch.float64, device="cuda")
        a = torch.rand(Z, Z, dtype=torch.float64, device="cuda")
        b = torch.rand(Z, Z, dtype=torch.float64, device="cuda")
        c = torch.empty(Z, Z, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s.expected_var_dev(d_out.data_ptr())          # (builds the per-table arrays and the workspace: once, not timed)
        s.sync()

        def mm():
            for _ in range(T - 1):
                torch.matmul(a, b, out=c)

        def wait():
            s.sync()
            torch.cuda.synchronize()

        arms = {"V": (lambda: s.expected_var_dev(d_out.data_ptr()), T - 1),
                "VI": (lambda: s.expected_var_dev(d_out.data_ptr(), ivp=True), 2 * T - 2),
                "MM": (mm, T - 1)}
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, (fn, _) in arms.items():
                wait()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                wait()
                if block:
                    ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        res = {"Z": Z, "flop_per_product": 2 * Z ** 3, "arms": {}}
        for k, (_, products) in arms.items():
            m = statistics.median(ms[k])
            res["arms"][k] = {"ms": round(m, 3), "min_ms": round(min(ms[k]), 3), "max_ms": round(max(ms[k]), 3), "products": products,
                              "ms_per_product": round(m / products, 4), "TFLOPs": round(products * 2 * Z ** 3 / (m * 1e-3) / 1e12, 2)}
        for k in ("V", "VI"):
            res[k + "_over_MM_per_product"] = round(res["arms"][k]["ms_per_product"] / res["arms"]["MM"]["ms_per_product"], 3)
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms ({v['TFLOPs']} TF)" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
print(json.dumps(out))
