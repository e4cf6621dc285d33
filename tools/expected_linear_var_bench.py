#!/usr/bin/env python3
"""What the variance of linear functionals costs against the existing passes over the same bytes (include/cpm_expected_linear_var.h,
csrc/cpm_expected_linear_var.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096, cpm_synth_tables) and Melbourne's Z = 2,357 with dense tables.  Arms, ONE process and one context per
shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up, the median of the others), each with
and without the IVP (N = 2T - 1 or T operators, N - 1 of them with a product):
  elv/K     expected_linear_var_dev with K functionals and d_zone, K in --functionals (1, NB = 4 and 24 by default)
  grad      expected_grad_dev with G_next and grad_pi0: N - 1 forward operators and N backward ones over the same block of p
  forward   expected_dev: what the forward operators of `grad` cost
  var       expected_var_dev, the only other second moment (N - 1 products Z x Z x Z)
Reported per arm: ms per call; for elv the microseconds per operator (one operator covers all passes of the call) and the TB/s of p
counting the block once per pass of at most 4 functionals; for grad the same of its backward share (the call less `forward` at
(N - 1) / N).  Prints one JSON line (plus progress lines).  --calls 2 --blocks 1 under a kernel trace gives the per-kernel times."""
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
ap.add_argument("--shapes", default="headline,melbourne_dense")
ap.add_argument("--functionals", default="1,4,24")
ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=3, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--no-var", action="store_true", help="leave out the expected_var_dev arm (Z^3 work per operator)")
args = ap.parse_args()
T, TSEED, NB = 24, 0x5EED7AB1E, 4
SHAPES = {"headline": 4096, "melbourne_dense": 2357}
KS = [int(k) for k in args.functionals.split(",")]
KMAX = max(KS)

out = {"device": cpm.device_info(0)["name"], "T": T, "NB": NB, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(TSEED)
        rng = np.random.default_rng(1)
        words = s.expected_words()
        d_coeff = torch.from_numpy(rng.uniform(-1.0, 1.0, KMAX * words)).cuda()
        d_w = torch.from_numpy(rng.integers(0, 50, Z).astype(np.float64)).cuda()
        d_res = torch.empty(2 * KMAX, dtype=torch.float64, device="cuda")
        d_zone = torch.empty(2 * KMAX * Z, dtype=torch.float64, device="cuda")
        d_gnext = torch.from_numpy(rng.uniform(-1.0, 1.0, Z)).cuda()
        d_grad = torch.empty(Z * T, dtype=torch.float64, device="cuda")
        d_gpi0 = torch.empty(Z, dtype=torch.float64, device="cuda")
        d_exp = torch.empty(words, dtype=torch.float64, device="cuda")
        d_var = torch.empty(s.expected_var_words(), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        arms = {}
        for ivp in (False, True):
            tag = "ivp" if ivp else "day"
            for K in KS:
                arms[f"elv/{K}/{tag}"] = lambda K=K, ivp=ivp: s.expected_linear_var_dev(K, d_coeff.data_ptr(), d_res.data_ptr(), d_w.data_ptr(), ivp,
                                                                                       d_zone.data_ptr())
            arms[f"grad/{tag}"] = lambda ivp=ivp: s.expected_grad_dev(d_coeff.data_ptr(), d_grad.data_ptr(), ivp=ivp, d_gnext_ptr=d_gnext.data_ptr(),
                                                                      d_grad_pi0_ptr=d_gpi0.data_ptr())
            arms[f"forward/{tag}"] = lambda ivp=ivp: s.expected_dev(d_exp.data_ptr(), 0, ivp)
            if not args.no_var:
                arms[f"var/{tag}"] = lambda ivp=ivp: s.expected_var_dev(d_var.data_ptr(), d_w.data_ptr(), ivp)
        for fn in arms.values():                  # (the per-table arrays and the workspaces: once, not timed)
            fn()
        s.sync()
        ms = {k: [] for k in arms}
        for blk in range(args.blocks + 1):
            for k, fn in arms.items():
                s.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                s.sync()
                if blk:
                    ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"Z": Z, "bytes_per_operator_p": Z * Z * 8, "arms": {}}
        for ivp in (False, True):
            tag = "ivp" if ivp else "day"
            N = 2 * T - 1 if ivp else T
            r = {"operators": N}
            for K in KS:
                m = med[f"elv/{K}/{tag}"]
                passes = (K + NB - 1) // NB
                r[f"elv/{K}"] = {"ms": round(m, 4), "min_ms": round(min(ms[f"elv/{K}/{tag}"]), 4), "max_ms": round(max(ms[f"elv/{K}/{tag}"]), 4),
                                 "us_per_operator": round(m * 1e3 / N, 2), "us_per_operator_and_pass": round(m * 1e3 / N / passes, 2),
                                 "TBps_per_pass": round(passes * (N - 1) * Z * Z * 8 / (m * 1e-3) / 1e12, 3)}
            g, f = med[f"grad/{tag}"], med[f"forward/{tag}"]
            back = g - f * (N - 1) / N                     # (the forward arm applies N operators, the gradient N - 1)
            r["grad"] = {"ms": round(g, 4), "forward_ms": round(f, 4), "backward_ms": round(back, 4), "us_per_backward_operator": round(back * 1e3 / N, 2),
                         "TBps_backward": round(N * Z * Z * 8 / (back * 1e-3) / 1e12, 3)}
            if not args.no_var:
                r["var"] = {"ms": round(med[f"var/{tag}"], 4)}
            r["elv_pass_over_grad_backward"] = {str(K): round(med[f"elv/{K}/{tag}"] / ((K + NB - 1) // NB) / back, 3) for K in KS}
            res["arms"][tag] = r
            print(f"# {name} {tag}: " + ", ".join(f"elv/{K} {r[f'elv/{K}']['ms']} ms ({r[f'elv/{K}']['TBps_per_pass']} TB/s)" for K in KS)
                  + f"; grad backward {r['grad']['backward_ms']} ms ({r['grad']['TBps_backward']} TB/s)", file=sys.stderr, flush=True)
        out["shapes"][name] = res
print(json.dumps(out))
