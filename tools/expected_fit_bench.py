#!/usr/bin/env python3
"""What value-and-gradient of a noise-free objective costs end to end: Evaluator.expected_fit (include/cpm_expected_fit.h: one device
call, one forward propagation, B * (16 + T) words to the host) against Evaluator.expected_gradient_batch (two forward propagations,
two host round trips of whole tensors, numpy cotangents and reductions).  Development tool; bench.py is the contract bench.

Shapes: the headline (Z = 4,096) and Melbourne's Z = 2,357 with the synthetic datamatrix at Melbourne's density (the compact-row route
of build_p_dest) and at density 1 (the dense route); T = 24, the IVP, e_dest = 1.7 with its tangent built on the device.
Arms per B in --batches, ONE process and one context per shape, in interleaved blocks of calls (block 0 a warm-up, the median of the
others):
  fit / fit_dest           Evaluator.expected_fit(pts[:B], {objective: 1}, dest=...): wall time, host work included
  batch / batch_dest       Evaluator.expected_gradient_batch(pts[:B], objective, dest=...): wall time, host work included
  fit_dev / fit_dest_dev   Sampler.expected_fit_dev alone, pipelined between two synchronisations: device time
  grad_dev / grad_dest_dev build_p_drive_batch + expected_grad[_dest]_batch_dev on a resident cotangent (G_next NULL, grad_pi0 not
                           wanted: the forward and backward operators expected_fit_dev runs): device time.  fit_dev - grad_dev is
                           what the new kernels (densities, objectives, cotangent, chain rule, the travel product) cost.
Prints one JSON line (plus progress lines on stderr)."""
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
from carparkingmaps_amd import model_selection as ms

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="headline,melbourne_dataset,melbourne_dense")
ap.add_argument("--batches", default="1,2,4,8,16")
ap.add_argument("--objective", default="activity_error", choices=ms.FIT_WEIGHT_KEYS)
ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=3, help="interleaved blocks per arm (plus one warm-up block)")
args = ap.parse_args()
T, TSEED, E_DEST = 24, 0x5EED7AB1E, 1.7
SHAPES = {"headline": (4096, 0.0868), "melbourne_dataset": (2357, 0.0868), "melbourne_dense": (2357, 1.0)}
BATCHES = [int(b) for b in args.batches.split(",")]
BMAX = max(BATCHES)
OB = args.objective

out = {"device": cpm.device_info(0)["name"], "T": T, "objective": OB, "ivp": True, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, density = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED, density=density)
        rng = np.random.default_rng(1)
        ev = ms.Evaluator(s, C=1, seed=1, measured_activity=rng.uniform(0.0, 1.0, T), measured_parking=rng.uniform(0.0, 1.0, (Z, T)))
        pts = [ms.Point(e_drive=float(e), p_min=float(a), p_max=float(b), e_dest=E_DEST)
               for a, b, e in zip(rng.uniform(0.05, 0.2, BMAX), rng.uniform(0.7, 0.95, BMAX), rng.uniform(0.3, 1.5, BMAX))]
        w3 = [1.0 if k == OB else 0.0 for k in ms.FIT_WEIGHT_KEYS]
        words = s.expected_words()
        d_rec = torch.empty(BMAX * s.fit_words(), dtype=torch.float64, device="cuda")
        d_cot = torch.from_numpy(rng.uniform(-1.0, 1.0, BMAX * words)).cuda()
        d_grad = torch.empty(BMAX * Z * T, dtype=torch.float64, device="cuda")
        d_dest = torch.empty(BMAX * Z * T, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        lo, hi, ex = [p.p_min for p in pts], [p.p_max for p in pts], [p.e_drive for p in pts]

        def fit_dev(B, dest):
            s.expected_fit_dev(lo[:B], hi[:B], ex[:B], w3, d_rec.data_ptr(), 0, True, dest)

        def grad_dev(B, dest):
            s.build_p_drive_batch(lo[:B], hi[:B], ex[:B])
            if dest:
                s.expected_grad_dest_batch_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_dest.data_ptr(), ivp=True)
            else:
                s.expected_grad_batch_dev(d_cot.data_ptr(), d_grad.data_ptr(), ivp=True)

        arms = {}
        for B in BATCHES:
            for dest, tag in ((False, ""), (True, "_dest")):
                arms[f"fit{tag}/{B}"] = lambda B=B, dest=dest: ev.expected_fit(pts[:B], {OB: 1.0}, ivp=True, dest=dest)
                arms[f"batch{tag}/{B}"] = lambda B=B, dest=dest: ev.expected_gradient_batch(pts[:B], OB, ivp=True, dest=dest)
                arms[f"fit{tag}_dev/{B}"] = lambda B=B, dest=dest: fit_dev(B, dest)
                arms[f"grad{tag}_dev/{B}"] = lambda B=B, dest=dest: grad_dev(B, dest)
        # the tables, the tangent, the per-table arrays, the chain rule's s table and the workspaces: once, not timed
        ev.expected_gradient_batch(pts, OB, ivp=True, dest=True)
        check = ev.expected_fit(pts, {OB: 1.0}, ivp=True, dest=True)
        s.sync()
        ms_ = {k: [] for k in arms}
        for blk in range(args.blocks + 1):
            for k, fn in arms.items():
                s.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                s.sync()
                if blk:
                    ms_[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        med = {k: statistics.median(v) for k, v in ms_.items()}
        res = {"Z": Z, "density": density, "sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "F_of_point_0": check[0]["F"], "batches": {}}
        for B in BATCHES:
            r = {}
            for tag in ("", "_dest"):
                f, b = med[f"fit{tag}/{B}"], med[f"batch{tag}/{B}"]
                fd, gd = med[f"fit{tag}_dev/{B}"], med[f"grad{tag}_dev/{B}"]
                r["fit" + tag] = {"wall_ms": round(f, 4), "min_ms": round(min(ms_[f"fit{tag}/{B}"]), 4), "max_ms": round(max(ms_[f"fit{tag}/{B}"]), 4),
                                  "device_ms": round(fd, 4), "speedup_over_batch": round(b / f, 3)}
                r["batch" + tag] = {"wall_ms": round(b, 4), "min_ms": round(min(ms_[f"batch{tag}/{B}"]), 4), "max_ms": round(max(ms_[f"batch{tag}/{B}"]), 4)}
                r["grad" + tag + "_dev"] = {"device_ms": round(gd, 4)}
                r["new_kernels" + tag] = {"device_ms": round(fd - gd, 4)}
            res["batches"][str(B)] = r
            print(f"# {name} B={B}: fit {r['fit']['wall_ms']} ms vs gradient_batch {r['batch']['wall_ms']} ms (x{r['fit']['speedup_over_batch']}); dest "
                  f"{r['fit_dest']['wall_ms']} vs {r['batch_dest']['wall_ms']} ms (x{r['fit_dest']['speedup_over_batch']}); device {r['fit']['device_ms']} ms, "
                  f"new kernels {r['new_kernels']['device_ms']} ms", file=sys.stderr, flush=True)
        out["shapes"][name] = res
print(json.dumps(out))
