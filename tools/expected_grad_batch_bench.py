#!/usr/bin/env python3
"""What the batched adjoint of the expected densities costs against the single calls it replaces (include/cpm_expected_grad_batch.h,
csrc/cpm_expected_grad_batch.h; development tool, bench.py is the contract bench).

Shapes: those of tools/expected_grad_bench.py -- the headline (Z = 4,096, cpm_synth_tables), Melbourne's Z = 2,357 with dense tables and
with tables built from a datamatrix.  Every call runs with the IVP, G_next and grad_pi0: 2T - 2 forward and 2T - 1 backward operators.
Arms per B in --batches, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations
(block 0 a warm-up, the median of the others):
  batch    build_p_drive_batch of B points, then ONE expected_grad_batch_dev
  single   B times: build_p_drive of the point, then expected_grad_dev with its cotangents (the B = 1 kernels: the baseline)
  batch_dest / single_dest   the same pair with the tangent (expected_grad_dest_batch_dev / expected_grad_dest_dev)
  forward  build_p_drive_batch, then expected_batch_dev: what the forward operators of `batch` cost
Reported per arm: ms per call; for the batched arms also the speed-up over `single`, the microseconds per backward operator (the call
less the forward operators at the `forward` rate, over 2T - 1; an operator covers all passes of the batch) and the TB/s of p -- and dP
-- that is, counting the block once per pass of at most 8 fleets.  Prints one JSON line (plus progress lines).  --calls 2 --blocks 1
under a kernel trace gives the per-kernel times."""
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
ap.add_argument("--batches", default="1,2,4,8,16")
ap.add_argument("--calls", type=int, default=5, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=3, help="interleaved blocks per arm (plus one warm-up block)")
args = ap.parse_args()
T, TSEED = 24, 0x5EED7AB1E
SHAPES = {"headline": (4096, False), "melbourne_dense": (2357, False), "melbourne_dataset": (2357, True)}
BATCHES = [int(b) for b in args.batches.split(",")]
BMAX = max(BATCHES)

out = {"device": cpm.device_info(0)["name"], "T": T, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, dataset = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED)                 # (build_p_drive[_batch] reads it)
        if dataset:
            s.build_p_dest(1.7, want=False)
            s.build_p_dest_tangent()
        else:
            s.synth_tables(TSEED)
            block = np.random.default_rng(2).uniform(-1.0, 1.0, (Z, Z, 1))
            s.set_p_dest_tangent(np.asfortranarray(np.broadcast_to(block, (Z, Z, T))))
            del block
        rng = np.random.default_rng(1)
        p_min, p_max, e_drive = rng.uniform(0.05, 0.2, BMAX), rng.uniform(0.7, 0.95, BMAX), rng.uniform(0.3, 1.5, BMAX)
        words = s.expected_words()
        d_out = torch.empty(BMAX * words, dtype=torch.float64, device="cuda")
        d_cot = torch.from_numpy(rng.uniform(-1.0, 1.0, BMAX * words)).cuda()
        d_gnext = torch.from_numpy(rng.uniform(-1.0, 1.0, BMAX * Z)).cuda()
        d_grad = torch.empty(BMAX * Z * T, dtype=torch.float64, device="cuda")
        d_dest = torch.empty(BMAX * Z * T, dtype=torch.float64, device="cuda")
        d_gpi0 = torch.empty(BMAX * Z, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        cot, gnext, grad, dest, gpi0 = (a.data_ptr() for a in (d_cot, d_gnext, d_grad, d_dest, d_gpi0))

        def batch(B, with_dest):
            s.build_p_drive_batch(p_min[:B], p_max[:B], e_drive[:B])
            if with_dest:
                s.expected_grad_dest_batch_dev(cot, grad, dest, ivp=True, d_gnext_ptr=gnext, d_grad_pi0_ptr=gpi0)
            else:
                s.expected_grad_batch_dev(cot, grad, ivp=True, d_gnext_ptr=gnext, d_grad_pi0_ptr=gpi0)

        def single(B, with_dest):
            for b in range(B):
                s.build_p_drive(p_min[b], p_max[b], e_drive[b], want=False)
                a = dict(ivp=True, d_gnext_ptr=gnext + 8 * b * Z, d_grad_pi0_ptr=gpi0 + 8 * b * Z)
                if with_dest:
                    s.expected_grad_dest_dev(cot + 8 * b * words, grad + 8 * b * Z * T, dest + 8 * b * Z * T, **a)
                else:
                    s.expected_grad_dev(cot + 8 * b * words, grad + 8 * b * Z * T, **a)

        def forward(B):
            s.build_p_drive_batch(p_min[:B], p_max[:B], e_drive[:B])
            s.expected_batch_dev(d_out.data_ptr(), ivp=True)

        arms = {}
        for B in BATCHES:
            arms[f"batch/{B}"] = lambda B=B: batch(B, False)
            arms[f"single/{B}"] = lambda B=B: single(B, False)
            arms[f"batch_dest/{B}"] = lambda B=B: batch(B, True)
            arms[f"single_dest/{B}"] = lambda B=B: single(B, True)
            arms[f"forward/{B}"] = lambda B=B: forward(B)
        batch(BMAX, True)                         # (the per-table arrays and the workspaces: once, not timed)
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
        res = {"Z": Z, "sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "bytes_per_operator_p": Z * Z * 8, "batches": {}}
        nb, nf = 2 * T - 1, 2 * T - 2
        for B in BATCHES:
            passes = (B + 7) // 8
            r = {}
            for kind, blocks_read in (("", 1), ("_dest", 2)):
                b_ms, s_ms, f_ms = med[f"batch{kind}/{B}"], med[f"single{kind}/{B}"], med[f"forward/{B}"]
                back = b_ms - f_ms * nf / (nf + 1)             # (the forward arm applies 2T - 1 operators, the gradient 2T - 2)
                r["batch" + kind] = {"ms": round(b_ms, 4), "min_ms": round(min(ms[f"batch{kind}/{B}"]), 4), "max_ms": round(max(ms[f"batch{kind}/{B}"]), 4),
                                     "backward_ms": round(back, 4), "us_per_backward_operator": round(back * 1e3 / nb, 2),
                                     "TBps_per_pass": round(passes * blocks_read * nb * Z * Z * 8 / (back * 1e-3) / 1e12, 3),
                                     "speedup_over_single": round(s_ms / b_ms, 3)}
                r["single" + kind] = {"ms": round(s_ms, 4), "min_ms": round(min(ms[f"single{kind}/{B}"]), 4), "max_ms": round(max(ms[f"single{kind}/{B}"]), 4),
                                      "ms_per_point": round(s_ms / B, 4)}
            r["forward"] = {"ms": round(med[f"forward/{B}"], 4)}
            res["batches"][str(B)] = r
            print(f"# {name} B={B}: batch {r['batch']['ms']} ms vs single {r['single']['ms']} ms (x{r['batch']['speedup_over_single']}); "
                  f"dest {r['batch_dest']['ms']} vs {r['single_dest']['ms']} ms (x{r['batch_dest']['speedup_over_single']})", file=sys.stderr, flush=True)
        out["shapes"][name] = res
print(json.dumps(out))
