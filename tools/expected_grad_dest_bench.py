#!/usr/bin/env python3
"""What the adjoint along a tangent of p_destin costs (include/cpm_expected_grad_dest.h, csrc/cpm_expected_grad_dest.h; development
tool, bench.py is the contract bench).

Shapes and method are those of tools/expected_grad_bench.py: the headline (Z = 4,096, cpm_synth_tables), Melbourne's Z = 2,357 with
dense tables and with tables built from a datamatrix (sparse row packs: the products read the array ensure_dense_p expands).  ONE process
and one context per shape, the arms in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up, the median
of the others):
  E, EI  expected_dev without / with the IVP: the forward operators' rate, charged to the gradient arms
  G      expected_grad_dev: T - 1 forward operators, T backward operators of which T - 1 read p
  GD     expected_grad_dest_dev, tangent warm: the same operators, each product streaming p and dP
  GDI    expected_grad_dest_dev with the IVP and G_next: 2T - 2 forward operators, 2T - 1 backward operators
  TT     expected_trip_tangent_dev: one pass over dP, the mean plane and the distance matrix
  BT     build_p_dest_tangent, cold (the first call, which allocates the table) and warm (median of three more), with the bytes its
         passes move and the TB/s that is.  The dataset shape builds from the compact rows; the two dense shapes get a full
         datamatrix (density 1) AFTER their other arms are timed, which takes the dense route.
The tangent of the two dense shapes is an uploaded random table (their tables come from no datamatrix); the dataset shape's is the
built one.  Prints one JSON line (plus progress lines).  --calls 3 --blocks 1 under a kernel trace gives the per-kernel times."""
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
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
T, TSEED = 24, 0x5EED7AB1E
SHAPES = {"headline": (4096, False), "melbourne_dense": (2357, False), "melbourne_dataset": (2357, True)}


def timed(s, fn, n=1):
    s.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    s.sync()
    return (time.perf_counter() - t0) / n * 1e3


def build_arm(s, Z, compact):
    """cold and warm build_p_dest_tangent of the installed tables, with the bytes of its passes"""
    cold = timed(s, s.build_p_dest_tangent)
    warm = statistics.median(timed(s, s.build_p_dest_tangent) for _ in range(3))
    table = Z * Z * T * 8
    if compact:                                   # memset + the rows' cells twice (32-byte cell, p, destination) + the scattered stores
        cells = int(np.count_nonzero(s.get_p_dest_tangent())) if Z <= 2500 else 0
        moved = table + 2 * cells * 44 + cells * 8
    else:                                         # k_tan_log: means + p in, l out; k_tan_rowsum: p + l in; k_tan_final: p + l in, dP out
        moved = 8 * table
    return {"route": "compact rows" if compact else "dense", "cold_ms": round(cold, 3), "warm_ms": round(warm, 3), "bytes": moved,
            "warm_TBps": round(moved / (warm * 1e-3) / 1e12, 3)}


out = {"device": cpm.device_info(0)["name"], "T": T, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, dataset = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        res = {"Z": Z, "bytes_per_operator_p": Z * Z * 8, "bytes_per_operator_p_and_dP": 2 * Z * Z * 8, "arms": {}}
        if dataset:
            s.synth_datamatrix(TSEED)
            s.build_p_drive(0.1, 0.9, 0.5, want=False)
            s.build_p_dest(1.7, want=False)
            res["arms"]["BT"] = build_arm(s, Z, s.get_info(cpm.CPM_INFO_SPARSE_TABLES) != 0)
        else:
            s.synth_tables(TSEED)
            s.synth_datamatrix(TSEED)             # (the trip tangent reads the mean plane and the distances)
            block = np.random.default_rng(2).uniform(-1.0, 1.0, (Z, Z, 1))
            s.set_p_dest_tangent(np.asfortranarray(np.broadcast_to(block, (Z, Z, T))))
            del block
        res["sparse_pack_words"] = s.get_info(cpm.CPM_INFO_SPARSE_TABLES)
        rng = np.random.default_rng(1)
        d_out = torch.empty(s.expected_words(), dtype=torch.float64, device="cuda")
        d_cot = torch.from_numpy(rng.uniform(-1.0, 1.0, s.expected_words())).cuda()
        d_gnext = torch.from_numpy(rng.uniform(-1.0, 1.0, Z)).cuda()
        d_grad = torch.empty(Z * T, dtype=torch.float64, device="cuda")
        d_dest = torch.empty(Z * T, dtype=torch.float64, device="cuda")
        d_gpi0 = torch.empty(Z, dtype=torch.float64, device="cuda")
        d_dw = torch.empty(2 * Z * T, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s.expected_dev(d_out.data_ptr())          # (builds the per-table arrays: once, not timed)
        s.expected_grad_dest_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_dest.data_ptr())   # (and the workspace, at its larger size)
        s.sync()
        # (name: call, forward operators, backward operators that read p, bytes a backward operator streams)
        arms = {"E": (lambda: s.expected_dev(d_out.data_ptr()), T, 0, 0),
                "EI": (lambda: s.expected_dev(d_out.data_ptr(), ivp=True), 2 * T - 1, 0, 0),
                "G": (lambda: s.expected_grad_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_grad_pi0_ptr=d_gpi0.data_ptr()), T - 1, T - 1, Z * Z * 8),
                "GD": (lambda: s.expected_grad_dest_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_dest.data_ptr(), d_grad_pi0_ptr=d_gpi0.data_ptr()),
                       T - 1, T - 1, 2 * Z * Z * 8),
                "GDI": (lambda: s.expected_grad_dest_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_dest.data_ptr(), ivp=True, d_gnext_ptr=d_gnext.data_ptr(),
                                                         d_grad_pi0_ptr=d_gpi0.data_ptr()), 2 * T - 2, 2 * T - 1, 2 * Z * Z * 8),
                "TT": (lambda: s.expected_trip_tangent_dev(d_dw.data_ptr()), 0, 0, 0)}
        ms = {k: [] for k in arms}
        for blk in range(args.blocks + 1):
            for k, (fn, _, _, _) in arms.items():
                v = timed(s, fn, args.calls)
                if blk:
                    ms[k].append(v)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k, (_, fwd, bwd, per_op) in arms.items():
            a = {"ms": round(med[k], 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4)}
            if fwd and not bwd:
                a["us_per_operator"] = round(med[k] * 1e3 / fwd, 2)
            if bwd:
                base = "EI" if k == "GDI" else "E"
                fwd_ms = med[base] / arms[base][1] * fwd       # the forward operators at the forward arm's rate
                a["backward_ms"] = round(med[k] - fwd_ms, 4)
                a["us_per_backward_operator"] = round((med[k] - fwd_ms) * 1e3 / bwd, 2)
                a["backward_TBps"] = round(bwd * per_op / ((med[k] - fwd_ms) * 1e-3) / 1e12, 3)
            if k == "TT":
                a["bytes"] = 2 * Z * Z * T * 8 + Z * Z * 8
                a["TBps"] = round(a["bytes"] / (med[k] * 1e-3) / 1e12, 3)
            res["arms"][k] = a
        res["GD_over_G_per_backward_operator"] = round(res["arms"]["GD"]["us_per_backward_operator"] / res["arms"]["G"]["us_per_backward_operator"], 3)
        if not dataset:                           # the dense route of the builder, on a full datamatrix
            s.synth_datamatrix(TSEED, density=1.0)
            s.build_p_dest(1.7, want=False)
            res["arms"]["BT"] = build_arm(s, Z, s.get_info(cpm.CPM_INFO_SPARSE_TABLES) != 0)
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v.get('ms', v.get('warm_ms'))} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
line = json.dumps(out)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
print(line)
