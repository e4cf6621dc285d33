#!/usr/bin/env python3
"""What the forward tangent of the expected densities costs on the device: one Sampler.expected_tangent_dev call
(include/cpm_expected_tangent.h) of K = 3 directions (d p_drive / d (e_drive, p_min, p_max)) and of K = 4 (a fourth along
d p_destin / d e_dest, which adds the pass over the tangent table), against Sampler.expected_dev alone -- by bytes K = 3 should cost
about one expected_dev, the dest direction about one more -- and against Sampler.expected_fit_dev at B = 1 with and without dest, the
reverse-mode call that gives the gradient of one scalar.  Development tool; bench.py is the contract bench.

Shapes: the README's -- the headline (Z = 4,096) and Melbourne's Z = 2,357 with the synthetic datamatrix at Melbourne's density (the
compact-row route of build_p_dest) and at density 1 (the dense route); T = 24, the IVP, e_dest = 1.7 with its tangent built on the
device.  ONE process and one context per shape; the arms run in interleaved blocks of calls between two synchronisations (block 0 a
warm-up, the median of the others): device time.  Prints one JSON line (plus progress lines on stderr)."""
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
ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
args = ap.parse_args()
T, TSEED, E_DEST = 24, 0x5EED7AB1E, 1.7
SHAPES = {"headline": (4096, 0.0868), "melbourne_dataset": (2357, 0.0868), "melbourne_dense": (2357, 1.0)}
PT = (0.1, 0.9, 0.5)   # p_min, p_max, e_drive

out = {"device": cpm.device_info(0)["name"], "T": T, "ivp": True, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z, density = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED, density=density)
        rng = np.random.default_rng(1)
        s.set_measured_activity(rng.uniform(0.0, 1.0, T))
        s.set_measured(np.asfortranarray(rng.uniform(0.0, 1.0, (Z, T))))
        s.build_p_drive(*PT, want=False)
        s.build_p_dest(E_DEST, want=False)
        s.build_p_dest_tangent()
        zt = Z * T
        d_dirs = torch.zeros(4 * zt, dtype=torch.float64, device="cuda")
        s.build_p_drive_tangent_dev(*PT, d_dirs.data_ptr())        # three direction tables; the fourth direction is c_dest alone
        d_out = torch.empty(4 * 2 * zt, dtype=torch.float64, device="cuda")
        d_exp = torch.empty(2 * zt, dtype=torch.float64, device="cuda")
        d_rec = torch.empty(s.fit_words(), dtype=torch.float64, device="cuda")
        w3 = [1.0, 0.0, 0.0]
        arms = {
            "expected_dev": lambda: s.expected_dev(d_exp.data_ptr(), 0, True),
            "tangent_K3": lambda: s.expected_tangent_dev(3, d_out.data_ptr(), d_dirs.data_ptr(), ivp=True, d_expected_ptr=d_exp.data_ptr()),
            "tangent_K4_dest": lambda: s.expected_tangent_dev(4, d_out.data_ptr(), d_dirs.data_ptr(), c_dest=[0.0, 0.0, 0.0, 1.0], ivp=True,
                                                              d_expected_ptr=d_exp.data_ptr()),
            "fit_dev": lambda: s.expected_fit_dev([PT[0]], [PT[1]], [PT[2]], w3, d_rec.data_ptr(), 0, True, False),
            "fit_dest_dev": lambda: s.expected_fit_dev([PT[0]], [PT[1]], [PT[2]], w3, d_rec.data_ptr(), 0, True, True),
        }
        for fn in arms.values():      # the per-table arrays and the workspaces: once, not timed
            fn()
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
        res = {"Z": Z, "density": density, "arms": {k: {"device_ms": round(med[k], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms_.items()},
               "K3_over_expected": round(med["tangent_K3"] / med["expected_dev"], 3),
               "dest_direction_over_expected": round((med["tangent_K4_dest"] - med["tangent_K3"]) / med["expected_dev"], 3),
               "K3_over_fit": round(med["tangent_K3"] / med["fit_dev"], 3), "K4_dest_over_fit_dest": round(med["tangent_K4_dest"] / med["fit_dest_dev"], 3)}
        print(f"# {name}: expected_dev {med['expected_dev']:.3f} ms, tangent K=3 {med['tangent_K3']:.3f} ms (x{res['K3_over_expected']}), K=4 with dest "
              f"{med['tangent_K4_dest']:.3f} ms; expected_fit_dev {med['fit_dev']:.3f} ms, with dest {med['fit_dest_dev']:.3f} ms", file=sys.stderr, flush=True)
        out["shapes"][name] = res
print(json.dumps(out))
