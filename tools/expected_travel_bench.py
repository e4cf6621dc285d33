#!/usr/bin/env python3
"""What the expected travel costs (include/cpm_expected_travel.h, csrc/cpm_expected_travel.h; development tool, bench.py is the
contract bench).

Shapes: those of tools/expected_bench.py -- the headline (Z = 4,096, cpm_synth_tables), Melbourne's Z = 2,357 with dense tables and
with tables built from the datamatrix (sparse row packs) -- each with cpm_synth_datamatrix's datamatrix and distances resident.
Arms, ONE process and one context per shape, in interleaved blocks between two synchronisations (block 0 a warm-up, the median of the
others):
  E     expected_dev: T operators (the stream rate the weights build is judged against)
  ET    expected_dev, then expected_travel_dev (seconds, km and totals) with warm weights
  W     ONE build of the trip weights: the distance matrix is uploaded again in front of every build (not timed; it empties the cache
        of the weights and nothing else), then expected_trip_dev and a synchronisation are timed, one build per measurement
  R     one resample_dev(travel=True) of 1,000 cars per zone, for scale
Reported: ms per call; for W the HBM bytes T * Z^2 * 16 + Z^2 * 8 and the TB/s that is, and its ratio to E's TB/s.  Prints one JSON
line (plus progress lines)."""
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
ap.add_argument("--shapes", default="headline,melbourne_dense,melbourne_dataset")
ap.add_argument("--calls", type=int, default=20, help="calls per timed block (E, ET)")
ap.add_argument("--builds", type=int, default=4, help="weights builds per block (W)")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--cpz", type=int, default=1000)
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
SHAPES = {"headline": (4096, False), "melbourne_dense": (2357, False), "melbourne_dataset": (2357, True)}

out = {"device": cpm.device_info(0)["name"], "T": T, "calls_per_block": args.calls, "builds_per_block": args.builds, "blocks": args.blocks,
       "cars_per_zone": args.cpz, "shapes": {}}
for name in args.shapes.split(","):
    Z, dataset = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED)
        if dataset:
            s.build_p_drive(0.1, 0.9, 0.5, want=False)
            s.build_p_dest(2, want=False)
        else:
            s.synth_tables(TSEED)
        dist = s.get_distance()
        s.init_states(Z * args.cpz, args.cpz)
        s.solve_ivp(SEED, want=False)
        d_out = torch.empty(s.expected_words(), dtype=torch.float64, device="cuda")
        d_trav = torch.empty(s.expected_words(), dtype=torch.float64, device="cuda")
        d_tot = torch.empty(2, dtype=torch.float64, device="cuda")
        d_w = torch.empty(2 * T * Z, dtype=torch.float64, device="cuda")
        d_counts = torch.empty(s.counts_words(), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.expected_dev(d_out.data_ptr())          # (builds the per-table arrays and the weights: once, not timed)
        s.expected_trip_dev(d_w.data_ptr())
        s.sync()
        builds0 = s.expected_trip_builds()

        def e_arm():
            s.expected_dev(d_out.data_ptr())

        def et_arm():
            s.expected_dev(d_out.data_ptr())
            s.expected_travel_dev(d_out.data_ptr(), 1, d_trav.data_ptr(), d_tot.data_ptr())

        def r_arm():
            s.resample_dev(SEED, d_counts.data_ptr(), travel=True)

        ms = {"E": [], "ET": [], "W": [], "R": []}
        for block in range(args.blocks + 1):
            for k, fn, n in (("E", e_arm, args.calls), ("ET", et_arm, args.calls), ("R", r_arm, max(2, args.calls // 4))):
                s.sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                s.sync()
                if block:
                    ms[k].append((time.perf_counter() - t0) / n * 1e3)
            for _ in range(args.builds):
                s.set_distance(dist)              # (synchronises; the next call builds the weights again)
                t0 = time.perf_counter()
                s.expected_trip_dev(d_w.data_ptr())
                s.sync()
                if block:
                    ms["W"].append((time.perf_counter() - t0) * 1e3)
        assert s.expected_trip_builds() == builds0 + (args.blocks + 1) * args.builds
        med = {k: statistics.median(v) for k, v in ms.items()}
        e_bytes, w_bytes = T * Z * Z * 8, T * Z * Z * 16 + Z * Z * 8
        res = {"Z": Z, "sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "arms": {
            k: {"ms": round(med[k], 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4)} for k in ms}}
        res["arms"]["E"]["TBps"] = round(e_bytes / (med["E"] * 1e-3) / 1e12, 3)
        res["arms"]["W"].update(hbm_bytes=w_bytes, TBps=round(w_bytes / (med["W"] * 1e-3) / 1e12, 3))
        res["W_over_E_rate"] = round(res["arms"]["W"]["TBps"] / res["arms"]["E"]["TBps"], 3)
        res["ET_over_E"] = round(med["ET"] / med["E"], 4)
        res["ET_over_R"] = round(med["ET"] / med["R"], 4)
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
print(json.dumps(out))
