#!/usr/bin/env python3
"""What the variance of travel functionals costs beside the linear operator it extends (include/cpm_expected_travel_var.h,
csrc/cpm_expected_travel_var.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096, cpm_synth_tables and cpm_synth_datamatrix) and Melbourne's Z = 2,357 with dense tables.  Arms, ONE
process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up, the
median of the others), each with and without the IVP (N = 2T - 1 or T operators):
  etv/K     expected_travel_var_dev with K functionals and d_zone, K in --functionals (1, 4 and 24 by default): N products, passes of
            at most NB = 2 functionals, each streaming the hour's block of p AND of the mean plane
  elv/K     expected_linear_var_dev at the same K: N - 1 products, passes of at most 4, each streaming the block of p
Reported per arm: ms per call, the microseconds per operator (one operator covers all passes of the call), per operator and pass, and
the TB/s of the streamed planes counting them once per pass; and etv over elv at the same K.
Then one build of the trip variance weights v_sec beside one build of the trip weights: the distance matrix is set again from
centroids (a device kernel; it invalidates the trip weights and nothing else), followed by nothing, expected_trip_dev, or
expected_trip_var_dev (which builds both), synchronised; the differences are the builds.
Prints one JSON line (plus progress lines)."""
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
args = ap.parse_args()
T, TSEED, NB_ETV, NB_ELV = 24, 0x5EED7AB1E, 2, 4
SHAPES = {"headline": 4096, "melbourne_dense": 2357}
KS = [int(k) for k in args.functionals.split(",")]
KMAX = max(KS)


def blocks(s, arms):
    for fn in arms.values():                      # (the per-table arrays and the workspaces: once, not timed)
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
    return ms


out = {"device": cpm.device_info(0)["name"], "T": T, "NB_etv": NB_ETV, "NB_elv": NB_ELV, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
for name in args.shapes.split(","):
    Z = SHAPES[name]
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(TSEED)
        s.synth_datamatrix(TSEED, 1.0)                # (every cell holds a mean and a standard deviation: the full cost of var_sec)
        rng = np.random.default_rng(1)
        zt = Z * T
        d_coeff = torch.from_numpy(rng.uniform(-1.0, 1.0, KMAX * 4 * zt)).cuda()
        d_w = torch.from_numpy(rng.integers(0, 50, Z).astype(np.float64)).cuda()
        d_res = torch.empty(2 * KMAX, dtype=torch.float64, device="cuda")
        d_zone = torch.empty(2 * KMAX * Z, dtype=torch.float64, device="cuda")
        d_trip = torch.empty(2 * zt, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        arms = {}
        for ivp in (False, True):
            tag = "ivp" if ivp else "day"
            for K in KS:
                arms[f"etv/{K}/{tag}"] = lambda K=K, ivp=ivp: s.expected_travel_var_dev(K, d_coeff.data_ptr(), d_res.data_ptr(), d_w.data_ptr(), ivp,
                                                                                       d_zone.data_ptr())
                arms[f"elv/{K}/{tag}"] = lambda K=K, ivp=ivp: s.expected_linear_var_dev(K, d_coeff.data_ptr(), d_res.data_ptr(), d_w.data_ptr(), ivp,
                                                                                       d_zone.data_ptr())
        ms = blocks(s, arms)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"Z": Z, "bytes_per_plane": Z * Z * 8, "arms": {}}
        for ivp in (False, True):
            tag = "ivp" if ivp else "day"
            N = 2 * T - 1 if ivp else T
            r = {"operators": N}
            for K in KS:
                for arm, nb, products, planes in (("etv", NB_ETV, N, 2), ("elv", NB_ELV, N - 1, 1)):
                    m = med[f"{arm}/{K}/{tag}"]
                    passes = (K + nb - 1) // nb
                    r[f"{arm}/{K}"] = {"ms": round(m, 4), "min_ms": round(min(ms[f"{arm}/{K}/{tag}"]), 4), "max_ms": round(max(ms[f"{arm}/{K}/{tag}"]), 4),
                                       "passes": passes, "us_per_operator": round(m * 1e3 / N, 2), "us_per_operator_and_pass": round(m * 1e3 / N / passes, 2),
                                       "TBps_streamed": round(planes * passes * products * Z * Z * 8 / (m * 1e-3) / 1e12, 3)}
            r["etv_over_elv"] = {str(K): round(med[f"etv/{K}/{tag}"] / med[f"elv/{K}/{tag}"], 3) for K in KS}
            res["arms"][tag] = r
            print(f"# {name} {tag}: " + ", ".join(f"etv/{K} {r[f'etv/{K}']['ms']} ms ({r[f'etv/{K}']['TBps_streamed']} TB/s) elv/{K} {r[f'elv/{K}']['ms']} ms"
                                                   for K in KS), file=sys.stderr, flush=True)
        # one build of v_sec beside one build of the trip weights
        lat, lon = -37.8 + 0.3 * rng.random(Z), 144.9 + 0.4 * rng.random(Z)
        stale = lambda: s.set_distance_from_centroids(lat, lon)
        build = blocks(s, {"stale": stale, "trip": lambda: (stale(), s.expected_trip_dev(d_trip.data_ptr())),
                           "trip_and_var": lambda: (stale(), s.expected_trip_var_dev(d_trip.data_ptr()))})
        b = {k: statistics.median(v) for k, v in build.items()}
        res["builds"] = {"stale_ms": round(b["stale"], 4), "trip_weights_ms": round(b["trip"] - b["stale"], 4), "v_sec_ms": round(b["trip_and_var"] - b["trip"], 4),
                         "trip_TBps": round(2 * T * Z * Z * 8 / ((b["trip"] - b["stale"]) * 1e-3) / 1e12, 3),
                         "v_sec_TBps": round(3 * T * Z * Z * 8 / ((b["trip_and_var"] - b["trip"]) * 1e-3) / 1e12, 3), "builds": s.expected_trip_var_builds()}
        print(f"# {name}: builds {res['builds']}", file=sys.stderr, flush=True)
        out["shapes"][name] = res
print(json.dumps(out))
