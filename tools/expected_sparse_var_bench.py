#!/usr/bin/env python3
"""The seed variances from sparse tables (include/cpm_expected_sparse_var.h, csrc/cpm_expected_sparse_var.h) against the dense calls
(development tool; bench.py is the contract bench).

Melbourne's shape (Z = 2,357, T = 24, cpm_synth_datamatrix at density 0.0868) on the two routes that give compact rows:
  melbourne_dataset  build_p_dest on the datamatrix (the dense array does not exist until a dense call expands the rows)
  melbourne_upload   that p_destin read back and uploaded under CPM_OPT_SPARSE_UPLOAD (the uploaded dense array stays resident)
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others), each dense arm beside its sparse twin (s...), with and without the IVP (N = 2T - 1 or T operators); the
yardstick is always the dense arm of the same run:
  elv/K  selv/K   expected_linear_var_dev with K functionals and d_zone, K in --functionals (1, 4 and 24 by default)
  etv/K  setv/K   expected_travel_var_dev likewise
Reported per arm: ms per call, microseconds per operator and per operator and pass, and the bytes of one pass of one operator's product
(dense: the Z * Z * 8 block of p, twice that with the mean plane for travel; sparse: 12 bytes per stored cell and 4 per row, and per
stored cell the gathers the kernel issues: the state line of 16 * NB bytes, and for travel the mean word and the distance).
Then one build of v_sec: set_distance (which makes the trip weights of both forms stale; a blocking copy) followed by nothing,
expected_trip_dev or expected_trip_var_dev of either form; the differences are the builds.
Cold cost after a table change, per route and arm: the installing call plus the first variance call and a synchronisation.
Device memory (hipMemGetInfo through torch) on a context that never made an expected call: tables installed, after
Evaluator(expected_sparse=True).expected_noise(travel=True), after the default Evaluator's.  The bits of the two forms are compared once
per shape.

--count-twin LIB: the pass size of the sparse count pass is a compile-time constant (CPM_EXPS_ELV_NB in csrc/cpm_expected_sparse_var.h);
LIB is a build of the library with the other value.  The tool then runs itself as child processes, alternating the default library and
LIB (CPM_LIB_PATH), --twin-rounds times each, on the dataset route with the count arms alone, and reports every child's selv / elv.
Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="melbourne_dataset,melbourne_upload")
ap.add_argument("--zones", type=int, default=2357)
ap.add_argument("--functionals", default="1,4,24")
ap.add_argument("--calls", type=int, default=3, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=3, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--cold", type=int, default=2, help="cold measurements per arm")
ap.add_argument("--count-only", action="store_true", help="the count arms alone, no builds, cold costs or memory (the children of --count-twin)")
ap.add_argument("--count-twin", default="", help="a build of the library with the other CPM_EXPS_ELV_NB")
ap.add_argument("--twin-rounds", type=int, default=2)
args = ap.parse_args()
T, TSEED, NB_ELV, NB_ETV = 24, 0x5EED7AB1E, 4, 2
Z = args.zones
KS = [int(k) for k in args.functionals.split(",")]
KMAX = max(KS)

if args.count_twin:
    runs = []
    for rnd in range(args.twin_rounds):
        for label, lib in (("default", ""), ("twin", os.path.abspath(args.count_twin))):
            env = dict(os.environ)
            env.pop("CPM_LIB_PATH", None)
            if lib:
                env["CPM_LIB_PATH"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--count-only", "--shapes", "melbourne_dataset", "--zones", str(Z), "--functionals",
                   args.functionals, "--calls", str(args.calls), "--blocks", str(args.blocks)]
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=900)
            if p.returncode != 0:
                sys.exit(f"child {label} round {rnd} ended with {p.returncode}")      # (nothing more is started on the device)
            r = json.loads(p.stdout.decode().strip().splitlines()[-1])["shapes"]["melbourne_dataset"]
            runs.append({"library": label, "round": rnd, "bits_equal": r["bits_equal"],
                         "selv_over_elv": {tag: r["arms"][tag]["sparse_over_dense"] for tag in r["arms"]},
                         "selv_ms": {tag: {k: v["ms"] for k, v in r["arms"][tag].items() if k.startswith("selv")} for tag in r["arms"]}})
            print(f"# {label} round {rnd}: {runs[-1]['selv_over_elv']}", file=sys.stderr, flush=True)
    print(json.dumps({"count_twin": runs}))
    sys.exit(0)

import numpy as np
import torch
import carparkingmaps_amd as cpm
from carparkingmaps_amd import model_selection as M


def used_mb():
    free, total = torch.cuda.mem_get_info()
    return round((total - free) / 2 ** 20, 1)


def timed(fn, s):
    s.sync()
    t0 = time.perf_counter()
    fn()
    s.sync()
    return round(1e3 * (time.perf_counter() - t0), 3)


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


out = {"device": cpm.device_info(0)["name"], "Z": Z, "T": T, "NB_elv": NB_ELV, "NB_etv": NB_ETV, "calls_per_block": args.calls, "blocks": args.blocks,
       "library": os.path.basename(os.environ.get("CPM_LIB_PATH", "") or "default"), "shapes": {}}
rng = np.random.default_rng(1)
zt = Z * T
d_coeff = torch.from_numpy(rng.uniform(-1.0, 1.0, KMAX * 4 * zt)).cuda()
d_w = torch.from_numpy(rng.integers(0, 50, Z).astype(np.float64)).cuda()
d_res, d_res2 = (torch.empty(2 * KMAX, dtype=torch.float64, device="cuda") for _ in range(2))
d_zone, d_zone2 = (torch.empty(2 * KMAX * Z, dtype=torch.float64, device="cuda") for _ in range(2))
d_trip, d_trip2 = (torch.empty(2 * zt, dtype=torch.float64, device="cuda") for _ in range(2))
m_act = rng.uniform(0.0, 1.0, T)
m_park = np.asfortranarray(rng.uniform(0.0, 1.0, (Z, T)))
with cpm.Sampler(Z, T) as s0:                                      # the table on the host, from a context of its own (reading it expands the rows)
    s0.synth_datamatrix(TSEED)
    p_host = s0.build_p_dest(2, want=True)
cells = int(np.count_nonzero(p_host))                              # (the dataset's compact rows also keep its cells of weight 0: a lower bound there)
torch.cuda.empty_cache()
for name in args.shapes.split(","):
    upload = name == "melbourne_upload"
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        dist = s.get_distance()
        if upload:
            s.set_sparse_upload(True)
            install = [lambda: s.set_p_dest(p_host)] * 2
        else:
            install = [lambda: s.build_p_dest(2, want=False), lambda: s.build_p_dest(1.9, want=False)]
        torch.cuda.synchronize()
        install[0]()
        s.sync()
        res = {"sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "cells_nonzero": cells, "density": round(cells / (Z * Z * T), 5)}
        assert res["sparse_pack_words"] > 0, "the tables have no compact rows"
        elv = lambda K, ivp, sp, r=d_res, z=d_zone: s.expected_linear_var_dev(K, d_coeff.data_ptr(), r.data_ptr(), d_w.data_ptr(), ivp, z.data_ptr(), sparse=sp)
        etv = lambda K, ivp, sp, r=d_res, z=d_zone: s.expected_travel_var_dev(K, d_coeff.data_ptr(), r.data_ptr(), d_w.data_ptr(), ivp, z.data_ptr(), sparse=sp)
        if not args.count_only:
            # memory: the sparse noise first, on a context that never made an expected call; then the default Evaluator's
            ev = {sp: M.Evaluator(s, 10 * Z, 1, measured_activity=m_act, measured_parking=m_park, expected_sparse=sp) for sp in (True, False)}
            for e in ev.values():
                e._e_dest = M.e_dest_key(2)                        # (the tables are installed already)
            pt = M.Point(0.5, 0.1, 0.9, 2)
            mem = {"tables_installed": used_mb(), "p_dense_before": s.get_info(cpm.CPM_INFO_P_DENSE)}
            first = {"sparse_noise_ms": timed(lambda: ev[True].expected_noise(pt, travel=True), s)}
            mem["after_sparse_noise"], mem["p_dense_after_sparse_noise"] = used_mb(), s.get_info(cpm.CPM_INFO_P_DENSE)
            first["dense_noise_ms"] = timed(lambda: ev[False].expected_noise(pt, travel=True), s)
            mem["after_dense_noise"], mem["p_dense_after_dense_noise"] = used_mb(), s.get_info(cpm.CPM_INFO_P_DENSE)
            res["memory_mb"], res["first_noise_on_a_fresh_context_ms"] = mem, first
            s.build_p_drive(0.1, 0.9, 0.5, want=False)
        # the bits of the two forms, once
        elv(KMAX, True, True)
        elv(KMAX, True, False, d_res2, d_zone2)
        s.sync()
        bits = bool(torch.equal(d_res.view(torch.int64), d_res2.view(torch.int64))) and bool(torch.equal(d_zone.view(torch.int64), d_zone2.view(torch.int64)))
        if not args.count_only:
            etv(KMAX, True, True)
            etv(KMAX, True, False, d_res2, d_zone2)
            s.expected_trip_var_dev(d_trip.data_ptr(), sparse=True)
            s.expected_trip_var_dev(d_trip2.data_ptr())
            s.sync()
            bits = bits and bool(torch.equal(d_res.view(torch.int64), d_res2.view(torch.int64)))
            bits = bits and bool(torch.equal(d_zone.view(torch.int64), d_zone2.view(torch.int64)))
            bits = bits and bool(torch.equal(d_trip[:zt].view(torch.int64), d_trip2[:zt].view(torch.int64)))
        res["bits_equal"] = bits
        if not args.count_only:
            # cold: the installing call plus the first variance call, alternating tables and arms
            cold = {"sparse": [], "dense": []}
            for i in range(2 * args.cold):
                arm = "sparse" if i % 2 == 0 else "dense"
                inst = install[(i // 2 + 1) % 2]
                cold[arm].append(timed(lambda: (inst(), elv(4, True, arm == "sparse")), s))
            res["cold_install_plus_first_linear_var_ms"] = {k: {"median": statistics.median(v), "all": v} for k, v in cold.items()}
            res["install_only_ms"] = statistics.median([timed(install[i % 2], s) for i in range(args.cold)])
            install[0]()
        arms = {}
        for ivp in (False, True):
            tag = "ivp" if ivp else "day"
            for K in KS:
                for sp, pre in ((False, ""), (True, "s")):
                    arms[f"{pre}elv/{K}/{tag}"] = lambda K=K, ivp=ivp, sp=sp: elv(K, ivp, sp)
                    if not args.count_only:
                        arms[f"{pre}etv/{K}/{tag}"] = lambda K=K, ivp=ivp, sp=sp: etv(K, ivp, sp)
        ms = blocks(s, arms)
        med = {k: statistics.median(v) for k, v in ms.items()}
        row_bytes = cells // T * 12 + Z * 4
        res["bytes_per_operator_and_pass"] = {"elv": Z * Z * 8, "etv": 2 * Z * Z * 8, "selv_rows": row_bytes, "setv_rows": row_bytes,
                                              "selv_gathers_per_cell": 16 * NB_ELV, "setv_gathers_per_cell": 16 * NB_ETV + 16, "cells_per_hour": cells // T}
        res["arms"] = {}
        for ivp in (False, True):
            tag = "ivp" if ivp else "day"
            N = 2 * T - 1 if ivp else T
            r = {"operators": N, "sparse_over_dense": {}}
            for K in KS:
                for arm, nb in (("elv", NB_ELV), ("etv", NB_ETV)):
                    if arm == "etv" and args.count_only:
                        continue
                    passes = (K + nb - 1) // nb
                    for pre in ("", "s"):
                        k = f"{pre}{arm}/{K}/{tag}"
                        r[f"{pre}{arm}/{K}"] = {"ms": round(med[k], 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4), "passes": passes,
                                                "us_per_operator": round(med[k] * 1e3 / N, 2), "us_per_operator_and_pass": round(med[k] * 1e3 / N / passes, 2)}
                    r["sparse_over_dense"][f"{arm}/{K}"] = round(med[f"s{arm}/{K}/{tag}"] / med[f"{arm}/{K}/{tag}"], 3)
            res["arms"][tag] = r
            print(f"# {name} {tag}: sparse / dense {r['sparse_over_dense']}", file=sys.stderr, flush=True)
        if not args.count_only:
            stale = lambda: s.set_distance(dist)
            build = blocks(s, {"stale": stale, "trip": lambda: (stale(), s.expected_trip_dev(d_trip.data_ptr())),
                               "strip": lambda: (stale(), s.expected_trip_dev(d_trip.data_ptr(), sparse=True)),
                               "trip_and_var": lambda: (stale(), s.expected_trip_var_dev(d_trip.data_ptr())),
                               "strip_and_var": lambda: (stale(), s.expected_trip_var_dev(d_trip.data_ptr(), sparse=True))})
            b = {k: statistics.median(v) for k, v in build.items()}
            res["builds"] = {"stale_ms": round(b["stale"], 4), "trip_weights_ms": {"dense": round(b["trip"] - b["stale"], 4), "sparse": round(b["strip"] - b["stale"], 4)},
                             "v_sec_ms": {"dense": round(b["trip_and_var"] - b["trip"], 4), "sparse": round(b["strip_and_var"] - b["strip"], 4)},
                             "builds": {"dense": s.expected_trip_var_builds(), "sparse": s.expected_trip_var_builds(sparse=True)}}
            print(f"# {name}: builds {res['builds']}, cold {res['cold_install_plus_first_linear_var_ms']}, memory {res['memory_mb']}, "
                  f"bits_equal {res['bits_equal']}", file=sys.stderr, flush=True)
        out["shapes"][name] = res
print(json.dumps(out))
