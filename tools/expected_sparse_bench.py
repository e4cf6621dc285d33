#!/usr/bin/env python3
"""The expected densities from sparse tables (include/cpm_expected_sparse.h, csrc/cpm_expected_sparse.h) against the dense call
(development tool; bench.py is the contract bench).

Melbourne's shape (Z = 2,357, T = 24, cpm_synth_datamatrix at density 0.0868) on the two routes that give compact rows:
  melbourne_dataset  build_p_dest on the datamatrix (the dense array does not exist until a dense call expands the rows)
  melbourne_upload   that p_destin read back and uploaded under CPM_OPT_SPARSE_UPLOAD (the uploaded dense array stays resident)
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others), each dense arm beside its sparse twin (S...):
  E / SE      expected_dev: T operators             EI / SEI    with the IVP: 2T - 1 operators
  B<n> / SB<n>  expected_batch_dev over n = 1, 2, 4, 8, 16 fleets
Cold cost after a table change, once per route and arm: the installing call (build_p_dest with another e_dest, or set_p_dest) plus the
first expected call and a synchronisation -- where the dense expansion shows.  Device memory (hipMemGetInfo through torch) after the
tables are installed, after the first sparse call and after the first dense call.  Reported per sparse arm: the bytes an operator
reads of the cells (12 per stored cell + the column pointers, per pass of at most eight fleets) and the TB/s that is; for the dense
arms Z * Z * 8 per pass.  The bits of the two forms are compared once per shape.  Prints one JSON line (plus progress lines)."""
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
ap.add_argument("--shapes", default="melbourne_dataset,melbourne_upload")
ap.add_argument("--zones", type=int, default=2357)
ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--cold", type=int, default=3, help="cold measurements per arm")
args = ap.parse_args()
T, TSEED = 24, 0x5EED7AB1E
Z = args.zones
FLEETS = (1, 2, 4, 8, 16)
PASS = 8  # fleets of one pass over p (kExpMaxNB)


def used_mb():
    free, total = torch.cuda.mem_get_info()
    return round((total - free) / 2 ** 20, 1)


def timed(fn, s):
    s.sync()
    t0 = time.perf_counter()
    fn()
    s.sync()
    return round(1e3 * (time.perf_counter() - t0), 3)


out = {"device": cpm.device_info(0)["name"], "Z": Z, "T": T, "calls_per_block": args.calls, "blocks": args.blocks, "shapes": {}}
d_out = torch.empty(max(FLEETS) * 2 * T * Z, dtype=torch.float64, device="cuda")
d_ref = torch.empty(2 * T * Z, dtype=torch.float64, device="cuda")
rng = np.random.default_rng(1)
tables = {B: np.asfortranarray(rng.uniform(0.05, 0.95, (Z, T, B))) for B in FLEETS}
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
        if upload:
            s.set_sparse_upload(True)
            install = [lambda: s.set_p_dest(p_host)] * 2
        else:
            install = [lambda: s.build_p_dest(2, want=False), lambda: s.build_p_dest(1.9, want=False)]
        torch.cuda.synchronize()
        install[0]()
        s.sync()
        res = {"sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "cells_nonzero": cells, "density": round(cells / (Z * Z * T), 5),
               "memory_mb": {"tables_installed": used_mb(), "p_dense_before": s.get_info(cpm.CPM_INFO_P_DENSE)}}
        assert res["sparse_pack_words"] > 0, "the tables have no compact rows"
        # cold: the first pair on a context that never made an expected call, then alternating tables
        cold = {"sparse": [], "dense": []}
        cold["sparse"].append(timed(lambda: s.expected_dev(d_out.data_ptr(), sparse=True), s))
        res["memory_mb"]["after_first_sparse_call"] = used_mb()
        res["memory_mb"]["p_dense_after_sparse"] = s.get_info(cpm.CPM_INFO_P_DENSE)
        cold["dense"].append(timed(lambda: s.expected_dev(d_ref.data_ptr()), s))
        res["memory_mb"]["after_first_dense_call"] = used_mb()
        res["bits_equal"] = bool(torch.equal(d_out[:2 * T * Z].view(torch.int64), d_ref.view(torch.int64)))
        res["cold_first_call_only_ms"] = {k: v[0] for k, v in cold.items()}
        cold = {"sparse": [], "dense": []}
        for i in range(2 * args.cold):
            arm = "sparse" if i % 2 == 0 else "dense"
            inst = install[(i // 2 + 1) % 2]
            cold[arm].append(timed(lambda: (inst(), s.expected_dev(d_out.data_ptr(), sparse=(arm == "sparse"))), s))
        res["cold_install_plus_first_call_ms"] = {k: {"median": statistics.median(v), "all": v} for k, v in cold.items()}
        res["install_only_ms"] = statistics.median([timed(install[i % 2], s) for i in range(args.cold)])
        install[0]()
        for sp in (True, False):
            s.expected_dev(d_out.data_ptr(), sparse=sp)             # (per-table arrays of both forms: built, not timed)
        s.sync()
        arms = {}
        for sp, pre in ((False, ""), (True, "S")):
            arms[pre + "E"] = (lambda sp=sp: s.expected_dev(d_out.data_ptr(), sparse=sp), T, 1, sp)
            arms[pre + "EI"] = (lambda sp=sp: s.expected_dev(d_out.data_ptr(), ivp=True, sparse=sp), 2 * T - 1, 1, sp)
            for B in FLEETS:
                arms[f"{pre}B{B}"] = (lambda sp=sp: s.expected_batch_dev(d_out.data_ptr(), sparse=sp), T, -(-B // PASS), sp)
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, (fn, _, _, _) in arms.items():
                if "B" in k:
                    s.set_p_drive_batch(tables[int(k.split("B")[1])])
                s.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                s.sync()
                if block:
                    ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        sparse_bytes = cells // T * 12 + (Z + 1) * 4                # per operator and pass, mean over the hours
        res["bytes_per_operator"] = {"dense": Z * Z * 8, "sparse": sparse_bytes}
        res["arms"] = {}
        for k, (_, ops, passes, sp) in arms.items():
            m = statistics.median(ms[k])
            nbytes = passes * (sparse_bytes if sp else Z * Z * 8)
            res["arms"][k] = {"ms": round(m, 4), "min_ms": round(min(ms[k]), 4), "max_ms": round(max(ms[k]), 4),
                              "us_per_operator": round(m * 1e3 / ops, 2), "TBps": round(ops * nbytes / (m * 1e-3) / 1e12, 3)}
        res["sparse_over_dense"] = {k: round(res["arms"]["S" + k]["ms"] / res["arms"][k]["ms"], 3) for k in arms if not k.startswith("S")}
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
        print(f"# {name}: cold {res['cold_install_plus_first_call_ms']}, memory {res['memory_mb']}, bits_equal {res['bits_equal']}", file=sys.stderr, flush=True)
print(json.dumps(out))
