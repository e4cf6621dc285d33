#!/usr/bin/env python3
"""The adjoint, the trip weights and the fit from sparse tables (include/cpm_expected_sparse_grad.h, csrc/cpm_expected_sparse_grad.h)
against the dense calls (development tool; bench.py is the contract bench).

Melbourne's shape (Z = 2,357, T = 24, cpm_synth_datamatrix at density 0.0868) on the two routes that give compact rows:
  melbourne_dataset  build_p_dest on the datamatrix (the dense array does not exist until a dense call expands the rows)
  melbourne_upload   that p_destin read back and uploaded under CPM_OPT_SPARSE_UPLOAD (the uploaded dense array stays resident)
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others), each dense arm beside its sparse twin (S...); the yardstick is always the dense arm of the same run:
  E / SE        expected_dev with the IVP (the forward half, for the backward pass's share)      EN / SEN   without
  G / SG        expected_grad_dev with G_next: T operators           GI / SGI   with the IVP: 2T - 1 operators
  GB<n> / SGB<n>  expected_grad_batch_dev with the IVP over n = 1, 2, 4, 8, 16 fleets
  F<n> / SF<n>  expected_fit_dev with the IVP at n = 1, 8 points      EV / SEV   Evaluator.expected_fit at 8 points, end to end
  T / ST        the trip-weight build behind set_distance (which makes both caches stale, and is a blocking copy of Z * Z * 8 bytes)
  D             that set_distance alone: the build itself is T - D and ST - D ("trip_build_alone")
The backward pass of a gradient call = the call minus (operators - 1) / operators of the forward call; per backward operator the bytes
of its own product (dense: Z * Z * 8; sparse: 12 per stored cell + 4 per row) plus the segments' sums it writes and reads back.
Cold cost after a table change, per route and arm: the installing call plus the first gradient call and a synchronisation.  Device
memory (hipMemGetInfo through torch): tables installed, after a sparse fit, after a dense fit.  The bits of the two forms are compared
once per shape.  Prints one JSON line (plus progress lines)."""
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
from carparkingmaps_amd import model_selection as M

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="melbourne_dataset,melbourne_upload")
ap.add_argument("--zones", type=int, default=2357)
ap.add_argument("--calls", type=int, default=10, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--cold", type=int, default=3, help="cold measurements per arm")
args = ap.parse_args()
T, TSEED = 24, 0x5EED7AB1E
Z = args.zones
FLEETS = (1, 2, 4, 8, 16)
FITS = (1, 8)
PASS = 8  # fleets of one pass over p (kExpMaxNB)


def grad_segments(z):
    strips = (z + 127) // 128
    return max(1, min((1024 + strips - 1) // strips, z // 32, 64))


def used_mb():
    free, total = torch.cuda.mem_get_info()
    return round((total - free) / 2 ** 20, 1)


def timed(fn, s):
    s.sync()
    t0 = time.perf_counter()
    fn()
    s.sync()
    return round(1e3 * (time.perf_counter() - t0), 3)


out = {"device": cpm.device_info(0)["name"], "Z": Z, "T": T, "calls_per_block": args.calls, "blocks": args.blocks, "segments": grad_segments(Z),
       "shapes": {}}
nmax = max(FLEETS)
rng = np.random.default_rng(1)
d_cot = torch.from_numpy(rng.normal(0.0, 1.0, nmax * 2 * T * Z)).cuda()
d_gn = torch.from_numpy(rng.normal(0.0, 1.0, nmax * Z)).cuda()
d_grad = torch.empty(nmax * T * Z, dtype=torch.float64, device="cuda")
d_ref = torch.empty(nmax * T * Z, dtype=torch.float64, device="cuda")
d_exp = torch.empty(2 * T * Z, dtype=torch.float64, device="cuda")
d_w = torch.empty(2 * T * Z, dtype=torch.float64, device="cuda")
d_rec = torch.empty(max(FITS) * (16 + T), dtype=torch.float64, device="cuda")
d_rec2 = torch.empty(max(FITS) * (16 + T), dtype=torch.float64, device="cuda")
tables = {B: np.asfortranarray(rng.uniform(0.05, 0.95, (Z, T, B))) for B in FLEETS}
points = {n: ([0.05 + 0.01 * i for i in range(n)], [0.9 - 0.01 * i for i in range(n)], [0.5 + 0.05 * i for i in range(n)]) for n in FITS}
weights = np.array([0.7, 1.3, 2.1])
m_act = rng.uniform(0.0, 1.0, T)
m_park = np.asfortranarray(rng.uniform(0.0, 1.0, (Z, T)))
with cpm.Sampler(Z, T) as s0:                                      # the table on the host, from a context of its own (reading it expands the rows)
    s0.synth_datamatrix(TSEED)
    p_host = s0.build_p_dest(2, want=True)
cells = int(np.count_nonzero(p_host))                              # (the dataset's compact rows also keep its cells of weight 0: a lower bound there)
torch.cuda.empty_cache()
nseg = grad_segments(Z)
for name in args.shapes.split(","):
    upload = name == "melbourne_upload"
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.set_measured_activity(m_act)
        s.set_measured(m_park)
        dist = s.get_distance()
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
        fit = lambda n, sp, rec=d_rec: s.expected_fit_dev(*points[n], weights, rec.data_ptr(), 0, True, False, sparse=sp)
        grad = lambda sp, ivp, dst=d_grad: s.expected_grad_dev(d_cot.data_ptr(), dst.data_ptr(), 0, ivp, d_gn.data_ptr(), 0, sparse=sp)
        # memory: a sparse fit first, on a context that never made an expected call; then a dense one
        first = {"sparse_fit_ms": timed(lambda: fit(8, True), s)}
        res["memory_mb"]["after_sparse_fit"] = used_mb()
        res["memory_mb"]["p_dense_after_sparse_fit"] = s.get_info(cpm.CPM_INFO_P_DENSE)
        first["dense_fit_ms"] = timed(lambda: fit(8, False, d_rec2), s)
        res["memory_mb"]["after_dense_fit"] = used_mb()
        res["memory_mb"]["p_dense_after_dense_fit"] = s.get_info(cpm.CPM_INFO_P_DENSE)
        res["first_fit_on_a_fresh_context_ms"] = first
        bits = bool(torch.equal(d_rec.view(torch.int64), d_rec2.view(torch.int64)))
        grad(True, True)
        grad(False, True, d_ref)
        s.sync()
        res["bits_equal"] = bits and bool(torch.equal(d_grad[:T * Z].view(torch.int64), d_ref[:T * Z].view(torch.int64)))
        # cold: the installing call plus the first gradient call, alternating tables and arms
        cold = {"sparse": [], "dense": []}
        for i in range(2 * args.cold):
            arm = "sparse" if i % 2 == 0 else "dense"
            inst = install[(i // 2 + 1) % 2]
            cold[arm].append(timed(lambda: (inst(), grad(arm == "sparse", True)), s))
        res["cold_install_plus_first_grad_ms"] = {k: {"median": statistics.median(v), "all": v} for k, v in cold.items()}
        res["install_only_ms"] = statistics.median([timed(install[i % 2], s) for i in range(args.cold)])
        install[0]()
        for sp in (True, False):                                   # (per-table arrays and trip weights of both forms: built, not timed)
            grad(sp, True)
            s.expected_trip_dev(d_w.data_ptr(), sparse=sp)
        s.sync()
        ev = {sp: M.Evaluator(s, 10 * Z, 1, measured_activity=m_act, measured_parking=m_park, expected_sparse=sp) for sp in (True, False)}
        for e in ev.values():
            e._e_dest, e._fit_measured = M.e_dest_key(2), True    # (the tables and the measured arrays are installed already)
        pts = [M.Point(points[8][2][i], points[8][0][i], points[8][1][i], 2) for i in range(8)]
        w_ev = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}

        def trip(sp):
            s.set_distance(dist)
            s.expected_trip_dev(d_w.data_ptr(), sparse=sp)

        arms = {}
        for sp, pre in ((False, ""), (True, "S")):
            arms[pre + "E"] = (lambda sp=sp: s.expected_dev(d_exp.data_ptr(), 0, True, sparse=sp), sp)
            arms[pre + "EN"] = (lambda sp=sp: s.expected_dev(d_exp.data_ptr(), 0, False, sparse=sp), sp)
            arms[pre + "G"] = (lambda sp=sp: grad(sp, False), sp)
            arms[pre + "GI"] = (lambda sp=sp: grad(sp, True), sp)
            for B in FLEETS:
                arms[f"{pre}GB{B}"] = (lambda sp=sp: s.expected_grad_batch_dev(d_cot.data_ptr(), d_grad.data_ptr(), 0, True, d_gn.data_ptr(), 0, sparse=sp), sp)
            for n in FITS:
                arms[f"{pre}F{n}"] = (lambda sp=sp, n=n: fit(n, sp), sp)
            arms[pre + "EV"] = (lambda sp=sp: ev[sp].expected_fit(pts, w_ev), sp)
            arms[pre + "T"] = (lambda sp=sp: trip(sp), sp)
        arms["D"] = (lambda: s.set_distance(dist), False)
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, (fn, _) in arms.items():
                if "GB" in k:
                    s.set_p_drive_batch(tables[int(k.split("GB")[1])])
                s.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                s.sync()
                if block:
                    ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        res["arms"] = {k: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
        res["sparse_over_dense"] = {k: round(res["arms"]["S" + k]["ms"] / res["arms"][k]["ms"], 3) for k in arms if not k.startswith("S") and k != "D"}
        copy = res["arms"]["D"]["ms"]
        alone = {"dense_ms": round(res["arms"]["T"]["ms"] - copy, 4), "sparse_ms": round(res["arms"]["ST"]["ms"] - copy, 4)}
        alone["sparse_over_dense"] = round(alone["sparse_ms"] / alone["dense_ms"], 3)
        res["trip_build_alone"] = alone
        part = 2 * nseg * Z * 8                                     # the segments' sums: written by the product, read by the finishing kernel
        own = {"": Z * Z * 8, "S": cells // T * 12 + Z * 4}
        res["bytes_per_backward_product"] = {"dense": own[""], "sparse": own["S"], "segments_sums_either": part}
        back = {}
        for pre in ("", "S"):
            for g, e, ops in (("G", "EN", T), ("GI", "E", 2 * T - 1)):
                total, fwd = res["arms"][pre + g]["ms"], res["arms"][pre + e]["ms"] * (ops - 1) / ops
                b = total - fwd
                back[pre + g] = {"backward_ms": round(b, 4), "share": round(b / total, 3), "us_per_backward_operator": round(b * 1e3 / ops, 2),
                                 "TBps_own_bytes": round(ops * own[pre] / (b * 1e-3) / 1e12, 3)}
        res["backward"] = back
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
        print(f"# {name}: cold {res['cold_install_plus_first_grad_ms']}, memory {res['memory_mb']}, bits_equal {res['bits_equal']}", file=sys.stderr, flush=True)
print(json.dumps(out))
