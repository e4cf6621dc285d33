#!/usr/bin/env python3
"""The e_dest direction from a compact tangent (include/cpm_expected_sparse_dest.h, csrc/cpm_expected_sparse_dest.h) against the dense
calls (development tool; bench.py is the contract bench).

Melbourne's shape (Z = 2,357, T = 24, cpm_synth_datamatrix at density 0.0868) on the two routes that give compact rows:
  melbourne_dataset  build_p_dest on the datamatrix; the tangents from the two builders
  melbourne_upload   that p_destin and its tangent read back and uploaded (CPM_OPT_SPARSE_UPLOAD; the two setters)
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others), each dense arm beside its sparse twin (S...); the yardstick is always the dense arm of the same run:
  B / SB          the builder of d p_destin / d e_dest (dataset route only)
  GD / SGD        expected_grad_dest_dev with G_next: T operators        GDI / SGDI   with the IVP: 2T - 1 operators
  GDB<n> / SGDB<n>  expected_grad_dest_batch_dev with the IVP over n = 1, 2, 4, 8, 16 fleets
  TT / STT        expected_trip_tangent_dev
  FD<n> / SFD<n>  expected_fit_dev with CPM_FIT_DEST and the IVP at n = 1, 8 points, all three objectives weighed
  EVD / SEVD      Evaluator.expected_fit(dest=True) at 8 points, end to end
Device memory (hipMemGetInfo through torch) on a fresh context: tables installed, after the compact tangent and a sparse four-parameter
fit, after the dense tangent and a dense one; the two info words beside each.  The bits of the two forms are compared once per shape.
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
from carparkingmaps_amd import _lib
from carparkingmaps_amd import model_selection as M

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="melbourne_dataset,melbourne_upload")
ap.add_argument("--zones", type=int, default=2357)
ap.add_argument("--calls", type=int, default=5, help="calls per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
args = ap.parse_args()
T, TSEED, E_DEST = 24, 0x5EED7AB1E, 2
Z = args.zones
FLEETS = (1, 2, 4, 8, 16)
FITS = (1, 8)


def used_mb():
    free, total = torch.cuda.mem_get_info()
    return round((total - free) / 2 ** 20, 1)


def timed(fn, s):
    s.sync()
    t0 = time.perf_counter()
    fn()
    s.sync()
    return round(1e3 * (time.perf_counter() - t0), 3)


def words(s):
    return {"p_dense": s.get_info(cpm.CPM_INFO_P_DENSE), "tangent_dense": s.get_info(_lib.CPM_INFO_DEST_TANGENT_DENSE),
            "tangent_compact": s.get_info(_lib.CPM_INFO_DEST_TANGENT_COMPACT)}


out = {"device": cpm.device_info(0)["name"], "Z": Z, "T": T, "calls_per_block": args.calls, "blocks": args.blocks,
       "dense_array_mb": round(8 * Z * Z * T / 2 ** 20, 1), "shapes": {}}
nmax = max(FLEETS)
rng = np.random.default_rng(1)
d_cot = torch.from_numpy(rng.normal(0.0, 1.0, nmax * 2 * T * Z)).cuda()
d_gn = torch.from_numpy(rng.normal(0.0, 1.0, nmax * Z)).cuda()
d_grad = torch.empty(nmax * T * Z, dtype=torch.float64, device="cuda")
d_dest = torch.empty(nmax * T * Z, dtype=torch.float64, device="cuda")
d_ref = torch.empty(nmax * T * Z, dtype=torch.float64, device="cuda")
d_w = torch.empty(2 * T * Z, dtype=torch.float64, device="cuda")
d_rec = torch.empty(max(FITS) * (16 + T), dtype=torch.float64, device="cuda")
d_rec2 = torch.empty(max(FITS) * (16 + T), dtype=torch.float64, device="cuda")
tables = {B: np.asfortranarray(rng.uniform(0.05, 0.95, (Z, T, B))) for B in FLEETS}
points = {n: ([0.05 + 0.01 * i for i in range(n)], [0.9 - 0.01 * i for i in range(n)], [0.5 + 0.05 * i for i in range(n)]) for n in FITS}
weights = np.array([0.7, 1.3, 2.1])
m_act = rng.uniform(0.0, 1.0, T)
m_park = np.asfortranarray(rng.uniform(0.0, 1.0, (Z, T)))
p_host = dp_host = None
if "melbourne_upload" in args.shapes:                              # the table and its tangent on the host, from a context of its own
    with cpm.Sampler(Z, T) as s0:
        s0.synth_datamatrix(TSEED)
        p_host = s0.build_p_dest(E_DEST, want=True)
        dp_host = s0.build_p_dest_tangent(want=True)
    torch.cuda.empty_cache()
for name in args.shapes.split(","):
    upload = name == "melbourne_upload"
    with cpm.Sampler(Z, T) as s:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.set_measured_activity(m_act)
        s.set_measured(m_park)
        if upload:
            s.set_sparse_upload(True)
            s.set_p_dest(p_host)
            tangent = {True: lambda: s.set_p_dest_tangent(dp_host, sparse=True), False: lambda: s.set_p_dest_tangent(dp_host)}
        else:
            s.build_p_dest(E_DEST, want=False)
            tangent = {True: lambda: s.build_p_dest_tangent(sparse=True), False: lambda: s.build_p_dest_tangent()}
        s.sync()
        res = {"sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "memory_mb": {"tables_installed": used_mb()}, "info": {"tables_installed": words(s)}}
        assert res["sparse_pack_words"] > 0, "the tables have no compact rows"
        fit = lambda n, sp, rec=d_rec: s.expected_fit_dev(*points[n], weights, rec.data_ptr(), 0, True, True, sparse=sp, compact_tangent=sp)
        gdest = lambda sp, ivp, dst=d_dest: s.expected_grad_dest_dev(d_cot.data_ptr(), d_grad.data_ptr(), dst.data_ptr(), 0, ivp, d_gn.data_ptr(), 0,
                                                                     sparse=sp)
        # memory: the compact tangent and a sparse four-parameter fit first, on a context that never made an expected call; then the dense pair
        first = {"sparse_tangent_ms": timed(tangent[True], s), "sparse_fit_ms": timed(lambda: fit(8, True), s)}
        res["memory_mb"]["after_sparse_fit"], res["info"]["after_sparse_fit"] = used_mb(), words(s)
        first["dense_tangent_ms"], first["dense_fit_ms"] = timed(tangent[False], s), timed(lambda: fit(8, False, d_rec2), s)
        res["memory_mb"]["after_dense_fit"], res["info"]["after_dense_fit"] = used_mb(), words(s)
        res["memory_mb"]["dense_minus_sparse"] = round(res["memory_mb"]["after_dense_fit"] - res["memory_mb"]["after_sparse_fit"], 1)
        res["first_calls_on_a_fresh_context_ms"] = first
        bits = bool(torch.equal(d_rec.view(torch.int64), d_rec2.view(torch.int64)))
        gdest(True, True)
        gdest(False, True, d_ref)
        s.sync()
        res["bits_equal"] = bits and bool(torch.equal(d_dest[:T * Z].view(torch.int64), d_ref[:T * Z].view(torch.int64)))
        for sp in (True, False):                                   # (trip weights of both forms: built, not timed)
            s.expected_trip_dev(d_w.data_ptr(), sparse=sp)
        s.sync()
        ev = {sp: M.Evaluator(s, 10 * Z, 1, measured_activity=m_act, measured_parking=m_park, expected_sparse=sp, expected_sparse_dest=sp) for sp in (True, False)}
        for e in ev.values():                                      # (the tables, the tangents and the measured arrays are installed already)
            e._e_dest = e._tangent = e._tangent_compact = M.e_dest_key(E_DEST)
            e._fit_measured = True
        pts = [M.Point(points[8][2][i], points[8][0][i], points[8][1][i], E_DEST) for i in range(8)]
        w_ev = {"activity_error": 0.7, "parking_error": 1.3, "A_drive": 2.1}
        arms = {}
        for sp, pre in ((False, ""), (True, "S")):
            if not upload:
                arms[pre + "B"] = tangent[sp]
            arms[pre + "GD"] = lambda sp=sp: gdest(sp, False)
            arms[pre + "GDI"] = lambda sp=sp: gdest(sp, True)
            for B in FLEETS:
                arms[f"{pre}GDB{B}"] = lambda sp=sp: s.expected_grad_dest_batch_dev(d_cot.data_ptr(), d_grad.data_ptr(), d_dest.data_ptr(), 0, True,
                                                                                    d_gn.data_ptr(), 0, sparse=sp)
            arms[pre + "TT"] = lambda sp=sp: s.expected_trip_tangent_dev(d_w.data_ptr(), sparse=sp)
            for n in FITS:
                arms[f"{pre}FD{n}"] = lambda sp=sp, n=n: fit(n, sp)
            arms[pre + "EVD"] = lambda sp=sp: ev[sp].expected_fit(pts, w_ev, dest=True)
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, fn in arms.items():
                if "GDB" in k:
                    s.set_p_drive_batch(tables[int(k.split("GDB")[1])])
                s.sync()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                s.sync()
                if block:
                    ms[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        res["arms"] = {k: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}
        res["sparse_over_dense"] = {k: round(res["arms"]["S" + k]["ms"] / res["arms"][k]["ms"], 3) for k in arms if not k.startswith("S")}
        out["shapes"][name] = res
        print(f"# {name}: " + ", ".join(f"{k} {v['ms']} ms" for k, v in res["arms"].items()), file=sys.stderr, flush=True)
        print(f"# {name}: memory {res['memory_mb']}, info {res['info']}, bits_equal {res['bits_equal']}", file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
print(json.dumps(out))
