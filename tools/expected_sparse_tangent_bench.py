#!/usr/bin/env python3
"""The forward tangent from the compact rows (include/cpm_expected_sparse_tangent.h, csrc/cpm_expected_sparse_tangent.h) against the
dense call (development tool; bench.py is the contract bench).

Melbourne's shape (Z = 2,357, T = 24, cpm_synth_datamatrix at density 0.0868) on the two routes that give compact rows:
  melbourne_dataset  build_p_dest on the datamatrix; the tangents from the two builders
  melbourne_upload   that p_destin and its tangent read back and uploaded (CPM_OPT_SPARSE_UPLOAD; the two setters)
Arms, ONE process and one context per shape, in interleaved blocks of pipelined calls between two synchronisations (block 0 a warm-up,
the median of the others), each dense arm beside its sparse twin (S...); the yardstick is always the dense arm of the same run:
  T3 / ST3      expected_tangent_dev, K = 3 (the directions of p_drive), T operators      T3I / ST3I   with the IVP: 2T - 1 operators
  T4 / ST4      K = 4, the last direction along the tangent of p_destin (c_dest = 1)      T4I / ST4I   with the IVP
  JAC / SJAC    Evaluator.expected_jacobian(dest=True), end to end
Cold costs, one call each: the first K = 4 call after the tables were installed again (the per-table arrays, the transpose of the rows
and of the tangent), and after a new tangent alone (k_exps_cells_dp); the dense call's beside them.  Device memory (hipMemGetInfo
through torch) on a fresh context: tables installed, after a sparse refine_expected_lm with a Jacobian along e_dest, after a dense one;
the info words beside each.  The bits of the two forms are compared once per shape.  Prints one JSON line (plus progress lines)."""
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
ap.add_argument("--lm-steps", type=int, default=2)
args = ap.parse_args()
T, TSEED, E_DEST = 24, 0x5EED7AB1E, 2
Z = args.zones
C4 = [0.0, 0.0, 0.0, 1.0]


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
rng = np.random.default_rng(1)
zt = Z * T
d_dpd = torch.zeros(4 * zt, dtype=torch.float64, device="cuda")
d_out = torch.empty(4 * 2 * zt, dtype=torch.float64, device="cuda")
d_ref = torch.empty(4 * 2 * zt, dtype=torch.float64, device="cuda")
d_prim = torch.empty(2 * zt, dtype=torch.float64, device="cuda")
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
        if upload:
            s.set_sparse_upload(True)
            tables = lambda: s.set_p_dest(p_host)
            tangent = {True: lambda: s.set_p_dest_tangent(dp_host, sparse=True), False: lambda: s.set_p_dest_tangent(dp_host)}
        else:
            tables = lambda: s.build_p_dest(E_DEST, want=False)
            tangent = {True: lambda: s.build_p_dest_tangent(sparse=True), False: lambda: s.build_p_dest_tangent()}
        tables()
        s.build_p_drive_tangent_dev(0.1, 0.9, 0.5, d_dpd.data_ptr())      # directions 1 .. 3; direction 4 moves p_destin alone
        s.sync()
        res = {"sparse_pack_words": s.get_info(cpm.CPM_INFO_SPARSE_TABLES), "memory_mb": {"tables_installed": used_mb()}, "info": {"tables_installed": words(s)}}
        assert res["sparse_pack_words"] > 0, "the tables have no compact rows"
        ev = {sp: M.Evaluator(s, 10 * Z, 1, measured_activity=m_act, measured_parking=m_park, expected_sparse=sp, expected_sparse_dest=sp,
                              expected_sparse_tangent=sp) for sp in (True, False)}
        for e in ev.values():                                      # (the tables are installed already: the evaluators must not build them again)
            e._e_dest = M.e_dest_key(E_DEST)
        pt = M.Point(0.5, 0.1, 0.9, E_DEST)
        w_lm = {"activity_error": 1.0, "parking_error": 1.0}
        jac = {sp: (lambda q, sp=sp: ev[sp].expected_jacobian(q, ivp=True, dest=True)) for sp in (True, False)}
        if upload:                                                 # (the evaluators would call the builders: install the uploaded tangents here)
            tangent[True]()
            ev[True]._tangent_compact = ev[True]._e_dest
        first = {"sparse_lm_ms": timed(lambda: M.refine_expected_lm(ev[True], [pt], w_lm, steps=args.lm_steps, jacobian=jac[True]), s)}
        res["memory_mb"]["after_sparse_lm"], res["info"]["after_sparse_lm"] = used_mb(), words(s)
        if upload:
            tangent[False]()
            ev[False]._tangent = ev[False]._e_dest
        first["dense_lm_ms"] = timed(lambda: M.refine_expected_lm(ev[False], [pt], w_lm, steps=args.lm_steps, jacobian=jac[False]), s)
        res["memory_mb"]["after_dense_lm"], res["info"]["after_dense_lm"] = used_mb(), words(s)
        res["memory_mb"]["dense_minus_sparse"] = round(res["memory_mb"]["after_dense_lm"] - res["memory_mb"]["after_sparse_lm"], 1)
        res["first_calls_on_a_fresh_context_ms"] = first
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        tan = lambda sp, K, ivp, dst=d_out: s.expected_tangent_dev(K, dst.data_ptr(), d_dpd.data_ptr(), 0, C4[:K], 0, ivp, 0, d_prim.data_ptr(), sparse=sp)
        tan(True, 4, True)
        tan(False, 4, True, d_ref)
        s.sync()
        res["bits_equal"] = bool(torch.equal(d_out.view(torch.int64), d_ref.view(torch.int64)))
        # cold costs: the tables installed again (and their tangent with them), then a new tangent alone
        cold = {}
        for sp, pre in ((True, "sparse"), (False, "dense")):
            tables()
            tangent[sp]()
            cold[pre + "_after_new_tables_ms"] = timed(lambda: tan(sp, 4, True), s)
            tangent[sp]()
            cold[pre + "_after_new_tangent_ms"] = timed(lambda: tan(sp, 4, True), s)
            cold[pre + "_warm_ms"] = timed(lambda: tan(sp, 4, True), s)
        tangent[True]()
        for e in ev.values():
            e._tangent = e._tangent_compact = e._e_dest
        res["cold_ms"] = cold
        arms = {}
        for sp, pre in ((False, ""), (True, "S")):
            for K in (3, 4):
                arms[f"{pre}T{K}"] = lambda sp=sp, K=K: tan(sp, K, False)
                arms[f"{pre}T{K}I"] = lambda sp=sp, K=K: tan(sp, K, True)
            arms[pre + "JAC"] = lambda sp=sp: jac[sp](pt)
        ms = {k: [] for k in arms}
        for block in range(args.blocks + 1):
            for k, fn in arms.items():
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
        print(f"# {name}: cold {cold}", file=sys.stderr, flush=True)
        print(f"# {name}: memory {res['memory_mb']}, info {res['info']}, bits_equal {res['bits_equal']}", file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
print(json.dumps(out))
