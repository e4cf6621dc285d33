#!/usr/bin/env python3
"""What the charge costs (include/cpm_charge.h, csrc/cpm_charge.h; development tool, bench.py is the contract bench).

Shapes: the headline (Z = 4,096 x 1,000 cars per zone, cpm_synth_tables, the distance matrix of random centroids) and Melbourne's
(Z = 2,357, cpm_synth_datamatrix at density 0.0868: sparse packs, its own distance matrix) x 1,000 and x 100.  Arms, ONE process, one
context each, the same seeds:
  A   resample_dev: the step without charge (what bench.py times as ms_per_step)
  B   resample_charge_dev: the same step with k_charge_init in front, k_grouped_charge behind every hour's launches and k_charge_close at
      the end
  T   where the shape has a datamatrix: resample_dev with CPM_FLAG_TRAVEL, the other side kernel that draws once per driver
      (k_grouped_travel), for scale
in interleaved blocks of pipelined steps between two synchronisations (block 0 a warm-up, the median of the others), and
  C   once, not interleaved, where the shape has a datamatrix: the route a user had before -- resample_paths_dev +
      paths_expand_dev(travel=True) (32 bytes per car-hour of f64 matrices) + a torch loop over the hours that implements the
      recurrence on the device -- whose four arrays must equal arm B's.
Reported per shape: ms per resample of every arm, B - A in all and in microseconds per hour, the bytes of the per-car side array, and
B / C.  Prints one JSON line (plus progress lines)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carparkingmaps_amd as cpm

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="headline,melbourne_x1000,melbourne_x100")
ap.add_argument("--steps", type=int, default=100, help="resamples per timed block")
ap.add_argument("--blocks", type=int, default=5, help="interleaved blocks per arm (plus one warm-up block)")
ap.add_argument("--no-compat", action="store_true", help="skip arm C")
args = ap.parse_args()
T, SEED, TSEED = 24, 0x5EEDCA125, 0x5EED7AB1E
SHAPES = {"headline": (4096, 1000, False), "melbourne_x1000": (2357, 1000, True), "melbourne_x100": (2357, 100, True)}
CAP, WHKM, INITIAL = 20000, 25.0, 6000
POWERS = (0, 2300, 3700, 11000)


def make(Z, cpz, dataset):
    s = cpm.Sampler(Z, T)
    if dataset:
        s.synth_datamatrix(TSEED)
        s.build_p_drive(0.1, 0.9, 0.5, want=False)
        s.build_p_dest(2, want=False)
    else:
        s.synth_tables(TSEED)
        rng = np.random.default_rng(7)
        s.set_distance_from_centroids(-37.8 + 0.5 * rng.random(Z), 144.9 + 0.7 * rng.random(Z))
    s.init_states(Z * cpz, cpz)
    s.solve_ivp(SEED, want=False)
    return s


def torch_charge(state, trans, Z, zone_power):
    """the recurrence of include/cpm_charge.h hour by hour on the device: state (T, n) int64 1-based, trans (4, T, n) f64"""
    n = state.shape[1]
    E = torch.full((n,), INITIAL, dtype=torch.int64, device="cuda")
    charge = torch.zeros(Z * T, dtype=torch.int64, device="cuda")
    used = torch.zeros(Z * T, dtype=torch.int64, device="cuda")
    short = torch.zeros(Z * T, dtype=torch.int64, device="cuda")
    P = zone_power.to(torch.int64)
    for t in range(T):
        z = state[t] - 1
        cell = z * T + t
        drove = trans[0, t] == 1
        u = torch.round(trans[3, t] * WHKM)              # (half to even)
        u = torch.where(u >= 0, u, torch.zeros_like(u))
        sh = drove & (u > E.to(torch.float64))
        drawn = torch.where(drove, torch.where(sh, E, torch.where(sh, torch.zeros_like(u), u).to(torch.int64)), torch.zeros_like(E))
        give = torch.where(drove, torch.zeros_like(E), torch.minimum(P[z], CAP - E))
        short.index_add_(0, cell, sh.to(torch.int64))
        used.index_add_(0, cell, drawn)
        charge.index_add_(0, cell, give)
        E = E - drawn + give
    return charge, used, short.to(torch.int32), E.to(torch.int32)


out = {"device": cpm.device_info(0)["name"], "T": T, "steps_per_block": args.steps, "blocks": args.blocks, "shapes": {},
       "params": {"capacity_wh": CAP, "wh_per_km": WHKM, "initial_wh": INITIAL, "zone_power_wh": "[0, 2300, 3700, 11000][z % 4]"}}
for name in args.shapes.split(","):
    Z, cpz, dataset = SHAPES[name]
    n = Z * cpz
    ARMS = ("A", "B", "T") if dataset else ("A", "B")
    ctx = {a: make(Z, cpz, dataset) for a in ARMS}
    d_counts = [torch.zeros(ctx["A"].counts_words(), dtype=torch.int64, device="cuda") for _ in range(2)]
    d_charge = torch.zeros(Z * T, dtype=torch.int64, device="cuda")
    d_used = torch.zeros(Z * T, dtype=torch.int64, device="cuda")
    d_short = torch.zeros(Z * T, dtype=torch.int32, device="cuda")
    d_soc = torch.zeros(n, dtype=torch.int32, device="cuda")
    zp_host = np.array([POWERS[z % 4] for z in range(Z)], dtype=np.uint32)
    d_zp = torch.from_numpy(zp_host.view(np.int32)).cuda()
    params = cpm.ChargeParams(capacity_wh=CAP, initial_wh=INITIAL, wh_per_km=WHKM, zone_power_wh=zp_host)
    res = {"Z": Z, "cars_per_zone": cpz, "sparse_pack_words": ctx["A"].get_info(cpm.CPM_INFO_SPARSE_TABLES), "side_array_bytes": 8 * n,
           "output_bytes": 20 * Z * T + 4 * n}
    blocking = {}
    for a, s in ctx.items():
        blocking[a] = s.resample(SEED, travel=(a == "T"), charge=params if a == "B" else None)
        res[a] = {"step": s.last_step()}
    b = blocking["B"]
    res["counts_equal_in_both_arms"] = bool(np.array_equal(b["parking"], blocking["A"]["parking"]) and np.array_equal(b["driving"], blocking["A"]["driving"]))
    res["energy_identity_holds"] = bool(n * INITIAL + int(b["charge"].sum()) - int(b["used"].sum()) == int(b["soc"].astype(np.int64).sum()))
    res["drivers_per_resample"] = int(b["driving"].sum())
    res["short_trips"] = int(b["short"].sum())
    res["wh_charged"], res["wh_used"] = int(b["charge"].sum()), int(b["used"].sum())
    per = {a: [] for a in ARMS}
    for blk in range(args.blocks + 1):                       # (block 0: warm-up, not recorded)
        for a, s in ctx.items():
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                if a != "B":
                    s.resample_dev(SEED, d_counts[i & 1].data_ptr(), travel=(a == "T"))
                else:
                    s.resample_charge_dev(SEED, d_counts[i & 1].data_ptr(), d_charge.data_ptr(), d_used.data_ptr(), d_short.data_ptr(), d_soc.data_ptr(),
                                          capacity_wh=CAP, initial_wh=INITIAL, wh_per_km=WHKM, d_zone_power_ptr=d_zp.data_ptr())
            s.sync()
            dt = time.perf_counter() - t0
            if int(d_counts[(args.steps - 1) & 1][-1]) != 0:
                print(f"{name} {a}: status word set", flush=True)
            if blk:
                per[a].append(1e3 * dt / args.steps)
        if blk:
            print(f"{name} block {blk}: " + ", ".join(f"{a} {per[a][-1]:.4f}" for a in ARMS) + " ms per resample", flush=True)
    for a in ARMS:
        res[a]["step_after_timed_blocks"] = ctx[a].last_step()
        res[a]["ms_per_resample"] = round(float(np.median(per[a])), 4)
        res[a]["ms_per_resample_blocks"] = [round(x, 4) for x in per[a]]
    extra = res["B"]["ms_per_resample"] - res["A"]["ms_per_resample"]
    res["B"]["ms_over_A"] = round(extra, 4)
    res["B"]["us_per_hour_over_A"] = round(1e3 * extra / T, 2)
    if "T" in res:
        res["T"]["us_per_hour_over_A"] = round(1e3 * (res["T"]["ms_per_resample"] - res["A"]["ms_per_resample"]) / T, 2)
    dev = dict(charge=d_charge.cpu().numpy().reshape(Z, T), used=d_used.cpu().numpy().reshape(Z, T), short=d_short.cpu().numpy().reshape(Z, T),
               soc=d_soc.cpu().numpy().view(np.uint32))
    res["B"]["device_arrays_equal_blocking"] = bool(all(np.array_equal(dev[k], b[k]) for k in dev))
    if dataset and not args.no_compat:
        s = ctx["A"]
        d_paths = torch.zeros(T * n, dtype=torch.int32, device="cuda")
        d_state = torch.zeros((T, n), dtype=torch.int64, device="cuda")
        d_trans = torch.zeros((4, T, n), dtype=torch.float64, device="cuda")
        walls = []
        for _ in range(2):                                   # (the first pass warms torch's kernels up: the second is reported)
            s.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.resample_paths_dev(SEED, d_counts[0].data_ptr(), d_paths.data_ptr(), travel=True)
            s.paths_expand_dev(SEED, d_paths.data_ptr(), d_state.data_ptr(), d_trans.data_ptr(), travel=True)
            s.sync()
            t1 = time.perf_counter()
            got = torch_charge(d_state, d_trans, Z, d_zp)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            walls.append((1e3 * (t1 - t0), 1e3 * (t2 - t1)))
        c = dict(charge=got[0].cpu().numpy().reshape(Z, T), used=got[1].cpu().numpy().reshape(Z, T), short=got[2].cpu().numpy().reshape(Z, T),
                 soc=got[3].cpu().numpy().view(np.uint32))
        res["C"] = {"paths_and_expand_ms": round(walls[-1][0], 2), "torch_loop_ms": round(walls[-1][1], 2), "ms": round(sum(walls[-1]), 2),
                    "matrix_bytes": 40 * T * n, "arrays_equal_arm_B": {k: bool(np.array_equal(c[k], b[k])) for k in c}}
        res["B_over_C"] = round(res["B"]["ms_per_resample"] / res["C"]["ms"], 5)
        del d_paths, d_state, d_trans, got
    out["shapes"][name] = res
    print(f"{name}: {json.dumps(res)}", flush=True)
    for s in ctx.values():
        s.close()
    del d_counts, d_charge, d_used, d_short, d_soc, blocking
    torch.cuda.empty_cache()
print(json.dumps(out), flush=True)
