#!/usr/bin/env python3
"""Development aid, run on the GPU box: the 24-hour resample with hour T as the plain sampler (CPM_OPT_LAST_HOUR 0) and as the count-only
kernel (1, csrc/cpm_count.h), same context, interleaved ROUNDS times; counts, status word and CPM_INFO_LAST_HOUR checked per block.
    tools/last_hour_bench.py --zones 4096 --cpz 1000 --steps 200 --rounds 4
    tools/last_hour_bench.py --melbourne --cpz 1000          (Melbourne-shaped tables, Z = 2,357 unless --zones is given)
    tools/last_hour_bench.py --batch 4                       (the same through resample_batch_dev, B fleets; ms per batch step)"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import carparkingmaps_amd as cpm

ap = argparse.ArgumentParser()
ap.add_argument("--zones", type=int, default=None)
ap.add_argument("--cpz", type=int, default=1000)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--melbourne", action="store_true")
ap.add_argument("--batch", type=int, default=0, help="B > 1: time resample_batch_dev with B p_drive tables instead of resample_dev")
args = ap.parse_args()
Z = args.zones if args.zones else (2357 if args.melbourne else 4096)
T, cpz, B = 24, args.cpz, args.batch
C = Z * cpz
SEED, TSEED = 0x5EEDCA125, 0x5EED7AB1E
st = torch.cuda.Stream()
s = cpm.Sampler(Z, T, 0, stream=st)
if args.melbourne:
    s.synth_datamatrix(TSEED)
    s.build_p_drive(0.1, 0.9, 0.5, want=False)
    s.build_p_dest(2, want=False)
else:
    s.synth_tables(TSEED)
s.init_states(C, cpz)
s.solve_ivp(SEED, want=False)
if B > 1:
    base = s.get_p_drive()
    rng = np.random.default_rng(4)
    s.set_p_drive_batch(np.asfortranarray(np.stack([np.clip(base * rng.uniform(0.5, 1.1), 0, 1) for _ in range(B)], axis=2)))
    seeds = [SEED] * B
    buf = torch.zeros(s.batch_counts_words(), dtype=torch.int64, device="cuda:0")
    step = lambda: s.resample_batch_dev(seeds, buf.data_ptr())
    steps = max(2, args.steps // B)
else:
    buf = torch.zeros(s.counts_words(), dtype=torch.int64, device="cuda:0")
    step = lambda: s.resample_dev(SEED, buf.data_ptr())
    steps = args.steps
nw = s.counts_words()
ref = None
ok = True
res = {0: [], 1: []}
for r in range(args.rounds):
    for mode in (0, 1):
        s.set_last_hour(bool(mode))
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps * 1e3
        h = buf.cpu()
        status = int(h.view(-1, nw)[:, -1].abs().sum())
        if ref is None:
            ref = h.clone()
        same = bool((h == ref).all())
        info = s.get_info(cpm.CPM_INFO_LAST_HOUR)
        ok = ok and same and status == 0 and info == mode
        res[mode].append(dt)
        print(f"round {r} last_hour {mode}: {dt:.4f} ms/{'batch step' if B > 1 else 'resample'}  info_last_hour={info} status={status} counts_equal_first={same}", flush=True)
for mode in (0, 1):
    print(f"last_hour {mode}: median {statistics.median(res[mode]):.4f} ms  min {min(res[mode]):.4f}  max {max(res[mode]):.4f}")
print(f"shape: Z={Z} cpz={cpz} melbourne={args.melbourne} batch={B} steps={steps}  checks {'ok' if ok else 'FAILED'}")
sys.exit(0 if ok else 1)
