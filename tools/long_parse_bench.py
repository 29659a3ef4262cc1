#!/usr/bin/env python
"""Parsing long sentences: eval forward (both passes) + cky_spans of a text-only DioraMLP of width 400 on one GPU, beside the CPU
oracle on the same batches; prints one JSON line.

Shapes: (B 8, L 96) and (B 8, L 128), the lengths only a forward-only plan reaches, and (B 64, L 65) next to (B 64, L 64) to show
that nothing falls off a cliff at the old bound.  A library that refuses a shape (a build from before the forward-only plans at
L > 64) is recorded as refused.  Device figures: median wall-clock of --reps calls after a warm-up call that creates the plan, host
work and the copy of the spans included.  The oracle (oracle/diora_ref.py in fp32 on --threads host threads, inside + outside pass +
its CKY) is the only other thing that runs these lengths; it is timed once per shape on --oracle-batch sentences and scaled to B.

    python tools/long_parse_bench.py [--out profiles/long_parse_bench.json] [--no-oracle]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402
from oracle import diora_ref as R               # noqa: E402

SHAPES = ((64, 64), (64, 65), (8, 96), (8, 128))
D = 400


def device_ms(m, x, reps):
    def once():
        m(x, x)
        return m.cky_spans()
    with torch.no_grad():
        once()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            once()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def oracle_s(P, x):
    t0 = time.perf_counter()
    with torch.no_grad():
        o = R.diora_forward(P, x, outside=True, keep_pairs=True)
        R.cky_trees(o['pair_s_in'], x.shape[0], x.shape[1])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--oracle-batch', type=int, default=1)
    ap.add_argument('--no-oracle', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.set_num_threads(a.threads)
    P = R.init_params(D, share=True, seed=1)
    m = DioraMLP(D).cuda().eval()
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].clone()
    m.load_state_dict(sd)
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L))
        row = dict(B=B, L=L, D=D)
        try:
            med, lo, hi = device_ms(m, x.cuda(), a.reps)
            row.update(device_ms=round(med, 3), device_ms_min=round(lo, 3), device_ms_max=round(hi, 3),
                       sentences_per_s=round(B / med * 1e3, 1))
        except _lib.ChartLibError as e:
            row.update(refused=str(e))
        if not a.no_oracle:
            n = min(B, a.oracle_batch)
            s = oracle_s(P, x[:n])
            row.update(oracle_s_per_sentence=round(s / n, 2), oracle_s_batch=round(s / n * B, 1), oracle_threads=a.threads)
            if 'device_ms' in row:
                row['speedup_vs_oracle'] = round(s / n * B * 1e3 / row['device_ms'], 0)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='long_parse', mfma_mode='bf16x3', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
