#!/usr/bin/env python
"""Hard (single-tree, S-DIORA) charts beside soft ones: a text-only DioraMLP of width 400 on one GPU; prints one JSON line.

Shapes: (B 64, L 20), (B 64, L 40), (B 8, L 128).  Variants of the chart: soft (cliora_chart_forward), hard_dense (the one-hot
weights through the dense compose kernels, CLIORA_FWD_HARD_DENSE: every split composed) and hard (level_compose_hard: the selected
pair of every cell alone).  Figures: the eval forward (both passes, torch.no_grad) for every shape; forward + backward (random
cotangents on the four charts) for the first two; and the tree decodes, hard_spans_device beside cky_spans_device, on the hard chart.
Each is the median wall-clock of --reps calls between torch.cuda.synchronize fences after a warm-up call that creates the plan, host
work included.  A library without the hard entry (an older build through CLIORA_CHART_LIB: the yardstick of the same session)
is recorded as refused for the hard variants.

    python tools/hard_bench.py [--out profiles/hard_bench.json]
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

SHAPES = ((64, 20), (64, 40), (8, 128))
TRAIN_SHAPES = ((64, 20), (64, 40))
D = 400
VARIANTS = (('soft', False, False), ('hard_dense', True, True), ('hard', True, False))
CHARTS = ('inside_h', 'inside_s', 'outside_h', 'outside_s')


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(float(np.median(ts)), 3), ms_min=round(float(min(ts)), 3), ms_max=round(float(max(ts)), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.manual_seed(1)
    m = DioraMLP(D).cuda()
    rows = []
    for B, L in SHAPES:
        g = torch.Generator().manual_seed(L)
        x = torch.randn(B, L, D, generator=g).cuda()
        C = L * (L + 1) // 2
        cots = [torch.randn(B, C, w, generator=g).cuda() for w in (D, 1, D, 1)]
        row = dict(B=B, L=L, D=D)
        for name, hard, dense in VARIANTS:
            m.hard, m.hard_dense = hard, dense

            def forward():
                with torch.no_grad():
                    m(x, x)

            def step():
                for p in m.parameters():
                    p.grad = None
                xg = x.clone().requires_grad_(True)
                m(xg, xg)
                torch.autograd.backward([getattr(m, k) for k in CHARTS], cots)
            try:
                m.eval()
                row[name + '_forward'] = timed(forward, a.reps)
                if hard and not dense:
                    row['hard_spans'] = timed(lambda: m.hard_spans_device(), a.reps)
                    row['cky_spans'] = timed(lambda: m.cky_spans_device(), a.reps)
                if (B, L) in TRAIN_SHAPES:
                    m.train()
                    row[name + '_forward_backward'] = timed(step, a.reps)
            except _lib.ChartLibError as e:
                row[name + '_refused'] = str(e)
        if 'hard_forward' in row:
            for other in ('soft', 'hard_dense'):
                row['hard_forward_speedup_vs_' + other] = round(row[other + '_forward']['ms'] / row['hard_forward']['ms'], 3)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='hard', mfma_mode='bf16x3', reps=a.reps, library=_lib.lib().cliora_version().decode(), library_path=os.path.basename(_lib.LIB_PATH),
               shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
