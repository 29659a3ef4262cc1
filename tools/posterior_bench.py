#!/usr/bin/env python
"""cliora_span_posteriors with the MBR pass on, beside cliora_cky_spans on the same chart; prints one JSON line.

Shapes: (B 64, L 20, D 400) and (B 8, L 128, D 400), one eval forward of a text-only DioraMLP each; then each call alone on the
current stream between two events: the median of --reps after a warm-up call (which also raises the LDS limit of the long
instance).  No ratio is a target: the figure says what the sum-product pass costs next to the max-product decode it sits beside.

    python tools/posterior_bench.py [--out profiles/posterior_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402
from cliora_amd.posterior import span_posteriors   # noqa: E402

SHAPES = ((64, 20), (8, 128))
D = 400


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'posterior_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(1)
    m = DioraMLP(D).cuda().eval()
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L)).cuda()
        with torch.no_grad():
            m(x, x)
        spans = torch.empty((B, L - 1, 2), dtype=torch.int32, device='cuda')
        cky = event_ms(lambda: m.cky_spans_device(out=spans), a.reps)
        post = event_ms(lambda: span_posteriors(m, mbr=True, out=spans), a.reps)
        marg = event_ms(lambda: span_posteriors(m), a.reps)
        row = dict(B=B, L=L, D=D, cky_spans_ms=round(cky[0], 4), cky_spans_ms_min=round(cky[1], 4), cky_spans_ms_max=round(cky[2], 4),
                   posteriors_mbr_ms=round(post[0], 4), posteriors_mbr_ms_min=round(post[1], 4), posteriors_mbr_ms_max=round(post[2], 4),
                   posteriors_only_ms=round(marg[0], 4), ratio_to_cky_spans=round(post[0] / cky[0], 2))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='posterior', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
