#!/usr/bin/env python
"""cliora_kbest_spans at K = 1 / 4 / 8 / 16 beside cliora_cky_spans on the same chart; prints one JSON line.

Shapes: (B 64, L 20), (B 64, L 40) and (B 8, L 128), D 400, one eval forward of a text-only DioraMLP each; then each C entry alone
on the current stream between two events, into buffers allocated beforehand: the median of --reps after a warm-up call (which also
raises the LDS limit of an instance that needs more than 64 KB).  No ratio is a target -- nothing comparable exists; the K = 1 ratio
says what the list machinery costs over the one-best decode it generalises.

    python tools/kbest_bench.py [--out profiles/kbest_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402

SHAPES = ((64, 20), (64, 40), (8, 128))
KS = (1, 4, 8, 16)
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
    ap.add_argument('--out', default=os.path.join('profiles', 'kbest_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(1)
    m = DioraMLP(D).cuda().eval()
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L)).cuda()
        with torch.no_grad():
            m(x, x)
        plan, ws = m._plan, C.c_void_p(m._wss[0].data_ptr())
        spans = torch.empty((B, L - 1, 2), dtype=torch.int32, device='cuda')
        cky = event_ms(lambda: m.cky_spans_device(out=spans), a.reps)
        row = dict(B=B, L=L, D=D, cky_spans_ms=round(cky[0], 4), cky_spans_ms_min=round(cky[1], 4), cky_spans_ms_max=round(cky[2], 4))
        for K in KS:
            out = torch.empty((B, K, L - 1, 2), dtype=torch.int32, device='cuda')
            scores = torch.empty((B, K), dtype=torch.float32, device='cuda')
            count = torch.empty(B, dtype=torch.int32, device='cuda')
            need = _lib.fn('cliora_kbest_scratch_bytes')(plan.handle, K)
            scratch = torch.empty(need, dtype=torch.uint8, device='cuda') if need else None
            t = event_ms(lambda: _lib.call('cliora_kbest_spans', plan.handle, ws, None, K, _lib.ptr(out), _lib.ptr(scores), _lib.ptr(count),
                                           _lib.ptr(scratch), None, _lib.stream()), a.reps)
            row['k%d_ms' % K], row['k%d_ms_min' % K], row['k%d_ms_max' % K] = round(t[0], 4), round(t[1], 4), round(t[2], 4)
            row['k%d_scratch_bytes' % K] = int(need)
            if K == 1:
                assert torch.equal(out[:, 0], spans)            # the same tree
        row['k1_ratio_to_cky_spans'] = round(row['k1_ms'] / cky[0], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='kbest', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
