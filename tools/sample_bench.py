#!/usr/bin/env python
"""cliora_sample_trees at S = 1 / 16 / 256 beside cliora_cky_spans and cliora_span_posteriors on the same chart; prints one JSON line.

Shapes: (B 64, L 20), (B 64, L 40) and (B 8, L 128), D 400, one eval forward of a text-only DioraMLP each; then each C entry alone
on the current stream between two events, into buffers allocated beforehand: the median of --reps after a warm-up call (which also
raises the LDS limit of an instance that needs more than 64 KB).  No time is a target -- the call is bound by the latency of its
level and node chains, not by throughput; the S = 1 ratio to cliora_span_posteriors says what the inside pass alone costs (the
posteriors add the outside pass), the step from S = 16 to S = 256 what a wavefront's walk costs.

    python tools/sample_bench.py [--out profiles/sample_bench.json]
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
SS = (1, 16, 256)
D = 400
SEED = 12345


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
    ap.add_argument('--out', default=os.path.join('profiles', 'sample_bench.json'))
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
        marg = torch.empty((B, plan.C), dtype=torch.float32, device='cuda')
        log_z = torch.empty(B, dtype=torch.float32, device='cuda')
        post = event_ms(lambda: _lib.call('cliora_span_posteriors', plan.handle, ws, None, _lib.ptr(marg), _lib.ptr(log_z), None, None, None,
                                          None, _lib.stream()), a.reps)
        row = dict(B=B, L=L, D=D, cky_spans_ms=round(cky[0], 4), cky_spans_ms_min=round(cky[1], 4), cky_spans_ms_max=round(cky[2], 4),
                   span_posteriors_ms=round(post[0], 4), span_posteriors_ms_min=round(post[1], 4), span_posteriors_ms_max=round(post[2], 4))
        for S in SS:
            out = torch.empty((B, S, L - 1, 2), dtype=torch.int32, device='cuda')
            log_prob = torch.empty((B, S), dtype=torch.float32, device='cuda')
            lz = torch.empty(B, dtype=torch.float32, device='cuda')
            t = event_ms(lambda: _lib.call('cliora_sample_trees', plan.handle, ws, None, None, S, SEED, 0, 1.0, _lib.ptr(out),
                                           _lib.ptr(log_prob), _lib.ptr(lz), None, _lib.stream()), a.reps)
            row['s%d_ms' % S], row['s%d_ms_min' % S], row['s%d_ms_max' % S] = round(t[0], 4), round(t[1], 4), round(t[2], 4)
            assert torch.equal(lz.view(torch.int32), log_z.view(torch.int32))        # the same inside table
            assert bool((out[:, :, -1, 1] == L - 1).all())                           # every sample ends with the root
        row['s1_ratio_to_cky_spans'] = round(row['s1_ms'] / cky[0], 2)
        row['s1_ratio_to_span_posteriors'] = round(row['s1_ms'] / post[0], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='sample', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
