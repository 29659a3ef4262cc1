#!/usr/bin/env python
"""cliora_constrained_parse beside cliora_cky_spans and cliora_span_posteriors on the same chart; prints one JSON line.

Shapes: (B 64, L 20), (B 64, L 40) and (B 8, L 128), D 400, one eval forward of a text-only DioraMLP each; then each C entry alone
on the current stream between two events, into buffers allocated beforehand: the median of --reps after a warm-up call (which also
raises the LDS limit of an instance that needs more than 64 KB).  Three runs of the new entry: (a) no brackets, without and with the
marginals, (b) L / 4 nested required brackets per sentence, (c) the same with the marginals.  With no brackets and the marginals on,
the call does the work of cliora_cky_spans and cliora_span_posteriors together, so its ratio to their sum is reported; there is no
pass / fail number (DESIGN.md section 19 explains a ratio above 1).

    python tools/constrained_bench.py [--out profiles/constrained_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.constrained import pack_brackets    # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402

SHAPES = ((64, 20), (64, 40), (8, 128))
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


def nested(L, b):
    """L / 4 nested required brackets, shifted by the sentence's row."""
    rows, lo, hi = [], b % 2, L - 1 - ((b + 1) % 2)
    while hi - lo >= 1 and len(rows) < max(1, L // 4):
        rows.append((lo, hi))
        lo, hi = lo + 1, hi - (1 if len(rows) % 2 else 0)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'constrained_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(1)
    m = DioraMLP(D).cuda().eval()
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L)).cuda()
        with torch.no_grad():
            m(x, x)
        plan, ws = m._plan, _lib.ptr(m._wss[0])
        spans = torch.empty((B, L - 1, 2), dtype=torch.int32, device='cuda')
        cky = event_ms(lambda: m.cky_spans_device(out=spans), a.reps)
        marg = torch.empty((B, plan.C), dtype=torch.float32, device='cuda')
        log_z = torch.empty(B, dtype=torch.float32, device='cuda')
        post = event_ms(lambda: _lib.call('cliora_span_posteriors', plan.handle, ws, None, _lib.ptr(marg), _lib.ptr(log_z), None, None, None,
                                          None, _lib.stream()), a.reps)
        row = dict(B=B, L=L, D=D, cky_spans_ms=round(cky[0], 4), cky_spans_ms_min=round(cky[1], 4), cky_spans_ms_max=round(cky[2], 4),
                   span_posteriors_ms=round(post[0], 4), span_posteriors_ms_min=round(post[1], 4), span_posteriors_ms_max=round(post[2], 4))
        brackets = pack_brackets([nested(L, b) for b in range(B)]).cuda()
        out = torch.empty((B, L - 1, 2), dtype=torch.int32, device='cuda')
        sc, lz, lzc, lp = (torch.empty(B, dtype=torch.float32, device='cuda') for _ in range(4))
        feas = torch.empty(B, dtype=torch.int32, device='cuda')
        mu = torch.empty((B, plan.C), dtype=torch.float32, device='cuda')
        status = torch.zeros(1, dtype=torch.int32, device='cuda')

        def run(br, with_mu):
            _lib.call('cliora_constrained_parse', plan.handle, ws, None, _lib.ptr(br) if br is not None else None,
                      int(br.shape[1]) if br is not None else 0, _lib.ptr(out), _lib.ptr(sc), _lib.ptr(lz), _lib.ptr(lzc), _lib.ptr(lp),
                      _lib.ptr(feas), _lib.ptr(mu) if with_mu else None, _lib.ptr(status), _lib.stream())

        for name, br, with_mu in (('none', None, False), ('none_marginals', None, True), ('nested', brackets, False),
                                  ('nested_marginals', brackets, True)):
            t = event_ms(lambda: run(br, with_mu), a.reps)
            row[name + '_ms'], row[name + '_ms_min'], row[name + '_ms_max'] = round(t[0], 4), round(t[1], 4), round(t[2], 4)
            assert int(status) == 0 and bool((feas == 1).all())
            assert torch.equal(lz.view(torch.int32), log_z.view(torch.int32))          # the same unconstrained inside table
            if br is None:
                assert torch.equal(out, spans) and bool((lp == 0).all())
                if with_mu:
                    assert torch.equal(mu.view(torch.int32), marg.view(torch.int32))
            else:
                assert bool((lp < 0).all())
        row['brackets_per_sentence'] = int(brackets.shape[1])
        row['none_marginals_ratio_to_cky_plus_posteriors'] = round(row['none_marginals_ms'] / (cky[0] + post[0]), 2)
        row['none_ratio_to_cky_spans'] = round(row['none_ms'] / cky[0], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='constrained', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
