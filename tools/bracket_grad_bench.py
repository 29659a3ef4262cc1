#!/usr/bin/env python
"""cliora_bracket_grad beside cliora_constrained_parse (with marginals) on the same chart, and the chart step with and without a
cotangent on the split scores; prints one JSON line.

Shapes: B 64 at L 20, 40 and 64, D 400, one eval forward of a text-only DioraMLP each; then each C entry alone on the current stream
between two events, into buffers allocated beforehand: the median of --reps after a warm-up call (which also raises the LDS limit of
an instance that needs more than 64 KB).  Two bracket sets: none (the kernel returns after the mask) and L / 4 nested required
brackets per sentence.  The sibling to read the figures against is the constrained call with marginals, which runs half the passes
(one inside pair, one outside, plus the best tree); there is no pass / fail number.
Then the c2 chart (B 64, L 20, D 400) forward + backward through the autograd node, with random cotangents on the four outputs, without
and with a split cotangent (cliora_chart_backward against cliora_chart_backward_split).  --bench-gate FILE: a JSON object (the
bench.py step times of the parent commit and of this one, taken in one session) stored under "bench_gate" as it is.

    python tools/bracket_grad_bench.py [--out profiles/bracket_grad_bench.json]
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
from cliora_amd.structured import split_score_count    # noqa: E402
from constrained_bench import event_ms, nested  # noqa: E402

SHAPES = ((64, 20), (64, 40), (64, 64))
D = 400


def stat(row, name, t):
    row[name + '_ms'], row[name + '_ms_min'], row[name + '_ms_max'] = round(t[0], 4), round(t[1], 4), round(t[2], 4)


def chart_step(reps, B=64, L=20):
    """Forward + backward of the chart node alone, without / with a split cotangent."""
    torch.manual_seed(2)
    m = DioraMLP(D).cuda().train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, L, D, generator=g).cuda().requires_grad_(True)
    C = L * (L + 1) // 2
    cots = [torch.randn(B, C, w, generator=g).cuda() for w in (D, 1, D, 1)]
    m(x, x)
    d_split = 1e-2 * torch.randn(split_score_count(m._plan), generator=g).cuda()

    def step(split):
        m(x, x)
        if split:
            m._wss.split_cot[0] = d_split
        torch.autograd.backward([m.inside_h, m.inside_s, m.outside_h, m.outside_s], cots)
    row = dict(B=B, L=L, D=D)
    stat(row, 'forward_backward', event_ms(lambda: step(False), reps))
    stat(row, 'forward_backward_split', event_ms(lambda: step(True), reps))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'bracket_grad_bench.json'))
    ap.add_argument('--bench-gate', default=None)
    a = ap.parse_args()
    torch.manual_seed(1)
    m = DioraMLP(D).cuda().eval()
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L)).cuda()
        with torch.no_grad():
            m(x, x)
        plan, ws = m._plan, _lib.ptr(m._wss[0])
        brackets = pack_brackets([nested(L, b) for b in range(B)]).cuda()
        out = torch.empty((B, L - 1, 2), dtype=torch.int32, device='cuda')
        sc, lz, lzc, lp, lp2 = (torch.empty(B, dtype=torch.float32, device='cuda') for _ in range(5))
        feas, feas2 = (torch.empty(B, dtype=torch.int32, device='cuda') for _ in range(2))
        mu = torch.empty((B, plan.C), dtype=torch.float32, device='cuda')
        status = torch.zeros(1, dtype=torch.int32, device='cuda')
        d_split = torch.empty(split_score_count(plan), dtype=torch.float32, device='cuda')

        def parse(br):
            _lib.call('cliora_constrained_parse', plan.handle, ws, None, _lib.ptr(br) if br is not None else None,
                      int(br.shape[1]) if br is not None else 0, _lib.ptr(out), _lib.ptr(sc), _lib.ptr(lz), _lib.ptr(lzc), _lib.ptr(lp),
                      _lib.ptr(feas), _lib.ptr(mu), _lib.ptr(status), _lib.stream())

        def grad(br):
            _lib.call('cliora_bracket_grad', plan.handle, ws, None, _lib.ptr(br) if br is not None else None,
                      int(br.shape[1]) if br is not None else 0, None, _lib.ptr(d_split), _lib.ptr(lp2), _lib.ptr(feas2), _lib.ptr(status),
                      _lib.stream())

        row = dict(B=B, L=L, D=D, brackets_per_sentence=int(brackets.shape[1]))
        for name, br in (('none', None), ('nested', brackets)):
            stat(row, 'constrained_marginals_' + name, event_ms(lambda: parse(br), a.reps))
            stat(row, 'bracket_grad_' + name, event_ms(lambda: grad(br), a.reps))
            assert int(status) == 0 and bool((feas2 == 1).all())
            assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32))            # the same two inside tables
            assert bool((d_split == 0).all()) == (br is None)
            row['bracket_grad_%s_ratio_to_constrained_marginals' % name] = round(row['bracket_grad_%s_ms' % name] /
                                                                                 row['constrained_marginals_%s_ms' % name], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='bracket_grad', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows, chart_step_c2=chart_step(a.reps))
    if a.bench_gate:
        with open(a.bench_gate) as f:
            res['bench_gate'] = json.load(f)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
