#!/usr/bin/env python
"""cliora_tree_expectation beside cliora_bracket_grad and cliora_span_posteriors on the same chart; prints one JSON line.

Shapes: B 64 at L 20, 40 and 64, D 400, one eval forward of a text-only DioraMLP each; then each C entry alone on the current stream
between two events, into buffers allocated beforehand: the median of --reps after a warm-up call (which also raises the LDS limit of
an instance that needs more than 64 KB).  Three settings of the new entry: random costs (w_cost 1, w_entropy 0), the entropy alone
(no costs, w_cost 0, w_entropy 1), and both.  The siblings to read the figures against, in the same session: cliora_bracket_grad with
L / 4 nested required brackets per sentence (four log-space tables, two inside and two outside passes) and cliora_span_posteriors
without the MBR tree (two tables).  There is no pass / fail number.  --bench-gate FILE: a JSON object (the
bench.py step times of the parent commit and of this one, taken in one session) stored under "bench_gate" as it is.

    python tools/expectation_bench.py [--out profiles/expectation_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.constrained import pack_brackets    # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402
from cliora_amd.structured import split_score_count    # noqa: E402
from bracket_grad_bench import stat             # noqa: E402
from constrained_bench import event_ms, nested  # noqa: E402

SHAPES = ((64, 20), (64, 40), (64, 64))
D = 400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'expectation_bench.json'))
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
        g = torch.Generator().manual_seed(100 + L)
        cost = torch.rand(B, plan.C, generator=g).cuda()
        ones, zeros = torch.ones(B, device='cuda'), torch.zeros(B, device='cuda')
        brackets = pack_brackets([nested(L, b) for b in range(B)]).cuda()
        risk, ent, lz, lz2, lp = (torch.empty(B, dtype=torch.float32, device='cuda') for _ in range(5))
        feas = torch.empty(B, dtype=torch.int32, device='cuda')
        mu = torch.empty((B, plan.C), dtype=torch.float32, device='cuda')
        status = torch.zeros(1, dtype=torch.int32, device='cuda')
        d_split = torch.empty(split_score_count(plan), dtype=torch.float32, device='cuda')

        def expect(c, wc, we):
            _lib.call('cliora_tree_expectation', plan.handle, ws, None, _lib.ptr(c) if c is not None else None, _lib.ptr(wc), _lib.ptr(we),
                      _lib.ptr(d_split), _lib.ptr(risk), _lib.ptr(ent), _lib.ptr(lz), _lib.ptr(status), _lib.stream())

        def grad():
            _lib.call('cliora_bracket_grad', plan.handle, ws, None, _lib.ptr(brackets), int(brackets.shape[1]), None, _lib.ptr(d_split),
                      _lib.ptr(lp), _lib.ptr(feas), _lib.ptr(status), _lib.stream())

        def post():
            _lib.call('cliora_span_posteriors', plan.handle, ws, None, _lib.ptr(mu), _lib.ptr(lz2), None, None, None, _lib.ptr(status),
                      _lib.stream())

        row = dict(B=B, L=L, D=D, brackets_per_sentence=int(brackets.shape[1]))
        stat(row, 'span_posteriors', event_ms(post, a.reps))
        stat(row, 'bracket_grad_nested', event_ms(grad, a.reps))
        assert bool((feas == 1).all())
        for name, args in (('cost', (cost, ones, zeros)), ('entropy', (None, zeros, ones)), ('both', (cost, ones, ones))):
            stat(row, 'tree_expectation_' + name, event_ms(lambda: expect(*args), a.reps))
            assert int(status) == 0 and bool(torch.isfinite(d_split).all()) and bool((d_split != 0).any())
            assert torch.equal(lz.view(torch.int32), lz2.view(torch.int32))             # the inside table of the posteriors
            for sib in ('bracket_grad_nested', 'span_posteriors'):
                row['tree_expectation_%s_ratio_to_%s' % (name, sib)] = round(row['tree_expectation_%s_ms' % name] / row[sib + '_ms'], 2)
        row['mean_entropy'], row['mean_log_z'] = round(float(ent.mean()), 4), round(float(lz.mean()), 4)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='tree_expectation', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
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
