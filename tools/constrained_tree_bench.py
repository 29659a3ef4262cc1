#!/usr/bin/env python
"""cliora_kbest_spans_constrained and cliora_sample_trees_constrained beside cliora_kbest_spans and cliora_sample_trees on the same
chart in the same run; prints one JSON line.

Shapes: (B 64, L 20), (B 64, L 40) and (B 8, L 128), D 400, one eval forward of a text-only DioraMLP each; then each C entry alone
on the current stream between two events, into buffers allocated beforehand: the median of --reps after a warm-up call (which also
raises the LDS limit of an instance that needs more than 64 KB).  K 1 / 16 and S 16 / 256, each (a) with no brackets and (b) with
L / 4 nested required brackets per sentence (tests/constrained_cases.nested_required).  With no brackets a call does the unconstrained
entry's work plus the mask and, for the sampler, nothing else (the second inside table is computed only where a cell is disallowed),
so its ratio to the unconstrained entry is reported; there is no pass / fail number (DESIGN.md section 25 reads the ratios).

    python tools/constrained_tree_bench.py [--out profiles/constrained_tree_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.constrained import pack_brackets    # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402
from constrained_cases import nested_required   # noqa: E402

SHAPES = ((64, 20), (64, 40), (8, 128))
KS, SS = (1, 16), (16, 256)
D, SEED = 400, 0x5eed


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


def put(row, name, t):
    row[name + '_ms'], row[name + '_ms_min'], row[name + '_ms_max'] = round(t[0], 4), round(t[1], 4), round(t[2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'constrained_tree_bench.json'))
    a = ap.parse_args()
    torch.manual_seed(1)
    m = DioraMLP(D).cuda().eval()
    p, st = _lib.ptr, _lib.stream
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L)).cuda()
        with torch.no_grad():
            m(x, x)
        plan, ws = m._plan, _lib.ptr(m._wss[0])
        brackets = pack_brackets([nested_required(L, b) for b in range(B)]).cuda()
        M = int(brackets.shape[1])
        row = dict(B=B, L=L, D=D, brackets_per_sentence=M)
        status = torch.zeros(1, dtype=torch.int32, device='cuda')
        count, feas, count_c = (torch.empty(B, dtype=torch.int32, device='cuda') for _ in range(3))
        for K in KS:
            spans, spans_c = (torch.empty((B, K, L - 1, 2), dtype=torch.int32, device='cuda') for _ in range(2))
            scores, scores_c = (torch.empty((B, K), dtype=torch.float32, device='cuda') for _ in range(2))
            need = max(_lib.fn('cliora_kbest_scratch_bytes')(plan.handle, K), _lib.fn('cliora_kbest_constrained_scratch_bytes')(plan.handle, K, M))
            scratch = torch.empty(max(need, 4), dtype=torch.uint8, device='cuda')
            base = event_ms(lambda: _lib.call('cliora_kbest_spans', plan.handle, ws, None, K, p(spans), p(scores), p(count), p(scratch),
                                              None, st()), a.reps)
            put(row, 'kbest_K%d' % K, base)

            def run(br):
                _lib.call('cliora_kbest_spans_constrained', plan.handle, ws, None, p(br) if br is not None else None,
                          M if br is not None else 0, K, p(spans_c), p(scores_c), p(count_c), p(feas), p(scratch), p(status), st())

            for name, br in (('none', None), ('nested', brackets)):
                t = event_ms(lambda: run(br), a.reps)
                put(row, 'kbest_constrained_K%d_%s' % (K, name), t)
                assert int(status) == 0 and bool((feas == 1).all())
                if br is None:                       # the unconstrained entry's bits
                    assert torch.equal(spans_c, spans) and torch.equal(scores_c.view(torch.int32), scores.view(torch.int32))
                row['kbest_K%d_%s_ratio' % (K, name)] = round(t[0] / base[0], 2)
        log_z, log_z2, log_zc = (torch.empty(B, dtype=torch.float32, device='cuda') for _ in range(3))
        for S in SS:
            spans, spans_c = (torch.empty((B, S, L - 1, 2), dtype=torch.int32, device='cuda') for _ in range(2))
            lp, lp_c = (torch.empty((B, S), dtype=torch.float32, device='cuda') for _ in range(2))
            base = event_ms(lambda: _lib.call('cliora_sample_trees', plan.handle, ws, None, None, S, SEED, 0, 1.0, p(spans), p(lp), p(log_z),
                                              None, st()), a.reps)
            put(row, 'sample_S%d' % S, base)

            def run(br):
                _lib.call('cliora_sample_trees_constrained', plan.handle, ws, None, None, p(br) if br is not None else None,
                          M if br is not None else 0, S, SEED, 0, 1.0, p(spans_c), p(lp_c), p(log_zc), p(log_z2), p(feas), p(status), st())

            for name, br in (('none', None), ('nested', brackets)):
                t = event_ms(lambda: run(br), a.reps)
                put(row, 'sample_constrained_S%d_%s' % (S, name), t)
                assert int(status) == 0 and bool((feas == 1).all())
                assert torch.equal(log_z2.view(torch.int32), log_z.view(torch.int32))      # the same unconstrained inside table
                if br is None:
                    assert torch.equal(spans_c, spans) and torch.equal(lp_c.view(torch.int32), lp.view(torch.int32))
                else:
                    assert bool((log_zc < log_z2).all())
                row['sample_S%d_%s_ratio' % (S, name)] = round(t[0] / base[0], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='constrained_tree', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
