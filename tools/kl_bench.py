#!/usr/bin/env python
"""cliora_tree_kl beside cliora_tree_expectation and cliora_span_posteriors on the same charts; prints one JSON line.

Shapes: B 64 at L 20, 40 and 64, D 400, one eval forward each of two text-only DioraMLPs of different random weights (teacher and
student) on the same batch; then each C entry alone on the current stream between two events, into buffers allocated beforehand: the
median of --reps after a warm-up call (which also raises the LDS limit of an instance that needs more than 64 KB).  The new entry with
and without d_split_p (weights 0.7 / -0.4).  The siblings to read the figures against, on the teacher's chart in the same session:
cliora_tree_expectation with both weights (four fp64 tables, one chart) and cliora_span_posteriors without the MBR tree (two tables).
There is no pass / fail number.  --bench-gate FILE: a JSON object (the bench.py step times of the parent commit
and of this one, taken in one session) stored under "bench_gate" as it is.

    python tools/kl_bench.py [--out profiles/kl_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd.diora import DioraMLP           # noqa: E402
from cliora_amd.structured import split_score_count    # noqa: E402
from bracket_grad_bench import stat             # noqa: E402
from constrained_bench import event_ms          # noqa: E402

SHAPES = ((64, 20), (64, 40), (64, 64))
D = 400


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'kl_bench.json'))
    ap.add_argument('--bench-gate', default=None)
    a = ap.parse_args()
    torch.manual_seed(1)
    teacher = DioraMLP(D).cuda().eval()
    torch.manual_seed(2)
    student = DioraMLP(D).cuda().eval()
    rows = []
    for B, L in SHAPES:
        x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(L)).cuda()
        with torch.no_grad():
            teacher(x, x)
            student(x, x)
        pp, pq = teacher._plan, student._plan
        wp, wq = _lib.ptr(teacher._wss[0]), _lib.ptr(student._wss[0])
        cost = torch.rand(B, pp.C, generator=torch.Generator().manual_seed(100 + L)).cuda()
        ones = torch.ones(B, device='cuda')
        wk, wc = torch.full((B,), 0.7, device='cuda'), torch.full((B,), -0.4, device='cuda')
        kl, ce, ent, lzp, lzq, risk, ent2, lz2, lz3 = (torch.empty(B, dtype=torch.float32, device='cuda') for _ in range(9))
        mu = torch.empty((B, pp.C), dtype=torch.float32, device='cuda')
        status = torch.zeros(1, dtype=torch.int32, device='cuda')
        d_p, d_q = (torch.empty(split_score_count(pp), dtype=torch.float32, device='cuda') for _ in range(2))

        def tree_kl(with_p):
            _lib.call('cliora_tree_kl', pp.handle, wp, pq.handle, wq, None, _lib.ptr(wk), _lib.ptr(wc), _lib.ptr(d_p) if with_p else None,
                      _lib.ptr(d_q), _lib.ptr(kl), _lib.ptr(ce), _lib.ptr(ent), _lib.ptr(lzp), _lib.ptr(lzq), _lib.ptr(status), _lib.stream())

        def expect():
            _lib.call('cliora_tree_expectation', pp.handle, wp, None, _lib.ptr(cost), _lib.ptr(ones), _lib.ptr(ones), _lib.ptr(d_p),
                      _lib.ptr(risk), _lib.ptr(ent2), _lib.ptr(lz2), _lib.ptr(status), _lib.stream())

        def post():
            _lib.call('cliora_span_posteriors', pp.handle, wp, None, _lib.ptr(mu), _lib.ptr(lz3), None, None, None, _lib.ptr(status),
                      _lib.stream())

        row = dict(B=B, L=L, D=D)
        stat(row, 'span_posteriors', event_ms(post, a.reps))
        stat(row, 'tree_expectation_both', event_ms(expect, a.reps))
        for name, with_p in (('student_grad', False), ('both_grads', True)):
            stat(row, 'tree_kl_' + name, event_ms(lambda: tree_kl(with_p), a.reps))
            assert int(status) == 0 and bool(torch.isfinite(d_q).all()) and bool((d_q != 0).any())
            assert torch.equal(lzp.view(torch.int32), lz3.view(torch.int32))           # the inside table of the posteriors
            assert torch.equal(ent.view(torch.int32), ent2.view(torch.int32))          # the entropy of cliora_tree_expectation
            for sib in ('tree_expectation_both', 'span_posteriors'):
                row['tree_kl_%s_ratio_to_%s' % (name, sib)] = round(row['tree_kl_%s_ms' % name] / row[sib + '_ms'], 2)
        row['mean_kl'], row['mean_cross_entropy'], row['mean_entropy_p'] = (round(float(v.mean()), 4) for v in (kl, ce, ent))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='tree_kl', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
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
