#!/usr/bin/env python
"""cliora_bracket_margin beside cliora_bracket_grad and cliora_constrained_parse (no marginals) on the same chart; prints one JSON line.

Shapes: B 64 at L 20, 40 and 64, D 400, one eval forward of a text-only DioraMLP each; then each C entry alone on the current stream
between two events, into buffers allocated beforehand: the median of --reps after a warm-up call.  Two bracket sets: none (the margin
kernel runs one pass, the gradient kernel returns after the mask) and L / 4 nested required brackets per sentence; the margin call as
the structured hinge (margin 1, penalty inf) and as a ramp (margin 1, penalty 1), without span outputs -- what a backward runs.  The
siblings to read the figures against: the constrained call without marginals (one fp32 best-tree pass, one fp64 inside pair) and the
gradient call (four fp64 tables); there is no pass / fail number.  --bench-gate FILE: a JSON object (the
bench.py step times of the parent commit and of this one, taken in one session) stored under "bench_gate" as it is.

    python tools/margin_bench.py [--out profiles/margin_bench.json]
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
from bracket_grad_bench import D, SHAPES, stat  # noqa: E402
from constrained_bench import event_ms, nested  # noqa: E402

INF = float('inf')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join('profiles', 'margin_bench.json'))
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
        f = [torch.empty(B, dtype=torch.float32, device='cuda') for _ in range(8)]
        i = [torch.empty(B, dtype=torch.int32, device='cuda') for _ in range(4)]
        status = torch.zeros(1, dtype=torch.int32, device='cuda')
        d_split = torch.empty(split_score_count(plan), dtype=torch.float32, device='cuda')
        args = lambda br: (_lib.ptr(br) if br is not None else None, int(br.shape[1]) if br is not None else 0)

        def parse(br):
            _lib.call('cliora_constrained_parse', plan.handle, ws, None, *args(br), _lib.ptr(out), _lib.ptr(f[0]), _lib.ptr(f[1]), _lib.ptr(f[2]),
                      _lib.ptr(f[3]), _lib.ptr(i[0]), None, _lib.ptr(status), _lib.stream())

        def grad(br):
            _lib.call('cliora_bracket_grad', plan.handle, ws, None, *args(br), None, _lib.ptr(d_split), _lib.ptr(f[4]), _lib.ptr(i[1]),
                      _lib.ptr(status), _lib.stream())

        def margin(br, penalty):
            _lib.call('cliora_bracket_margin', plan.handle, ws, None, *args(br), 1.0, penalty, None, _lib.ptr(d_split), _lib.ptr(f[5]),
                      _lib.ptr(f[6]), _lib.ptr(f[7]), _lib.ptr(i[2]), _lib.ptr(i[3]), None, None, _lib.ptr(status), _lib.stream())

        row = dict(B=B, L=L, D=D, brackets_per_sentence=int(brackets.shape[1]))
        for name, br in (('none', None), ('nested', brackets)):
            stat(row, 'constrained_%s' % name, event_ms(lambda: parse(br), a.reps))
            stat(row, 'bracket_grad_%s' % name, event_ms(lambda: grad(br), a.reps))
            stat(row, 'margin_hinge_%s' % name, event_ms(lambda: margin(br, INF), a.reps))
            assert int(status) == 0 and bool((i[3] == 1).all()) and bool((f[5] >= 0).all())
            assert bool((d_split == 0).all()) == (br is None)
            if br is not None:
                row['mean_hinge'], row['mean_violations'] = round(float(f[5].mean()), 4), round(float(i[2].float().mean()), 2)
            stat(row, 'margin_ramp_%s' % name, event_ms(lambda: margin(br, 1.0), a.reps))
            for form in ('hinge', 'ramp'):
                for sib in ('constrained', 'bracket_grad'):
                    row['margin_%s_%s_ratio_to_%s' % (form, name, sib)] = round(row['margin_%s_%s_ms' % (form, name)] / row['%s_%s_ms' % (sib, name)], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='margin', reps=a.reps, library=_lib.lib().cliora_version().decode(), shapes=rows)
    if a.bench_gate:
        with open(a.bench_gate) as fh:
            res['bench_gate'] = json.load(fh)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
