#!/usr/bin/env python
"""Both passes + trees of an unfiltered set of sentences (lengths up to 128) on one GPU: forward_ragged(max_len=128) with the ragged
decode, beside the only route there was before it; prints one JSON line.

The route before: the sentences of up to 64 words through forward_ragged (its default) with the ragged decode, the longer ones
grouped by exact length and run through the uniform forward (both passes, the wavefront schedule) and cky_spans, at most --long-batch
of a length per call.  Two seeded sets: (a) 64 sentences with lengths uniform in 5..128; (b) 1 000 sentences with lengths uniform in
5..40 plus 10 with lengths uniform in 65..128.  A text-only DioraMLP of width 400 over 1024-wide embeddings.  Every figure is the
median wall-clock of --reps calls after a warm-up call that creates the plans, host work and the copies of the spans included.  No
ratio is promised: the padded chart runs its levels one after the other (inside pass, then outside pass), the uniform forward runs
the two passes as a wavefront, so a pack of few long sentences may well be slower than its sentences run one length at a time.

    python tools/long_ragged_bench.py [--out profiles/long_ragged_bench.json]
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
from cliora_amd import harness as H             # noqa: E402
from cliora_amd import ragged                   # noqa: E402

D = 400


def ragged_route(net, sentences, max_len):
    """forward_ragged + cky_spans_ragged per pack, the spans copied to the host; -> (spans per sentence, number of packs)."""
    out = [None] * len(sentences)

    def per_pack(idx, lens, d):
        spans, status = ragged.cky_spans_ragged(d, lens)
        host = torch.cat([spans.reshape(-1), status, d._ragged_status]).cpu().numpy()
        if host[-2:].any():
            raise _lib.ChartLibError('the padded chart rejected a sentence length')
        rows = host[:-2].reshape(spans.shape)
        for b, i in enumerate(idx):
            out[i] = rows[b, :len(sentences[i]) - 1]

    packs = ragged.forward_ragged(net, sentences, per_pack=per_pack, max_len=max_len)
    return out, len(packs)


def split_route(net, sentences, long_batch):
    """Before max_len: sentences of up to 64 words as above, the longer ones by exact length through the uniform forward + cky_spans."""
    short = [i for i, s in enumerate(sentences) if len(s) <= ragged.MAX_L]
    out = [None] * len(sentences)
    got, calls = ragged_route(net, [sentences[i] for i in short], ragged.MAX_L)
    for i, sp in zip(short, got):
        out[i] = sp
    by_len = {}
    for i, s in enumerate(sentences):
        if len(s) > ragged.MAX_L:
            by_len.setdefault(len(s), []).append(i)
    dev = next(net.parameters()).device
    with torch.no_grad():
        for n in sorted(by_len):
            for r in range(0, len(by_len[n]), long_batch):
                part = by_len[n][r:r + long_batch]
                net(torch.tensor([sentences[i] for i in part]).to(dev), compute_loss=False)
                sp = np.asarray(net.diora.cky_spans())
                for b, i in enumerate(part):
                    out[i] = sp[b]
                calls += 1
    return out, calls


def timed(fn, reps):
    fn()                                    # plans, tables, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--long-batch', type=int, default=ragged.DEFAULT_MAX_LONG_BATCH)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = H.build_net(D, torch.nn.Embedding(20000, 1024), obj_feats=False).cuda().eval()
    rs = np.random.RandomState(0)
    sets = (('a', [int(n) for n in rs.randint(5, 129, size=64)]),
            ('b', [int(n) for n in rs.randint(5, 41, size=1000)] + [int(n) for n in rs.randint(65, 129, size=10)]))
    rows = []
    for name, lengths in sets:
        sentences = [rs.randint(1, 20000, size=n).tolist() for n in lengths]
        r_med, r_lo, r_hi, (r_spans, r_calls) = timed(lambda: ragged_route(net, sentences, 128), a.reps)
        s_med, s_lo, s_hi, (s_spans, s_calls) = timed(lambda: split_route(net, sentences, a.long_batch), a.reps)
        same = sum(int(np.array_equal(x, y)) for x, y in zip(r_spans, s_spans))
        row = dict(set=name, sentences=len(lengths), longer_than_64=sum(n > 64 for n in lengths), max_length=max(lengths),
                   ragged_128_ms=round(r_med, 2), ragged_128_ms_min=round(r_lo, 2), ragged_128_ms_max=round(r_hi, 2), ragged_128_packs=r_calls,
                   split_route_ms=round(s_med, 2), split_route_ms_min=round(s_lo, 2), split_route_ms_max=round(s_hi, 2),
                   split_route_calls=s_calls, ragged_over_split=round(r_med / s_med, 3), same_trees=same)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    res = dict(bench='long_ragged', device=torch.cuda.get_device_name(0), D=D, mfma_mode='bf16x3', reps=a.reps, long_batch=a.long_batch,
               max_waste=ragged.DEFAULT_MAX_WASTE, library=_lib.lib().cliora_version().decode(), sets=rows)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
