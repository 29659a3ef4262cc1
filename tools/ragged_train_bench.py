#!/usr/bin/env python
"""Training on mixed-length sentences: Trainer.step_ragged (padded charts, cliora_chart_forward_ragged_train /
cliora_chart_backward_ragged) against Trainer.step over exact-length buckets of the same sentences, on one GPU; prints one JSON line.

Sets as tools/ragged_bench.py: lengths uniform in 5..40, (a) 64 sentences, (b) 1000 sentences, a text-only DioraMLP of width 400 over
1024-wide embeddings of 20 000 words, 100 negatives.  One pass over a set is
  bucketed: one Trainer.step (forward, backward, clip + Adam) per batch of one exact length, at most 64 sentences each;
  ragged:   one Trainer.step_ragged per 64 sentences in the caller's order, each packed into padded charts (ragged.pack);
  one call: (set b) ONE Trainer.step_ragged over the whole set -- pack() then sorts all of it by length, so the padded charts carry
            little padding, at the price of a single optimizer step where the other two take 36 and 16.
All do the same arithmetic per sentence; the passes differ in their number of charts and of optimizer steps, which is the point: few
sentences per length leave the bucketed path one small step per length.  Every figure is the median wall-clock of --reps passes
after a warm-up pass, host work included.

    python tools/ragged_train_bench.py [--out profiles/ragged_train_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import harness as H             # noqa: E402
from cliora_amd import ragged                   # noqa: E402
from ragged_bench import timed                  # noqa: E402


def bucket_batches(sentences, dev, max_batch=64):
    by_len = {}
    for s in sentences:
        by_len.setdefault(len(s), []).append(s)
    out = []
    for n in sorted(by_len):
        for r in range(0, len(by_len[n]), max_batch):
            out.append(torch.tensor(by_len[n][r:r + max_batch]).to(dev))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    V = 20000
    net = H.build_net(a.size, torch.nn.Embedding(V, 1024), obj_feats=False).cuda()
    tr = H.Trainer(net, lr=1e-4)
    dev = next(net.parameters()).device
    neg = torch.arange(1, 101).to(dev)
    rs = np.random.RandomState(0)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, reps=a.reps, sets=[])
    for name, count in (('a', 64), ('b', 1000)):
        sents = [rs.randint(1, V, size=n).tolist() for n in rs.randint(5, 41, size=count)]
        batches = bucket_batches(sents, dev)
        chunks = [sents[r:r + 64] for r in range(0, count, 64)]

        def bucketed():
            return [tr.step(dict(sentences=t, neg_samples=neg), sync=False)['total_loss'] for t in batches]

        def padded():
            return [tr.step_ragged(c, neg_samples=neg)['total_loss'] for c in chunks]

        tb, _ = timed(bucketed, a.reps)
        tp, _ = timed(padded, a.reps)
        packs = sum(len(ragged.pack([len(s) for s in c])) for c in chunks)
        whole = None
        if len(chunks) > 1:
            tw, _ = timed(lambda: tr.step_ragged(sents, neg_samples=neg)['total_loss'], a.reps)
            whole = dict(steps=1, packs=len(ragged.pack([len(s) for s in sents])), ms=round(tw * 1e3, 3), sentences_per_s=round(count / tw, 1),
                         speedup_vs_bucketed=round(tb / tw, 2))
        res['sets'].append(dict(set=name, sentences=count, tokens=sum(map(len, sents)), distinct_lengths=len(set(map(len, sents))),
                                bucketed=dict(steps=len(batches), ms=round(tb * 1e3, 3), sentences_per_s=round(count / tb, 1)),
                                step_ragged=dict(steps=len(chunks), packs=packs, ms=round(tp * 1e3, 3), sentences_per_s=round(count / tp, 1),
                                                 speedup_vs_bucketed=round(tb / tp, 2)), step_ragged_one_call=whole))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
