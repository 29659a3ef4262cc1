#!/usr/bin/env python
"""Mixed-length parsing: sentences/s of cliora_amd.ragged.parse_ragged against the existing path on one GPU; prints one JSON line.

The existing path buckets the sentences by exact length and runs forward + cky() per bucket (in batches of at most 64), which is
what a caller had to do before.  It is timed twice: as the module is built (outside pass on) and with the outside pass off, the fair
yardstick for a caller who only wants trees.  parse_ragged is timed per `max_waste` of the packer (0 = exact-length buckets).  Two
sets, lengths uniform in 5..40: (a) 64 sentences, (b) 1000 sentences.  A text-only DioraMLP of width 400 over 1024-wide embeddings.
Every figure is the median wall-clock of --reps runs after a warm-up run that creates the plans, host work and copies included.

    python tools/ragged_bench.py [--out profiles/ragged_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import harness as H             # noqa: E402
from cliora_amd import ragged                   # noqa: E402

WASTES = (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, float('inf'))


def bucketed(net, sentences, max_batch=64):
    """The existing path: one forward + cky() per batch of one exact length; trees in the caller's order."""
    by_len = {}
    for i, s in enumerate(sentences):
        by_len.setdefault(len(s), []).append(i)
    trees = [None] * len(sentences)
    dev = next(net.parameters()).device
    with torch.no_grad():
        for n in sorted(by_len):
            idx = by_len[n]
            for r in range(0, len(idx), max_batch):
                part = idx[r:r + max_batch]
                net(torch.tensor([sentences[i] for i in part]).to(dev), compute_loss=False)
                for i, t in zip(part, net.diora.cky()):
                    trees[i] = t
    return trees


def timed(fn, reps):
    fn()                                    # plans, tables, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = H.build_net(a.size, torch.nn.Embedding(20000, 1024), obj_feats=False).cuda().eval()
    rs = np.random.RandomState(0)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, reps=a.reps, sets=[])
    for name, count in (('a', 64), ('b', 1000)):
        sents = [rs.randint(1, 20000, size=n).tolist() for n in rs.randint(5, 41, size=count)]
        row = dict(set=name, sentences=count, distinct_lengths=len(set(map(len, sents))))
        net.diora.outside = True
        t, want = timed(lambda: bucketed(net, sents), a.reps)
        row['bucketed_outside_on'] = dict(ms=round(t * 1e3, 3), sentences_per_s=round(count / t, 1))
        net.diora.outside = False
        t, _ = timed(lambda: bucketed(net, sents), a.reps)
        net.diora.outside = True
        row['bucketed'] = dict(ms=round(t * 1e3, 3), sentences_per_s=round(count / t, 1))
        base = t
        row['parse_ragged'] = []
        for w in WASTES:
            packs = ragged.pack([len(s) for s in sents], 64, w)
            t, got = timed(lambda: ragged.parse_ragged(net, sents, max_waste=w), a.reps)
            row['parse_ragged'].append(dict(max_waste=w if w != float('inf') else 'inf', packs=len(packs), ms=round(t * 1e3, 3),
                                            sentences_per_s=round(count / t, 1), speedup_vs_bucketed=round(base / t, 2),
                                            same_trees=sum(str(x) == str(y) for x, y in zip(got, want))))
        res['sets'].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
