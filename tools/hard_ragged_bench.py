#!/usr/bin/env python
"""Hard (S-DIORA) charts on mixed-length sentences: the padded hard chart (cliora_chart_forward_ragged_hard, cliora_hard_spans_ragged)
beside the paths a hard net had before it and beside the soft padded chart, on one GPU; prints one JSON line and writes it to --out.

Sets as tools/ragged_bench.py: lengths uniform in 5..40, (a) 64 sentences, (b) 1000 sentences, a text-only DioraMLP of width 400 over
1024-wide embeddings of 20 000 words, 100 negatives, split-bf16 arithmetic (the default).  ONE net serves every row: its chart module's
`.hard` is switched, so the hard and the soft rows share weights and sentences.  Per set, all in this one run:
  parse    ragged.parse_ragged_hard  |  ragged.parse_ragged (soft, Viterbi)  |  hard parsing bucketed by exact length (the inside pass
           + hard_tree per batch of one length, at most 64 sentences each)
  forward  both passes through ragged.forward_ragged on the hard net  |  hard forwards bucketed by exact length, outside pass on
  train    Trainer.step_ragged on the hard net, one call per 64 sentences in the caller's order  |  one Trainer.step per exact-length
           batch on the same hard net  |  Trainer.step_ragged on the soft net
Every figure is the median wall-clock of --reps passes after a warm-up pass, host work and copies included, each pass ended by a
device synchronise.  No threshold is asserted: the figures are reported as found.

    python tools/hard_ragged_bench.py [--out profiles/hard_ragged_bench.json]
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
from ragged_train_bench import bucket_batches   # noqa: E402


def bucketed_hard(net, batches, trees):
    """One hard forward per exact-length batch with the module's `outside` as it is; trees: also hard_tree per batch."""
    out = []
    with torch.no_grad():
        for t in batches:
            net.diora(*net.embed(t))
            if trees:
                out.extend(net.diora.hard_tree())
    return out


def row(t, count, base=None):
    d = dict(ms=round(t * 1e3, 3), sentences_per_s=round(count / t, 1))
    if base is not None:
        d['speedup'] = round(base / t, 2)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--out', default=os.path.join('profiles', 'hard_ragged_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hard_ragged_bench needs the GPU: nothing here is measured without one')
    torch.manual_seed(0)
    V = 20000
    net = H.build_net(a.size, torch.nn.Embedding(V, 1024), obj_feats=False, hard=True).cuda()
    tr = H.Trainer(net, lr=1e-4)
    dev = next(net.parameters()).device
    neg = torch.arange(1, 101).to(dev)
    rs = np.random.RandomState(0)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, reps=a.reps, sets=[])
    for name, count in (('a', 64), ('b', 1000)):
        sents = [rs.randint(1, V, size=n).tolist() for n in rs.randint(5, 41, size=count)]
        batches = bucket_batches(sents, dev)
        chunks = [sents[r:r + 64] for r in range(0, count, 64)]
        s = dict(set=name, sentences=count, tokens=sum(map(len, sents)), distinct_lengths=len(set(map(len, sents))), buckets=len(batches),
                 packs=len(ragged.pack([len(x) for x in sents])))
        # ---- parse
        net.eval()
        net.diora.hard, net.diora.outside = True, False
        tb, _ = timed(lambda: bucketed_hard(net, batches, True), a.reps)
        th, hard_trees = timed(lambda: ragged.parse_ragged_hard(net, sents), a.reps)
        net.diora.hard = False
        ts, _ = timed(lambda: ragged.parse_ragged(net, sents), a.reps)
        net.diora.hard = True
        s['parse'] = dict(hard_bucketed=row(tb, count), parse_ragged_hard=row(th, count, tb), parse_ragged_soft_viterbi=row(ts, count),
                          hard_over_soft=round(ts / th, 2), trees=len(hard_trees))
        # ---- both passes
        net.diora.outside = True
        tb, _ = timed(lambda: bucketed_hard(net, batches, False), a.reps)
        tf, _ = timed(lambda: ragged.forward_ragged(net, sents), a.reps)
        s['forward'] = dict(hard_bucketed=row(tb, count), forward_ragged_hard=row(tf, count, tb))
        # ---- training
        net.train()
        tb, _ = timed(lambda: [tr.step(dict(sentences=t, neg_samples=neg), sync=False)['total_loss'] for t in batches], a.reps)
        tp, _ = timed(lambda: [tr.step_ragged(c, neg_samples=neg)['total_loss'] for c in chunks], a.reps)
        net.diora.hard = False
        tq, _ = timed(lambda: [tr.step_ragged(c, neg_samples=neg)['total_loss'] for c in chunks], a.reps)
        net.diora.hard = True
        s['train'] = dict(hard_bucketed_steps=dict(steps=len(batches), **row(tb, count)),
                          step_ragged_hard=dict(steps=len(chunks), **row(tp, count, tb)), step_ragged_soft=dict(steps=len(chunks), **row(tq, count)),
                          hard_over_soft=round(tq / tp, 2))
        res['sets'].append(s)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
