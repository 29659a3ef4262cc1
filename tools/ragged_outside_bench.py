#!/usr/bin/env python
"""Mixed-length batches WITH the outside pass: cliora_amd.ragged.forward_ragged + the ragged decode against the existing path on one
GPU; prints one JSON line.

The existing path buckets the sentences by exact length and runs the forward with the outside pass on + cky() per bucket (batches of
at most 64).  The new path packs them (ragged.pack, the default max_waste), runs each pack through cliora_chart_forward_ragged and
decodes it with cliora_cky_spans_ragged, one device-to-host copy per pack.  Sets as tools/ragged_bench.py: lengths uniform in 5..40,
(a) 64 sentences, (b) 1000 sentences, a text-only DioraMLP of width 400 over 1024-wide embeddings.  Then the CLIORA evaluation on a
synthetic set of 1000 examples (D 400, 36 regions of 2048 features): evaluate.evaluate over exact-length buckets against
evaluate.evaluate_ragged (the former also computes the eval losses per bucket, the latter leaves them out).  Every figure is the
median wall-clock of --reps runs after a warm-up run, host work and copies included.

    python tools/ragged_outside_bench.py [--out profiles/ragged_outside_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import evaluate as EV           # noqa: E402
from cliora_amd import harness as H             # noqa: E402
from cliora_amd import ragged                   # noqa: E402
from ragged_bench import bucketed, timed        # noqa: E402


def ragged_outside(net, sentences):
    """Both passes + trees, in the caller's order."""
    diora = net.diora
    trees = [None] * len(sentences)

    def decode(idx, lens, d):
        spans, status = ragged.cky_spans_ragged(d, lens)
        host = torch.cat([spans.reshape(-1), status, d._ragged_status]).cpu().numpy()
        assert not host[-2:].any()
        rows = host[:-2].reshape(spans.shape)
        for b, i in enumerate(idx):
            trees[i] = diora.trees_from_spans(rows[b:b + 1, :len(sentences[i]) - 1])[0]

    packs = ragged.forward_ragged(net, sentences, per_pack=decode)
    return trees, packs


def examples(count, rs, V, R, img):
    gen = torch.Generator().manual_seed(1)
    out = []
    for i, n in enumerate(rs.randint(5, 41, size=count)):
        n = int(n)
        xy = torch.randint(0, 300, (R, 2), generator=gen).float()
        boxes = torch.cat([xy, xy + torch.randint(1, 150, (R, 2), generator=gen).float()], -1)
        target = {}
        for j in range(3):
            s = rs.randint(0, n)
            target[j] = (s, rs.randint(s + 1, n + 1), boxes[rs.randint(0, R)].tolist())
        gold = [(s, rs.randint(s + 1, n)) for s in rs.randint(0, n - 1, size=n // 2)]
        out.append(dict(sentence=rs.randint(1, V, size=n).tolist(), example_id=i, GT=gold + [(0, n - 1)], VG_GT=(target, None), boxes=boxes,
                        obj_feats=torch.randn(R, img, generator=gen)))
    return out


def bucket_batches(exs, max_batch=64):
    by_len = {}
    for ex in exs:
        by_len.setdefault(len(ex['sentence']), []).append(ex)
    out = []
    for n in sorted(by_len):
        for r in range(0, len(by_len[n]), max_batch):
            part = by_len[n][r:r + max_batch]
            out.append(dict(sentences=torch.tensor([e['sentence'] for e in part]), obj_feats=torch.stack([e['obj_feats'] for e in part]),
                            boxes=torch.stack([e['boxes'] for e in part]), neg_samples=torch.arange(1, 101),
                            VG_GT=[e['VG_GT'] for e in part], GT=[e['GT'] for e in part], example_ids=[e['example_id'] for e in part]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--size', type=int, default=400)
    ap.add_argument('--out', default=None)
    ap.add_argument('--skip-eval', action='store_true')
    a = ap.parse_args()
    torch.manual_seed(0)
    net = H.build_net(a.size, torch.nn.Embedding(20000, 1024), obj_feats=False).cuda().eval()
    rs = np.random.RandomState(0)
    res = dict(device=torch.cuda.get_device_name(0), size=a.size, reps=a.reps, sets=[])
    for name, count in (('a', 64), ('b', 1000)):
        sents = [rs.randint(1, 20000, size=n).tolist() for n in rs.randint(5, 41, size=count)]
        net.diora.outside = True
        tb, want = timed(lambda: bucketed(net, sents), a.reps)
        tr, (got, packs) = timed(lambda: ragged_outside(net, sents), a.reps)
        fix = [len(set(len(sents[i]) for i in p) - {max(len(sents[i]) for i in p)}) for p in packs]
        res['sets'].append(dict(set=name, sentences=count, distinct_lengths=len(set(map(len, sents))),
                                bucketed_outside_on=dict(ms=round(tb * 1e3, 3), sentences_per_s=round(count / tb, 1)),
                                ragged_outside=dict(packs=len(packs), ms=round(tr * 1e3, 3), sentences_per_s=round(count / tr, 1),
                                                    speedup_vs_bucketed=round(tb / tr, 2), fixup_rescore_launches_per_pack=fix,
                                                    same_trees=sum(str(x) == str(y) for x, y in zip(got, want)))))
    if not a.skip_eval:
        V = 2000
        torch.manual_seed(1)
        vl = H.build_net(a.size, torch.nn.Embedding(V, 1024), obj_feats=True, img_dim=2048).cuda().eval()
        exs = examples(1000, np.random.RandomState(2), V, 36, 2048)
        idx2word = {i: 'w%d' % i for i in range(V)}
        batches = bucket_batches(exs)
        for bm in batches:
            for k in ('sentences', 'obj_feats', 'boxes', 'neg_samples'):
                bm[k] = bm[k].cuda()
        te, m0 = timed(lambda: EV.evaluate(vl, batches, idx2word), a.reps)
        tg, m1 = timed(lambda: EV.evaluate_ragged(vl, exs, idx2word), a.reps)
        res['cliora_eval'] = dict(examples=len(exs), buckets=len(batches),
                                  evaluate_bucketed=dict(ms=round(te * 1e3, 3), ground_acc=m0['ground_acc'], ccra=m0['ccra'], corpus_f1=m0['corpus_f1']),
                                  evaluate_ragged=dict(ms=round(tg * 1e3, 3), speedup=round(te / tg, 2), ground_acc=m1['ground_acc'], ccra=m1['ccra'],
                                                       corpus_f1=m1['corpus_f1']))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
