#!/usr/bin/env python
"""Per-batch time of cliora_amd.evaluate against the same loop with the reference's host-side grounding (parse.py:176-264: a CPU
copy of atten_score, a .max() per phrase and per predicted span, a box_iou per phrase), on a synthetic c3-sized batch
(B 64, L 20, R 36, about 5 phrases per sentence).  Both include the eval forward with losses; the grounding stage alone is
timed as well.  Prints one JSON line.

    python tools/eval_bench.py [--iters 20] [--warmup 3] [--dim 400]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import harness as H                    # noqa: E402
from cliora_amd.evaluate import evaluate, ground_batch      # noqa: E402
from cliora_amd.interchange import SpanF1              # noqa: E402


def box_iou(a, b):
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[:, :2])
    rb = torch.min(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def host_ground(diora, bm, f1):
    """parse.py:176-264 as the reference runs it (host copies, per-phrase and per-span .max(), box_iou)."""
    att = diora.atten_score.cpu()
    boxes = bm['boxes'].cpu()
    recall = ccr = total = 0
    spans = diora.cky_spans()
    for b, (target, _) in enumerate(bm['VG_GT']):
        pred = set(map(tuple, spans[b][:-1].tolist()))
        gold = set(bm['GT'][b][:-1])
        hit_ = len(pred & gold)
        f1.add_counts(hit_, len(pred), len(gold))
        for s, e, gt_box in target.values():
            words = att[b, s:e]
            wid = words.max(1)[0].max(0)[1]
            box = words[wid].max(0)[1]
            hit = bool(box_iou(boxes[b, box][None], torch.tensor([gt_box])).max() > 0.5)
            recall += hit
            ccr += hit and (e - 1 == s or (s, e - 1) in pred)
            total += 1
        out = []
        for s, e in pred:
            words = att[b, s:e + 1]
            wid = words.max(1)[0].max(0)[1]
            out.append(boxes[b, words[wid].max(0)[1]].tolist())
    return recall, ccr, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dim', type=int, default=400)
    a = ap.parse_args()
    B, L, R, V, K = 64, 20, 36, 2000, 100
    torch.manual_seed(0)
    rs = np.random.RandomState(1)
    net = H.build_net(a.dim, torch.nn.Embedding(V, 64), obj_feats=True, img_dim=2048, k_neg=K, vg_loss=True, use_contr=True).cuda()
    for p in net.img_encoder.parameters():
        p.data.normal_(0, 0.02)
    xy = torch.randint(0, 300, (B, R, 2)).float()
    boxes = torch.cat([xy, xy + torch.randint(1, 200, (B, R, 2)).float()], -1)
    vg, gt = [], []
    for b in range(B):
        t = {}
        for j in range(5):
            s = int(rs.randint(0, L))
            t[j] = (s, int(rs.randint(s + 1, min(L, s + 4) + 1)), boxes[b, rs.randint(0, R)].tolist())
        vg.append((t, None))
        gt.append([(int(s), int(s) + 1) for s in rs.randint(0, L - 1, size=10)] + [(0, L - 1)])
    bm = dict(sentences=torch.randint(1, V, (B, L)).cuda(), obj_feats=torch.randn(B, R, 2048).cuda(), boxes=boxes.cuda(),
              neg_samples=torch.randperm(V)[:K].cuda(), VG_GT=vg, GT=gt, example_ids=list(range(B)))
    idx2word = {i: str(i) for i in range(V)}
    net.eval()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3

    def host_loop():
        f1 = SpanF1()
        with torch.no_grad():
            out = net(bm['sentences'], bm['obj_feats'], bm['neg_samples'], compute_loss=True)
            [float(v) for v in (out['reconstruct_softmax_loss'], out['vg_loss'], out['contrastive_loss'], out.total())]
            host_ground(net.diora, bm, f1)

    with torch.no_grad():
        net(bm['sentences'], bm['obj_feats'], bm['neg_samples'], compute_loss=True)
    res = dict(shape=dict(B=B, L=L, R=R, D=a.dim, phrases=5 * B), iters=a.iters,
               evaluate_ms=timed(lambda: evaluate(net, [bm], idx2word)),
               host_loop_ms=timed(host_loop),
               ground_batch_ms=timed(lambda: ground_batch(net.diora, bm)),
               host_ground_ms=timed(lambda: host_ground(net.diora, bm, SpanF1())),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
