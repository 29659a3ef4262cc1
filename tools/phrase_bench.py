#!/usr/bin/env python
"""Phrase search and embedding timings on one GPU; prints one JSON line.

  * cliora_knn_ip (self-search of N unit rows, D = 800, k = 100) per MFMA mode at N in --sizes: device-event time after a warm-up,
    the algorithmic TFLOP/s 2 N^2 D / t and its share of the mode's MFMA peak (split-bf16: three bf16 products per product against
    2.5 PF dense bf16; f32: 157.3 TF);
  * the same search as chunked torch.mm + torch.topk (a baseline only, never on the product path) and the agreement of the two;
  * embed_phrases on a c3-sized batch (B 64, L 20, D 400, five entity phrases per sentence) against the reference's host gather
    (forward, then chart.cpu() and chart[batch_index, idx] as phrase_embed.py:79-92 does).

    python tools/phrase_bench.py [--sizes 20000,100000,400000] [--out profiles/phrase_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd import harness as H             # noqa: E402
from cliora_amd.phrases import embed_phrases, knn_ip      # noqa: E402

PEAK = {'bf16x3': 2.5e15 / 3, 'f32': 157.3e12}       # products per second at the nominal peaks, as FLOP/s of the fp32 product


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, out


def torch_search(x, k, chunk=2048):
    Ds, Is = [], []
    for r in range(0, x.shape[0], chunk):
        v, i = torch.topk(torch.mm(x[r:r + chunk], x.T), k, dim=1)
        Ds.append(v)
        Is.append(i)
    return torch.cat(Ds), torch.cat(Is)


def search_rows(sizes, D=800, k=100, torch_max=None):
    out = []
    for N in sizes:
        g = torch.Generator(device='cuda').manual_seed(N)
        x = torch.nn.functional.normalize(torch.randn(N, D, device='cuda', generator=g), dim=1)
        flop = 2.0 * N * N * D
        row = dict(N=N, D=D, k=k)
        res = {}
        for mode in ('bf16x3', 'f32'):
            prev = _lib.set_mfma_mode(mode)
            try:
                ms, (Dv, Iv) = timed(lambda: knn_ip(x, x, k), 2 if N <= 100000 else 1)
            finally:
                _lib.set_mfma_mode(prev)
            tf = flop / (ms * 1e-3)
            row[mode] = dict(ms=round(ms, 3), tflops=round(tf / 1e12, 2), share_of_peak=round(tf / PEAK[mode], 3),
                             floor_ms=round(flop / PEAK[mode] * 1e3, 2))
            res[mode] = (Dv, Iv)
        if torch_max is None or N <= torch_max:
            ms, (Dt, It) = timed(lambda: torch_search(x, k), 1)
            row['torch_mm_topk'] = dict(ms=round(ms, 3))
            n = min(N, 4096)
            for mode, (Dv, Iv) in res.items():
                same = (torch.sort(Iv[:n], 1).values == torch.sort(It[:n], 1).values).all(1).float().mean().item()
                row[mode]['agree_with_torch'] = dict(rows_same_id_set=round(same, 4), max_abs_score_diff=float((Dv[:n] - Dt[:n]).abs().max()))
            row['bf16x3']['speedup_vs_torch'] = round(row['torch_mm_topk']['ms'] / row['bf16x3']['ms'], 2)
        out.append(row)
        del x, res
        torch.cuda.empty_cache()
    return out


def embed_row(B=64, L=20, D=400, V=2000, E=300, per=5, reps=20):
    torch.manual_seed(0)
    net = H.build_net(D, torch.nn.Embedding(V, E)).cuda()
    rs = np.random.RandomState(0)
    ents = []
    for _ in range(B):
        lst = []
        for _ in range(per):
            size = int(rs.randint(2, L + 1))
            lst.append(('X', int(rs.randint(0, L - size + 1)), size))
        ents.append(lst)
    bm = dict(sentences=torch.randint(1, V, (B, L), device='cuda'), example_ids=[str(i) for i in range(B)], entity_labels=ents)
    ms_dev, _ = timed(lambda: embed_phrases(net, [bm], 'entities'), reps)

    def host():
        with torch.no_grad():
            net.eval()
            net.diora.outside = True
            net(bm['sentences'], None, None, compute_loss=False)
            d = net.diora
            bi = [i for i, lst in enumerate(ents) for _ in lst]
            pos = [e[1] for lst in ents for e in lst]
            size = [e[2] for lst in ents for e in lst]
            off = net.diora.index.get_offset(L)
            idx = [off[s - 1] + p for p, s in zip(pos, size)]
            return np.concatenate([d.inside_h.cpu()[bi, idx].numpy(), d.outside_h.cpu()[bi, idx].numpy()], 1)
    ms_host, _ = timed(host, reps)
    return dict(B=B, L=L, D=D, phrases=B * per, embed_phrases_ms=round(ms_dev, 3), host_gather_ms=round(ms_host, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='20000,100000,400000')
    ap.add_argument('--torch-max', type=int, default=None, help='largest N for the torch baseline')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), search=search_rows([int(s) for s in a.sizes.split(',')], torch_max=a.torch_max),
               embed=embed_row())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
