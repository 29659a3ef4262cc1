#!/usr/bin/env python
"""Negative sampling: device time per draw of cliora_neg_sample (NegativeSampler.sample_many) against numpy's
RandomState.choice(V, k, replace=False, p) on the same host, and calculate_freq_dist against a Counter loop over the same corpus.

    python tools/neg_sample_bench.py [--reps 200] [--out profiles/neg_sample_bench.json]

Prints one JSON line.  Per draw (S draws per call), after a warm-up: `device_us_per_draw` = CUDA events around replays of a CUDA
graph of 20 calls (the kernels alone, one launch after the other); `eager_us_per_draw` = CUDA events around back-to-back Python
calls (sample_many: allocation, ctypes, launches -- bound by the host when the kernels are short).
Host times: wall clock per numpy draw, p normalised in float64 (the reference's float32 normalisation fails numpy's sum check at
V = 400k; `ref_float32_sum_ok` says whether it passes at each V).  Weights: Zipf-like counts ** 0.75 + 1e-2 / V.
"""
import argparse
import json
import os
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from cliora_amd.sampling import NegativeSampler, calculate_freq_dist       # noqa: E402


def zipf_counts(V, rs):
    return np.floor(1e7 / np.arange(1, V + 1) ** 1.05)[rs.permutation(V)].astype(np.float32)


def graph_us_per_draw(sampler, S, k, reps, per_graph=20):
    """Device time: `per_graph` calls captured into one CUDA graph, replayed -- no Python or launch-API time between the kernels."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            sampler.sample_many(S, k)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            sampler.sample_many(S, k)
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = max(1, reps // per_graph)
    a.record()
    for _ in range(n):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (n * per_graph * S)


def eager_us_per_draw(sampler, S, k, reps):
    for _ in range(5):
        sampler.sample_many(S, k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        sampler.sample_many(S, k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * S)


def host_us_per_draw(freq, k, reps):
    w = freq ** np.float32(0.75) + np.float32(1e-2 / freq.size)
    ref32 = w / sum(w)                                  # the reference's float32 normalisation
    rng = np.random.RandomState(0)
    try:
        rng.choice(freq.size, k, p=ref32, replace=False)
        ok32 = True
    except ValueError:
        ok32 = False
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    rng.choice(freq.size, k, p=p, replace=False)
    t = time.perf_counter()
    for _ in range(reps):
        rng.choice(freq.size, k, p=p, replace=False)
    return (time.perf_counter() - t) * 1e6 / reps, ok32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--k', type=int, default=100)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    rs = np.random.RandomState(0)
    res = dict(what='neg_sample', k=a.k, device=torch.cuda.get_device_name(0), draws=[])
    for V in (8000, 20000, 400000):
        freq = zipf_counts(V, rs)
        s = NegativeSampler(torch.from_numpy(freq).cuda(), 0.75, seed=1)
        row = dict(V=V)
        for S in (1, 500):
            reps = a.reps if S == 1 else max(20, a.reps // 10)
            row['device_us_per_draw_S%d' % S] = round(graph_us_per_draw(s, S, a.k, reps), 3)
            row['eager_us_per_draw_S%d' % S] = round(eager_us_per_draw(s, S, a.k, reps), 3)
        host, ok32 = host_us_per_draw(freq, a.k, max(10, a.reps // (1 + V // 20000)))
        row['numpy_us_per_draw'] = round(host, 1)
        row['ref_float32_sum_ok'] = ok32
        res['draws'].append(row)
    # counts: 2 M tokens in sentences of 5..40 over V = 20k
    V = 20000
    p = 1.0 / np.arange(1, V + 1) ** 1.05
    ids = rs.choice(V, 2000000, p=p / p.sum())
    cuts = np.cumsum(rs.randint(5, 41, size=2000000 // 5))
    cuts = cuts[cuts < ids.size]
    sents = [x.tolist() for x in np.split(ids, cuts)]
    calculate_freq_dist(sents[:10], V, 'cuda')
    torch.cuda.synchronize()
    t = time.perf_counter()
    freq = calculate_freq_dist(sents, V, 'cuda')
    torch.cuda.synchronize()
    dev_s = time.perf_counter() - t
    t = time.perf_counter()
    c = Counter({i: 0 for i in range(V)})
    for x in sents:
        c.update(x)
    ref = np.asarray([v for _, v in sorted(c.items())], dtype=np.float32)
    host_s = time.perf_counter() - t
    assert np.array_equal(freq.cpu().numpy(), ref)
    res['freq_dist'] = dict(tokens=int(ids.size), sentences=len(sents), V=V, device_path_ms=round(dev_s * 1e3, 2),
                            counter_loop_ms=round(host_s * 1e3, 1), equal=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
