#!/usr/bin/env python
"""Generate negatives.npz by RUNNING the reference's negative sampler (cliora/blocks/negative_sampler.py): calculate_freq_dist,
NegativeSampler(...).dist and seeded draws of NegativeSampler.sample.

Needs a checkout of the reference; the tests only read the file it writes.
Usage:  python tests/golden/make_golden_negatives.py [reference checkout, default /root/reference]

Contents:
  corpus_ids / corpus_lens  a Zipf-like corpus of 600 sentences over V = 300 (flattened ids, sentence lengths);
  freq300                   calculate_freq_dist(corpus, 300) (float32);
  dist300                   NegativeSampler(freq300, 0.75).dist (float32);
  freq64, incl64, first64   at V = 64, k = 10, set_seed(1234): counts of 20 000 draws, per id: draws that include it and draws
                            that take it first (freq64: float32 Zipf counts);
  freq8, pairs8             at V = 8, k = 2, set_seed(1234): pairs8[i, j] = number of the 20 000 draws that are (i, j) in order.
The draws' own ids are not a contract (the reference's sampler is unseeded): the tests compare statistics.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else '/root/reference')
from cliora.blocks.negative_sampler import NegativeSampler, calculate_freq_dist       # noqa: E402

N_DRAWS = 20000


def zipf_counts(V, n, rs, a=1.1):
    p = 1.0 / np.arange(1, V + 1) ** a
    p = p[rs.permutation(V)]
    return np.bincount(rs.choice(V, n, p=p / p.sum()), minlength=V)


def main():
    rs = np.random.RandomState(20261016)
    V = 300
    p = 1.0 / np.arange(1, V + 1) ** 1.05
    p = p[rs.permutation(V)]
    p[rs.choice(V, 20, replace=False)] = 0.0                           # words that never occur: count 0, weight eps / V
    lens = rs.randint(3, 25, size=600)
    corpus = [list(rs.choice(V, n, p=p / p.sum())) for n in lens]
    freq300 = calculate_freq_dist(corpus, V)
    dist300 = NegativeSampler(freq300, 0.75).dist.astype(np.float32)

    freq64 = zipf_counts(64, 5000, rs).astype(np.float32)
    ns = NegativeSampler(freq64, 0.75)
    ns.set_seed(1234)
    incl64 = np.zeros(64, np.int64)
    first64 = np.zeros(64, np.int64)
    for _ in range(N_DRAWS):
        d = ns.sample(10)
        incl64[d] += 1
        first64[d[0]] += 1

    freq8 = np.array([50, 20, 9, 4, 2, 1, 0, 7], np.float32)
    ns = NegativeSampler(freq8, 0.75)
    ns.set_seed(1234)
    pairs8 = np.zeros((8, 8), np.int64)
    for _ in range(N_DRAWS):
        a, b = ns.sample(2)
        pairs8[a, b] += 1

    path = os.path.join(HERE, 'negatives.npz')
    np.savez_compressed(path, corpus_ids=np.concatenate(corpus).astype(np.int32), corpus_lens=lens.astype(np.int32), freq300=freq300,
                        dist300=dist300, freq64=freq64, incl64=incl64, first64=first64, freq8=freq8, pairs8=pairs8,
                        n_draws=np.int64(N_DRAWS))
    print('wrote negatives.npz', os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
