"""The K best binary trees of every sentence from the chart's per-split scores (cliora_kbest_spans).

The CKY decode (``DioraBase.cky``) returns the one best tree over the potentials r[cell, k] = s[cell, k] - max_k s[cell, .]; this is
the list of the K best over the same potentials (include/cliora_chart.h): their spans, their scores (the sum
of r over a tree's internal cells, so ``exp(score - log_z)`` with the log_z of ``posterior.span_posteriors`` is the tree's share of
the posterior mass), and how many there are.  Rank 0 is the CKY tree.  The reference has no counterpart.

    kb = kbest_spans(net.diora, 8)                       # after a forward; device tensors, nothing synchronised
    mass = kb.log_prob(span_posteriors(net.diora).log_z).exp().sum(1)
    trees = net.diora.kbest(8)                           # per sentence [(nested tuples as net.diora.cky(), score)]

The order is the contract: every cell holds at most K derivations (value, split k, left rank i, right rank j); a leaf holds one of
value 1.0; a candidate is (val_left[i] + val_right[j]) + (s_k - smax) in fp32, in that order; the list is the first K candidates by
value descending, then split, left rank, right rank ascending.  ``kbest_numpy`` restates it in fp32 for tests, bit for bit.
The same lists among the trees that keep required and forbidden brackets: ``constrained.constrained_kbest``.
"""
import numpy as np
import torch

from . import _lib
from .query import ChartQuery, per_sentence, sentences_of, walk

MAX_K = 16               # csrc/kbest_kernels.hpp KBEST_MAX_K: 4 bits per rank in a derivation's packed key


def tree_count(n, k):
    """min(k, Catalan(n - 1)): the trees a sentence of n words has, up to k (Catalan(5) = 42 > MAX_K)."""
    return min(k, (1, 1, 2, 5, 14)[n - 1]) if 1 <= n <= 5 else k


class KBest(object):
    """spans (B, K, L-1, 2) int32 -- tree t's n - 1 spans in cky_spans' order, (-1, -1) beyond them and beyond count; scores (B, K)
    fp32, -inf beyond count; count (B,) int32; status (number of workspaces,) int32 -- lengths outside [1, L], which the caller of a
    mixed-length run must check.  Device tensors; nothing is synchronised."""

    def __init__(self, spans, scores, count, status):
        self.spans, self.scores, self.count, self.status = spans, scores, count, status

    def log_prob(self, log_z):
        """scores - log_z[:, None]: the log of each tree's posterior mass, log_z from span_posteriors on the same chart."""
        return self.scores - log_z[:, None]


def kbest_spans(diora, k, lengths=None):
    """cliora_kbest_spans on a chart module after its forward.  k: 1 .. 16.  lengths: None (every sentence has L words) or an int32
    tensor (B,) for a right-padded batch.  Allocates the scratch the library asks for.  -> KBest."""
    q = ChartQuery(diora)
    plan, k = q.plan, int(k)
    q.check_int32('lengths', lengths)
    width = max(k, 0)                                      # a bad k is the library's to refuse, with its message
    spans, scores, count = q.empty(torch.int32, width, plan.L - 1, 2), q.empty(torch.float32, width), q.empty(torch.int32)
    status = q.status()
    need = _lib.fn('cliora_kbest_scratch_bytes')(plan.handle, k)
    scratch = torch.empty(need, dtype=torch.uint8, device=q.dev) if need else None
    q.launch('cliora_kbest_spans', per_sentence(q.moved(lengths)), k, per_sentence(spans), per_sentence(scores), per_sentence(count),
             scratch, status=status)
    return KBest(spans, scores, count, status)


def _walk(key, n, rank):
    """The kernel's walk over the derivations key[level][pos, rank] = (split, left rank, right rank): left subtree, right subtree,
    then the node.  -> [(start, end)], children before parents."""
    def choose(level, pos, r):
        return key[level][pos, r]
    return [row[:2] for row in walk(n, choose, rank)]


def kbest_numpy(pair_s, lengths, k, L=None):
    """The k-best lists restated in fp32 in the kernel's operation order, for tests: `pair_s[level]` (B, L - level, level[, 1]) are
    the per-split inside scores of the (padded) chart of length L (inferred from level 1 when not given), sentence b its first
    lengths[b] words -- the layout ``posterior_numpy`` takes.  Every candidate of a cell at once: (k, i, j) in key order, a stable
    sort by value descending, the first K.  -> (spans (B, K, L-1, 2) int32, scores (B, K) float32, count (B,) int32) as the kernel
    writes them; a length outside [1, L] gives count 0."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError('k must be in 1..%d' % MAX_K)
    lengths, L = sentences_of(pair_s, lengths, L)
    spans = np.full((len(lengths), k, max(L - 1, 0), 2), -1, dtype=np.int32)
    scores = np.full((len(lengths), k), -np.inf, dtype=np.float32)
    count = np.zeros(len(lengths), dtype=np.int32)
    for b, n in enumerate(lengths):
        if not 1 <= n <= L:
            continue
        cnt = [tree_count(level + 1, k) for level in range(n)]
        val = np.full((n, n, k), -np.inf, dtype=np.float32)                  # [level, pos, rank]
        val[0, :, 0] = 1.0
        key = {}
        for level in range(1, n):
            s = np.asarray(pair_s[level][b], dtype=np.float32).reshape(-1, level)[:n - level]
            rel = s - s.max(axis=1, keepdims=True)
            ks = np.arange(level)
            cl, cr = np.array([cnt[x] for x in ks]), np.array([cnt[level - x - 1] for x in ks])
            ii, jj = np.arange(k)[None, :, None], np.arange(k)[None, None, :]
            valid = ((ii < cl[:, None, None]) & (jj < cr[:, None, None])).reshape(-1)
            kk, ii, jj = (a.reshape(-1)[valid] for a in np.broadcast_arrays(ks[:, None, None], ii, jj))
            key[level] = np.zeros((n - level, cnt[level], 3), dtype=np.int64)
            for pos in range(n - level):
                cand = (val[ks, pos][:, :, None] + val[level - ks - 1, pos + ks + 1][:, None, :]) + rel[pos][:, None, None]
                cand = cand.reshape(-1)[valid]
                top = np.argsort(-cand, kind='stable')[:cnt[level]]
                val[level, pos, :cnt[level]] = cand[top]
                key[level][pos] = np.stack([kk[top], ii[top], jj[top]], axis=1)
        count[b] = cnt[n - 1]
        scores[b, :count[b]] = val[n - 1, 0, :count[b]] - np.float32(n)
        for t in range(count[b]):
            rows = _walk(key, n, t)
            spans[b, t, :len(rows)] = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return spans, scores, count
