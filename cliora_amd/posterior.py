"""Span posteriors, log-partition and minimum-Bayes-risk trees from the chart's per-split scores (cliora_span_posteriors).

The CKY decode (``DioraBase.cky``) is max-product over the potentials r[cell, k] = s[cell, k] - max_k s[cell, .]; this is the
sum-product pass over the same potentials (include/cliora_chart.h): how sure the parser is of a bracket
(``marginals``), how peaked the distribution over trees is (``log_z``: 0 when one tree holds all the mass, log Catalan(n - 1) when
every split of every cell ties), and the tree with the most expected correct brackets (``mbr=True``).  The reference has no
counterpart; the distribution is the one whose mode its parser returns.

    post = span_posteriors(net.diora)                    # after a forward; device tensors, nothing synchronised
    table = marginal_table(post.marginals, L)            # (B, L, L): table[b, start, end]
    trees = net.diora.mbr()                              # nested tuples, as net.diora.cky()

``posterior_numpy`` (fp64, from the definitions) and ``mbr_numpy`` (fp32, the kernel's operation order) restate the kernel for
tests, as ``ragged.decode_ragged_numpy`` restates the ragged decode.
"""
import numpy as np
import torch

from . import _lib
from .query import ChartQuery, per_sentence, sentences_of, walk_spans


def cell_id(L, level, pos):
    """Cell (level, pos) -- words [pos, pos + level] -- in the cell order of inside_s for a chart of length L."""
    rem = L - level
    return L * (L + 1) // 2 - rem * (rem + 1) // 2 + pos


def cell_uses(n, level, pos):
    """The n - 1 - level uses of cell (level, pos) in a sentence of n words, in the kernel's order, as closed forms:
    -> [(parent level, parent pos, the parent's split, sibling level, sibling pos)]: first as a left child with the right sibling
    (j, pos + level + 1), then as a right child with the left sibling (j, pos - j - 1)."""
    uses = [(level + j + 1, pos, level, j, pos + level + 1) for j in range(n - 1 - pos - level)]
    uses += [(level + j + 1, pos - j - 1, j, j, pos - j - 1) for j in range(pos)]
    return uses


class SpanPosteriors(object):
    """marginals (B, C) fp32, log_z (B,) fp32, status (number of workspaces,) int32 -- lengths outside [1, L], which the caller of
    a mixed-length run must check -- and, with mbr=True, spans (B, L-1, 2) / split (B, C) int32 of the MBR tree (else None).  Device
    tensors; nothing is synchronised."""

    def __init__(self, marginals, log_z, spans, split, status, L):
        self.marginals, self.log_z, self.spans, self.split, self.status, self.L = marginals, log_z, spans, split, status, L

    def table(self):
        return marginal_table(self.marginals, self.L)


def span_posteriors(diora, lengths=None, mbr=False, out=None):
    """cliora_span_posteriors on a chart module after its forward.  lengths: None (every sentence has L words) or an int32 tensor
    (B,) for a right-padded batch; mbr: also decode the MBR tree.  out: a contiguous int32 tensor (B, L-1, 2) on the chart's device
    to decode the MBR spans into (cliora_amd.evaluate: its output buffer).  -> SpanPosteriors."""
    q = ChartQuery(diora)
    plan = q.plan
    q.check_int32('lengths', lengths)
    spans = q.spans(out) if mbr else None
    marg, log_z = q.empty(torch.float32, plan.C), q.empty(torch.float32)
    split = q.empty(torch.int32, plan.C) if mbr else None
    status = q.status(zeroed=False)
    need = _lib.fn('cliora_span_posteriors_scratch_bytes')(plan.handle)
    scratch = torch.empty(need, dtype=torch.uint8, device=q.dev) if need else None
    q.launch('cliora_span_posteriors', per_sentence(q.moved(lengths)), per_sentence(marg), per_sentence(log_z), per_sentence(split),
             per_sentence(spans), scratch, status=status)
    return SpanPosteriors(marg, log_z, spans, split, status, plan.L)


def marginal_table(marginals, L):
    """(B, C) posteriors in cell order -> dense (B, L, L) indexed [start, end] (end inclusive, as the spans of cky_spans); 0 below
    the diagonal.  A torch tensor stays on its device; a numpy array gives a numpy array."""
    is_np = isinstance(marginals, np.ndarray)
    m = torch.from_numpy(marginals) if is_np else marginals
    start, end = torch.triu_indices(L, L, device=m.device)
    level = end - start
    rem = L - level
    cell = L * (L + 1) // 2 - rem * (rem + 1) // 2 + start
    table = torch.zeros((m.shape[0], L, L), dtype=m.dtype, device=m.device)
    table[:, start, end] = m[:, cell]
    return table.numpy() if is_np else table


def _logsumexp(x):
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


def inside_numpy(pair_s, b, n, beta=1.0):
    """Sentence b's first n words in fp64: -> (r[level, pos, split] = s - max_k s, al[level, pos] = the inside table under beta r;
    beta = 1: the posteriors', other values: cliora_amd.sample)."""
    r = np.zeros((n, n, max(n, 1)), dtype=np.float64)
    al = np.zeros((n, n), dtype=np.float64)
    for level in range(1, n):
        s = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
        r[level, :n - level, :level] = s - s.max(axis=1, keepdims=True)
        k = np.arange(level)
        for pos in range(n - level):
            t = al[k, pos] + al[level - k - 1, pos + k + 1] + beta * r[level, pos, :level]
            al[level, pos] = _logsumexp(t)
    return r, al


def posterior_numpy(pair_s, lengths, L=None):
    """The posteriors restated in fp64 from the definitions, for tests: `pair_s[level]` (B, L - level, level[, 1]) are the per-split
    inside scores of the (padded) chart of length L (inferred from level 1 when not given), sentence b its first lengths[b] words.
    -> (marginals (B, C) float64, 0 outside each triangle; log_z (B,) float64).  Tables indexed [level, pos]; the uses of a cell are
    those of ``cell_uses``, taken a sibling level j at a time."""
    lengths, L = sentences_of(pair_s, lengths, L)
    Cc = L * (L + 1) // 2
    mu = np.zeros((len(lengths), Cc), dtype=np.float64)
    log_z = np.zeros(len(lengths), dtype=np.float64)
    for b, n in enumerate(lengths):
        r, al = inside_numpy(pair_s, b, n)
        be = np.zeros((n, n), dtype=np.float64)
        for level in range(n - 2, -1, -1):
            for pos in range(n - level):
                j = np.arange(n - 1 - pos - level)                      # right siblings (j, pos + level + 1): the parent's split is `level`
                right = be[level + j + 1, pos] + al[j, pos + level + 1 + 0 * j] + r[level + j + 1, pos, level]
                j = np.arange(pos)                                      # left siblings (j, pos - j - 1): the parent's split is j
                left = be[level + j + 1, pos - j - 1] + al[j, pos - j - 1] + r[level + j + 1, pos - j - 1, j]
                be[level, pos] = _logsumexp(np.concatenate([right, left]))
        log_z[b] = al[n - 1, 0] if n else 0.0
        for level in range(n):
            c0 = cell_id(L, level, 0)
            mu[b, c0:c0 + n - level] = np.exp(al[level, :n - level] + be[level, :n - level] - log_z[b])
    return mu, log_z


def mbr_numpy(marginals, lengths, L):
    """The MBR decode restated in fp32 in the kernel's operation order, for tests: v[leaf] = 0, v[cell] = max_k(v[left] + v[right])
    + mu[cell], first maximum wins.  -> (per sentence the list of (start, end), children before parents; split (B, C) int32, -1 at
    the leaves and outside each triangle)."""
    marginals = np.asarray(marginals, dtype=np.float32)
    split = np.full(marginals.shape, -1, dtype=np.int32)
    out = []
    for b, n in enumerate(int(x) for x in lengths):
        val = {(0, p): np.float32(0.0) for p in range(n)}
        bp = {}
        for level in range(1, n):
            for pos in range(n - level):
                cand = np.array([val[(k, pos)] + val[(level - k - 1, pos + k + 1)] for k in range(level)], dtype=np.float32)
                k = int(np.argmax(cand))
                val[(level, pos)] = np.float32(cand[k] + marginals[b, cell_id(L, level, pos)])
                bp[(level, pos)] = k
                split[b, cell_id(L, level, pos)] = k
        out.append(walk_spans(n, lambda level, pos: bp[(level, pos)]))
    return out, split
