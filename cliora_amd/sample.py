"""Binary trees sampled from the chart's posterior over parses (cliora_sample_trees).

The CKY decode (``DioraBase.cky``) returns the mode of the distribution that weighs a tree exp(sum of r over its internal cells),
r[cell, k] = s[cell, k] - max_k s[cell, .]; ``posterior.span_posteriors`` its marginals and log_z, ``kbest.kbest_spans`` its 16
heaviest trees.  This draws from it (include/cliora_chart.h), at an inverse temperature beta >= 0 that scales
r: beta = 1 is the posterior itself, beta = 0 uniform over the Catalan(n - 1) trees.  The reference has no counterpart.

    ts = sample_spans(net.diora, 64, seed=7)             # after a forward; device tensors, nothing synchronised
    freq = span_frequencies(ts.spans, L)                 # (B, C): tends to span_posteriors(net.diora).marginals at beta = 1
    trees = net.diora.sample_trees(64, seed=7)           # per sentence [(nested tuples as net.diora.cky(), log_prob)]

The draw is the contract: top-down from the root, at cell (level, pos) with N = level splits w_k = exp(a[left_k] + a[right_k] + beta
r_k - a[cell]) over the fp64 inside table a, c_k = w_0 + .. + w_k, split = #{k : c_k <= u c_{N-1}} clamped to N - 1, and u = (m + 0.5)
2^-53 from Philox4x32-10 at counter (level * 256 + pos, sample_lo, sample_hi, sentence id) under key (seed_lo, seed_hi).  A draw
depends on (seed, sentence id, sample index, cell) and the sentence's scores alone.  ``sample_numpy`` restates it in fp64 for tests.
The same draws from the distribution given required and forbidden brackets: ``constrained.constrained_samples``.
"""
import collections
import numpy as np
import torch

from .posterior import inside_numpy
from .query import ChartQuery, per_sentence, sentences_of, walk

MAX_S = 1 << 20          # csrc/sample_kernels.hpp SAMPLE_MAX_S

# spans (B, S, L-1, 2) int32 -- sample s's n - 1 spans in cky_spans' order, (-1, -1) beyond; log_prob (B, S) fp32 -- beta * (sum of r
# over the sample's splits) - log_z; log_z (B,) fp32; status (number of workspaces,) int32 -- lengths outside [1, L], which the caller
# of a mixed-length run must check.  Device tensors; nothing is synchronised.
TreeSamples = collections.namedtuple('TreeSamples', 'spans log_prob log_z status')


def sample_spans(diora, S, seed, lengths=None, ids=None, first_sample=0, beta=1.0):
    """cliora_sample_trees on a chart module after its forward.  S: 1 .. 2^20 samples per sentence, numbered first_sample ..
    first_sample + S - 1; seed: 64 bits.  lengths: None (every sentence has L words) or an int32 tensor (B,) for a right-padded batch.
    ids: None or an int32 tensor (B,) of the caller's sentence numbers (None: the row in the chart, over every workspace).
    -> TreeSamples."""
    q = ChartQuery(diora)
    plan, S = q.plan, int(S)
    q.check_int32('lengths', lengths)
    q.check_int32('ids', ids)
    ids = q.default_ids(ids)
    width = min(max(S, 0), MAX_S)                          # a bad S is the library's to refuse, with its message
    spans, log_prob, log_z = q.empty(torch.int32, width, plan.L - 1, 2), q.empty(torch.float32, width), q.empty(torch.float32)
    status = q.status()
    q.launch('cliora_sample_trees', per_sentence(q.moved(lengths)), per_sentence(ids), S, int(seed) & (2 ** 64 - 1),
             int(first_sample) & (2 ** 64 - 1), float(beta), per_sentence(spans), per_sentence(log_prob), per_sentence(log_z), status=status)
    return TreeSamples(spans, log_prob, log_z, status)


def span_frequencies(spans, L):
    """(B, S, L-1, 2) sampled spans -> (B, C) float32: the share of a sentence's samples that hold each cell, in the cell order of
    inside_s -- what ``SpanPosteriors.marginals`` holds on the internal cells (it tends to them at beta = 1); 0 at the leaves, which
    no sample lists.  A torch tensor stays on its device; a numpy array gives a numpy array."""
    is_np = isinstance(spans, np.ndarray)
    t = torch.from_numpy(spans) if is_np else spans
    B, S = t.shape[0], t.shape[1]
    Cc = L * (L + 1) // 2
    start, end = t[..., 0].reshape(B, -1).long(), t[..., 1].reshape(B, -1).long()
    rem = L - (end - start)
    cell = torch.where(start >= 0, Cc - rem * (rem + 1) // 2 + start, torch.full_like(start, Cc))     # padding rows: a bin of their own
    freq = torch.zeros((B, Cc + 1), dtype=torch.float32, device=t.device)
    freq.scatter_add_(1, cell, torch.ones_like(cell, dtype=torch.float32))
    freq = freq[:, :Cc] / max(S, 1)
    return freq.numpy() if is_np else freq


_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of counters (c0, c1, c2, c3) (arrays, broadcast) under key (k0, k1): the four output words as uint64 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _U32 for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]              # 32 x 32 bits: no overflow in 64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c


def draw_uniform(level, pos, sample, sentence_id, seed):
    """u of cell (level, pos) for sample index `sample` (arrays broadcast) of sentence `sentence_id` under `seed`: float64 in (0, 1)."""
    sample = np.asarray(sample, dtype=np.uint64)
    seed = int(seed) & (2 ** 64 - 1)
    x = philox4x32_10(np.asarray(level, dtype=np.uint64) * np.uint64(256) + np.asarray(pos, dtype=np.uint64), sample & _U32,
                      sample >> np.uint64(32), np.uint64(int(sentence_id) & 0xFFFFFFFF), seed & 0xFFFFFFFF, seed >> 32)
    m = ((x[0] >> np.uint64(5)) << np.uint64(26)) | (x[1] >> np.uint64(6))
    return (m.astype(np.float64) + 0.5) * 2.0 ** -53


def split_weights(r, al, level, pos, beta):
    """w_k of cell (level, pos), k = 0 .. level - 1: the conditional probabilities of its splits (they sum to 1 up to rounding)."""
    k = np.arange(level)
    return np.exp(al[k, pos] + al[level - k - 1, pos + k + 1] + beta * r[level, pos, :level] - al[level, pos])


def sample_numpy(pair_s, lengths, S, seed, ids=None, first_sample=0, beta=1.0, L=None):
    """The sampler restated in fp64 from the definitions, for tests: `pair_s[level]` (B, L - level, level[, 1]) are the per-split
    inside scores of the (padded) chart of length L (inferred from level 1 when not given), sentence b its first lengths[b] words --
    the layout ``posterior_numpy`` takes.  -> (spans (B, S, L-1, 2) int32, log_prob (B, S) float64, log_z (B,) float64, margin (B, S)
    float64) as the kernel writes them (a length outside [1, L]: rows -1, zeros); margin[b, s] is the smallest |u c_{N-1} - c_k| /
    c_{N-1} over the sample's decisions and all k (inf when it has none): how far the sample is from drawing another tree."""
    S = int(S)
    if not 1 <= S <= MAX_S:
        raise ValueError('S must be in 1..%d' % MAX_S)
    beta = float(beta)
    if not (beta >= 0 and np.isfinite(beta)):
        raise ValueError('beta must be finite and >= 0')
    lengths, L = sentences_of(pair_s, lengths, L)
    ids = list(range(len(lengths))) if ids is None else [int(x) for x in ids]
    spans = np.full((len(lengths), S, max(L - 1, 0), 2), -1, dtype=np.int32)
    log_prob = np.zeros((len(lengths), S), dtype=np.float64)
    log_z = np.zeros(len(lengths), dtype=np.float64)
    margin = np.full((len(lengths), S), np.inf, dtype=np.float64)
    samples = np.uint64(int(first_sample) & (2 ** 64 - 1)) + np.arange(S, dtype=np.uint64)
    for b, n in enumerate(lengths):
        if not 1 <= n <= L:
            continue
        r, al = inside_numpy(pair_s, b, n, beta)
        log_z[b] = al[n - 1, 0]
        cum = {(level, pos): np.cumsum(split_weights(r, al, level, pos, beta)) for level in range(1, n) for pos in range(n - level)}
        lv, ps = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        u = draw_uniform(lv[None], ps[None], samples[:, None, None], ids[b], seed)          # [sample, level, pos]
        for s in range(S):
            acc = [0.0]

            def choose(level, pos, _):
                c = cum[(level, pos)]
                thr = u[s, level, pos] * c[-1]
                k = min(int((c <= thr).sum()), level - 1)
                margin[b, s] = min(margin[b, s], float(np.abs(thr - c).min() / c[-1]))
                acc[0] += beta * r[level, pos, k]
                return k, None, None
            tree = [row[:2] for row in walk(n, choose)]
            spans[b, s, :len(tree)] = np.asarray(tree, dtype=np.int32).reshape(-1, 2)
            log_prob[b, s] = acc[0] - log_z[b]
    return spans, log_prob, log_z, margin
