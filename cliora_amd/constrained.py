"""Parsing under required and forbidden brackets (cliora_constrained_parse).

``DioraBase.cky``, ``posterior.span_posteriors``, ``kbest.kbest_spans`` and ``sample.sample_spans`` answer questions about the
unconditioned distribution over trees, which weighs a tree exp(sum of r over its internal cells), r[cell, k] = s[cell, k] - max_k
s[cell, .].  This conditions it on what the caller knows about the sentence (include/cliora_chart.h): spans that
must be constituents -- the annotated phrases of a caption, a partial bracketing -- and spans that must not be.  Per sentence: the
best tree that qualifies, ``log_prob`` = log_z_c - log_z, the log of the joint probability that every bracket holds at once (which the
per-span marginals cannot give), and the span posteriors given the brackets.  The reference has no counterpart.

    req = brackets_from_entity_labels(batch_map['entity_labels'])       # per sentence [(start, end)], crossing phrases dropped
    cp = constrained_parse(net.diora, pack_brackets(req), marginals=True)    # after a forward; device tensors, nothing synchronised
    trees = net.diora.cky_constrained(req)                              # nested tuples as net.diora.cky(), None where infeasible

A cell [i, j] is allowed iff it crosses no required bracket [s, e] (i < s <= j < e or s < i <= e < j) and equals no forbidden one; in
a binary tree "nothing crosses [s, e]" is "[s, e] is a constituent", so the qualifying trees are the trees built from allowed cells.
``constrained_numpy`` restates the kernel for tests: the best tree in fp32 in the kernel's operation order, the rest in fp64 from the
definitions.

The other two questions about the conditioned distribution (cliora_kbest_spans_constrained, cliora_sample_trees_constrained; DESIGN.md
section 25): its K best trees and draws from it, with their restatements ``constrained_kbest_numpy`` and ``constrained_sample_numpy``.

    kb = constrained_kbest(net.diora, pack_brackets(req), 16)           # ConstrainedKBest: rank 0 is constrained_parse's tree
    ts = constrained_samples(net.diora, pack_brackets(req), 64, seed=7) # every draw keeps the brackets; log_prob given them
"""
import collections

import numpy as np
import torch

from . import _lib, kbest as _kbest, sample as _sample
from .posterior import cell_id, cell_uses, inside_numpy
from .query import ChartQuery, host_copy, per_sentence, sentences_of, walk, walk_spans

MAX_M = 256              # csrc/constrained_kernels.hpp CON_MAX_M: bracket rows per sentence
REQUIRED, FORBIDDEN = 1, 0

# spans (B, L-1, 2) int32 -- the best qualifying tree's n - 1 spans in cky_spans' order, (-1, -1) beyond and where there is none;
# score (B,) fp32 -- the sum of its potentials, as KBest.scores; log_z, log_z_c, log_prob (B,) fp32; feasible (B,) int32; marginals
# (B, C) fp32 or None; status (number of workspaces,) int32 -- sentences with a bad length or a bad row, which the caller must check.
# Device tensors; nothing is synchronised.  (constrained_numpy: the same fields as numpy arrays, fp64 but spans and score; status an int.)
ConstrainedParse = collections.namedtuple('ConstrainedParse', 'spans score log_z log_z_c log_prob feasible marginals status')


def pack_brackets(required, forbidden=None, M=None):
    """Per-sentence lists of (start, end) -- inclusive word positions -- -> the int32 (B, M, 3) tensor of rows (start, end, kind) that
    cliora_constrained_parse takes: a sentence's required spans (kind 1), then its forbidden ones (kind 0), then (-1, -1, -1) rows.
    M: rows per sentence (default: the most any sentence needs); at most 256."""
    required = [list(r) for r in required]
    forbidden = [[] for _ in required] if forbidden is None else [list(f) for f in forbidden]
    if len(forbidden) != len(required):
        raise ValueError('required holds %d sentences, forbidden %d' % (len(required), len(forbidden)))
    need = max([len(r) + len(f) for r, f in zip(required, forbidden)] or [0])
    M = need if M is None else int(M)
    if M < need:
        raise ValueError('M = %d, but a sentence has %d brackets' % (M, need))
    if not 0 <= M <= MAX_M:
        raise ValueError('M must be in 0..%d' % MAX_M)
    out = torch.full((len(required), M, 3), -1, dtype=torch.int32)
    for b, (req, forb) in enumerate(zip(required, forbidden)):
        rows = [(int(s), int(e), REQUIRED) for s, e in req] + [(int(s), int(e), FORBIDDEN) for s, e in forb]
        if rows:
            out[b, :len(rows)] = torch.tensor(rows, dtype=torch.int32)
    return out


def crosses(a, b):
    """Whether spans a = (i, j) and b = (s, e) cross: they overlap and neither holds the other."""
    (i, j), (s, e) = a, b
    return i < s <= j < e or s < i <= e < j


def brackets_from_entity_labels(entity_labels, min_size=2, drop_crossing=True):
    """batch_map['entity_labels'] -> per sentence the list of its phrases as (start, end): a (label, pos, size) entry is the span
    (pos, pos + size - 1); ``None`` entries are skipped and sizes below `min_size` dropped, as ``phrases.entity_rows`` does; a phrase
    listed twice is kept once.  drop_crossing: keep the first-come laminar subset -- a phrase that crosses one kept before it is
    dropped, so the required set is never infeasible by itself."""
    out = []
    for lst in entity_labels:
        keep = []
        for el in lst:
            if el is None:
                continue
            pos, size = int(el[1]), int(el[2])
            span = (pos, pos + size - 1)
            if size < min_size or span in keep:
                continue
            if drop_crossing and any(crosses(span, k) for k in keep):
                continue
            keep.append(span)
        out.append(keep)
    return out


def constrained_parse(diora, brackets, lengths=None, marginals=False, out=None):
    """cliora_constrained_parse on a chart module after its forward.  brackets: an int32 tensor (B, M, 3) of rows (start, end, kind)
    (``pack_brackets``), or None for no bracket at all.  lengths: None (every sentence has L words) or an int32 tensor (B,) for a
    right-padded batch.  marginals: also run the outside pass.  out: a contiguous int32 tensor (B, L-1, 2) on the chart's device to
    decode the spans into.  -> ConstrainedParse."""
    q = ChartQuery(diora)
    spans = q.spans(out)
    q.check_int32('lengths', lengths)
    M = q.check_brackets(brackets)
    score, log_z, log_zc, log_prob = (q.empty(torch.float32) for _ in range(4))
    feasible = q.empty(torch.int32)
    marg = q.empty(torch.float32, q.plan.C) if marginals else None
    status = q.status()
    q.launch('cliora_constrained_parse', per_sentence(q.moved(lengths)), per_sentence(q.moved(brackets)), M, per_sentence(spans),
             per_sentence(score), per_sentence(log_z), per_sentence(log_zc), per_sentence(log_prob), per_sentence(feasible),
             per_sentence(marg), status=status)
    return ConstrainedParse(spans, score, log_z, log_zc, log_prob, feasible, marg, status)


def host_results(cp):
    """A ConstrainedParse's spans, feasible, log_prob and status in ONE device-to-host copy: -> (spans (B, L-1, 2) int32, feasible (B,)
    int32, log_prob (B,) float32, the number of rejected sentences)."""
    spans, feasible, log_prob, status = host_copy(cp.spans, cp.feasible, cp.log_prob, cp.status)
    return spans, feasible, log_prob, int(status.sum())


def refuse_rejected(count, entry='cliora_constrained_parse'):
    """The one message for a non-zero status of cliora_constrained_parse and of the other entries that take brackets."""
    if count:
        raise _lib.ChartLibError('%s rejected %d sentence(s): a length outside the chart, or a bracket that is '
                                 'not 0 <= start <= end < length with kind 0 or 1' % (entry, count))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def bad_row(row, n):
    """Whether a row (start, end, kind) is neither unused (start = -1) nor a bracket of a sentence of n words."""
    s, e, k = (int(v) for v in row)
    return s != -1 and not (0 <= s <= e < n and k in (REQUIRED, FORBIDDEN))


def allowed_cells(n, rows):
    """The definition, a test per (cell, row): -> (allowed[level, pos], required[level, pos]) bool arrays over the triangle of n words."""
    allowed = np.zeros((n, n), dtype=bool)
    required = np.zeros((n, n), dtype=bool)
    rows = [tuple(int(v) for v in r) for r in rows if int(r[0]) != -1]
    for level in range(n):
        for pos in range(n - level):
            span = (pos, pos + level)
            allowed[level, pos] = not any((k == REQUIRED and crosses(span, (s, e))) or (k == FORBIDDEN and span == (s, e))
                                          for s, e, k in rows)
            required[level, pos] = any(k == REQUIRED and span == (s, e) for s, e, k in rows)
    return allowed, required


def _lse(x):
    m = x.max() if x.size else -np.inf
    if not m > -np.inf:
        return -np.inf
    return m + np.log(np.exp(x - m).sum())


def constrained_numpy(pair_s, lengths, brackets, L=None):
    """The kernel restated for tests: `pair_s[level]` (B, L - level, level[, 1]) are the per-split inside scores of the (padded) chart
    of length L (inferred from level 1 when not given), sentence b its first lengths[b] words -- the layout ``posterior_numpy`` takes;
    brackets (B, M, 3) or None.  The best tree in fp32 in the kernel's operation order (cky_kernel's candidate, first maximum wins, a
    disallowed cell at -inf); log_z_c, log_z, log_prob and the marginals in fp64 from the definitions, with the mask by one test per
    (cell, row).  -> ConstrainedParse of numpy arrays as the kernel writes them; status: the number of rejected sentences."""
    lengths, L, brackets = sentences_of(pair_s, lengths, L, brackets)
    Bn, Cc = len(lengths), L * (L + 1) // 2
    spans = np.full((Bn, max(L - 1, 0), 2), -1, dtype=np.int32)
    score = np.full(Bn, -np.inf, dtype=np.float32)
    log_z = np.zeros(Bn, dtype=np.float64)
    log_zc = np.full(Bn, -np.inf, dtype=np.float64)
    log_prob = np.full(Bn, -np.inf, dtype=np.float64)
    feasible = np.zeros(Bn, dtype=np.int32)
    mu = np.zeros((Bn, Cc), dtype=np.float64)
    status = 0
    ninf32 = np.float32(-np.inf)
    for b, n in enumerate(lengths):
        if not 1 <= n <= L or any(bad_row(r, n) for r in brackets[b]):
            status += 1
            continue
        allowed, required = allowed_cells(n, brackets[b])
        # the best tree, fp32
        rel, val, bp = {}, np.full((n, n), ninf32, dtype=np.float32), {}
        val[0, :n] = np.where(allowed[0, :n], np.float32(1.0), ninf32)
        for level in range(1, n):
            s = np.asarray(pair_s[level][b], dtype=np.float32).reshape(-1, level)[:n - level]
            rel[level] = s - s.max(axis=1, keepdims=True)
            k = np.arange(level)
            for pos in range(n - level):
                if not allowed[level, pos]:
                    continue
                cand = (val[k, pos] + val[level - k - 1, pos + k + 1]) + rel[level][pos]
                bp[(level, pos)] = int(np.argmax(cand))
                val[level, pos] = cand[bp[(level, pos)]]
        # the sums, fp64
        r = {}
        al, au = np.full((n, n), -np.inf), np.zeros((n, n))
        al[0, :n] = np.where(allowed[0, :n], 0.0, -np.inf)
        for level in range(1, n):
            s = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
            r[level] = s - s.max(axis=1, keepdims=True)
            k = np.arange(level)
            for pos in range(n - level):
                au[level, pos] = _lse(au[k, pos] + au[level - k - 1, pos + k + 1] + r[level][pos])
                if allowed[level, pos]:
                    al[level, pos] = _lse(al[k, pos] + al[level - k - 1, pos + k + 1] + r[level][pos])
        log_z[b], log_zc[b] = au[n - 1, 0], al[n - 1, 0]
        log_prob[b] = log_zc[b] - log_z[b]
        if not val[n - 1, 0] > ninf32:
            continue
        feasible[b] = 1
        score[b] = val[n - 1, 0] - np.float32(n)
        rows = walk_spans(n, lambda level, pos: bp[(level, pos)])
        spans[b, :len(rows)] = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
        be = np.full((n, n), -np.inf)
        be[n - 1, 0] = 0.0
        for level in range(n - 2, -1, -1):
            for pos in range(n - level):
                if allowed[level, pos]:
                    be[level, pos] = _lse(np.array([be[pl, pp] + al[sl, sp] + r[pl][pp, k] for pl, pp, k, sl, sp in cell_uses(n, level, pos)]))
        for level in range(n):
            for pos in range(n - level):
                if allowed[level, pos]:
                    mu[b, cell_id(L, level, pos)] = 1.0 if required[level, pos] else np.exp(al[level, pos] + be[level, pos] - log_zc[b])
    return ConstrainedParse(spans, score, log_z, log_zc, log_prob, feasible, mu, status)


# ---- the K best trees and sampled trees under brackets ------------------------------------------------------------------------------
class ConstrainedKBest(_kbest.KBest):
    """``kbest.KBest`` of the trees that keep the brackets (cliora_kbest_spans_constrained) plus feasible (B,)
    int32: 0 where no tree qualifies (count 0) and for a rejected sentence.  count (B,): min(k, the number of qualifying trees);
    status counts bad lengths AND bad rows, which the caller must check (``refuse_rejected``).  Device tensors; nothing is synchronised."""

    def __init__(self, spans, scores, count, status, feasible):
        _kbest.KBest.__init__(self, spans, scores, count, status)
        self.feasible = feasible


# ``sample.TreeSamples`` of the draws given the brackets (cliora_sample_trees_constrained) plus log_z_c (B,) fp32 -- the constrained
# log-partition at beta; log_prob = beta * (sum of r over the draw's splits) - log_z_c -- and feasible (B,) int32.  Without a qualifying
# tree: rows -1, log_prob and log_z_c -inf, log_z the real value.  Device tensors; nothing is synchronised.
ConstrainedTreeSamples = collections.namedtuple('ConstrainedTreeSamples', _sample.TreeSamples._fields + ('log_z_c', 'feasible'))


def constrained_kbest(diora, brackets, k, lengths=None):
    """cliora_kbest_spans_constrained on a chart module after its forward: the k best trees (1 .. 16) among those that keep the
    brackets -- an int32 tensor (B, M, 3) of rows (start, end, kind) (``pack_brackets``), or None for no bracket at all, which gives
    ``kbest.kbest_spans``' tensors bit for bit.  Rank 0 is ``constrained_parse``'s tree and score.  lengths: None or an int32 tensor (B,)
    for a right-padded batch.  Allocates the scratch the library asks for.  -> ConstrainedKBest."""
    q = ChartQuery(diora)
    plan, k = q.plan, int(k)
    q.check_int32('lengths', lengths)
    M = q.check_brackets(brackets)
    width = max(k, 0)                                      # a bad k is the library's to refuse, with its message
    spans, scores = q.empty(torch.int32, width, plan.L - 1, 2), q.empty(torch.float32, width)
    count, feasible = q.empty(torch.int32), q.empty(torch.int32)
    status = q.status()
    need = _lib.fn('cliora_kbest_constrained_scratch_bytes')(plan.handle, k, M)
    scratch = torch.empty(need, dtype=torch.uint8, device=q.dev) if need else None
    q.launch('cliora_kbest_spans_constrained', per_sentence(q.moved(lengths)), per_sentence(q.moved(brackets)), M, k, per_sentence(spans),
             per_sentence(scores), per_sentence(count), per_sentence(feasible), scratch, status=status)
    return ConstrainedKBest(spans, scores, count, status, feasible)


def constrained_samples(diora, brackets, S, seed, lengths=None, ids=None, first_sample=0, beta=1.0):
    """cliora_sample_trees_constrained on a chart module after its forward: S trees per sentence (1 .. 2^20, numbered first_sample ..
    first_sample + S - 1) drawn from the posterior over parses given the brackets, at inverse temperature beta.  brackets: as
    ``constrained_kbest`` takes them; None gives ``sample.sample_spans``' spans, log_prob and log_z bit for bit.  lengths, ids: as
    ``sample.sample_spans`` takes them.  -> ConstrainedTreeSamples."""
    q = ChartQuery(diora)
    plan, S = q.plan, int(S)
    q.check_int32('lengths', lengths)
    q.check_int32('ids', ids)
    M = q.check_brackets(brackets)
    ids = q.default_ids(ids)
    width = min(max(S, 0), _sample.MAX_S)                  # a bad S is the library's to refuse, with its message
    spans, log_prob = q.empty(torch.int32, width, plan.L - 1, 2), q.empty(torch.float32, width)
    log_z, log_zc, feasible = q.empty(torch.float32), q.empty(torch.float32), q.empty(torch.int32)
    status = q.status()
    q.launch('cliora_sample_trees_constrained', per_sentence(q.moved(lengths)), per_sentence(ids), per_sentence(q.moved(brackets)), M, S,
             int(seed) & (2 ** 64 - 1), int(first_sample) & (2 ** 64 - 1), float(beta), per_sentence(spans), per_sentence(log_prob),
             per_sentence(log_zc), per_sentence(log_z), per_sentence(feasible), status=status)
    return ConstrainedTreeSamples(spans, log_prob, log_z, status, log_zc, feasible)


# ---- their restatements ---------------------------------------------------------------------------------------------------------------
ConstrainedKBestNumpy = collections.namedtuple('ConstrainedKBestNumpy', 'spans scores count feasible status')
ConstrainedSamplesNumpy = collections.namedtuple('ConstrainedSamplesNumpy', 'spans log_prob log_z log_z_c feasible margin status')


def constrained_kbest_numpy(pair_s, lengths, brackets, k, L=None):
    """cliora_kbest_spans_constrained restated in fp32 in the kernel's operation order, for tests: ``kbest.kbest_numpy`` (its inputs,
    its candidate expression and order: every candidate of a cell at once, (split, left rank, right rank) in key order, a stable sort
    by value descending, the first k) with a cell's count from its children's, 0 at a cell ``allowed_cells`` disallows.  brackets
    (B, M, 3) or None.  -> ConstrainedKBestNumpy as the kernel writes them; status: the number of rejected sentences."""
    k = int(k)
    if not 1 <= k <= _kbest.MAX_K:
        raise ValueError('k must be in 1..%d' % _kbest.MAX_K)
    lengths, L, brackets = sentences_of(pair_s, lengths, L, brackets)
    Bn = len(lengths)
    spans = np.full((Bn, k, max(L - 1, 0), 2), -1, dtype=np.int32)
    scores = np.full((Bn, k), -np.inf, dtype=np.float32)
    count, feasible, status = np.zeros(Bn, dtype=np.int32), np.zeros(Bn, dtype=np.int32), 0
    ii, jj = np.arange(k)[None, :, None], np.arange(k)[None, None, :]
    for b, n in enumerate(lengths):
        if not 1 <= n <= L or any(bad_row(r, n) for r in brackets[b]):
            status += 1
            continue
        allowed, _ = allowed_cells(n, brackets[b])
        cnt = np.zeros((n, n), dtype=np.int64)                               # [level, pos]
        cnt[0, :n] = allowed[0, :n]
        val = np.full((n, n, k), -np.inf, dtype=np.float32)                  # [level, pos, rank]
        val[0, :, 0] = 1.0
        key = {}
        for level in range(1, n):
            s = np.asarray(pair_s[level][b], dtype=np.float32).reshape(-1, level)[:n - level]
            rel = s - s.max(axis=1, keepdims=True)                           # over every split, allowed or not
            ks = np.arange(level)
            key[level] = np.zeros((n - level, k, 3), dtype=np.int64)
            for pos in range(n - level):
                if not allowed[level, pos]:
                    continue
                cl, cr = cnt[ks, pos], cnt[level - ks - 1, pos + ks + 1]
                valid = ((ii < cl[:, None, None]) & (jj < cr[:, None, None])).reshape(-1)
                kk, ci, cj = (a.reshape(-1)[valid] for a in np.broadcast_arrays(ks[:, None, None], ii, jj))
                cand = (val[ks, pos][:, :, None] + val[level - ks - 1, pos + ks + 1][:, None, :]) + rel[pos][:, None, None]
                cand = cand.reshape(-1)[valid]
                top = np.argsort(-cand, kind='stable')[:k]
                cnt[level, pos] = len(top)
                val[level, pos, :len(top)] = cand[top]
                key[level][pos, :len(top)] = np.stack([kk[top], ci[top], cj[top]], axis=1)
        count[b] = cnt[n - 1, 0]
        feasible[b] = count[b] > 0
        scores[b, :count[b]] = val[n - 1, 0, :count[b]] - np.float32(n)
        for t in range(count[b]):
            rows = _kbest._walk(key, n, t)
            spans[b, t, :len(rows)] = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return ConstrainedKBestNumpy(spans, scores, count, feasible, status)


def choose_split(w, u, finite):
    """The draw of one cell: w the weights of its N splits, u its uniform, finite[k] whether both children of split k have a finite
    inside value (a split without has w_k = exactly 0).  split = #{k : c_k <= u c_{N-1}} over the inclusive sums c, clamped to the
    largest k with finite[k] -- N - 1 where every child is finite, ``sample.sample_numpy``'s clamp.  -> (split, margin = the smallest
    |u c_{N-1} - c_k| / c_{N-1})."""
    c = np.cumsum(w)
    thr = u * c[-1]
    k = min(int((c <= thr).sum()), int(np.flatnonzero(finite)[-1]))
    return k, float(np.abs(thr - c).min() / c[-1])


def constrained_sample_numpy(pair_s, lengths, brackets, S, seed, ids=None, first_sample=0, beta=1.0, L=None):
    """cliora_sample_trees_constrained restated in fp64 from the definitions, for tests: ``sample.sample_numpy`` (its inputs, its
    ``draw_uniform`` and ``split_weights``) over the inside table of the cells ``allowed_cells`` allows.  brackets (B, M, 3) or None.
    -> ConstrainedSamplesNumpy as the kernel writes them (log_prob = beta sum r - log_z_c; without a qualifying tree rows -1, log_prob
    and log_z_c -inf; a rejected sentence the same with log_z 0); margin (B, S) as sample_numpy's; status: the rejected sentences."""
    S = int(S)
    if not 1 <= S <= _sample.MAX_S:
        raise ValueError('S must be in 1..%d' % _sample.MAX_S)
    beta = float(beta)
    if not (beta >= 0 and np.isfinite(beta)):
        raise ValueError('beta must be finite and >= 0')
    lengths, L, brackets = sentences_of(pair_s, lengths, L, brackets)
    Bn = len(lengths)
    ids = list(range(Bn)) if ids is None else [int(x) for x in ids]
    spans = np.full((Bn, S, max(L - 1, 0), 2), -1, dtype=np.int32)
    log_prob = np.full((Bn, S), -np.inf, dtype=np.float64)
    log_z, log_zc = np.zeros(Bn, dtype=np.float64), np.full(Bn, -np.inf, dtype=np.float64)
    feasible, status = np.zeros(Bn, dtype=np.int32), 0
    margin = np.full((Bn, S), np.inf, dtype=np.float64)
    samples = np.uint64(int(first_sample) & (2 ** 64 - 1)) + np.arange(S, dtype=np.uint64)
    for b, n in enumerate(lengths):
        if not 1 <= n <= L or any(bad_row(r, n) for r in brackets[b]):
            status += 1
            continue
        allowed, _ = allowed_cells(n, brackets[b])
        r, au = inside_numpy(pair_s, b, n, beta)
        al = np.full((n, n), -np.inf)
        al[0, :n] = np.where(allowed[0, :n], 0.0, -np.inf)
        for level in range(1, n):
            k = np.arange(level)
            for pos in range(n - level):
                if allowed[level, pos]:
                    al[level, pos] = _lse(al[k, pos] + al[level - k - 1, pos + k + 1] + beta * r[level, pos, :level])
        log_z[b], log_zc[b] = au[n - 1, 0], al[n - 1, 0]
        if not log_zc[b] > -np.inf:
            continue
        feasible[b] = 1
        lv, ps = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        u = _sample.draw_uniform(lv[None], ps[None], samples[:, None, None], ids[b], seed)  # [sample, level, pos]
        weights = {}                                  # of the cells a walk can reach: the finite ones
        for s in range(S):
            acc = [0.0]

            def choose(level, pos, _):
                if (level, pos) not in weights:
                    ks = np.arange(level)
                    weights[(level, pos)] = (_sample.split_weights(r, al, level, pos, beta),
                                             (al[ks, pos] + al[level - ks - 1, pos + ks + 1]) > -np.inf)
                w, finite = weights[(level, pos)]
                k, m = choose_split(w, u[s, level, pos], finite)
                margin[b, s] = min(margin[b, s], m)
                acc[0] += beta * r[level, pos, k]
                return k, None, None
            rows = [row[:2] for row in walk(n, choose)]
            spans[b, s, :len(rows)] = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
            log_prob[b, s] = acc[0] - log_zc[b]
    return ConstrainedSamplesNumpy(spans, log_prob, log_z, log_zc, feasible, margin, status)
