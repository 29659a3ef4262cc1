"""The exact word-prediction loss over the whole vocabulary (include/cliora_chart.h: cliora_vocab_nll_forward / _backward).

The reference trains and reports a sampled loss (cliora/net/trainer.py:46-78: the positive against k_neg negatives drawn by word
frequency), whose value depends on k_neg and on the draw.  The exact quantity for token t with outside vector o_t is

    s[t][v] = <mat^T o_t, emb[v]>            (trainer.py:58-66, for every word v)
    nll[t]  = logsumexp_v s[t][v] - s[t][tok_t]

the held-out likelihood of the masked word, comparable across runs, vocabularies and checkpoints.  The logits are never written
(T x V is 4.5e10 floats for a test split at V = 400k): the kernels keep a running log-sum-exp per token, and the backward
recomputes the probabilities from the saved lse.

    loss, nll, lse, tgt, rank, status = vocab_nll(Q, K, tokens, weights=None, want_rank=False)      # Q = outside rows @ mat
    m = word_prediction(net, batches)        # {'nll', 'perplexity', 'acc@k', 'mrr', 'tokens', 'out_of_range'}

vocab_nll_numpy is the fp64 restatement the tests compare with.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream, device_guard


def supported(Q, K, tokens, weights=None):
    """True when the kernels take these tensors as they are: fp32 Q, K and weights, int64 tokens, all on a GPU."""
    floats = [t for t in (Q, K, weights) if t is not None]
    return all(t.is_cuda and t.dtype == torch.float32 for t in floats) and tokens.is_cuda and tokens.dtype == torch.int64


def workspace_bytes(T, V, E, want_backward=False):
    return _lib.fn('cliora_vocab_workspace_bytes')(T, V, E, int(bool(want_backward)))


def _rows(t):
    """A 2-d fp32 tensor whose rows are contiguous (any leading dimension >= the width is taken as it is)."""
    t = t.float()
    return t if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


class VocabNLL(torch.autograd.Function):
    """(Q, K, tokens, weights, want_rank) -> (loss, nll, lse, tgt, rank, status); only `loss` is differentiable, and lse (with the part of it
    that fp32 drops) is all the backward keeps of the forward.  Both calls run on the current stream."""

    @staticmethod
    def forward(ctx, Q, K, tokens, weights, want_rank):
        Q, K = _rows(Q), _rows(K)
        tokens, weights = tokens.contiguous(), weights.contiguous().float()
        T, E = Q.shape
        V = K.shape[0]
        if K.shape[1] != E or tokens.shape != (T,) or weights.shape != (T,):
            raise ValueError('vocab_nll: Q %s, K %s, tokens %s, weights %s do not fit' % (tuple(Q.shape), tuple(K.shape), tuple(tokens.shape),
                                                                                        tuple(weights.shape)))
        dev = Q.device
        with device_guard(Q):
            loss = torch.empty(1, device=dev)
            nll, lse, lse_lo, tgt = (torch.empty(T, device=dev) for _ in range(4))
            rank = torch.empty(T, device=dev, dtype=torch.int32) if want_rank else None
            status = torch.empty(1, device=dev, dtype=torch.int32)
            nb = workspace_bytes(T, V, E)                # the backward allocates its own: nothing of this one is needed there
            ws = torch.empty(max(nb, 1), device=dev, dtype=torch.uint8)
            _lib.call('cliora_vocab_nll_forward', T, V, E, ptr(Q), _ld(Q), ptr(K), _ld(K), ptr(tokens), ptr(weights), ptr(loss), ptr(nll), ptr(lse),
                      ptr(lse_lo), ptr(tgt), ptr(rank), ptr(status), ptr(ws), nb, stream())
        ctx.save_for_backward(Q, K, tokens, weights, lse, lse_lo)
        outs = (nll, lse, tgt, status) + ((rank,) if want_rank else ())
        ctx.mark_non_differentiable(*outs)
        return loss.reshape(()), nll, lse, tgt, rank, status

    @staticmethod
    def backward(ctx, g, *unused):
        Q, K, tokens, weights, lse, lse_lo = ctx.saved_tensors
        T, E = Q.shape
        V = K.shape[0]
        with device_guard(Q):
            g = g.contiguous().float().reshape(1)
            dQ = torch.empty((T, E), device=Q.device) if ctx.needs_input_grad[0] else None
            dK = torch.empty((V, E), device=Q.device) if ctx.needs_input_grad[1] else None
            nb = workspace_bytes(T, V, E, True)
            ws = torch.empty(max(nb, 1), device=Q.device, dtype=torch.uint8)
            _lib.call('cliora_vocab_nll_backward', T, V, E, ptr(Q), _ld(Q), ptr(K), _ld(K), ptr(tokens), ptr(weights), ptr(lse), ptr(lse_lo), ptr(g),
                      ptr(dQ), E, ptr(dK), E, ptr(ws), nb, stream())
        return dQ, dK, None, None, None


def _torch_nll(Q, K, tokens, weights, want_rank):
    """The same quantities in torch (CPU, or tensors the kernels do not take), with the edge semantics of the kernels."""
    T, V = Q.shape[0], K.shape[0]
    logits = Q @ K.t()
    ok = (tokens >= 0) & (tokens < V)
    safe = torch.where(ok, tokens, torch.zeros_like(tokens))
    lse = torch.logsumexp(logits, dim=1) if T else logits.new_zeros(0)
    tgt = logits.gather(1, safe.view(-1, 1)).view(-1) if T else logits.new_zeros(0)
    nan = torch.full_like(tgt, float('nan'))
    tgt = torch.where(ok, tgt, nan)
    nll = torch.where(ok, lse - tgt, nan)
    sel = ok & (weights != 0)
    loss = (weights[sel] * nll[sel]).sum()
    rank = None
    if want_rank:
        idx = torch.arange(V, device=Q.device).view(1, -1)
        lo = torch.where(torch.isnan(logits), torch.full_like(logits, -float('inf')), logits)      # NaN lowest (a -inf ties with it: not told apart here)
        t = lo.gather(1, safe.view(-1, 1))
        before = (lo > t) | ((lo == t) & (idx < safe.view(-1, 1)))
        rank = torch.where(ok, before.sum(1), torch.full_like(safe, -1)).to(torch.int32)
    status = (~ok).sum().to(torch.int32).reshape(1)
    return loss, nll.detach(), lse.detach(), tgt.detach(), rank, status


def vocab_nll(Q, K, tokens, weights=None, want_rank=False):
    """Q (T, E): the projected outside rows o_t . mat; K (V, E): the embedding table; tokens (T,) int64; weights (T,) or None (1 / T:
    the mean).  -> (loss 0-d, in the graph of Q and K; nll, lse, tgt (T,); rank (T,) int32 or None; status (1,) int32: the number of
    ids outside [0, V)), all on the device of Q.  On the GPU with fp32 / int64 tensors this is the HIP path; elsewhere torch."""
    T = Q.shape[0]
    tokens = tokens.reshape(-1)
    if weights is None:
        weights = torch.full((T,), 1.0 / max(T, 1), device=Q.device, dtype=torch.float32 if Q.is_cuda else Q.dtype)
    if supported(Q, K, tokens, weights):
        return VocabNLL.apply(Q, K, tokens, weights, bool(want_rank))
    return _torch_nll(Q, K, tokens, weights.to(Q.dtype), want_rank)


def _order_key(score):
    """cliora_knn_ip's order of fp64 scores as sortable numbers: NaN below every number, -0 as +0."""
    s = np.where(np.isnan(score), -np.inf, score) + 0.0
    return s, np.isnan(score)


def vocab_nll_numpy(Q, K, tokens, weights=None, want_grad=False, g=1.0):
    """The fp64 restatement: a dict of loss, nll, lse, tgt, rank, status and, with want_grad, dQ and dK (the analytic gradient of
    g * loss), with the edge semantics of the kernels: an id outside [0, V) is counted in status, gets nll = tgt = NaN and rank = -1 and
    adds nothing to loss or gradients; a token with weight 0 adds nothing by selection; rank counts the words that order before the
    target by descending score, ascending index on ties, NaN lowest."""
    Q, K = np.asarray(Q, dtype=np.float64), np.asarray(K, dtype=np.float64)
    tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)
    T, V = Q.shape[0], K.shape[0]
    w = np.full(T, 1.0 / max(T, 1)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    ok = (tokens >= 0) & (tokens < V)
    safe = np.where(ok, tokens, 0)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        s = Q @ K.T
        m = np.max(np.where(np.isnan(s), -np.inf, s), axis=1, keepdims=True) if T else np.zeros((0, 1))
        m = np.where(np.isfinite(m), m, 0.0)
        lse = (m + np.log(np.sum(np.exp(s - m), axis=1, keepdims=True))).reshape(-1)
        tgt = np.where(ok, s[np.arange(T), safe], np.nan)
        nll = np.where(ok, lse - tgt, np.nan)
        sel = ok & (w != 0)
        loss = float(np.sum(w[sel] * nll[sel]))
        key, isnan = _order_key(s)
        tk, tn = key[np.arange(T), safe][:, None], isnan[np.arange(T), safe][:, None]
        idx = np.arange(V)[None, :]
        # v before the target: a number before a NaN; among numbers the larger, among equals (and among NaNs) the smaller index
        before = np.where(tn, ~isnan | (idx < safe[:, None]), ~isnan & ((key > tk) | ((key == tk) & (idx < safe[:, None]))))
        rank = np.where(ok, before.sum(axis=1), -1).astype(np.int32)
        out = {'loss': loss, 'nll': nll, 'lse': lse, 'tgt': tgt, 'rank': rank, 'status': int((~ok).sum())}
        if want_grad:
            c = np.exp(s - lse[:, None])
            c[np.arange(T), safe] -= 1.0
            c = np.where(sel[:, None], c * w[:, None], 0.0)
            Qs = np.where(sel[:, None], Q, 0.0)
            out['dQ'] = g * (c @ K)
            out['dK'] = g * (c.T @ Qs)
    return out


def word_prediction(net, batches, ks=(1, 5, 10)):
    """Held-out word prediction of a harness.Net over batch_map dicts (as evaluate.evaluate takes them): the eval forward per batch,
    the leaf rows of outside_h, one torch.mm with the loss's `mat`, one vocab_nll call per batch and ONE host copy at the end.
    -> {'nll': mean nll per token (nats), 'perplexity': exp of it, 'acc@k': {k: share of tokens whose word is among the k best},
        'mrr': mean 1 / (rank + 1), 'tokens': tokens counted, 'out_of_range': ids outside the table (not counted)}."""
    head = net.reconstruct_softmax_loss
    table = head.embeddings.weight
    dev = table.device
    was_training, had_outside = net.training, net.diora.outside
    net.diora.outside = True
    net.eval()
    nlls, ranks = [], []
    try:
        with torch.no_grad():
            for bm in batches:
                tokens = bm['sentences'].to(dev)
                obj = bm.get('obj_feats') if net.obj_feats else None
                net(tokens, obj.to(dev) if obj is not None else None, None, compute_loss=False)
                L = tokens.shape[1]
                rows = net.diora.outside_h[:, :L].reshape(-1, head.mat.shape[0])
                _, nll, _, _, rank, _ = vocab_nll(torch.mm(rows, head.mat), table, tokens.reshape(-1), want_rank=True)
                nlls.append(nll)
                ranks.append(rank)
    finally:                                 # the caller's mode and pass selection, as they were
        net.train(was_training)
        net.diora.outside = had_outside
    if not nlls:
        return {'nll': float('nan'), 'perplexity': float('nan'), 'acc@k': {k: float('nan') for k in ks}, 'mrr': float('nan'), 'tokens': 0,
                'out_of_range': 0}
    both = torch.stack([torch.cat(nlls).double(), torch.cat(ranks).double()]).cpu().numpy()        # the one host copy
    return word_prediction_metrics(both[0], both[1].astype(np.int64), ks)


def word_prediction_metrics(nll, rank, ks=(1, 5, 10)):
    """The metrics of word_prediction from per-token nll and rank on the host (rank -1: an id outside the table, left out)."""
    ok = rank >= 0
    n = int(ok.sum())
    mean = float(np.mean(nll[ok])) if n else float('nan')
    perplexity = mean if math.isnan(mean) else math.exp(mean) if mean < 700 else float('inf')       # NaN stays NaN; exp overflows above 709
    return {'nll': mean, 'perplexity': perplexity,
            'acc@k': {int(k): float(np.mean(rank[ok] < k)) if n else float('nan') for k in ks},
            'mrr': float(np.mean(1.0 / (rank[ok] + 1.0))) if n else float('nan'), 'tokens': n, 'out_of_range': int((~ok).sum())}
