"""Training on brackets: the loss -log_prob of ``cliora_constrained_parse`` and its gradient (cliora_bracket_grad).

``constrained.constrained_parse`` says how likely the model finds a set of brackets, jointly: log_prob = log_z_c - log_z under the
distribution over binary trees that weighs a tree exp(sum of r over its internal cells), r[cell, k] = s[cell, k] - max_k s[cell, .].
This module makes that number trainable: distant supervision from the phrases a caption is annotated with, the log-likelihood of a
gold tree (require its n - 2 inner brackets), penalties on forbidden brackets -- one loss.

    net.diora(x_span, x_word)                                           # a training forward, L <= 64
    req = brackets_from_entity_labels(batch_map['entity_labels'])
    loss = recon + 0.5 * net.diora.bracket_nll(req)                     # or bracket_nll(net.diora, pack_brackets(req))
    loss.backward()

The gradient with respect to the per-split inside scores is a difference of two edge-marginal tables, which the kernel forms in fp64
(csrc/bracket_grad_kernels.hpp) and writes in the layout of the split-score rows of the forward workspace.

The hand-off to the chart.  The split scores are no output of the chart's autograd node (they live in the forward workspace), so the
cotangent cannot travel along an autograd edge.  ``bracket_log_prob`` is an autograd Function whose formal input is the chart's
``inside_s``: autograd therefore runs its backward before ``ChartFunction.backward`` of the same forward, and runs that backward even
when the bracket loss is the only loss (it gets a zero cotangent for inside_s).  The Function's backward launches
cliora_bracket_grad with weights = the incoming cotangent and ADDS the result into the one-element slot that the forward's workspace
holder (``diora.ChartWorkspaces.split_cot``) shares with the chart node's ctx; the chart node takes the slot's content, empties it and
calls cliora_chart_backward_split (cliora_chart_backward when the slot is empty).  Hence: other losses' cotangents sum with it inside
the library, two bracket_log_prob calls on one forward add up in the slot, and since every forward makes a new holder, a cotangent
can never reach the backward of another forward.  (A backward that stops short of the chart node -- ``torch.autograd.grad`` with
respect to inside_s itself -- leaves its cotangent in the slot of that forward.)  Refused with a ChartLibError before any launch: a
module that has run no forward, a forward under ``no_grad`` / in eval mode without gradients (no backward state was kept), a plan of
L > 64 (the backward stops at 64 words), a TreeLSTM module (its backward takes no such input), and a module whose
``workspace_slices`` yields more than one workspace (one chart node, one slot: run the loss per forward).
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr_or_null as _p, stream as _stream
from .constrained import allowed_cells, bad_row
from .diora import workspace_slices

# d_split (cliora_plan_split_score_count * workspaces,) fp32 -- G in the layout of the inside split-score rows; log_prob (B,) fp32;
# feasible (B,) int32; status (number of workspaces,) int32.  Device tensors; nothing is synchronised.
BracketGrad = collections.namedtuple('BracketGrad', 'd_split log_prob feasible status')


class _ChartView(object):
    """What bracket_grad reads of a chart module: the plan and the forward's holder (workspace + slot), kept by the loss's node."""
    __slots__ = ('_plan', '_wss')

    def __init__(self, plan, wss):
        self._plan, self._wss = plan, wss


def split_score_count(plan):
    return int(_lib.fn('cliora_plan_split_score_count')(plan.handle))


def split_rows_by_level(plan, d_split):
    """A d_split buffer of ONE workspace -> {level: (B, L - level, level)} views, the layout ``bracket_grad_numpy`` returns."""
    out, base = {}, 0
    for level in range(1, plan.L):
        n = plan.B * (plan.L - level) * level
        out[level] = d_split[base:base + n].view(plan.B, plan.L - level, level)
        base += n
    return out


def _check_brackets(brackets, nsent):
    if brackets is None:
        return 0
    if brackets.dtype != torch.int32 or brackets.dim() != 3 or brackets.shape[0] != nsent or brackets.shape[2] != 3:
        raise ValueError('brackets must be int32 (%d, M, 3)' % nsent)
    return int(brackets.shape[1])                          # a bad M is the library's to refuse, with its message


def bracket_grad(diora, brackets, weights=None, lengths=None):
    """cliora_bracket_grad on a chart module after its forward (any forward: this call needs no backward state).  brackets: int32
    (B, M, 3) (``constrained.pack_brackets``) or None; weights: fp32 (B,) or None = 1; lengths: int32 (B,) or None.  One d_split buffer
    per workspace of ``workspace_slices``, back to back.  -> BracketGrad of device tensors; nothing is synchronised."""
    if diora._plan is None:
        raise _lib.ChartLibError('bracket_grad: the module has run no forward')
    plan, parts = diora._plan, workspace_slices(diora)
    nws, B = len(parts), plan.B
    dev = parts[0][0].device
    M = _check_brackets(brackets, B * nws)
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.numel() != B * nws):
        raise ValueError('lengths must be int32, one per sentence of the chart (%d)' % (B * nws))
    if weights is not None and weights.numel() != B * nws:
        raise ValueError('weights must hold one value per sentence of the chart (%d)' % (B * nws))
    with torch.cuda.device(dev):
        count = split_score_count(plan)
        lengths = lengths.to(dev).contiguous() if lengths is not None else None
        brackets = brackets.to(dev).contiguous() if brackets is not None else None
        weights = weights.to(dev).contiguous().float().reshape(-1) if weights is not None else None
        buf = torch.empty(max(count * nws, 1), dtype=torch.float32, device=dev)      # (one word: no row, but the library wants an address)
        d_split = buf[:count * nws]
        log_prob = torch.empty(B * nws, dtype=torch.float32, device=dev)
        feasible = torch.empty(B * nws, dtype=torch.int32, device=dev)
        status = torch.zeros(nws, dtype=torch.int32, device=dev)
        for i, (ws, sl) in enumerate(parts):
            _lib.call('cliora_bracket_grad', plan.handle, C.c_void_p(ws.data_ptr()), _p(lengths[sl]) if lengths is not None else None,
                      _p(brackets[sl]) if M else None, M, _p(weights[sl]) if weights is not None else None,
                      C.c_void_p(buf.data_ptr() + 4 * i * count), _p(log_prob[sl]), _p(feasible[sl]),
                      C.c_void_p(status[i:i + 1].data_ptr()), _stream())
    return BracketGrad(d_split, log_prob, feasible, status)


class _BracketLogProb(torch.autograd.Function):
    """log_prob of the brackets as a function of the chart (formally: of its inside_s, see the module docstring)."""

    @staticmethod
    def forward(ctx, inside_s, diora, brackets):
        res = bracket_grad(diora, brackets)
        ctx.chart = _ChartView(diora._plan, diora._wss)            # the plan and the forward's holder (workspace + slot)
        ctx.brackets, ctx.shape = brackets, inside_s.shape
        ctx.set_materialize_grads(False)
        return res.log_prob

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return None, None, None
        holder = ctx.chart._wss
        d = bracket_grad(ctx.chart, ctx.brackets, weights=g).d_split
        slot = holder.split_cot
        slot[0] = d if slot[0] is None else slot[0] + d
        return torch.zeros(ctx.shape, dtype=torch.float32, device=d.device), None, None


def bracket_log_prob(diora, brackets):
    """log_prob (B,) fp32 of the brackets (int32 (B, M, 3), ``constrained.pack_brackets``; None: no bracket) under the last forward of
    `diora`, in its autograd graph: -inf, with a zero gradient, for a sentence no tree qualifies for (or with a bad row).  The
    mechanism and the refusals: the module docstring."""
    plan = diora._plan
    if plan is None:
        raise _lib.ChartLibError('bracket_log_prob: the module has run no forward')
    if plan.L > _lib.MAX_L:
        raise _lib.ChartLibError('bracket_log_prob: L = %d > %d is inference only (the backward stops at %d words), so the loss has '
                                 'nothing to train through; cliora_amd.constrained gives its value' % (plan.L, _lib.MAX_L, _lib.MAX_L))
    if getattr(diora, 'plan_arch', 0) != 0:
        raise _lib.ChartLibError('bracket_log_prob: a TreeLSTM chart takes no cotangent on its split scores (cliora_lstm_backward has no such input)')
    holder = diora._wss
    if len(holder) != 1 or getattr(holder, 'split_cot', None) is None:
        raise _lib.ChartLibError('bracket_log_prob: the module holds %d workspaces that no single chart node owns; call it after each '
                                 'forward of its own' % len(holder))
    inside_s = diora.chart.inside_s
    if not inside_s.requires_grad:
        raise _lib.ChartLibError('bracket_log_prob: the forward kept no backward state (it ran under torch.no_grad(), in eval mode '
                                 'without gradients, or on a padded chart); cliora_amd.constrained gives the value alone')
    return _BracketLogProb.apply(inside_s, diora, brackets)


def bracket_nll(diora, brackets, reduction='mean'):
    """-log_prob of the brackets over the sentences some tree qualifies for: their mean ('mean') or sum ('sum'), a 0-d tensor in the
    graph; 0 (with a graph) when no sentence is feasible.  Nothing is synchronised."""
    if reduction not in ('mean', 'sum'):
        raise ValueError("reduction must be 'mean' or 'sum'")
    lp = bracket_log_prob(diora, brackets)
    ok = torch.isfinite(lp)
    total = -torch.where(ok, lp, torch.zeros_like(lp)).sum()
    return total / ok.sum().clamp(min=1).to(lp.dtype) if reduction == 'mean' else total


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _tables(n, r, allowed):
    """Inside a[level, pos] and outside b[level, pos] in log space over the allowed cells of a sentence of n words (from the
    definitions: b[root] = 0, every parent pushes b[parent] + a[sibling] + r[parent, k] to its two children)."""
    a = np.full((n, n), -np.inf)
    a[0, :n] = np.where(allowed[0, :n], 0.0, -np.inf)
    for level in range(1, n):
        k, pos = np.arange(level)[None, :], np.arange(n - level)[:, None]
        t = a[k, pos] + a[level - k - 1, pos + k + 1] + r[level]          # (cells of the level, splits)
        m = t.max(axis=1)
        fin = m > -np.inf
        with np.errstate(invalid='ignore', divide='ignore'):
            v = np.where(fin, m + np.log(np.exp(t - np.where(fin, m, 0.0)[:, None]).sum(axis=1)), -np.inf)
        a[level, :n - level] = np.where(allowed[level, :n - level], v, -np.inf)
    b = np.full((n, n), -np.inf)
    b[n - 1, 0] = 0.0 if allowed[n - 1, 0] else -np.inf
    for level in range(n - 1, 0, -1):
        k = np.arange(level)
        for pos in range(n - level):
            if not b[level, pos] > -np.inf:
                continue
            left, right = (k, pos), (level - k - 1, pos + k + 1)
            base = b[level, pos] + r[level][pos]
            b[left] = np.where(allowed[left], np.logaddexp(b[left], base + a[right]), -np.inf)
            b[right] = np.where(allowed[right], np.logaddexp(b[right], base + a[left]), -np.inf)
    return a, b


def bracket_grad_numpy(pair_s, lengths, brackets, weights=None):
    """cliora_bracket_grad restated in fp64 from the formulas (tests): `pair_s[level]` (B, L - level, level[, 1]) the per-split inside
    scores of the (padded) chart, sentence b its first lengths[b] words; brackets (B, M, 3) or None; weights (B,) or None.
    -> {level: (B, L - level, level)} fp64, G = w d log_prob / d s; zero beyond a triangle, for a bad length or row, for an infeasible
    set and where no cell is disallowed."""
    lengths = [int(x) for x in lengths]
    Bn = len(lengths)
    levels = sorted(int(lv) for lv in pair_s)
    L = (max(levels) + 1) if levels else 1
    brackets = np.zeros((Bn, 0, 3), dtype=np.int32) if brackets is None else np.asarray(brackets)
    weights = np.ones(Bn) if weights is None else np.asarray(weights, dtype=np.float64)
    out = {level: np.zeros((Bn, L - level, level)) for level in range(1, L)}
    for b, n in enumerate(lengths):
        if not 1 <= n <= L or any(bad_row(row, n) for row in brackets[b]):
            continue
        allowed, _ = allowed_cells(n, brackets[b])
        if all(allowed[level, :n - level].all() for level in range(n)):
            continue
        s, r = {}, {}
        for level in range(1, n):
            s[level] = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
            r[level] = s[level] - s[level].max(axis=1, keepdims=True)
        ac, bc = _tables(n, r, allowed)
        au, bu = _tables(n, r, np.ones((n, n), dtype=bool))
        if not ac[n - 1, 0] > -np.inf:
            continue
        for level in range(1, n):
            k, pos = np.arange(level)[None, :], np.arange(n - level)[:, None]
            ec = bc[level, :n - level, None] + ac[k, pos] + ac[level - k - 1, pos + k + 1] + r[level] - ac[n - 1, 0]
            eu = bu[level, :n - level, None] + au[k, pos] + au[level - k - 1, pos + k + 1] + r[level] - au[n - 1, 0]
            d = np.exp(ec) - np.exp(eu)                                     # (-inf only ever meets -inf or a finite value: no NaN)
            d[np.arange(n - level), np.argmax(s[level], axis=1)] -= d.sum(axis=1)
            out[level][b, :n - level] = weights[b] * d
    return out
