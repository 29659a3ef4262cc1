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

The second half of the module reads the same distribution as an expectation (cliora_tree_expectation): the
expected value of a per-cell cost and the entropy of the distribution over trees, ``tree_objective``, with the same hand-off.

The third part is the max-margin family over the same potentials (cliora_bracket_margin): structured hinge,
perceptron and ramp losses, ``bracket_hinge``, whose subgradient -- a difference of two trees -- takes the same hand-off.

The fourth part compares TWO charts over the same sentences (cliora_tree_kl): the divergence KL(p || q) between
their distributions over trees and the cross-entropy, ``parse_kl`` / ``parse_divergence``, whose two gradients take the hand-off of
each chart's own forward.
"""
import collections

import numpy as np
import torch

from . import _lib
from .constrained import allowed_cells, bad_row, refuse_rejected
from .posterior import cell_id
from .query import ChartQuery, host_copy, per_sentence, walk

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


def _refuse_no_forward(diora, who):
    if diora._plan is None:
        raise _lib.ChartLibError('%s: the module has run no forward' % who)


def bracket_grad(diora, brackets, weights=None, lengths=None):
    """cliora_bracket_grad on a chart module after its forward (any forward: this call needs no backward state).  brackets: int32
    (B, M, 3) (``constrained.pack_brackets``) or None; weights: fp32 (B,) or None = 1; lengths: int32 (B,) or None.  One d_split buffer
    per workspace of ``workspace_slices``, back to back.  -> BracketGrad of device tensors; nothing is synchronised."""
    _refuse_no_forward(diora, 'bracket_grad')
    q = ChartQuery(diora)
    M = q.check_brackets(brackets)
    lengths = q.lengths_or_holders(lengths)
    q.check_int32('lengths', lengths)
    q.check_weights('weights', weights)
    d_arg, d_split = q.split_buffer()
    log_prob, feasible, status = q.empty(torch.float32), q.empty(torch.int32), q.status()
    q.launch('cliora_bracket_grad', per_sentence(q.moved(lengths)), per_sentence(q.moved(brackets)), M, per_sentence(q.moved_weights(weights)),
             d_arg, per_sentence(log_prob), per_sentence(feasible), status=status)
    return BracketGrad(d_split, log_prob, feasible, status)


# ---- the loss node: what the three autograd Functions of this module share ----------------------------------------------------------
def _trainable(diora, who, noun, instead, long_instead=''):
    """Whether a structured loss can train through the last forward of `diora`: the refusals of the module docstring, in their order.
    noun: what `who` computes, instead / long_instead: where its value alone comes from (the words that differ between the callers).
    -> the chart's inside_s, the formal input of the loss's node."""
    _refuse_no_forward(diora, who)
    plan = diora._plan
    if plan.L > _lib.MAX_L:
        raise _lib.ChartLibError('%s: L = %d > %d is inference only (the backward stops at %d words), so the %s has nothing to train '
                                 'through%s' % (who, plan.L, _lib.MAX_L, _lib.MAX_L, noun, long_instead))
    if getattr(diora, 'plan_arch', 0) != 0:
        raise _lib.ChartLibError('%s: a TreeLSTM chart takes no cotangent on its split scores (cliora_lstm_backward has no such input)' % who)
    holder = diora._wss
    if len(holder) != 1 or getattr(holder, 'split_cot', None) is None:
        raise _lib.ChartLibError('%s: the module holds %d workspaces that no single chart node owns; call it after each forward of its '
                                 'own' % (who, len(holder)))
    inside_s = diora.chart.inside_s
    if not inside_s.requires_grad:
        raise _lib.ChartLibError('%s: the forward kept no backward state (it ran under torch.no_grad(), in eval mode without gradients, '
                                 'or on a padded chart); %s' % (who, instead))
    return inside_s


def _keep(ctx, inside_s, diora, *args):
    """The forward side of the hand-off: the plan and the forward's holder (workspace + slot), inside_s's shape, the query's own
    arguments."""
    ctx.chart, ctx.args, ctx.shape = _ChartView(diora._plan, diora._wss), args, inside_s.shape
    ctx.set_materialize_grads(False)


def _hand_off(ctx, query, **weights):
    """The backward side: `query` again with the cotangents as its weights, its d_split ADDED into the slot of the forward's holder
    (the module docstring).  -> the node's gradients: zeros for inside_s, None for the rest; all None without a cotangent."""
    if all(w is None for w in weights.values()):
        return (None,) * (2 + len(ctx.args))
    d = query(ctx.chart, *ctx.args, **weights).d_split
    slot = ctx.chart._wss.split_cot
    slot[0] = d if slot[0] is None else slot[0] + d
    return (torch.zeros(ctx.shape, dtype=torch.float32, device=d.device),) + (None,) * (1 + len(ctx.args))


def _check_reduction(reduction):
    if reduction not in ('mean', 'sum'):
        raise ValueError("reduction must be 'mean' or 'sum'")


class _BracketLogProb(torch.autograd.Function):
    """log_prob of the brackets as a function of the chart (formally: of its inside_s, see the module docstring)."""

    @staticmethod
    def forward(ctx, inside_s, diora, brackets):
        _keep(ctx, inside_s, diora, brackets)
        return bracket_grad(diora, brackets).log_prob

    @staticmethod
    def backward(ctx, g):
        return _hand_off(ctx, bracket_grad, weights=g)


def bracket_log_prob(diora, brackets):
    """log_prob (B,) fp32 of the brackets (int32 (B, M, 3), ``constrained.pack_brackets``; None: no bracket) under the last forward of
    `diora`, in its autograd graph: -inf, with a zero gradient, for a sentence no tree qualifies for (or with a bad row).  The
    mechanism and the refusals: the module docstring."""
    inside_s = _trainable(diora, 'bracket_log_prob', 'loss', 'cliora_amd.constrained gives the value alone',
                          '; cliora_amd.constrained gives its value')
    return _BracketLogProb.apply(inside_s, diora, brackets)


def bracket_nll(diora, brackets, reduction='mean'):
    """-log_prob of the brackets over the sentences some tree qualifies for: their mean ('mean') or sum ('sum'), a 0-d tensor in the
    graph; 0 (with a graph) when no sentence is feasible.  Nothing is synchronised."""
    _check_reduction(reduction)
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


def _sentences(pair_s, lengths, brackets=None):
    """What the restatements below start with: -> (lengths as ints, their number, the chart's length from the levels of `pair_s`, the
    brackets as an array, (B, 0, 3) for None)."""
    lengths = [int(x) for x in lengths]
    L = (max(int(lv) for lv in pair_s) + 1) if len(pair_s) else 1
    return lengths, len(lengths), L, np.zeros((len(lengths), 0, 3), dtype=np.int32) if brackets is None else np.asarray(brackets)


def bracket_grad_numpy(pair_s, lengths, brackets, weights=None):
    """cliora_bracket_grad restated in fp64 from the formulas (tests): `pair_s[level]` (B, L - level, level[, 1]) the per-split inside
    scores of the (padded) chart, sentence b its first lengths[b] words; brackets (B, M, 3) or None; weights (B,) or None.
    -> {level: (B, L - level, level)} fp64, G = w d log_prob / d s; zero beyond a triangle, for a bad length or row, for an infeasible
    set and where no cell is disallowed."""
    lengths, Bn, L, brackets = _sentences(pair_s, lengths, brackets)
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


# ---- expectations: the expected cost and the entropy of the parse distribution (cliora_tree_expectation) ------
# The same distribution read as an expectation: risk = E_T[sum of cost over T's cells] -- with cost -1 on the annotated phrases, minus
# the expected number of gold brackets recovered, a soft counterpart of bracket_nll that takes crossing phrases and is never infeasible
# -- and the entropy H = -sum_T p(T) log p(T).  Both gradients are covariances that the kernel forms from an expectation-semiring
# inside-outside pass (csrc/expectation_kernels.hpp); the hand-off to the chart is the bracket loss's slot, into which they ADD.
#
#     risk, entropy = tree_objective(net.diora, span_costs(phrases, L=L, device=dev))        # (B,) each, in the graph
#     loss = recon + 0.5 * risk.mean() - 0.01 * entropy.mean()
#
# d_split (cliora_plan_split_score_count * workspaces,) fp32; risk, entropy, log_z (B,) fp32; status (number of workspaces,) int32.
TreeExpectation = collections.namedtuple('TreeExpectation', 'd_split risk entropy log_z status')


def tree_expectation(diora, cost=None, w_cost=None, w_entropy=None, lengths=None):
    """cliora_tree_expectation on a chart module after its forward (any forward: this call needs no backward state).  cost: fp32
    (B, C) in the cell order of inside_s or None = 0; w_cost: fp32 (B,) or None = 1; w_entropy: fp32 (B,) or None = 0; lengths: int32
    (B,) or None.  d_split = d (w_cost risk + w_entropy entropy) / d s, one buffer per workspace of ``workspace_slices``, back to
    back.  -> TreeExpectation of device tensors; nothing is synchronised."""
    _refuse_no_forward(diora, 'tree_expectation')
    q = ChartQuery(diora)
    lengths = q.lengths_or_holders(lengths)
    q.check_cost(cost)
    q.check_int32('lengths', lengths)
    q.check_weights('w_cost', w_cost)
    q.check_weights('w_entropy', w_entropy)
    cost = cost.to(q.dev).float().contiguous() if cost is not None else None
    d_arg, d_split = q.split_buffer()
    risk, entropy, log_z = (q.empty(torch.float32) for _ in range(3))
    status = q.status()
    q.launch('cliora_tree_expectation', per_sentence(q.moved(lengths)), per_sentence(cost), per_sentence(q.moved_weights(w_cost)),
             per_sentence(q.moved_weights(w_entropy)), d_arg, per_sentence(risk), per_sentence(entropy), per_sentence(log_z), status=status)
    return TreeExpectation(d_split, risk, entropy, log_z, status)


class _TreeObjective(torch.autograd.Function):
    """(risk, entropy) as functions of the chart (formally: of its inside_s, as _BracketLogProb)."""

    @staticmethod
    def forward(ctx, inside_s, diora, cost):
        _keep(ctx, inside_s, diora, cost)
        res = tree_expectation(diora, cost)
        return res.risk, res.entropy

    @staticmethod
    def backward(ctx, g_risk, g_entropy):
        some = g_risk if g_risk is not None else g_entropy
        zeros = torch.zeros_like(some) if some is not None else None
        return _hand_off(ctx, tree_expectation, w_cost=zeros if g_risk is None else g_risk, w_entropy=zeros if g_entropy is None else g_entropy)


def tree_objective(diora, cost=None):
    """(risk, entropy), two (B,) fp32 tensors in the autograd graph of the last forward of `diora`: the expected value of the
    per-cell cost (fp32 (B, C) in the cell order of inside_s, ``span_costs``; None = 0) over the trees, and the entropy of the
    distribution over trees.  Their cotangents reach the chart through the bracket loss's slot, into which they add: the objective
    sums with ``bracket_log_prob`` and with a second call on the same forward.  The refusals are ``bracket_log_prob``'s."""
    return _TreeObjective.apply(_trainable(diora, 'tree_objective', 'objective', 'tree_expectation gives the values alone'), diora, cost)


def _reduce(v, reduction):
    _check_reduction(reduction)
    return v.mean() if reduction == 'mean' else v.sum()


def expected_cost(diora, cost, reduction='mean'):
    """The expected cost of the parse over the batch, a 0-d tensor in the graph: its mean ('mean') or sum ('sum')."""
    return _reduce(tree_objective(diora, cost)[0], reduction)


def parse_entropy(diora, reduction='mean'):
    """The entropy of the distribution over trees over the batch, a 0-d tensor in the graph: its mean ('mean') or sum ('sum')."""
    return _reduce(tree_objective(diora, None)[1], reduction)


def span_costs(required, forbidden=None, L=None, device=None):
    """Per-sentence lists of (start, end) spans (``brackets_from_entity_labels(..., drop_crossing=False)``: crossing phrases are
    welcome) -> (B, C) fp32 costs in the cell order of inside_s for a chart of length L: [span is forbidden] - [span is required],
    i.e. -1 on a required span, +1 on a forbidden one, 0 elsewhere.  A span that is not 0 <= start <= end < L is ignored."""
    if L is None:
        raise ValueError('span_costs: L, the length of the chart, is required')
    L = int(L)
    out = np.zeros((len(required), L * (L + 1) // 2), dtype=np.float32)
    for lists, value in ((required, -1.0), (forbidden, 1.0)):
        for b, spans in enumerate(lists or ()):
            for s, e in set((int(s), int(e)) for s, e in spans):
                if 0 <= s <= e < L:
                    out[b, cell_id(L, e - s, s)] += value
    t = torch.from_numpy(out)
    return t.to(device) if device is not None else t


def tree_expectation_numpy(pair_s, lengths, cost, w_cost=None, w_entropy=None):
    """cliora_tree_expectation restated in fp64 from the definitions (tests): `pair_s[level]` (B, L - level, level[, 1]) the per-split
    inside scores of the (padded) chart, sentence b its first lengths[b] words; cost (B, C) or None; w_cost (B,) or None = 1;
    w_entropy (B,) or None = 0.  -> (G {level: (B, L - level, level)}, risk (B,), entropy (B,), log_z (B,)), zeros for a bad length.

    The expectation semiring in the linear domain, with no logarithm but log_z: a cell carries the pair (Z, Zv) = (sum of the weights
    of its subtrees, sum of weight x value), a product of pairs is (a b, a bv + av b); the outside pair (O, Ov) is pushed from every
    parent to its two children.  Then sum over the trees through edge e of weight x V(T) is Ov Z_l Z_r w + O (Z_l Z_r w)v."""
    lengths, Bn, L, _ = _sentences(pair_s, lengths)
    cost = np.zeros((Bn, L * (L + 1) // 2)) if cost is None else np.asarray(cost, dtype=np.float64)
    w_cost = np.ones(Bn) if w_cost is None else np.asarray(w_cost, dtype=np.float64)
    w_entropy = np.zeros(Bn) if w_entropy is None else np.asarray(w_entropy, dtype=np.float64)
    G = {level: np.zeros((Bn, L - level, level)) for level in range(1, L)}
    risk, entropy, log_z = np.zeros(Bn), np.zeros(Bn), np.zeros(Bn)
    for b, n in enumerate(lengths):
        if not 1 <= n <= L:
            continue
        wc, we = w_cost[b], w_entropy[b]
        c = np.zeros((n, n))
        for level in range(n):
            c0 = cell_id(L, level, 0)
            c[level, :n - level] = cost[b, c0:c0 + n - level]
        s, r, w, v = {}, {}, {}, {}
        for level in range(1, n):
            s[level] = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
            r[level] = s[level] - s[level].max(axis=1, keepdims=True)
            w[level] = np.exp(r[level])
            v[level] = wc * c[level, :n - level, None] - we * r[level]
        Z, Zv = np.zeros((n, n)), np.zeros((n, n))
        Z[0, :n], Zv[0, :n] = 1.0, wc * c[0, :n]
        edge, edge_v = {}, {}                               # per edge: Z_l Z_r w and its value part
        for level in range(1, n):
            k, pos = np.arange(level)[None, :], np.arange(n - level)[:, None]
            left, right = (k, pos), (level - k - 1, pos + k + 1)
            edge[level] = Z[left] * Z[right] * w[level]
            edge_v[level] = (Zv[left] * Z[right] + Z[left] * Zv[right]) * w[level] + edge[level] * v[level]
            Z[level, :n - level], Zv[level, :n - level] = edge[level].sum(axis=1), edge_v[level].sum(axis=1)
        O, Ov = np.zeros((n, n)), np.zeros((n, n))
        O[n - 1, 0] = 1.0
        for level in range(n - 1, 0, -1):
            k = np.arange(level)
            for pos in range(n - level):
                left, right = (k, pos), (level - k - 1, pos + k + 1)
                o = O[level, pos] * w[level][pos]
                ov = Ov[level, pos] * w[level][pos] + o * v[level][pos]
                O[left], Ov[left] = O[left] + o * Z[right], Ov[left] + ov * Z[right] + o * Zv[right]
                O[right], Ov[right] = O[right] + o * Z[left], Ov[right] + ov * Z[left] + o * Zv[left]
        total = Z[n - 1, 0]
        mean_v = Zv[n - 1, 0] / total
        log_z[b] = np.log(total)
        risk[b] = sum(float((O[level, :n - level] * Z[level, :n - level] * c[level, :n - level]).sum()) for level in range(n)) / total
        mean_r = 0.0
        for level in range(1, n):
            o, ov = O[level, :n - level, None], Ov[level, :n - level, None]
            nu = o * edge[level] / total
            d = (ov * edge[level] + o * edge_v[level]) / total - nu * mean_v
            mean_r += float((nu * r[level]).sum())
            d[np.arange(n - level), np.argmax(s[level], axis=1)] -= d.sum(axis=1)
            G[level][b, :n - level] = d
        entropy[b] = log_z[b] - mean_r
    return G, risk, entropy, log_z


# ---- max-margin losses: structured hinge, perceptron and ramp (cliora_bracket_margin) -------------------------
# The third way to train on brackets: the score of the best cost-augmented tree minus the score of the best tree that respects the
# brackets.  dis[cell] = 1 on a cell of levels 1 .. n - 2 that the brackets disallow, F(t) the sum of r over a tree's internal cells,
# D(t) the sum of dis over them:
#
#     A = max_t F(t) + margin D(t),   Bv = max_t F(t) - penalty D(t),   loss = A - Bv >= 0
#
# margin > 0 and penalty inf: the structured hinge with margin rescaling; margin 0: the perceptron loss; a finite penalty: the ramp
# loss, which stays defined on a bracket set that no tree satisfies.  The subgradient is a difference of two trees -- sparse, made of
# integers -- and reaches the chart through the bracket loss's slot, into which it ADDS; a hard chart, whose score
# matrix gets an exactly zero gradient from the reconstruction loss, is moved by it.
#
#     loss = recon + 0.5 * net.diora.bracket_hinge(req)                   # or bracket_hinge(net.diora, pack_brackets(req))
#
# d_split as BracketGrad's; loss, aug_score, ref_score (B,) fp32; violations, feasible (B,) int32; spans_aug, spans_ref (B, L-1, 2)
# int32 or None; status (number of workspaces,) int32.  Device tensors; nothing is synchronised.  (bracket_margin_numpy: the same fields
# as numpy arrays, d_split {level: (B, L - level, level)} and the scalars in fp64, status an int.)
BracketMargin = collections.namedtuple('BracketMargin', 'd_split loss aug_score ref_score violations feasible spans_aug spans_ref status')


def _check_margin(margin, penalty):
    margin, penalty = float(margin), float(penalty)
    if not (margin >= 0 and np.isfinite(margin)):
        raise ValueError('margin must be finite and >= 0')
    if not penalty >= 0:
        raise ValueError('penalty must be >= 0 (inf: the reference tree keeps every bracket)')
    return margin, penalty


def bracket_margin(diora, brackets, margin=1.0, penalty=float('inf'), weights=None, lengths=None, spans=False):
    """cliora_bracket_margin on a chart module after its forward (any forward: this call needs no backward state).  brackets, weights,
    lengths: as ``bracket_grad`` takes them; spans: also give the two trees.  One d_split buffer per workspace of
    ``workspace_slices``, back to back.  -> BracketMargin of device tensors; nothing is synchronised."""
    _refuse_no_forward(diora, 'bracket_margin')
    margin, penalty = _check_margin(margin, penalty)
    q = ChartQuery(diora)
    M = q.check_brackets(brackets)
    lengths = q.lengths_or_holders(lengths)
    q.check_int32('lengths', lengths)
    q.check_weights('weights', weights)
    d_arg, d_split = q.split_buffer()
    loss, aug, ref = (q.empty(torch.float32) for _ in range(3))
    viol, feasible = q.empty(torch.int32), q.empty(torch.int32)
    sp_a, sp_r = (q.empty(torch.int32, q.plan.L - 1, 2) for _ in range(2)) if spans else (None, None)
    status = q.status()
    q.launch('cliora_bracket_margin', per_sentence(q.moved(lengths)), per_sentence(q.moved(brackets)), M, margin, penalty,
             per_sentence(q.moved_weights(weights)), d_arg, per_sentence(loss), per_sentence(aug), per_sentence(ref), per_sentence(viol),
             per_sentence(feasible), per_sentence(sp_a), per_sentence(sp_r), status=status)
    return BracketMargin(d_split, loss, aug, ref, viol, feasible, sp_a, sp_r, status)


class _BracketMarginLoss(torch.autograd.Function):
    """(loss, feasible) of the brackets as functions of the chart (formally: of its inside_s, as _BracketLogProb)."""

    @staticmethod
    def forward(ctx, inside_s, diora, brackets, margin, penalty):
        _keep(ctx, inside_s, diora, brackets, margin, penalty)
        res = bracket_margin(diora, brackets, margin, penalty)
        ctx.mark_non_differentiable(res.feasible)
        return res.loss, res.feasible

    @staticmethod
    def backward(ctx, g, _):
        return _hand_off(ctx, bracket_margin, weights=g)


def _margin_node(diora, brackets, margin, penalty, who):
    _refuse_no_forward(diora, who)
    margin, penalty = _check_margin(margin, penalty)
    return _BracketMarginLoss.apply(_trainable(diora, who, 'loss', 'bracket_margin gives the value alone'), diora, brackets, margin, penalty)


def bracket_margin_loss(diora, brackets, margin=1.0, penalty=float('inf')):
    """loss (B,) fp32 of the brackets (int32 (B, M, 3), ``constrained.pack_brackets``; None: no bracket) under the last forward of
    `diora`, in its autograd graph: A - Bv of the module comment above; 0, with a zero gradient, for a sentence no tree qualifies for
    under an infinite penalty (or with a bad row).  The mechanism and the refusals are ``bracket_log_prob``'s."""
    return _margin_node(diora, brackets, margin, penalty, 'bracket_margin_loss')[0]


def bracket_hinge(diora, brackets, margin=1.0, penalty=float('inf'), reduction='mean'):
    """The max-margin loss over the feasible sentences -- under an infinite penalty those some tree qualifies for, under a finite one
    those without a bad row: their mean ('mean') or sum ('sum'), a 0-d tensor in the graph; 0 (with a graph) when there is none.
    Nothing is synchronised."""
    _check_reduction(reduction)
    loss, feasible = _margin_node(diora, brackets, margin, penalty, 'bracket_hinge')
    total = loss.sum()                                     # an infeasible or rejected sentence holds 0
    return total / feasible.sum().clamp(min=1).to(loss.dtype) if reduction == 'mean' else total


def bracket_violations(diora, brackets, lengths=None):
    """Per sentence, the number of constituents of the best (CKY) tree that cross a required bracket or equal a forbidden one -- against
    a full gold tree, its spans that are not in the gold tree: the margin = 0 call's violations.  -> (B,) int32 numpy array; one
    device-to-host copy; a rejected sentence raises."""
    res = bracket_margin(diora, brackets, margin=0.0, penalty=0.0, lengths=lengths)
    viol, status = host_copy(res.violations, res.status)
    refuse_rejected(int(status.sum()), 'cliora_bracket_margin')
    return viol


def _best_tree(n, rel, leaf, bonus):
    """The fp32 recurrence of the kernel over one sentence: val[leaf] = leaf, candidate (val_l + val_r) + rel in fp32, first maximum
    wins, then val[cell] = best + bonus[level][pos] (fp32; 0 where the cell has none).  -> (root value, [(start, end, split)] in the
    walk's order)."""
    val, bp = np.zeros((n, n), dtype=np.float32), {}
    val[0, :n] = leaf
    for level in range(1, n):
        k, pos = np.arange(level)[None, :], np.arange(n - level)[:, None]
        cand = (val[k, pos] + val[level - k - 1, pos + k + 1]) + rel[level]        # (cells of the level, splits), fp32
        bp[level] = np.argmax(cand, axis=1)
        val[level, :n - level] = cand[np.arange(n - level), bp[level]] + bonus[level]
    return val[n - 1, 0], [row[:3] for row in walk(n, lambda level, pos, _: (bp[level][pos], None, None))]


def bracket_margin_numpy(pair_s, lengths, brackets, margin, penalty, weights=None):
    """cliora_bracket_margin restated (tests): `pair_s[level]` (B, L - level, level[, 1]) the per-split inside scores of the (padded)
    chart, sentence b its first lengths[b] words; brackets (B, M, 3) or None; weights (B,) or None.  The two trees in float32 in the
    kernel's operation order, as ``constrained_numpy`` does its best tree; scores, loss and gradient in fp64 from those trees.
    -> BracketMargin of numpy arrays as the kernel writes them."""
    margin, penalty = _check_margin(margin, penalty)
    m32, p32, hard = np.float32(margin), np.float32(penalty), penalty == float('inf')
    lengths, Bn, L, brackets = _sentences(pair_s, lengths, brackets)
    weights = np.ones(Bn) if weights is None else np.asarray(weights, dtype=np.float32).astype(np.float64)
    G = {level: np.zeros((Bn, L - level, level)) for level in range(1, L)}
    loss, aug, ref = np.zeros(Bn), np.zeros(Bn), np.zeros(Bn)
    viol, feasible, status = np.zeros(Bn, dtype=np.int32), np.zeros(Bn, dtype=np.int32), 0
    sp_a, sp_r = (np.full((Bn, max(L - 1, 0), 2), -1, dtype=np.int32) for _ in range(2))
    ninf32 = np.float32(-np.inf)
    for b, n in enumerate(lengths):
        if not 1 <= n <= L or any(bad_row(row, n) for row in brackets[b]):
            status += 1
            continue
        allowed, _ = allowed_cells(n, brackets[b])
        dis = ~allowed
        dis[0, :] = False
        dis[max(n - 1, 0):, :] = False                # leaves and the root are in every tree: no cost
        s, rel, r = {}, {}, {}
        for level in range(1, n):
            s[level] = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
            s32 = np.asarray(pair_s[level][b], dtype=np.float32).reshape(-1, level)[:n - level]
            rel[level] = s32 - s32.max(axis=1, keepdims=True)
            r[level] = s[level] - s[level].max(axis=1, keepdims=True)
        ones = np.ones(n, dtype=np.float32)
        zero = np.float32(0.0)
        bonus_a = {level: np.where(dis[level, :n - level], m32, zero) for level in range(1, n)}
        if hard:
            leaf_b = np.where(allowed[0, :n], np.float32(1.0), ninf32)
            bonus_b = {level: np.where(allowed[level, :n - level], zero, ninf32) for level in range(1, n)}
        else:
            leaf_b = ones
            bonus_b = {level: np.where(dis[level, :n - level], -p32, zero) for level in range(1, n)}
        with np.errstate(invalid='ignore'):
            _, tree_a = _best_tree(n, rel, ones, bonus_a)
            root_b, tree_b = _best_tree(n, rel, leaf_b, bonus_b)
        score = lambda tree: sum(r[e - st][st, k] for st, e, k in tree)
        count = lambda tree: sum(int(dis[e - st, st]) for st, e, _ in tree)
        viol[b] = count(tree_a)
        aug[b] = score(tree_a) + float(m32) * viol[b]
        sp_a[b, :len(tree_a)] = np.asarray([t[:2] for t in tree_a], dtype=np.int32).reshape(-1, 2)
        if not root_b > ninf32:                       # no qualifying tree
            ref[b] = -np.inf
            continue
        feasible[b] = 1
        sp_r[b, :len(tree_b)] = np.asarray([t[:2] for t in tree_b], dtype=np.int32).reshape(-1, 2)
        ref[b] = score(tree_b) - (float(p32) * count(tree_b) if count(tree_b) else 0.0)
        diff = aug[b] - ref[b]
        if diff < 0:                                  # the two fp32 maxima within rounding of each other
            continue
        loss[b] = diff
        for tree, sign in ((tree_a, 1.0), (tree_b, -1.0)):
            for st, e, k in tree:
                level = e - st
                kstar = int(np.argmax(s[level][st]))
                G[level][b, st, k] += sign
                G[level][b, st, kstar] -= sign
        for level in range(1, n):
            G[level][b] *= weights[b]
            G[level][b][G[level][b] == 0] = 0.0       # +0 whatever the weight
    return BracketMargin(G, loss, aug, ref, viol, feasible, sp_a, sp_r, status)


# ---- two charts: the divergence between their parse distributions (cliora_tree_kl) -----------------------------
# Teacher p and student q are two chart modules after a forward on the same sentences (same B and L; width, regions, weight sharing,
# soft or hard may differ: only the split scores are read).  kl = KL(p || q) = sum_T p(T) log(p(T) / q(T)), cross_entropy =
# -sum_T p(T) log q(T), entropy_p their difference.  The student's gradient is a difference of edge marginals, the teacher's a
# covariance under p (csrc/kl_kernels.hpp); each reaches its own chart through the slot of that chart's forward, into which it ADDS.
#
#     teacher.eval(); with torch.no_grad(): teacher(x_span)               # any forward: eval, no_grad, hard, CLIORA, another width
#     net.diora(x_span, x_word)                                            # the student's training forward
#     loss = recon + 0.5 * net.diora.parse_divergence(teacher)             # or parse_divergence(teacher, net.diora)
#
# d_split_p (None without teacher_grad), d_split_q (cliora_plan_split_score_count * workspaces,) fp32; kl, cross_entropy, entropy_p,
# log_z_p, log_z_q (B,) fp32; status (number of workspaces,) int32.  Device tensors; nothing is synchronised.  (tree_kl_numpy: the
# same fields as numpy arrays, the gradients {level: (B, L - level, level)} and the scalars in fp64, status an int.)
TreeKL = collections.namedtuple('TreeKL', 'd_split_p d_split_q kl cross_entropy entropy_p log_z_p log_z_q status')


def tree_kl(teacher, student, w_kl=None, w_ce=None, lengths=None, teacher_grad=False, student_grad=True):
    """cliora_tree_kl on two chart modules after their forwards (any forward: this call needs no backward state).  w_kl: fp32 (B,)
    or None = 1; w_ce: fp32 (B,) or None = 0; lengths: int32 (B,) or None = the lengths of the student's padded training chart, else
    of the teacher's.  d_split_q = d (w_kl kl + w_ce cross_entropy) / d s^q, d_split_p the same with respect to s^p -- formed only
    with teacher_grad (student_grad) --, one buffer per workspace, back to back.  -> TreeKL of device tensors; nothing is synchronised."""
    _refuse_no_forward(teacher, 'tree_kl (teacher)')
    _refuse_no_forward(student, 'tree_kl (student)')
    q, qs = ChartQuery(teacher), ChartQuery(student)
    handle, ws = q.second(qs, 'tree_kl')
    if lengths is None:
        lengths = qs.lengths_or_holders(None)
        lengths = q.lengths_or_holders(None) if lengths is None else lengths
    q.check_int32('lengths', lengths)
    q.check_weights('w_kl', w_kl)
    q.check_weights('w_ce', w_ce)
    p_arg, d_split_p = q.split_buffer() if teacher_grad else (None, None)
    q_arg, d_split_q = q.split_buffer() if student_grad else (None, None)
    kl, ce, ent, lzp, lzq = (q.empty(torch.float32) for _ in range(5))
    status = q.status()
    q.launch('cliora_tree_kl', handle, ws, per_sentence(q.moved(lengths)), per_sentence(q.moved_weights(w_kl)),
             per_sentence(q.moved_weights(w_ce)), p_arg, q_arg, per_sentence(kl), per_sentence(ce), per_sentence(ent), per_sentence(lzp),
             per_sentence(lzq), status=status)
    return TreeKL(d_split_p, d_split_q, kl, ce, ent, lzp, lzq, status)


def _keeps_backward_state(diora):
    """Whether the last forward of `diora` can take a cotangent on its split scores: what ``_trainable`` demands, as a question."""
    plan, holder = diora._plan, getattr(diora, '_wss', None)
    return (plan is not None and plan.L <= _lib.MAX_L and getattr(diora, 'plan_arch', 0) == 0 and holder is not None and len(holder) == 1
            and getattr(holder, 'split_cot', None) is not None and diora.chart.inside_s.requires_grad)


class _ParseKL(torch.autograd.Function):
    """(kl, cross_entropy) as functions of the two charts (formally: of the inside_s of each chart that kept backward state, as
    _BracketLogProb).  in_p / in_q: that chart's inside_s, or None for a chart that takes no gradient."""

    @staticmethod
    def forward(ctx, teacher, student, in_p, in_q):
        ctx.charts = _ChartView(teacher._plan, teacher._wss), _ChartView(student._plan, student._wss)
        ctx.shapes = tuple(None if t is None else t.shape for t in (in_p, in_q))
        ctx.set_materialize_grads(False)
        res = tree_kl(teacher, student, student_grad=False)
        return res.kl, res.cross_entropy

    @staticmethod
    def backward(ctx, g_kl, g_ce):
        some = g_kl if g_kl is not None else g_ce
        if some is None:
            return None, None, None, None
        zeros = torch.zeros_like(some)
        res = tree_kl(*ctx.charts, w_kl=zeros if g_kl is None else g_kl, w_ce=zeros if g_ce is None else g_ce,
                      teacher_grad=ctx.shapes[0] is not None, student_grad=ctx.shapes[1] is not None)
        out = []
        for chart, shape, d in zip(ctx.charts, ctx.shapes, (res.d_split_p, res.d_split_q)):
            if shape is None:
                out.append(None)
                continue
            slot = chart._wss.split_cot
            slot[0] = d if slot[0] is None else slot[0] + d
            out.append(torch.zeros(shape, dtype=torch.float32, device=d.device))
        return (None, None) + tuple(out)


def _kl_node(p, q):
    """(kl, cross_entropy) of KL(p || q) in the graph of every one of the two charts that kept backward state (at least one does)."""
    ins = [m.chart.inside_s if _keeps_backward_state(m) else None for m in (p, q)]
    return _ParseKL.apply(p, q, *ins)


def parse_kl(teacher, student):
    """(kl, cross_entropy), two (B,) fp32 tensors in the autograd graph of the last forward of `student` -- and of `teacher`, when
    its forward kept backward state too: KL(p || q) and -sum_T p(T) log q(T), p the teacher's distribution over trees, q the
    student's.  One node; its backward launches the kernel once with the cotangents as weights and ADDS each gradient into the slot of
    its own chart's forward, so the loss sums with ``bracket_log_prob``, ``tree_objective``, ``bracket_hinge`` and a second call.  The
    student's refusals are ``bracket_log_prob``'s; the teacher may be any chart with a forward of the same B and L."""
    _refuse_no_forward(teacher, 'parse_kl (teacher)')
    _trainable(student, 'parse_kl', 'divergence', 'tree_kl gives the values alone')
    return _kl_node(teacher, student)


def parse_divergence(teacher, student, direction='forward', reduction='mean'):
    """The divergence between the two parse distributions over the batch, a 0-d tensor in the graph: its mean ('mean') or sum ('sum').
    direction 'forward': KL(teacher || student), what distillation minimises; 'reverse': KL(student || teacher), the roles swapped
    (mode seeking); 'symmetric': their sum, in two launches.  The refusals are ``parse_kl``'s, for the student in every direction."""
    if direction not in ('forward', 'reverse', 'symmetric'):
        raise ValueError("direction must be 'forward', 'reverse' or 'symmetric'")
    _check_reduction(reduction)
    _refuse_no_forward(teacher, 'parse_divergence (teacher)')
    _trainable(student, 'parse_divergence', 'divergence', 'tree_kl gives the values alone')
    total = None
    for p, q in {'forward': ((teacher, student),), 'reverse': ((student, teacher),),
                 'symmetric': ((teacher, student), (student, teacher))}[direction]:
        kl = _kl_node(p, q)[0]
        total = kl if total is None else total + kl
    return _reduce(total, reduction)


def tree_kl_numpy(pair_s_p, pair_s_q, lengths, w_kl=None, w_ce=None):
    """cliora_tree_kl restated in fp64 from the definitions (tests): `pair_s_p[level]`, `pair_s_q[level]` (B, L - level, level[, 1])
    the per-split inside scores of the teacher's and the student's (padded) chart, sentence b its first lengths[b] words; w_kl (B,) or
    None = 1; w_ce (B,) or None = 0.  -> TreeKL of numpy arrays, both gradients given, zeros for a bad length (counted in status).

    In another form than the kernel, as ``tree_expectation_numpy``: the linear domain, with no logarithm but the two log_z.  Under p a
    cell carries the pair (Z, Zv) of the expectation semiring with the edge value v = w_kl r^p - (w_kl + w_ce) r^q, under q the plain
    Z; the outside values (O, Ov) and O_q are pushed from every parent to its two children."""
    lengths, Bn, L, _ = _sentences(pair_s_p, lengths)
    w_kl = np.ones(Bn) if w_kl is None else np.asarray(w_kl, dtype=np.float64)
    w_ce = np.zeros(Bn) if w_ce is None else np.asarray(w_ce, dtype=np.float64)
    Gp, Gq = ({level: np.zeros((Bn, L - level, level)) for level in range(1, L)} for _ in range(2))
    kl, ce, ent, lzp, lzq, status = np.zeros(Bn), np.zeros(Bn), np.zeros(Bn), np.zeros(Bn), np.zeros(Bn), 0
    for b, n in enumerate(lengths):
        if not 1 <= n <= L:
            status += 1
            continue
        wk, wsum = w_kl[b], w_kl[b] + w_ce[b]
        sp, sq, rp, rq, wp, wq, v = {}, {}, {}, {}, {}, {}, {}
        for level in range(1, n):
            sp[level] = np.asarray(pair_s_p[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
            sq[level] = np.asarray(pair_s_q[level][b], dtype=np.float64).reshape(-1, level)[:n - level]
            rp[level] = sp[level] - sp[level].max(axis=1, keepdims=True)
            rq[level] = sq[level] - sq[level].max(axis=1, keepdims=True)
            wp[level], wq[level] = np.exp(rp[level]), np.exp(rq[level])
            v[level] = wk * rp[level] - wsum * rq[level]
        Z, Zv, Y = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))          # Y: the student's Z
        Z[0, :n], Y[0, :n] = 1.0, 1.0
        edge, edge_v, edge_q = {}, {}, {}
        for level in range(1, n):
            k, pos = np.arange(level)[None, :], np.arange(n - level)[:, None]
            left, right = (k, pos), (level - k - 1, pos + k + 1)
            edge[level] = Z[left] * Z[right] * wp[level]
            edge_v[level] = (Zv[left] * Z[right] + Z[left] * Zv[right]) * wp[level] + edge[level] * v[level]
            edge_q[level] = Y[left] * Y[right] * wq[level]
            Z[level, :n - level], Zv[level, :n - level] = edge[level].sum(axis=1), edge_v[level].sum(axis=1)
            Y[level, :n - level] = edge_q[level].sum(axis=1)
        O, Ov, Oq = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
        O[n - 1, 0] = Oq[n - 1, 0] = 1.0
        for level in range(n - 1, 0, -1):
            k = np.arange(level)
            for pos in range(n - level):
                left, right = (k, pos), (level - k - 1, pos + k + 1)
                o = O[level, pos] * wp[level][pos]
                ov = Ov[level, pos] * wp[level][pos] + o * v[level][pos]
                oq = Oq[level, pos] * wq[level][pos]
                O[left], Ov[left], Oq[left] = O[left] + o * Z[right], Ov[left] + ov * Z[right] + o * Zv[right], Oq[left] + oq * Y[right]
                O[right], Ov[right], Oq[right] = O[right] + o * Z[left], Ov[right] + ov * Z[left] + o * Zv[left], Oq[right] + oq * Y[left]
        total, total_q = Z[n - 1, 0], Y[n - 1, 0]
        mean_v = Zv[n - 1, 0] / total
        lzp[b], lzq[b] = np.log(total), np.log(total_q)
        mean_rp = mean_rq = 0.0
        for level in range(1, n):
            o, ov, oq = O[level, :n - level, None], Ov[level, :n - level, None], Oq[level, :n - level, None]
            nu, nu_q = o * edge[level] / total, oq * edge_q[level] / total_q
            dp = (ov * edge[level] + o * edge_v[level]) / total - nu * mean_v
            dq = wsum * (nu_q - nu)
            mean_rp += float((nu * rp[level]).sum())
            mean_rq += float((nu * rq[level]).sum())
            rows = np.arange(n - level)
            dp[rows, np.argmax(sp[level], axis=1)] -= dp.sum(axis=1)
            dq[rows, np.argmax(sq[level], axis=1)] -= dq.sum(axis=1)
            Gp[level][b, :n - level], Gq[level][b, :n - level] = dp, dq
        ent[b], ce[b] = lzp[b] - mean_rp, lzq[b] - mean_rq
        kl[b] = ce[b] - ent[b]
    return TreeKL(Gp, Gq, kl, ce, ent, lzp, lzq, status)
