"""Shared by test_hard_ragged_cpu.py and test_gpu_hard_ragged.py (not a test module): hard (S-DIORA) charts of mixed lengths in one
padded chart (cliora_chart_forward_ragged_hard, cliora_hard_spans_ragged).

The yardstick everywhere is cliora_amd.hard.hard_forward_ragged_torch: the fp64 hard chart of ONE sentence at its exact length, per
sentence, never the code under test.  Bounds are the project's: CPU_BOUND / FORWARD_BOUND / GRAD_STRICT of ragged_train_cases.py,
MARGIN_REL / RELU_MARGIN of hard_cases.py.

clear: every cell of every sentence's own triangle, both passes, keeps its best split MARGIN_REL * max|inside_s| (of that sentence)
ahead of the second best in the per-sentence fp64 restatement, so the device has to select the very same splits with no cell exempt;
test_hard_ragged_cpu.py asserts it (the seeds were chosen there).  The other cases are compared teacher-forced only.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import hard_cases as HC
import ragged_outside_cases as ROC
import ragged_train_cases as TC

CPU_BOUND = TC.CPU_BOUND                # 1e-12 * max(1, |want|)
FORWARD_BOUND = TC.FORWARD_BOUND        # 1e-4 * max(1, |want|)
GRAD_STRICT = TC.GRAD_STRICT            # 2e-4 of scale, element-wise in exact-fp32 mode
MARGIN_REL, RELU_MARGIN = HC.MARGIN_REL, HC.RELU_MARGIN
CHARTS = TC.CHARTS
MASKED = ROC.MASKED
# The one case whose ReLU clearance is taken over the pairs a hard chart composes, by hard_cases.SELECTED_PAIRS_ONLY's rule and for its
# reason: an eval forward (no gradient is taken) of 96 + 65 + 64 words has millions of pre-activations over all pairs.
SELECTED_PAIRS_ONLY = ('long',)


def _c(D, lengths, seed, share=True, normalize='unit', scale=1.0, clear=False, train=True, ties=False, what=''):
    return dict(D=D, lengths=list(lengths), L=max(lengths), seed=seed, share=share, normalize=normalize, scale=scale, clear=clear, train=train,
                ties=ties, what=what)


GPU_CASES = {
    'l5': _c(16, (1, 2, 3, 5, 5), 902, clear=True, what='lengths 1, 2, L and a repeat; one row tile with a tail'),
    'd24': _c(24, (4, 2, 3), 903, clear=True, what='padded width: Dp 32'),
    'b17': _c(48, [1 + i % 10 for i in range(17)], 900, what='more than 8 row tiles, a root at every level'),
    'd400': _c(400, (8, 5, 3, 8), 902, clear=True, what='five column blocks'),
    'unshared': _c(48, (5, 3, 1, 4, 5), 900, share=False, clear=True, what='outside-side weights'),
    'none': _c(16, (4, 2, 3, 4), 900, normalize='none', scale=16 ** -0.5, what="normalize='none': teacher-forced only"),
    'l64': _c(16, (64, 33, 2), 908, what='L 64, training: lane 63 of the tail, one mask word full'),
    'long': _c(16, (96, 65, 64, 2), 900, train=False, what='a long plan, eval only: root levels in both mask words'),
    'ties': _c(16, (1, 2, 3, 5, 5), 900, ties=True, what='inside_score_func.mat = 0: every split of a cell scores the same'),
}
CLEAR = tuple(sorted(n for n, c in GPU_CASES.items() if c['clear']))
CPU_CASES = (                           # D, lengths (1, 2, L and a repeat in each), share, normalize, weight scale
    (8, [5, 1, 3, 2, 4, 3], True, 'unit', 1.0),
    (12, [7, 7, 2, 6, 1, 3], False, 'unit', 1.0),
    (8, [5, 1, 3, 2, 5, 3], True, 'none', 8 ** -0.5),
    (8, [4, 1, 2, 4, 3], False, 'none', 8 ** -0.5),
)

# Largest errors measured on the MI355X by test_gpu_hard_ragged.py over GPU_CASES (it prints them before it asserts), beside their
# bounds, which are kept.  The charts on the own triangles, relative to max(1, |want|), bound FORWARD_BOUND = 1e-4:
MEASURED_FORWARD = {'f32': 7.2e-6, 'bf16x3': 9.7e-5}                     # both on `long` (outside_h; inside_h at 96 words: the inside pass
#                                                                         of the uniform hard chart, prefix-closed); l64: 3.3e-5; the short cases: at most 1.9e-5
# every parameter gradient and d x_span[b, :n_b], of the tensor's scale: exact mode, the maximum (bound GRAD_STRICT = 2e-4);
# split-bf16 mode, the largest median and the largest maximum (grad_check's bounds there: 5e-4 and 5e-2)
MEASURED_GRAD = {'f32 max': 4.4e-6, 'bf16x3 median': 2.6e-4, 'bf16x3 max': 3.5e-3}      # d400 leaf bias; l64 h_fcs.2.bias; l64 d x_span


def inputs(c):
    """-> (params by state_dict name, [x (n_b, D)], the padded batch (B, L, D) with seeded noise beyond each sentence)."""
    P, xs, _ = ROC.small_case(c['D'], c['lengths'], seed=c['seed'], share=c['share'], scale=c['scale'])
    if c['ties']:
        P = dict(P)
        P['inside_score_func.mat'] = torch.zeros_like(P['inside_score_func.mat'])
    return P, xs, ROC.padded(xs, c['L'])


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, cotangents and the fp64 per-sentence restatement under its OWN selection, computed once and left unchanged."""
    from cliora_amd.hard import hard_forward_ragged_torch
    c = dict(GPU_CASES[name])
    c['P'], c['xs'], c['xp'] = inputs(c)
    c['W'] = TC.weights(c['L'], c['lengths'], c['D'], seed=17)
    with torch.no_grad():
        c['ref'] = hard_forward_ragged_torch(c['P'], c['xp'], c['lengths'], c['share'], c['normalize'])
    return c


def own(L, lengths):
    """(B, C) bool tensor: the cells of each sentence's own triangle."""
    return torch.from_numpy(TC.own_mask(L, lengths))


def weighted_loss(charts, W, own_mask):
    """sum_k sum over own cells of W_k . chart_k -- by indexing: whatever sits beyond a triangle (NaN in the yardstick) is not read."""
    total = 0.0
    for t, w in zip(charts, W):
        t = t if t.dim() == 3 else t.unsqueeze(-1)
        total = total + (t[own_mask] * w.to(t.dtype)[own_mask]).sum()
    return total


def teacher_forced(c, selection, dtype, with_grads):
    """The per-sentence restatement under the given PADDED (device) selection in `dtype` -> (charts {name: (B, C, w)}, NaN beyond the
    triangles; gradients by parameter name + 'x_span' (B, L, D), or None)."""
    from cliora_amd.hard import hard_forward_ragged_torch
    Pd = {k: v.detach().to(dtype).requires_grad_(with_grads) for k, v in c['P'].items()}
    xd = c['xp'].detach().to(dtype).requires_grad_(with_grads)
    with torch.set_grad_enabled(with_grads):
        o = hard_forward_ragged_torch(Pd, xd, c['lengths'], c['share'], c['normalize'], selection=selection, dtype=dtype)
    charts = {k: (o[k].detach().unsqueeze(-1) if o[k].dim() == 2 else o[k].detach()) for k in CHARTS}
    if not with_grads:
        return charts, None
    weighted_loss([o[k] for k in CHARTS], c['W'], own(c['L'], c['lengths'])).backward()
    g = {k: v.grad.detach() for k, v in Pd.items() if v.grad is not None}
    g['x_span'] = xd.grad.detach()
    return charts, g


def masked_hard_padded(P, xp, lengths, share, normalize, dtype=torch.float64):
    """The schedule of cliora_chart_forward_ragged_hard in torch, on the pattern of ragged_outside_cases.masked_outside: the hard
    inside pass of the PADDED batch, -1e30 into inside_s beyond each triangle, the hard outside pass of the padded chart with each
    sentence's root cell (n - 1, 0) overwritten by the seed after its level.  Every cell takes the one-hot of the first maximum of its
    own scores, in the library's pair order.  -> dict of the four padded charts (in the graph) and sel_in / sel_out (B, C) int64 as
    the device specifies them: -1 at leaves, at each sentence's outside root and beyond the triangles."""
    from cliora_amd.hard import EPS, _first_argmax, _pair_tables
    B, L, D = xp.shape
    C = L * (L + 1) // 2
    off, tabs = _pair_tables(L)
    Pd = {k: v.to(dtype) for k, v in P.items()}
    x = xp.to(dtype)
    nrm = (lambda t: t / t.norm(p=2, dim=-1, keepdim=True).clamp(min=EPS)) if normalize == 'unit' else (lambda t: t)

    def side(pre):
        pre = 'inside' if share else pre
        return (Pd[pre + '_compose_func.h_fcs.0.weight'], Pd[pre + '_compose_func.h_fcs.0.bias'], Pd[pre + '_compose_func.h_fcs.2.weight'],
                Pd[pre + '_compose_func.h_fcs.2.bias'], Pd[pre + '_score_func.mat'])

    def cell_level(which, level, AH, AS, BH, BS, W):
        W1, b1, W2, b2, M = W
        a, b = tabs[which][level]
        N = a.shape[1]
        ah, bh = AH[:, a], BH[:, b]
        y = F.relu(F.linear(F.relu(F.linear(torch.cat([ah, bh], -1), W1, b1)), W2, b2))
        s = torch.einsum('blnd,de,blne->bln', ah, M, bh) + AS[:, a] + BS[:, b]
        k = _first_argmax(s.detach())
        p = F.one_hot(k, N).to(dtype)
        return nrm((y * p.unsqueeze(-1)).sum(2)), (s * p).sum(-1), k

    z = lambda *shape: torch.zeros(*shape, dtype=dtype)
    IH, IS, OH, OS = z(B, C, D), z(B, C), z(B, C, D), z(B, C)
    sel_in, sel_out = (torch.full((B, C), -1, dtype=torch.int64) for _ in range(2))
    IH[:, :L] = nrm(torch.tanh(F.linear(x, Pd['inside_compose_func.leaf_fc.weight'], Pd['inside_compose_func.leaf_fc.bias'])))
    for level in range(1, L):
        o, Lc = int(off[level]), L - level
        IH[:, o:o + Lc], IS[:, o:o + Lc], sel_in[:, o:o + Lc] = cell_level('in', level, IH, IS, IH, IS, side('inside'))
    own_mask = own(L, lengths)
    ISm = torch.where(own_mask, IS, torch.full_like(IS, MASKED))             # 1. the mask
    OH[:, C - 1:] = nrm(Pd['root_vector_out_h'].view(1, 1, D).expand(B, 1, D))
    for level in range(L - 2, -1, -1):
        o, Lc = int(off[level]), L - level
        OH[:, o:o + Lc], OS[:, o:o + Lc], sel_out[:, o:o + Lc] = cell_level('out', level, IH, ISm, OH, OS, side('outside'))
        for b, n in enumerate(lengths):                                        # 2. the root overwrite, after its level
            if n - 1 == level:
                OH[b, o], OS[b, o] = OH[b, C - 1], OS[b, C - 1]
                sel_out[b, o] = -1
    sel_in[~own_mask], sel_out[~own_mask] = -1, -1
    return dict(inside_h=IH, inside_s=ISm, outside_h=OH, outside_s=OS, sel_in=sel_in, sel_out=sel_out)
