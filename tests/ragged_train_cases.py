"""Shared by test_ragged_train_cpu.py and test_gpu_ragged_train.py (not a test module): training through a padded chart of mixed
lengths (cliora_chart_forward_ragged_train / cliora_chart_backward_ragged).

The yardstick everywhere is the fp64 oracle (oracle/diora_ref.py) on ONE sentence at its exact length, summed over the sentences,
never the code under test.  The loss of every gradient check puts seeded random weights on the cells of each sentence's own triangle
in all four charts: loss = sum_k sum_b sum_{cell in own(b)} W_k[b, cell] . chart_k[b, cell].
"""
import numpy as np
import torch

import ragged_outside_cases as ROC
from oracle import chart_layout as CL
from oracle import diora_ref as R

CPU_BOUND = 1e-12                       # fp64: |got - want| <= CPU_BOUND * max(1, |want|), every parameter and d x_span
FORWARD_BOUND = ROC.FORWARD_BOUND       # the project's forward bound, 1e-4 * max(1, |want|), on every cell of each own triangle
GRAD_STRICT = 2e-4                      # conftest.grad_check(..., strict=GRAD_STRICT): of scale, element-wise in exact-fp32 mode

CPU_CASES = (                           # D, lengths (1, 2, L and a repeated length in each)
    (8, [5, 1, 3, 2, 4, 3]),
    (12, [7, 7, 2, 6, 1, 3]),
)
# name -> (D, lengths, share, normalize, weight scale).  normalize = none: nothing bounds the vectors, and the forward bound is per
# element against max(1, |want|), so the weights are drawn at the variance-preserving scale 1 / sqrt(D) -- a layer of fan-in D then
# has a gain of at most 1 (W1, fan-in 2 D behind a ReLU: 1; W2: 1 / sqrt(2)) and the rows stay of order 1 at every level, where
# that bound means what it means for unit-normalised charts.  It is the 0.25 of the D 16 cases of test_gpu_ragged_outside.py, per width.
GPU_CASES = {
    'D32': (32, [7, 1, 3, 2, 6, 3], True, 'unit', 1.0),                  # the resident-kernel regime (the backward must not take it)
    'D24': (24, [7, 1, 3, 2, 6, 3], True, 'unit', 1.0),                  # padded width: Dp = 32
    'D128': (128, [12, 11, 1, 5, 5, 2, 8, 12], True, 'unit', 1.0),
    'D32-unshared': (32, [7, 1, 3, 2, 6, 3], False, 'unit', 1.0),
    'D32-none': (32, [7, 1, 3, 2, 6, 3], True, 'none', 32 ** -0.5),
}
# Largest errors measured on the MI355X by test_gpu_ragged_train.py over GPU_CASES (it prints them before it asserts), beside their
# bounds.  Item 1, the charts on the own triangles, relative to max(1, |want|), bound FORWARD_BOUND = 1e-4:
MEASURED_FORWARD = {'f32': 1.3e-6, 'bf16x3': 1.7e-5}                     # both at D 128
# Item 2, every parameter gradient and d x_span[b, :n_b], of the tensor's scale: exact mode, the maximum (bound GRAD_STRICT = 2e-4);
# split-bf16 mode, the largest median and the largest maximum (grad_check's bounds there: 5e-4 and 5e-2).
MEASURED_GRAD = {'f32 max': 2.0e-6, 'bf16x3 median': 2.9e-6, 'bf16x3 max': 1.5e-5}


def own_mask(L, lengths):
    """(B, C) bool: cell (level, pos) of the padded chart belongs to sentence b's triangle iff pos + level < n_b -- in closed form,
    the way ragged_mask_cotangents finds a cell's level (walk the level offsets)."""
    C = L * (L + 1) // 2
    out = np.zeros((len(lengths), C), dtype=bool)
    for b, n in enumerate(lengths):
        for cell in range(C):
            level, off = 0, 0
            while cell >= off + (L - level):
                off += L - level
                level += 1
            out[b, cell] = (cell - off) + level < n
    return out


def masked_rows(L, lengths):
    """The rows ragged_mask_cotangents writes as zero: (B, C) bool."""
    return ~own_mask(L, lengths)


def root_cell(L, n):
    """Chart row of the cell (n - 1, 0) as root_bwd computes it: the first cell of level lv = n - 1."""
    lv = n - 1
    return lv * L - lv * (lv - 1) // 2


def root_cut_rows(L, lengths, level):
    """The (sentence, chart row) pairs ragged_root_cut(level) zeroes: sentences with n_b - 1 == level < L - 1, their cell (level, 0)."""
    return [(b, root_cell(L, n)) for b, n in enumerate(lengths) if n - 1 == level and level < L - 1]


def weights(L, lengths, D, seed, beyond=0.0):
    """The four cotangents (B, C, w) fp64: seeded N(0, 1) on each own triangle, `beyond` elsewhere (0, or NaN: they must not leak)."""
    g = torch.Generator().manual_seed(seed)
    own = torch.from_numpy(own_mask(L, lengths))[:, :, None]
    out = []
    for w in (D, 1, D, 1):
        t = torch.randn(len(lengths), L * (L + 1) // 2, w, generator=g, dtype=torch.float32).double()     # what the device gets, exactly
        out.append(torch.where(own, t, torch.full_like(t, beyond)))
    return out


CHARTS = ('inside_h', 'inside_s', 'outside_h', 'outside_s')


def oracle_sum(P, xs, lengths, W, normalize='unit', share=True):
    """fp64: every sentence alone at its exact length, the weighted loss on its charts, differentiated by autograd and summed.
    -> (loss, {parameter name: gradient}, [d x (n_b, D)], [{chart name: (C_n, w)}])."""
    L = max(lengths)
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    total, dxs, charts = 0.0, [], []
    for b, (x, n) in enumerate(zip(xs, lengths)):
        x64 = x.detach().double().requires_grad_(True)
        o = R.diora_forward(P64, x64[None], outside=True, normalize=normalize, share=share)
        own = torch.from_numpy(ROC.own_cells(L, n))
        loss = sum((W[k][b, own] * o[name][0]).sum() for k, name in enumerate(CHARTS))
        loss.backward()
        total += float(loss.detach())
        dxs.append(x64.grad)
        charts.append({name: o[name][0].detach() for name in CHARTS})
    return total, {k: v.grad for k, v in P64.items()}, dxs, charts


def padded_autograd(P, xp, lengths, W, normalize='unit', share=True):
    """fp64: the schedule of cliora_chart_forward_ragged_train on the oracle's pieces (ragged_outside_cases.masked_outside on top of the
    padded inside pass), the same loss, differentiated by torch autograd.  -> (loss, {parameter name: gradient}, d x_span (B, L, D))."""
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    x64 = xp.detach().double().requires_grad_(True)
    pad = R.diora_forward(P64, x64, outside=False, normalize=normalize, share=share)
    oh, os_ = ROC.masked_outside(P64, pad, lengths, normalize, share)
    L = xp.shape[1]
    own = torch.from_numpy(own_mask(L, lengths))[:, :, None]
    zero = lambda t: torch.where(own, t, torch.zeros_like(t))          # the loss touches each own triangle only
    loss = sum((W[k] * zero(t)).sum() for k, t in enumerate((pad['inside_h'], pad['inside_s'], oh, os_)))
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in P64.items()}, x64.grad


def rel_err(got, want):
    """max |got - want| / max(1, |want|) over a tensor: the tensor's largest reference magnitude is the scale."""
    return float((got - want).abs().max()) / max(1.0, float(want.abs().max()))


# ---- Trainer.step_ragged against the oracle -----------------------------------------------------------------------------------
def oracle_step_loss(sd, sentences, neg, normalize='unit', share=True):
    """fp64: the token-weighted reconstruction loss of the sentences, each at its exact length, from a harness.Net's state_dict (fp64,
    requires_grad leaves) -- sum_b n_b * loss_b / sum_b n_b, i.e. one mean over all tokens.  In the graph."""
    P = {k[len('diora.'):]: v for k, v in sd.items() if k.startswith('diora.')}
    n_tokens = float(sum(len(s) for s in sentences))
    total = 0.0
    for s in sentences:
        tokens = torch.tensor([list(s)])
        x_span, _ = R.embed_forward(sd['embed.embeddings.weight'], sd['embed.mat'], sd['embed.mat1'], tokens)
        o = R.diora_forward(P, x_span, outside=True, normalize=normalize, share=share)
        loss = R.reconstruction_loss(sd['embed.embeddings.weight'], sd['reconstruct_softmax_loss.mat'], tokens, neg, o['outside_h'])
        total = total + loss * (len(s) / n_tokens)
    return total
