"""Shared by test_ragged_vl_train_cpu.py and test_gpu_ragged_vl_train.py (not a test module): training CLIORA through a padded chart
of mixed lengths (cliora_chart_forward_ragged_train_vl / cliora_chart_backward_ragged_vl, cliora_vg_loss_ragged,
cliora_contrastive_loss_ragged).

The yardsticks are the fp64 oracle (oracle/diora_ref.py) on ONE sentence at its exact length with its own regions, and the fp64
restatements below of the two mixed-length loss definitions, never the code under test.  A recorded (B, C, R) dropout mask of the
PADDED chart is replayed in the oracle by swapping R.F.dropout; sentence b's rows reach its exact-length chart through own_cells.
"""
import numpy as np
import torch

import ragged_outside_cases as ROC
import ragged_train_cases as TC
from oracle import chart_layout as CL
from oracle import diora_ref as R

CPU_BOUND = TC.CPU_BOUND
FORWARD_BOUND = TC.FORWARD_BOUND
GRAD_STRICT = TC.GRAD_STRICT
REGIONS = 5
CPU_CASES = (                           # D, lengths (1, 2, L and a repeated length in each), share
    (8, [5, 1, 3, 2, 4, 3], True),
    (12, [7, 7, 2, 6, 1, 3], True),
    (8, [5, 1, 3, 2, 4, 3], False),
)
# name -> (D, R, lengths, share): the lengths of ragged_train_cases.GPU_CASES
GPU_CASES = {
    'D32-R4': (32, 4, TC.GPU_CASES['D32'][1], True),
    'D24-R5': (24, 5, TC.GPU_CASES['D24'][1], True),                     # padded width: Dp = 32
    'D128-R36': (128, 36, TC.GPU_CASES['D128'][1], True),
    'D32-R4-unshared': (32, 4, TC.GPU_CASES['D32-unshared'][1], False),
}
# Largest errors measured on the MI355X by test_gpu_ragged_vl_train.py over GPU_CASES (it prints them before it asserts), beside
# their bounds.  The charts on the own triangles, relative to max(1, |want|), bound FORWARD_BOUND = 1e-4; every parameter gradient,
# d x_span[b, :n_b] and d obj_span, of the tensor's scale: exact mode, the maximum (bound GRAD_STRICT = 2e-4); split-bf16 mode, the
# largest median and the largest maximum (grad_check's bounds there: 5e-4 and 5e-2).
MEASURED_FORWARD = {'f32': 2.3e-6, 'bf16x3': 1.5e-5}                     # both at D 128 / R 36 (outside_s, inside_s)
MEASURED_GRAD = {'f32 max': 2.3e-6, 'bf16x3 median': 3.4e-6, 'bf16x3 max': 1.5e-4}      # all at D 128 / R 36
# The loss kernels against the fp64 restatements.  VG: test_gpu_heads.test_vg_loss's bound, 1e-5 of max(1, scale), value and gradient.
# Contrastive: test_gpu_harness.test_fused_contrastive_loss_matches_the_torch_formula's, 1e-5 on the value and 1e-6 of scale + 1e-9 on
# the gradients; like that test's, the seeded inputs keep every hinge argument away from its kink (asserted: HINGE_CLEARANCE), where
# fp32 and fp64 may take different sides.
VG_BOUND = 1e-5
CONTRASTIVE_VALUE_BOUND = 1e-5
CONTRASTIVE_GRAD_BOUND = (1e-6, 1e-9)
HINGE_CLEARANCE = 1e-6
LOSS_CASES = {                          # name -> (B, L, R, lengths)
    'B6': (6, 7, 36, [7, 1, 3, 2, 6, 3]),
    'B3': (3, 4, 70, [4, 2, 3]),
    'B2': (2, 3, 1, [3, 1]),
    'B64': (64, 20, 36, [20, 1] + [int(n) for n in np.random.RandomState(64).randint(1, 21, size=62)]),
}
# Largest errors measured on the MI355X over LOSS_CASES: the VG value and gradient (bound 1e-5), the contrastive value (bound 1e-5) and
# gradients (bound 1e-6 of scale + 1e-9); the smallest hinge clearance of the inputs is 9.4e-6 (B64).
MEASURED_LOSS = {'vg value': 1.3e-7, 'vg gradient': 4.1e-8, 'contrastive value': 2.5e-7, 'contrastive gradient': 1.9e-7}


def chart_len(C):
    return int(round((np.sqrt(8 * C + 1) - 1) / 2))


# ---- the two definitions in fp64 -----------------------------------------------------------------------------------------------------
def vg_loss_ragged(vg, lengths, alpha):
    """logits[a, c] = (1 / n_a) sum_{l < n_a} max_r vg[a, c, l, r];  alpha * cross_entropy(logits, arange(B)).  The words beyond n_a are
    never touched (sliced away, not masked)."""
    B = vg.shape[0]
    logits = torch.stack([vg[a, :, :n].max(-1).values.sum(-1) / n for a, n in enumerate(lengths)])
    return alpha * torch.nn.functional.cross_entropy(logits, torch.arange(B))


def half_cells(L, n):
    """The first C_n // 2 cells of own_order: padded-chart rows, in the order of a chart of length n."""
    return ROC.own_cells(L, n)[:(n * (n + 1) // 2) // 2]


def contrastive_loss_ragged(inside_s, outside_s, smax, lengths, margin, alpha, floor=1e-8, clearance=None):
    """The contrastive definition of DESIGN.md section 23 on the region maxima smax (B, B, C), sentence by sentence and by gathering
    the cells that enter -- nothing beyond a triangle is indexed.  clearance: a one-element list that receives the smallest distance
    of a hinge argument from the floor."""
    ins, outs = inside_s.reshape(inside_s.shape[0], -1), outside_s.reshape(outside_s.shape[0], -1)
    B, C = ins.shape
    L = chart_len(C)
    own = TC.own_mask(L, lengths)
    total = 0.0
    gap = float('inf')
    for x, n in enumerate(lengths):
        cells = torch.from_numpy(half_cells(L, n))
        if cells.numel() == 0:
            continue
        pos = smax[x, x, cells]                                       # k
        others = [y for y in range(B) if y != x]
        t = margin + smax[x][others][:, cells] - pos                  # (B - 1, k): every image y != x
        txt = t.clamp(min=floor).sum(0) / B
        gap = min(gap, float((t.detach() - floor).abs().min())) if t.numel() else gap
        img = []
        for j, cell in enumerate(cells.tolist()):
            texts = [a for a in others if own[a, cell]]               # the texts whose triangle holds the cell
            if not texts:
                img.append(pos.new_zeros(()))
                continue
            u = margin + smax[texts, x, cell] - pos[j]
            img.append(u.clamp(min=floor).sum() / B)
            gap = min(gap, float((u.detach() - floor).abs().min()))
        img = torch.stack(img)
        marg = torch.exp(ins[x, cells] + outs[x, cells] - ins[x, TC.root_cell(L, n)])
        total = total + (marg * (txt + img)).sum()
    if clearance is not None:
        clearance[0] = gap
    return alpha * total / B


def poison(t, keep, value=float('nan')):
    """t with `value` wherever the bool mask `keep` (broadcast from the left) is False."""
    k = keep.reshape(keep.shape + (1,) * (t.dim() - keep.dim()))
    return torch.where(k, t, torch.full_like(t, value))


def loss_inputs(name, dtype=torch.float64):
    """Seeded inputs of a LOSS_CASES entry, as float32 values in `dtype`: vg (B, B, L, R), smax (B, B, C), inside_s, outside_s (B, C, 1)."""
    B, L, Rn, lengths = LOSS_CASES[name]
    C = L * (L + 1) // 2
    g = torch.Generator().manual_seed(B * 100 + L)
    vg = torch.randn(B, B, L, Rn, generator=g)
    smax = torch.randn(B, B, C, generator=g)
    ins, outs = 0.3 * torch.randn(B, C, 1, generator=g), 0.3 * torch.randn(B, C, 1, generator=g)
    return [t.to(dtype) for t in (vg, smax, ins, outs)]


def word_mask(L, lengths):
    return torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]      # (B, L)


# ---- the chart: the oracle per sentence, with regions and a replayed mask ----------------------------------------------------------
def vl_case(D, Rn, lengths, seed, share=True):
    """Seeded parameters, sentences, region matrices (R, D) per sentence and the (B, C, R) pre-scaled keep mask of the padded chart."""
    P, xs, _ = ROC.small_case(D, lengths, seed=seed, share=share)
    objs = [torch.randn(Rn, D, generator=torch.Generator().manual_seed(seed + 500 + i)) for i in range(len(lengths))]
    L = max(lengths)
    torch.manual_seed(seed + 7)
    mask = torch.nn.functional.dropout(torch.ones(len(lengths), L * (L + 1) // 2, Rn), 0.1, True)
    return P, xs, objs, mask


class replayed_dropout(object):
    """R.F.dropout swapped for the duration: call i (one per level, leaves first) multiplies by the level's rows of `mask` (B, C_n, R),
    a mask in the order of the chart of length n that the oracle runs."""

    def __init__(self, mask, n):
        self.mask, self.off, self.calls = mask, [int(o) for o in CL.level_offsets(n)] + [n * (n + 1) // 2], 0

    def __enter__(self):
        self.orig = R.F.dropout

        def replay(x, p, training):
            i = self.calls
            self.calls += 1
            return x * self.mask[:, self.off[i]:self.off[i + 1]].to(x.dtype)
        R.F.dropout = replay
        return self

    def __exit__(self, *exc):
        R.F.dropout = self.orig
        return False


def oracle_forward(P64, x64, obj64, mask_rows, n, normalize='unit', share=True, x_word=None, obj_word=None):
    """The oracle on ONE sentence (x64 (n, D), obj64 (R, D)) in training mode with its rows of the recorded mask, in the graph."""
    with replayed_dropout(mask_rows[None], n) as rp:
        o = R.diora_forward(P64, x64[None], x64[None] if x_word is None else x_word[None], obj64[None],
                            obj64[None] if obj_word is None else obj_word[None], outside=True, normalize=normalize, share=share, training=True)
    assert rp.calls == n
    return o


def oracle_sum(P, xs, objs, lengths, W, mask, normalize='unit', share=True):
    """fp64: every sentence alone at its exact length with its regions and its rows of the mask, the weighted loss on its charts
    (ragged_train_cases), differentiated by autograd and summed.
    -> (loss, {parameter name: gradient}, [d x (n_b, D)], [d obj (R, D)], [{chart name: (C_n, w)}])."""
    L = max(lengths)
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    total, dxs, dobjs, charts = 0.0, [], [], []
    for b, (x, obj, n) in enumerate(zip(xs, objs, lengths)):
        x64, o64 = x.detach().double().requires_grad_(True), obj.detach().double().requires_grad_(True)
        own = torch.from_numpy(ROC.own_cells(L, n))
        o = oracle_forward(P64, x64, o64, mask[b, own].double(), n, normalize, share)
        loss = sum((W[k][b, own] * o[name][0]).sum() for k, name in enumerate(TC.CHARTS))
        loss.backward()
        total += float(loss.detach())
        dxs.append(x64.grad)
        dobjs.append(o64.grad)
        charts.append({name: o[name][0].detach() for name in TC.CHARTS})
    return total, {k: v.grad for k, v in P64.items()}, dxs, dobjs, charts


def padded_autograd(P, xp, objs, lengths, W, mask, normalize='unit', share=True):
    """fp64: the padded schedule on the oracle's pieces -- diora_forward(..., obj_span=..., outside=False) of the right-padded batch in
    training mode with the padded chart's mask, then ragged_outside_cases.masked_outside -- the same loss, differentiated by torch
    autograd.  -> (loss, {parameter name: gradient}, d x_span (B, L, D), d obj_span (B, R, D))."""
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    x64 = xp.detach().double().requires_grad_(True)
    o64 = torch.stack(objs).detach().double().requires_grad_(True)
    L = xp.shape[1]
    with replayed_dropout(mask.double(), L) as rp:
        pad = R.diora_forward(P64, x64, x64, o64, o64, outside=False, normalize=normalize, share=share, training=True)
    assert rp.calls == L
    oh, os_ = ROC.masked_outside(P64, pad, lengths, normalize, share)
    own = torch.from_numpy(TC.own_mask(L, lengths))[:, :, None]
    zero = lambda t: torch.where(own, t, torch.zeros_like(t))
    loss = sum((W[k] * zero(t)).sum() for k, t in enumerate((pad['inside_h'], pad['inside_s'], oh, os_)))
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in P64.items()}, x64.grad, o64.grad


# ---- Trainer.step_ragged(obj_feats=...) against the oracle ---------------------------------------------------------------------------
def oracle_step_loss(sd, sentences, obj_feats, neg, mask, margin, alpha_contr, alpha_vg, normalize='unit', share=True):
    """fp64, ONE pack holding `sentences` in this order with the (B, C, R) mask of its padded chart: the token-weighted reconstruction
    loss of the sentences, each at its exact length (ragged_train_cases.oracle_step_loss), plus the two restatements on the oracle's
    per-sentence charts and scores, assembled into the padded layout.  sd: a harness.Net's state_dict (fp64, requires_grad leaves).
    In the graph.  -> (total, dict of the three terms)."""
    P = {k[len('diora.'):]: v for k, v in sd.items() if k.startswith('diora.')}
    lengths = [len(s) for s in sentences]
    B, L = len(sentences), max(lengths)
    C = L * (L + 1) // 2
    n_tokens = float(sum(lengths))
    enc = lambda f: R.image_encoder_forward(sd['img_encoder.fc.weight'], sd['img_encoder.fc.bias'], sd['img_encoder.fc_vis.weight'],
                                            sd['img_encoder.fc_vis.bias'], f)
    o_span, o_word = enc(obj_feats)                                   # (B, R, D) each
    Rn = o_span.shape[1]
    rec = 0.0
    sums, words, ins, outs = [], [], [], []
    for b, s in enumerate(sentences):
        n = len(s)
        tokens = torch.tensor([list(s)])
        x_span, x_word = R.embed_forward(sd['embed.embeddings.weight'], sd['embed.mat'], sd['embed.mat1'], tokens)
        own = torch.from_numpy(ROC.own_cells(L, n))
        o = oracle_forward(P, x_span[0], o_span[b], mask[b, own].double(), n, normalize, share, x_word=x_word[0], obj_word=o_word[b])
        rec = rec + R.reconstruction_loss(sd['embed.embeddings.weight'], sd['reconstruct_softmax_loss.mat'], tokens, neg, o['outside_h']) * (n / n_tokens)
        pad = lambda t, w: torch.zeros(C, w, dtype=t.dtype).index_copy(0, own, t)
        sums.append(pad(o['inside_h'][0] + o['outside_h'][0], x_span.shape[-1]))
        ins.append(pad(o['inside_s'][0], 1))
        outs.append(pad(o['outside_s'][0], 1))
        words.append(torch.cat([x_word[0], torch.zeros(L - n, x_word.shape[-1], dtype=x_word.dtype)]))
    smax = torch.einsum('abx,cdx->acbd', torch.stack(sums), o_span).max(-1).values          # cliora.py:457 + trainer.py:101
    vg = torch.einsum('abx,cdx->acbd', torch.stack(words), o_word)                          # cliora.py:459-461, training mode
    l_vg = vg_loss_ragged(vg, lengths, alpha_vg)
    l_con = contrastive_loss_ragged(torch.stack(ins), torch.stack(outs), smax, lengths, margin, alpha_contr)
    return rec + l_vg + l_con, dict(reconstruct=rec, vg=l_vg, contrastive=l_con)
