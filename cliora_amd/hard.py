"""Hard (single-tree, S-DIORA) charts in plain torch: the yardstick of ``cliora_chart_forward_hard``.

``hard_forward_torch`` restates the chart recursion of a text-only DioraMLP (cliora/net/diora.py:283-398) with the softmax over a
cell's splits replaced by a detached one-hot weight row, so ``torch.autograd`` through it gives the gradients of "every cell encodes
its selected split" -- what the library's unchanged backward computes on a hard workspace.  The splits of a cell are walked in the
LIBRARY's order (the plan's pair tables, read on the host: no GPU needed), so a selection means the same split here and on the device.

``hard_forward_ragged_torch`` is the yardstick of ``cliora_chart_forward_ragged_hard``: the same restatement on
every sentence of a right-padded batch alone at its exact length, scattered into padded charts.

Nothing here runs on the product path.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .query import walk_spans

EPS = 1e-8      # cliora/net/utils.py:10


@functools.lru_cache(maxsize=None)
def _pair_tables(L):
    """Per pass and level the operand cells of the library's pair order: {'in' / 'out': {level: (a, b) int64 (Lc, N)}}, and the level
    offsets.  Inside: (left, right) child; outside: (sibling inside cell, parent outside cell)."""
    plan = _lib.Plan(1, L, 16, True, 'unit', 0, 0, forward_only=L > _lib.MAX_L)
    off = plan.table('level_offset').astype(np.int64)
    tabs = {}
    for side in ('in', 'out'):
        a, b, base = plan.table('pair_a_' + side), plan.table('pair_b_' + side), plan.table('pair_lvl_base_' + side)
        tabs[side] = {}
        for level in range(L):
            Lc, N = L - level, (level if side == 'in' else L - level - 1)
            if N > 0:
                lo = int(base[level])
                tabs[side][level] = tuple(torch.from_numpy(t[lo:lo + Lc * N].astype(np.int64).reshape(Lc, N)) for t in (a, b))
    return off, tabs


def _first_argmax(s):
    """The lowest index that attains the maximum over the last dim."""
    N = s.shape[-1]
    idx = torch.arange(N, device=s.device).expand_as(s)
    return torch.where(s == s.max(-1, keepdim=True).values, idx, torch.full_like(idx, N)).min(-1).values.clamp(max=N - 1)


def hard_forward_torch(params, x_span, share, normalize, outside=True, selection=None, dtype=torch.float64, soft=False):
    """The hard chart of a text-only DioraMLP.

    params: the module's parameters under their state_dict names ('inside_compose_func.h_fcs.0.weight', ..., 'root_vector_out_h');
    tensors that require grad stay in the graph.  x_span (B, L, D).  selection: None -- every cell takes the first argmax of ITS OWN
    scores -- or (sel_in, sel_out), (B, C) integer tensors as the device writes them (-1 where nothing is selected): teacher-forced,
    the chart then is the same function as the device's even where two splits nearly tie.  soft=True puts the softmax back (the
    reference's chart: what pins this restatement against the oracle).

    -> dict: inside_h / outside_h (B, C, D), inside_s / outside_s (B, C), split_s_in / split_s_out {level: (B, Lc, N)} the per-split
    scores, sel_in / sel_out (B, C) int64 (-1 at cells without a choice), margin_in / margin_out (B, C): best minus second-best split
    score of the cell (inf where it has fewer than two splits), relu_margin: the smallest |ReLU pre-activation| / std of its layer and
    level over the SELECTED pairs of both passes (the pairs a hard chart composes; every other pair is multiplied by 0, value and
    derivative), relu_margin_all: over every pair.
    """
    B, L, D = x_span.shape
    C = L * (L + 1) // 2
    off, tabs = _pair_tables(L)
    P = {k: v.to(dtype) for k, v in params.items()}
    x = x_span.to(dtype)
    nrm = (lambda t: t / t.norm(p=2, dim=-1, keepdim=True).clamp(min=EPS)) if normalize == 'unit' else (lambda t: t)

    def side(pre):
        pre = 'inside' if share else pre
        return (P[pre + '_compose_func.h_fcs.0.weight'], P[pre + '_compose_func.h_fcs.0.bias'], P[pre + '_compose_func.h_fcs.2.weight'],
                P[pre + '_compose_func.h_fcs.2.bias'], P[pre + '_score_func.mat'])

    z = lambda *shape: torch.zeros(*shape, dtype=dtype)
    IH, IS, OH, OS = z(B, C, D), z(B, C), z(B, C, D), z(B, C)
    sel = {'in': torch.full((B, C), -1, dtype=torch.int64), 'out': torch.full((B, C), -1, dtype=torch.int64)}
    margin = {'in': torch.full((B, C), float('inf'), dtype=dtype), 'out': torch.full((B, C), float('inf'), dtype=dtype)}
    split_s = {'in': {}, 'out': {}}
    given, clear = {'in': None, 'out': None}, [float('inf'), float('inf')]
    if selection is not None:
        given = {'in': selection[0].detach().cpu().long(), 'out': selection[1].detach().cpu().long()}

    def cell_level(which, level, AH, AS, BH, BS, W):
        """One level: operands a from the charts (AH, AS), b from (BH, BS) -> (h, s) of its cells."""
        W1, b1, W2, b2, M = W
        a, b = tabs[which][level]
        Lc, N = a.shape
        o = int(off[level])
        ah, bh = AH[:, a], BH[:, b]                                            # (B, Lc, N, D)
        z1 = F.linear(torch.cat([ah, bh], -1), W1, b1)
        z2 = F.linear(F.relu(z1), W2, b2)
        y = F.relu(z2)
        s = torch.einsum('blnd,de,blne->bln', ah, M, bh) + AS[:, a] + BS[:, b]
        split_s[which][level] = s
        if N > 1:
            top = s.detach().topk(2, dim=-1).values
            margin[which][:, o:o + Lc] = top[..., 0] - top[..., 1]
        if soft:
            p = torch.softmax(s, dim=-1)
        else:
            k = given[which][:, o:o + Lc] if given[which] is not None else _first_argmax(s.detach())
            sel[which][:, o:o + Lc] = k
            p = F.one_hot(k, N).to(dtype)                                      # detached: the selection carries no gradient
        for zz in (z1.detach(), z2.detach()):                                  # how far the ReLUs of the level stay from their kink
            r = zz.abs() / zz.std()
            clear[1] = min(clear[1], float(r.min()))
            if not soft:                                                       # ... those of the selected pairs: the only ones a hard chart evaluates
                clear[0] = min(clear[0], float(r[p > 0].min()))
        return nrm((y * p.unsqueeze(-1)).sum(2)), (s * p).sum(-1)

    # leaves: diora.py:58-63, 283-292
    IH[:, :L] = nrm(torch.tanh(F.linear(x, P['inside_compose_func.leaf_fc.weight'], P['inside_compose_func.leaf_fc.bias'])))
    Win = side('inside')
    for level in range(1, L):                                                  # diora.py:295-331
        o, Lc = int(off[level]), L - level
        h, s = cell_level('in', level, IH, IS, IH, IS, Win)
        IH[:, o:o + Lc], IS[:, o:o + Lc] = h, s
    if outside:                                                                # diora.py:337-398
        Wout = side('outside')
        OH[:, C - 1:] = nrm(P['root_vector_out_h'].view(1, 1, D).expand(B, 1, D))
        for level in range(L - 2, -1, -1):
            o, Lc = int(off[level]), L - level
            h, s = cell_level('out', level, IH, IS, OH, OS, Wout)              # [sibling, parent]: diora.py:366-368
            OH[:, o:o + Lc], OS[:, o:o + Lc] = h, s
    return dict(inside_h=IH, inside_s=IS, outside_h=OH, outside_s=OS, split_s_in=split_s['in'], split_s_out=split_s['out'],
                sel_in=sel['in'], sel_out=sel['out'], margin_in=margin['in'], margin_out=margin['out'], relu_margin=clear[0], relu_margin_all=clear[1])


def level_offsets(L):
    """Chart offset of every level: level * L - level * (level - 1) / 2."""
    return [level * L - level * (level - 1) // 2 for level in range(L)]


def own_rows(L, n):
    """The rows of a chart of length L that hold sentence n's own triangle, in the order of the cells of a chart of length n: row
    level_offset_L[level] + pos for pos < n - level, level by level -- int64 (n (n + 1) / 2,).  Only a cell's row moves between the
    exact-length and the padded chart; its selection does not."""
    off = level_offsets(L)
    return torch.tensor([off[level] + pos for level in range(n) for pos in range(n - level)], dtype=torch.int64)


def hard_forward_ragged_torch(params, x_span_padded, lengths, share, normalize, selection=None, dtype=torch.float64):
    """The yardstick of cliora_chart_forward_ragged_hard: ``hard_forward_torch`` on every sentence ALONE at its exact length (both
    passes), scattered into padded charts -- NaN beyond each sentence's triangle, so nothing there can be read by accident.

    x_span_padded (B, L, D), lengths: n_b in 1..L.  selection: None, or the PADDED (sel_in, sel_out) (B, C_L) arrays as the device
    writes them: sentence b is then teacher-forced by its own triangle's entries, re-rowed to the chart of length n_b (own_rows).
    Everything stays in the autograd graph of `params` and `x_span_padded`: a loss that reads own cells only (index them; a product
    with 0 would keep the NaN) is the sum of the per-sentence losses, and its gradients are theirs summed.

    -> dict: inside_h / outside_h (B, C_L, D), inside_s / outside_s (B, C_L); sel_in / sel_out (B, C_L) int64, -1 where a sentence
    selects nothing (leaves, its outside root, beyond its triangle); margin_in / margin_out (B, C_L), inf there; margin_rel: per
    sentence the smallest margin of both passes over max |inside_s| of that sentence (hard_cases.min_margin_rel's quantity);
    relu_margin / relu_margin_all: the smallest over the sentences, over the selected pairs / over every pair."""
    B, L, D = x_span_padded.shape
    C = L * (L + 1) // 2
    IH, OH = (torch.full((B, C, D), float('nan'), dtype=dtype) for _ in range(2))
    IS, OS = (torch.full((B, C), float('nan'), dtype=dtype) for _ in range(2))
    sel = [torch.full((B, C), -1, dtype=torch.int64) for _ in range(2)]
    margin = [torch.full((B, C), float('inf'), dtype=dtype) for _ in range(2)]
    margin_rel, relu, relu_all = [], float('inf'), float('inf')
    for b, n in enumerate(int(v) for v in lengths):
        rows = own_rows(L, n)
        given = None
        if selection is not None:
            given = tuple(s.detach().cpu().long()[b:b + 1, rows].clone() for s in selection)
            given[1][:, -1] = -1                                               # the sentence's own outside root selects nothing
        o = hard_forward_torch(params, x_span_padded[b:b + 1, :n], share, normalize, outside=True, selection=given, dtype=dtype)
        IH[b, rows], IS[b, rows], OH[b, rows], OS[b, rows] = o['inside_h'][0], o['inside_s'][0], o['outside_h'][0], o['outside_s'][0]
        sel[0][b, rows], sel[1][b, rows] = o['sel_in'][0], o['sel_out'][0]
        margin[0][b, rows], margin[1][b, rows] = o['margin_in'][0], o['margin_out'][0]
        scale = max(1e-30, float(o['inside_s'].detach().abs().max()))
        margin_rel.append(min(float(o['margin_in'].min()), float(o['margin_out'].min())) / scale)
        relu, relu_all = min(relu, o['relu_margin']), min(relu_all, o['relu_margin_all'])
    return dict(inside_h=IH, inside_s=IS, outside_h=OH, outside_s=OS, sel_in=sel[0], sel_out=sel[1], margin_in=margin[0],
                margin_out=margin[1], margin_rel=margin_rel, relu_margin=relu, relu_margin_all=relu_all)


def hard_spans_ragged_numpy(sel_in, lengths, L):
    """``hard_spans_numpy`` for a right-padded chart of length L, as cliora_hard_spans_ragged emits it: sentence b is walked from its own
    root (n_b - 1, 0) with the padded chart's level offsets -- n_b - 1 rows, the root last, (-1, -1) beyond; a length outside [1, L]
    gets -1 in every row."""
    return hard_spans_numpy(sel_in, L, lengths)


def hard_spans_numpy(sel_in, L, lengths=None):
    """The tree of a hard chart from its inside selections, as cliora_hard_spans emits it: int32 (B, L-1, 2) of (start, end) word
    positions, children before parents, left subtree first, the root last.  sel_in: (B, C) integers, the split of every cell above
    the leaves (cell (level, pos) with split k has the children (k, pos) and (level - k - 1, pos + k + 1)).  lengths: see
    hard_spans_ragged_numpy."""
    sel = np.asarray(sel_in.cpu() if torch.is_tensor(sel_in) else sel_in)
    B = sel.shape[0]
    off = level_offsets(L)
    out = np.zeros((B, max(L - 1, 0), 2), dtype=np.int32)
    for b in range(B):
        n = L if lengths is None else int(lengths[b])
        out[b, max(n - 1, 0) if 1 <= n <= L else 0:] = -1
        if not 1 <= n <= L:
            continue
        rows = walk_spans(n, lambda level, pos: min(max(int(sel[b, off[level] + pos]), 0), level - 1))     # (the device's clamp)
        out[b, :len(rows)] = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    return out


def inside_tree_from_spans(spans):
    """The mapping the reference's TreesFromDiora.parse_batch reads (analysis/diora_tree.py:47-64): {(b, 0): {(L-1, 0): [(level, pos),
    ...]}} -- the cells of sentence b's tree above the leaves, from its span list (B, L-1, 2)."""
    spans = np.asarray(spans)
    L = spans.shape[1] + 1
    return {(b, 0): {(L - 1, 0): [(int(e - s), int(s)) for s, e in spans[b]]} for b in range(spans.shape[0])}
