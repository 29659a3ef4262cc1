"""Shared by test_structured_cpu.py and test_gpu_structured.py (not a test module): the yardsticks of the bracket loss
(cliora_amd/structured.py, cliora_bracket_grad, cliora_chart_backward_split), its cases and the figures measured for it.

The yardstick chain: central differences of ``constrained_numpy``'s fp64 log_prob and enumeration of every binary tree for
``bracket_grad_numpy``; ``bracket_grad_numpy`` on the device's own per-split scores for the kernel; the fp64 oracle with a torch
restatement of the two inside recurrences, differentiated by autograd, for the gradient through the chart.
"""
import numpy as np
import torch

import constrained_cases as CC
import posterior_cases as PC

BOUND = PC.BOUND                 # max |G - fp64|: 1e-4, the bound the project holds mu to (every G entry is a difference of probabilities)
ENUM_RTOL = CC.ENUM_RTOL         # bracket_grad_numpy against enumeration: 1e-12
FD_H, FD_TOL = 1e-6, 1e-7        # central differences of the fp64 log_prob: eps / h ~ 1e-10 plus the O(h^2) truncation term
FD_NS = (3, 5, 7)
FD_MIN_GAP = 1e-3                # every row's top-two gap: the perturbation stays clear of a change of argmax
ROW_SUM_TOL = 1e-12
GRAD_BOUND = 2e-4                # the project's exact-mode gradient bound, of scale, element-wise
SUM_TOL = 1e-6                   # linearity of the chart backward in its cotangents, of scale

# (B, L, D) of the kernel-alone device tests
GPU_SHAPES = ((3, 3, 16), (3, 7, 16), (2, 13, 48), (2, 64, 32))
# Printed by test_gpu_structured.py on the MI355X: 'L n' -> max |G - fp64| over the test's bracket sets, against bracket_grad_numpy on
# the device's scores.  Expected: the fp32 rounding of the output (half an ulp of 1 is 3e-8).
MEASURED = {'L 3': 5.749e-9, 'L 7': 2.931e-8, 'L 13': 2.892e-8, 'L 64': 2.980e-8}
# Central differences on the host (test_structured_cpu.py): n 3 / 5 / 7 -> max |G - fd| 3.1e-11 / 3.7e-10 / 4.2e-10.  Ten Trainer.steps at D 32 /
# L 8 / B 8 with bracket_loss_weight 1 took the batch's bracket_nll from 2.982 to 1.668.


def gapped_scores(n, seed, scale=1.5):
    """{level: (1, n - level, level)} fp64 N(0, scale^2) scores, redrawn until every row's top-two gap exceeds FD_MIN_GAP."""
    rs = np.random.RandomState(seed)
    while True:
        s = {level: scale * rs.randn(1, n - level, level) for level in range(1, n)}
        ok = True
        for level in range(2, n):
            top = np.sort(s[level][0], axis=1)
            ok &= bool((top[:, -1] - top[:, -2] > FD_MIN_GAP).all())
        if ok:
            return s


def gold_tree_rows(n, seed):
    """The n - 2 inner brackets (required) of a random binary tree over n words."""
    rs = np.random.RandomState(seed)
    rows = []

    def build(lo, hi):
        if hi == lo:
            return
        if (lo, hi) != (0, n - 1):
            rows.append((lo, hi, 1))
        k = int(rs.randint(lo, hi))
        build(lo, k)
        build(k + 1, hi)
    build(0, n - 1)
    return rows


def bracket_sets(n, seed=0):
    """name -> [(start, end, kind)]: one required bracket, nested required, required plus forbidden, a full gold tree."""
    sets = {'single': [(0, 1, 1)] if n < 4 else [(1, n - 2, 1)],
            'nested': [(s, e, 1) for s, e in CC.nested_required(n, 0)] + ([(0, 1, 1)] if n >= 5 else []),
            'required+forbidden': ([(1, n - 1, 1), (1, 2, 0)] if n >= 4 else [(1, 2, 1), (0, 1, 0)]),
            'gold tree': gold_tree_rows(n, 40 + seed)}
    return sets


def spans_as_required(spans, n):
    """A tree's span list (cky_spans' rows of one sentence) -> required rows of its inner brackets."""
    return [(int(s), int(e), 1) for s, e in spans if s >= 0 and (int(s), int(e)) != (0, n - 1)]


def torch_log_prob(pair_s, n, rows):
    """log_z_c - log_z of ONE sentence from torch per-split scores {level: (n - level, level)} (fp64, in the graph): the two inside
    recurrences restated on torch ops for autograd."""
    from cliora_amd.constrained import allowed_cells
    allowed, _ = allowed_cells(n, np.asarray(rows, dtype=np.int32).reshape(-1, 3))
    ninf = torch.tensor(-float('inf'), dtype=torch.float64, device=pair_s[1].device) if n > 1 else None

    def inside(mask):
        a = {(0, p): (torch.zeros((), dtype=torch.float64, device=ninf.device) if mask[0, p] else ninf) for p in range(n)}
        for level in range(1, n):
            s = pair_s[level]
            r = s - s.max(dim=1, keepdim=True).values
            for pos in range(n - level):
                if not mask[level, pos]:
                    a[(level, pos)] = ninf
                    continue
                terms = [a[(k, pos)] + a[(level - k - 1, pos + k + 1)] + r[pos, k] for k in range(level)
                         if a[(k, pos)] is not ninf and a[(level - k - 1, pos + k + 1)] is not ninf]
                a[(level, pos)] = torch.logsumexp(torch.stack(terms), 0) if terms else ninf
        return a[(n - 1, 0)]
    return inside(allowed) - inside(np.ones_like(allowed))
