"""Shared by test_expectation_cpu.py and test_gpu_expectation.py (not a test module): the yardsticks of the expected cost and the
entropy of the parse distribution (cliora_amd/structured.py, cliora_tree_expectation), their cases and the figures measured for them.

The yardstick chain: enumeration of every binary tree (posterior_cases.all_trees) and central differences of the enumerated
objective for ``tree_expectation_numpy``; ``tree_expectation_numpy`` on the device's own per-split scores for the kernel; the fp64
oracle with a torch restatement of J = a mean risk + b mean entropy, differentiated by autograd, for the gradient through the chart.
"""
import numpy as np
import torch

import constrained_cases as CC
import posterior_cases as PC
import structured_cases as SC

BOUND = SC.BOUND                 # max |G - fp64| of max(1, max |G fp64|); risk, entropy, log_z relative to max(1, |.|): 1e-4
ENUM_RTOL = SC.ENUM_RTOL         # tree_expectation_numpy against enumeration: 1e-12
# Central differences of the enumerated J, h = 1e-6: the project's 1e-7 absolute (eps / h ~ 1e-10 plus the O(h^2) truncation term).
# Measured (test_expectation_cpu.py, wc 0.7, we -1.3): n 3 / 5 / 7 -> max |G - fd| 1.7e-10 / 9.5e-10 / 1.1e-9.
FD_H, FD_TOL, FD_NS = SC.FD_H, SC.FD_TOL, SC.FD_NS
ROW_SUM_TOL = SC.ROW_SUM_TOL
GRAD_BOUND, SUM_TOL = SC.GRAD_BOUND, SC.SUM_TOL
GPU_SHAPES = SC.GPU_SHAPES
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.7, -1.3))      # (wc, we): cost only, entropy only, mixed
# Printed by test_gpu_expectation.py on the MI355X: 'L n' -> (max |G - fp64| / max(1, max |G fp64|), max relative error of risk,
# entropy, log_z) over the test's weights and costs, against tree_expectation_numpy on the device's scores.  Expected: the fp32
# rounding of the outputs.
MEASURED = {'L 3': (2.713e-8, 3.503e-9, 1.388e-8, 1.104e-8), 'L 7': (1.546e-8, 4.130e-8, 2.296e-8, 4.746e-8),
            'L 13': (1.817e-8, 4.264e-8, 4.674e-8, 2.595e-8), 'L 64': (1.511e-8, 2.836e-8, 5.125e-8, 4.511e-8)}
# log_z is bitwise that of cliora_span_posteriors at all four shapes.  Ten Trainer.steps at D 32 / L 8 / B 8: risk_loss_weight 1 took the
# batch's mean risk from -0.4674 to -0.5175, entropy_loss_weight 1 the mean entropy from 4.5520 to 3.7680.


def cell_id(L, level, pos):
    rem = L - level
    return L * (L + 1) // 2 - rem * (rem + 1) // 2 + pos


def random_costs(B, L, seed):
    """(B, C) fp64 costs, uniform in [0, 1]."""
    return np.random.RandomState(seed).rand(B, L * (L + 1) // 2)


def tree_cells(tree, n):
    """Every cell (level, pos) of a tree over n words: its leaves and its internal nodes."""
    return [(0, p) for p in range(n)] + [(lv, p) for lv, p, _ in tree]


def enumerated(pair_s, n, cost_row, L, wc=1.0, we=0.0):
    """Sentence 0's first n words by enumeration in fp64: -> dict(risk, entropy, log_z, J, G {level: (n - level, level)}) with
    G the tree-by-tree gradient sum_T p(T) [e in T] (V(T) - E[V]) mapped through k* (the row's first maximum)."""
    s, r = {}, {}
    for level in range(1, n):
        s[level] = np.asarray(pair_s[level][0], dtype=np.float64).reshape(-1, level)[:n - level]
        r[level] = s[level] - s[level].max(axis=1, keepdims=True)
    trees = PC.all_trees(n)
    w = np.array([sum(r[lv][p, k] for lv, p, k in t) for t in trees], dtype=np.float64)
    log_z = CC.logsumexp(w)
    p = np.exp(w - log_z)
    tree_cost = np.array([sum(cost_row[cell_id(L, lv, q)] for lv, q in tree_cells(t, n)) for t in trees])
    risk = float((p * tree_cost).sum())
    entropy = float(-(p * (w - log_z)).sum())
    V = wc * tree_cost - we * w
    mean_v = float((p * V).sum())
    G = {level: np.zeros((n - level, level)) for level in range(1, n)}
    for t, tree in enumerate(trees):
        for level, pos, k in tree:
            kstar = int(np.argmax(s[level][pos]))
            d = p[t] * (V[t] - mean_v)
            G[level][pos, k] += d
            G[level][pos, kstar] -= d
    return dict(risk=risk, entropy=entropy, log_z=log_z, J=wc * risk + we * entropy, G=G)


def catalan(m):
    c = 1
    for i in range(m):
        c = c * 2 * (2 * i + 1) // (i + 2)
    return c


def crossing_spans(n, b):
    """Required and forbidden spans of a sentence of n words that include a crossing pair (n >= 3) and one span beyond the sentence."""
    req = [(0, 1), (1, 2)] if n == 3 else [(b % 2, n // 2), (n // 2 - 1 + b % 2, n - 1 - b % 2), (1, 2)]
    forb = [(0, n - 2)] if n > 3 else []
    return req + [(1, n + 3)], forb


def torch_objective(pair_s, n, cost_row, L):
    """(risk, entropy) of ONE sentence from torch per-split scores {level: (n - level, level)} (fp64, in the graph), by the identity
    E[f] = d log Z(t) / dt at t = 0 for potentials r + t f: risk and E[R] as autograd derivatives of the inside log-partition with
    respect to a per-cell and a per-edge tilt (create_graph, so that they can be differentiated again)."""
    dev = pair_s[1].device if n > 1 else 'cpu'
    tc = {(lv, p): torch.zeros((), dtype=torch.float64, device=dev, requires_grad=True) for lv in range(n) for p in range(n - lv)}
    te = torch.zeros((), dtype=torch.float64, device=dev, requires_grad=True)
    a = {(0, p): tc[(0, p)] * cost_row[cell_id(L, 0, p)] for p in range(n)}
    for level in range(1, n):
        sc = pair_s[level]
        r = sc - sc.max(dim=1, keepdim=True).values
        for pos in range(n - level):
            terms = torch.stack([a[(k, pos)] + a[(level - k - 1, pos + k + 1)] + r[pos, k] * (1 + te) for k in range(level)])
            a[(level, pos)] = torch.logsumexp(terms, 0) + tc[(level, pos)] * cost_row[cell_id(L, level, pos)]
    root = a[(n - 1, 0)]
    if n == 1:
        return root * 0 + cost_row[cell_id(L, 0, 0)], root * 0
    grads = torch.autograd.grad(root, list(tc.values()) + [te], create_graph=True)
    return sum(grads[:-1]), root - grads[-1]
