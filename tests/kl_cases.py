"""Shared by test_kl_cpu.py and test_gpu_kl.py (not a test module): the yardsticks of the divergence between two charts' parse
distributions (cliora_amd/structured.py, cliora_tree_kl), their cases and the figures measured for them.

The yardstick chain: enumeration of every binary tree (posterior_cases.all_trees) and central differences of the enumerated J for
``tree_kl_numpy``; ``tree_kl_numpy`` on the device's own per-split scores of both charts for the kernel; the fp64 oracle with a torch
restatement of J = a mean kl + b mean cross_entropy on the oracle's scores of both nets, differentiated by autograd, for the gradients
through the two charts.
"""
import numpy as np
import torch

import constrained_cases as CC
import expectation_cases as EC
import posterior_cases as PC
import structured_cases as SC

BOUND = EC.BOUND                 # max |G - fp64| of max(1, max |G fp64|); the five scalars relative to max(1, |.|): 1e-4
ENUM_RTOL = SC.ENUM_RTOL         # tree_kl_numpy against enumeration: 1e-12
FD_H, FD_TOL, FD_NS = SC.FD_H, SC.FD_TOL, SC.FD_NS      # central differences of the enumerated J, h = 1e-6: 1e-7 absolute (section 21's bound)
ROW_SUM_TOL = SC.ROW_SUM_TOL     # 1e-12, the restatement's rows; the kernel's fp32 rows: 1e-6
GPU_ROW_SUM_TOL = 1e-6
GRAD_BOUND, SUM_TOL = SC.GRAD_BOUND, SC.SUM_TOL          # through the chart in exact-fp32 mode: 2e-4 of scale (section 5); linearity: 1e-6 of scale
SAME_TOL = 1e-6                  # the same chart as both: |kl| and d_split_p, of scale
GPU_SHAPES = EC.GPU_SHAPES       # (B, L, D): L 3 the smallest chart with a choice, L 64 the LDS maximum and the one-lane-per-split edge
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.7, -0.4))          # (w_kl, w_ce): KL only, cross-entropy only, mixed
FD_WEIGHTS = WEIGHTS[2]
RAGGED_L, RAGGED_LENGTHS = 7, (5, 1, 2, 7)
A_KL, B_CE = 0.7, -0.4           # J through the chart
TEACHER_SEED, STUDENT_SEED = PC.GPU_SEED, PC.GPU_SEED + 17

# Printed by test_gpu_kl.py on the MI355X: 'L n' -> (max |d_split_p - fp64| / scale, max |d_split_q - fp64| / scale, max relative error
# of kl, cross_entropy, entropy_p, log_z_p, log_z_q) over the three weight settings, with and without d_split_p, against tree_kl_numpy
# on the device's scores.  Expected: the fp32 rounding of the outputs.
MEASURED = {'L 3': (5.043e-9, 1.281e-8, 1.197e-8, 1.283e-8, 1.388e-8, 1.104e-8, 2.264e-8),
            'L 7': (1.479e-8, 2.773e-8, 3.195e-8, 2.664e-8, 2.296e-8, 4.746e-8, 2.734e-8),
            'L 13': (1.428e-8, 1.457e-8, 3.126e-8, 4.320e-8, 4.674e-8, 2.595e-8, 3.584e-8),
            'L 64': (1.412e-8, 2.900e-8, 5.287e-8, 3.012e-8, 5.125e-8, 4.511e-8, 3.637e-8)}
# log_z_p / log_z_q are bitwise those of cliora_span_posteriors and entropy_p is bitwise that of cliora_tree_expectation at all four
# shapes.  Central differences on the host (test_kl_cpu.py, weights 0.7 / -0.4): n 3 / 5 / 7 -> max |G - fd| over both gradients
# 9.1e-11 / 4.4e-10 / 1.2e-9.  Ten Trainer.steps at D 32 / L 8 / B 8 with kl_loss_weight 1 and a frozen teacher of other random
# weights took the batch's mean KL(teacher || student) from 2.6143 to 1.7285.


def enumerated(pair_p, pair_q, n, w_kl=1.0, w_ce=0.0):
    """Sentence 0's first n words by enumeration in fp64 over BOTH score tables: -> dict(kl, cross_entropy, entropy_p, log_z_p,
    log_z_q, J, Gp, Gq {level: (n - level, level)}), the gradients tree by tree: Gq from sum_T (q(T) - p(T)) [e in T], Gp from
    sum_T p(T) [e in T] (V(T) - E_p[V]), each mapped through the first maximum of its OWN chart's row."""
    s, r = ({}, {}), ({}, {})
    for x, pair in enumerate((pair_p, pair_q)):
        for level in range(1, n):
            s[x][level] = np.asarray(pair[level][0], dtype=np.float64).reshape(-1, level)[:n - level]
            r[x][level] = s[x][level] - s[x][level].max(axis=1, keepdims=True)
    trees = PC.all_trees(n)
    Rp = np.array([sum(r[0][lv][p, k] for lv, p, k in t) for t in trees], dtype=np.float64)
    Rq = np.array([sum(r[1][lv][p, k] for lv, p, k in t) for t in trees], dtype=np.float64)
    lzp, lzq = CC.logsumexp(Rp), CC.logsumexp(Rq)
    p, q = np.exp(Rp - lzp), np.exp(Rq - lzq)
    ent, ce = float(-(p * (Rp - lzp)).sum()), float(-(p * (Rq - lzq)).sum())
    kl = float((p * ((Rp - lzp) - (Rq - lzq))).sum())
    V = w_kl * Rp - (w_kl + w_ce) * Rq
    mean_v = float((p * V).sum())
    Gp, Gq = ({level: np.zeros((n - level, level)) for level in range(1, n)} for _ in range(2))
    for t, tree in enumerate(trees):
        for level, pos, k in tree:
            for G, d, sc in ((Gp, p[t] * (V[t] - mean_v), s[0]), (Gq, (w_kl + w_ce) * (q[t] - p[t]), s[1])):
                G[level][pos, k] += d
                G[level][pos, int(np.argmax(sc[level][pos]))] -= d
    return dict(kl=kl, cross_entropy=ce, entropy_p=ent, log_z_p=lzp, log_z_q=lzq, J=w_kl * kl + w_ce * ce, Gp=Gp, Gq=Gq)


def torch_kl(pair_p, pair_q, n):
    """(kl, cross_entropy) of ONE sentence from torch per-split scores {level: (n - level, level)} of both charts (fp64, in the graph),
    modelled on expectation_cases.torch_objective: E_p[f] = d log Z_p(t) / dt at t = 0 for potentials r^p + t f, so E_p[R^p] and
    E_p[R^q] are autograd derivatives of the teacher's inside log-partition with respect to two tilts (create_graph, so that they can
    be differentiated again); log_z_q is the student's plain inside pass."""
    if n == 1:
        z = torch.zeros((), dtype=torch.float64)
        return z, z.clone()
    dev = pair_p[1].device
    tp, tq = (torch.zeros((), dtype=torch.float64, device=dev, requires_grad=True) for _ in range(2))
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    a, c = {(0, p): zero for p in range(n)}, {(0, p): zero for p in range(n)}
    for level in range(1, n):
        rp = pair_p[level] - pair_p[level].max(dim=1, keepdim=True).values
        rq = pair_q[level] - pair_q[level].max(dim=1, keepdim=True).values
        for pos in range(n - level):
            a[(level, pos)] = torch.logsumexp(torch.stack([a[(k, pos)] + a[(level - k - 1, pos + k + 1)] + rp[pos, k] * (1 + tp) + rq[pos, k] * tq
                                                           for k in range(level)]), 0)
            c[(level, pos)] = torch.logsumexp(torch.stack([c[(k, pos)] + c[(level - k - 1, pos + k + 1)] + rq[pos, k] for k in range(level)]), 0)
    lzp, lzq = a[(n - 1, 0)], c[(n - 1, 0)]
    e_rp, e_rq = torch.autograd.grad(lzp, [tp, tq], create_graph=True)
    entropy, ce = lzp - e_rp, lzq - e_rq
    return ce - entropy, ce

