"""Shared by test_margin_cpu.py and test_gpu_margin.py (not a test module): the yardsticks of the max-margin bracket losses
(cliora_amd/structured.py, cliora_bracket_margin), their cases and the figures measured for them.

The yardstick chain: enumeration of every binary tree in fp64, from the definitions, and central differences for
``bracket_margin_numpy``; ``bracket_margin_numpy`` on the device's own per-split scores for the kernel -- trees, violations, feasible
and the gradient exactly, the three scalars to the rounding of one fp32 store; the fp64 oracle with a torch restatement of the tree
score difference, teacher-forced by the device's two span lists, for the gradient through the chart.
"""
import numpy as np

import posterior_cases as PC
import structured_cases as SC

INF = float('inf')
PARAMS = ((1.0, INF), (0.0, INF), (1.0, 1.0), (0.5, 2.0))        # (margin, penalty): hinge, perceptron, two ramps
ENUM_NS = range(1, 8)
ENUM_SEEDS = (0, 1, 2)            # scores SC.gapped_scores(n, 3000 + 10 n + seed)
ENUM_TOL = 1e-12                  # loss, both scores: bracket_margin_numpy against enumeration
MIN_GAP = 1e-3                    # asserted per case: the fp64 gap between the two best trees of each pass
ENUM_MEASURED_MIN_GAP = 3.419e-3  # gap_search(): the smallest over every case of the three seeds, {0: 4.588e-2, 1: 3.419e-3, 2: 3.004e-2}
FD_H, FD_TOL = 1e-6, 1e-6         # central differences of the restated loss: it is piecewise linear, so only eps / h ~ 1e-10 is left
SCALAR_RTOL = 1e-6                # device loss / scores against fp64, of max(1, |want|): the rounding of one fp32 store (6e-8) with room
GRAD_BOUND = SC.GRAD_BOUND        # through the chart, exact mode: 2e-4 of scale
SUM_TOL = SC.SUM_TOL              # linearity of the chart backward in its cotangents: 1e-6 of scale

GPU_SHAPES = SC.GPU_SHAPES + ((2, 1, 16), (2, 2, 16))
PADDED_L, PADDED_LENGTHS = 5, (1, 2, 3, 5, 5)
# Printed by test_gpu_margin.py on the MI355X: 'L n' -> max over the bracket sets and PARAMS of |loss - fp64|, |aug - fp64|,
# |ref - fp64|, each over max(1, |fp64|).  Expected: the fp32 rounding of the output (half an ulp is 6e-8 relative).
MEASURED = {'L 3': (5.544e-8, 0.0, 5.544e-8), 'L 7': (5.107e-8, 5.700e-8, 4.131e-8), 'L 13': (5.940e-8, 5.639e-8, 4.807e-8),
            'L 64': (5.071e-8, 5.711e-8, 4.951e-8), 'L 1': (0.0, 0.0, 0.0), 'L 2': (0.0, 0.0, 0.0), 'padded L 5': (5.137e-8, 0.0, 0.0)}
# Ten Trainer.steps at D 32 / L 8 / B 8 with hinge_loss_weight 1: the batch's mean hinge before -> after.
MEASURED_TRAINING = {'penalty inf': (6.0534, 3.4744), 'penalty 2': (5.8462, 3.4665)}
# Through the chart, exact mode: the mean hinge of the four shapes agreed with the fp64 oracle's to 1e-6 (13.461899 against 13.461898).


def enum_scores(n, seed):
    return SC.gapped_scores(n, 3000 + 10 * n + seed)


def crossing_pair(n):
    """Two required brackets that cross: no tree holds both (n >= 3)."""
    return [(0, 1, 1), (1, 2, 1)] if n == 3 else [(0, 2, 1), (1, 3, 1)]


def enum_sets(n, seed=0):
    """name -> rows: structured_cases.bracket_sets (the rows that fit a short sentence), plus a crossing pair of required brackets."""
    if n >= 3:
        sets = dict(SC.bracket_sets(n, seed))
        sets['crossing'] = crossing_pair(n)
    else:
        sets = {'single': [(0, 1, 1)], 'forbidden leaf': [(0, 0, 0)], 'required leaf': [(n - 1, n - 1, 1)]}
    return {name: [r for r in rows if r[1] < n] for name, rows in sets.items()}


def crosses(a, b):
    (i, j), (s, e) = a, b
    return i < s <= j < e or s < i <= e < j


def disallowed(span, rows):
    """The definition: the span crosses a required bracket or equals a forbidden one."""
    return any((k == 1 and crosses(span, (s, e))) or (k == 0 and span == (s, e)) for s, e, k in rows)


def enumerate_margin(pair_s, n, rows, margin, penalty):
    """One sentence by enumeration in fp64, from the definitions.  pair_s {level: (1, n - level, level)}.  -> dict: aug / ref (the
    two maxima; ref -inf without a qualifying tree), loss (0 then), feasible, violations (of the augmented tree), tree_a / tree_b (the
    argmax trees as sets of (level, pos, split); tree_b None when infeasible), gap (the smaller of the two passes' top-two gaps)."""
    r = {}
    for level in range(1, n):
        s = np.asarray(pair_s[level][0], dtype=np.float64).reshape(-1, level)
        for pos in range(n - level):
            r[(level, pos)] = s[pos] - s[pos].max()
    trees = PC.all_trees(n)
    F = np.array([sum(r[(lv, p)][k] for lv, p, k in t) for t in trees], dtype=np.float64)
    D = np.array([sum(disallowed((p, p + lv), rows) for lv, p, _ in t if 1 <= lv <= n - 2) for t in trees], dtype=np.float64)
    obj_a = F + margin * D
    if penalty == INF:                                  # the qualifying trees of section 19: leaves and the root count too
        bad_fixed = any(disallowed((p, p), rows) for p in range(n)) or disallowed((0, n - 1), rows)
        obj_b = np.where((D == 0) & (not bad_fixed), F, -np.inf)
    else:
        obj_b = F - penalty * D

    def top(obj):
        order = np.argsort(-obj, kind='stable')
        gap = float(obj[order[0]] - obj[order[1]]) if len(order) > 1 and np.isfinite(obj[order[1]]) else np.inf
        return int(order[0]), gap
    ia, gap_a = top(obj_a)
    ib, gap_b = top(obj_b)
    feasible = bool(np.isfinite(obj_b[ib]))
    return dict(aug=float(obj_a[ia]), ref=float(obj_b[ib]) if feasible else -np.inf, loss=float(obj_a[ia] - obj_b[ib]) if feasible else 0.0,
                feasible=feasible, violations=int(D[ia]), tree_a=set(trees[ia]), tree_b=set(trees[ib]) if feasible else None,
                gap=min(gap_a, gap_b if feasible else np.inf))


def tree_of(spans_row, splits=None):
    """A span list of one sentence -> the set of its (start, end) rows (the -1 rows dropped)."""
    return set((int(s), int(e)) for s, e in spans_row if s >= 0)


def gap_search(seeds=ENUM_SEEDS):
    """seed -> the smallest enumerate_margin gap over every n, bracket set and parameter pair of the seed's cases."""
    out = {}
    for seed in seeds:
        out[seed] = min(enumerate_margin(enum_scores(n, seed), n, rows, m, p)['gap']
                        for n in ENUM_NS for rows in enum_sets(n, seed).values() for m, p in PARAMS)
    return out
