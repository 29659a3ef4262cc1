"""Shared by test_constrained_cpu.py and test_gpu_constrained.py (not a test module): the yardsticks of parsing under brackets
(cliora_amd/constrained.py, cliora_constrained_parse), its pinned cases and the figures measured for it.

The yardstick chain: enumeration of every binary tree in fp64 (posterior_cases.all_trees) for ``constrained_numpy``;
``constrained_numpy`` on the device's own per-split scores for the kernel -- never the code under test against itself.
"""
import functools
import itertools

import numpy as np

import posterior_cases as PC
import sample_cases as SC

BOUND = PC.BOUND                                     # |log_z_c - fp64|, |log_prob - fp64| (relative to max(1, |.|)), max |mu_c - fp64|: 1e-4
ENUM_RTOL = SC.ENUM_RTOL                             # constrained_numpy against enumeration: 1e-12
ENUM_NS = range(1, 8)
# Seeds of the enumeration cases, scores random_scores(1, max(n, 2), 100 n + seed): every one of 0 .. 2 keeps, over every bracket set
# of its case, an fp64 gap between the two best qualifying trees above BEST_GAP, so that the fp32 recurrence cannot pick the other one
# (its rounding over at most 13 additions of magnitudes below 64 stays under 13 * 64 * 6e-8 = 5e-5).  gap_search() recomputes them.
ENUM_SEEDS = (0, 1, 2)
BEST_GAP = 1e-4
ENUM_MIN_GAP = 3.326e-3                              # the smallest gap over all cases (n 5, seed 1), as gap_search() gives it: {0: 8.472e-3, 1: 3.326e-3, 2: 4.610e-3}
RANDOM_SETS = 3                                      # larger random bracket sets per (n, seed): 3 .. 6 rows each

# ---- the device -----------------------------------------------------------------------------------------------------------------------
GPU_LENGTHS = (1, 2, 3, 7, 13)
NUMPY_LENGTHS = (7, 13)
LONG_LENGTHS = (65, 128)                             # B 2: the long instance, above 64 KiB of LDS
GPU_SAMPLE_SEED = 0x5eed5a3b1e5
# Printed by test_gpu_constrained.py on the MI355X (text-only DioraMLP, D 16, B 3, unless named otherwise): what -> (max |log_z_c -
# fp64| / max(1, |.|), max |log_prob - fp64| / max(1, |.|), max |mu_c - fp64|) against constrained_numpy on the device's scores, the
# worst over the test's bracket sets.  All are the fp32 rounding of the outputs (half an ulp of 1 is 3e-8), under the 1e-4 bound.
MEASURED = {'L 7': (3.995e-8, 3.040e-8, 2.971e-8), 'L 13': (5.039e-8, 3.078e-8, 2.915e-8),
            'padded L 14': (2.538e-8, 4.076e-8, 2.773e-8), 'padded L 70': (2.929e-8, 4.356e-8, 2.839e-8),
            'L 7, infeasible neighbours': (6.059e-9, 2.624e-8, 1.955e-8), 'TreeLSTM L 5': (1.450e-8, 1.858e-8, 2.388e-8),
            'CLIORA L 7 (R 36)': (2.644e-8, 3.912e-8, 2.312e-8)}
# The links to the other decoders: max |exp(log_prob) - mu| over the single brackets of L 7 (required: mu, forbidden: 1 - mu) 3.052e-8;
# max |log_prob - sample.log_prob| with a sampled tree's spans required 0.0 at L 13, 65 and 128 (the same fp64 sum rounded once).
MEASURED_LINKS = {'single bracket L 7': 3.052e-8, 'sampled tree L 13': 0.0, 'sampled tree L 65': 0.0, 'sampled tree L 128': 0.0}


def enum_scores(n, seed):
    return PC.random_scores(1, max(n, 2), 100 * n + seed)


def cells(n):
    """Every (start, end) of a sentence of n words, leaves and root included."""
    return [(pos, pos + level) for level in range(n) for pos in range(n - level)]


@functools.lru_cache(maxsize=None)
def enumeration(n, seed):
    """-> (pair_s, trees, their fp64 weights sum of r, member[tree, start, end]: the tree holds the span (leaves too))."""
    pair_s = enum_scores(n, seed)
    r = {}
    for level in range(1, n):
        s = np.asarray(pair_s[level][0], dtype=np.float64).reshape(-1, level)
        for pos in range(n - level):
            r[(level, pos)] = s[pos] - s[pos].max()
    trees = PC.all_trees(n)
    w = np.array([sum(r[(lv, p)][k] for lv, p, k in t) for t in trees], dtype=np.float64)
    member = np.zeros((len(trees), n, n), dtype=bool)
    member[:, np.arange(n), np.arange(n)] = True
    for t, tree in enumerate(trees):
        for lv, p, _ in tree:
            member[t, p, p + lv] = True
    return pair_s, trees, w, member


def logsumexp(x):
    if x.size == 0:
        return -np.inf
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def enumerate_constrained(n, seed, rows):
    """rows: [(start, end, kind)].  By enumeration in fp64: -> dict(log_z, log_zc (-inf without a qualifying tree), best (the spans of
    the heaviest qualifying tree, or None), gap (between the two heaviest, inf with fewer than two), mu[start, end]: the share of the
    qualifying mass in trees that hold the span, zeros without one)."""
    _, trees, w, member = enumeration(n, seed)
    ok = np.ones(len(trees), dtype=bool)
    for s, e, kind in rows:
        ok &= member[:, s, e] if kind == 1 else ~member[:, s, e]
    wq = w[ok]
    out = dict(log_z=logsumexp(w), log_zc=logsumexp(wq), best=None, gap=np.inf, mu=np.zeros((n, n)))
    if wq.size:
        order = np.argsort(-wq, kind='stable')
        out['best'] = PC.tree_spans(trees[int(np.flatnonzero(ok)[order[0]])])
        if wq.size > 1:
            out['gap'] = float(wq[order[0]] - wq[order[1]])
        p = np.exp(wq - out['log_zc'])
        out['mu'] = np.tensordot(p, member[ok].astype(np.float64), axes=1)
    return out


def bracket_sets(n, seed):
    """Every single bracket and every pair of distinct brackets of either kind over every cell (a cell both required and forbidden
    among them), then RANDOM_SETS larger sets: -> [[(start, end, kind)]]."""
    items = [(s, e, kind) for s, e in cells(n) for kind in (1, 0)]
    sets = [[it] for it in items] + [list(p) for p in itertools.combinations(items, 2)]
    rs = np.random.RandomState(7000 + 100 * n + seed)
    for _ in range(RANDOM_SETS):
        size = min(len(items), int(rs.randint(3, 7)))
        sets.append([items[i] for i in rs.choice(len(items), size=size, replace=False)])
    return sets


def pack_rows(sets, M=None):
    """[[(start, end, kind)]] -> (len(sets), M, 3) int32, -1 rows beyond each set."""
    M = max(len(s) for s in sets) if M is None else M
    out = np.full((len(sets), M, 3), -1, dtype=np.int32)
    for b, rows in enumerate(sets):
        if rows:
            out[b, :len(rows)] = np.asarray(rows, dtype=np.int32)
    return out


def repeat_scores(pair_s, count):
    """The one sentence of pair_s as `count` sentences (views, no copy)."""
    return {level: np.broadcast_to(s, (count,) + s.shape[1:]) for level, s in pair_s.items()}


def gap_search(seeds=range(10)):
    """seed -> the smallest gap between the two best qualifying trees over every n and every bracket set of the seed's cases."""
    out = {}
    for seed in seeds:
        out[seed] = min(enumerate_constrained(n, seed, rows)['gap'] for n in ENUM_NS for rows in bracket_sets(n, seed))
    return out


# ---- bracket sets for the device tests ----------------------------------------------------------------------------------------------
def nested_required(n, b):
    """A nested (laminar) required set of a sentence of n words, shifted by the sentence's row b: about n / 4 brackets."""
    rows, lo, hi = [], b % 2, n - 1 - ((b + 1) % 2)
    while hi - lo >= 1 and len(rows) < max(1, n // 4):
        rows.append((lo, hi))
        lo, hi = lo + 1, hi - (1 if len(rows) % 2 else 0)
    return rows


span_key = SC.span_key
