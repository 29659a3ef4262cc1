"""Shared by test_kbest_cpu.py and test_gpu_kbest.py (not a test module): the yardsticks of the k-best decode (cliora_amd/kbest.py,
cliora_kbest_spans) and the figures measured for it.

The yardsticks: enumeration of every binary tree in fp64 (posterior_cases.all_trees) for ``kbest_numpy``; ``kbest_numpy`` on the
device's own per-split scores, bit for bit, for the kernel; the lists of the keys alone, written from the definition, for exact ties.
"""
import numpy as np

import posterior_cases as PC

KS = (1, 3, 8, 16)
CATALAN = [1, 1, 2, 5, 14, 42, 132, 429]             # Catalan(n - 1) at index n - 1: the trees of n = 1 .. 8 words

# ---- kbest_numpy against enumeration ------------------------------------------------------------------------------------------------
# n = 1 .. 8, seeds 0 .. 19, scores random_scores(1, max(n, 2), 100 n + seed).  GAP: the smallest fp64 difference between consecutive
# trees among the best K + 1 that the test demands of every case -- about 20 times the fp32 summation error of 7 additions at this
# scale; SCORE_BOUND: 7 roundings of half an ulp(16) = 7 * 9.5e-7 bound |score - fp64| by 7e-6.
ENUM_SEEDS = range(20)
GAP = 1e-4
SCORE_BOUND = 1e-5
# What test_kbest_cpu.py prints on the host (numpy fp32; no device involved): the smallest gap it meets over every case and the
# largest |score - fp64|.
MEASURED_MIN_GAP = 4.364e-4                           # n 8
MEASURED_MAX_SCORE_ERR = 8.345e-7                     # n 5

# ---- the device ---------------------------------------------------------------------------------------------------------------------
GPU_LENGTHS = (1, 2, 3, 7, 13)
# (L, K): 65 / 4 is the long instance (two splits per lane) with its lists in LDS (8 C K = 68.6 KB), 128 / 8 the long instance with its
# lists in global scratch (528 KB a sentence).
GPU_LONG = ((65, 4), (128, 8))
MASS_BOUND = PC.BOUND                                # |sum over all 14 trees of exp(score - log_z) - 1| at L 5: the project's bound
# Printed by test_gpu_kbest.py on the MI355X: {'mass': max |sum exp(score - log_z) - 1| at L 5}.
MEASURED = {'mass': 9.517e-8}


def enum_scores(n, seed):
    return PC.random_scores(1, max(n, 2), 100 * n + seed)


def ranked_trees(pair_s, b, n):
    """Every binary tree of sentence b's first n words with its fp64 total, best first: -> (trees, totals)."""
    r = {}
    for level in range(1, n):
        s = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)
        for pos in range(n - level):
            r[(level, pos)] = s[pos] - s[pos].max()
    trees = PC.all_trees(n)
    w = np.array([sum(r[(lv, p)][k] for lv, p, k in t) for t in trees], dtype=np.float64)
    order = np.argsort(-w, kind='stable')
    return [trees[i] for i in order], w[order]


def key_order_lists(n, K):
    """The lists when every candidate of a cell ties: the first K of (split, left rank, right rank) in lexicographic order, by level
    (the position does not matter).  -> {level: [(k, i, j)]}, from the definition alone."""
    lists = {0: [None]}
    for level in range(1, n):
        lists[level] = [(k, i, j) for k in range(level) for i in range(len(lists[k]))
                        for j in range(len(lists[level - k - 1]))][:K]
    return lists


def key_order_spans(n, K):
    """The spans of the trees of key_order_lists' root list, children before parents."""
    lists = key_order_lists(n, K)

    def spans(level, pos, rank):
        if level == 0:
            return []
        k, i, j = lists[level][rank]
        return spans(k, pos, i) + spans(level - k - 1, pos + k + 1, j) + [(pos, pos + level)]
    return [spans(n - 1, 0, t) for t in range(len(lists[n - 1]))] if n > 1 else [[]]
