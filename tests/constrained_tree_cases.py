"""Shared by test_constrained_tree_cpu.py and test_gpu_constrained_tree.py (not a test module): the device cases of the K best and
sampled trees under brackets (cliora_kbest_spans_constrained, cliora_sample_trees_constrained) and the figures measured for them.
The yardsticks and their bounds are constrained_cases.py's and sample_cases.py's.
"""
import constrained_cases as CC

KS = (1, 4, 16)
LENGTHS = tuple(sorted(CC.GPU_LENGTHS + (6,)))       # 6: the first length at which Catalan(L - 1) exceeds 16
# The draws of the device tests use constrained_cases.GPU_SAMPLE_SEED.  On the fp64 oracle's scores of the same sentences it gives
# constrained_sample_numpy no margin below sample_cases.MARGIN on any case below (test_constrained_tree_cpu.py asserts it; the smallest
# is ORACLE_MIN_MARGIN), so no other seed had to be picked.
ORACLE_MIN_MARGIN = 8.197e-6                         # L 7, nested + forbidden (the device's scores there: 8.152e-6)
# Printed by test_gpu_constrained_tree.py on the MI355X (text-only DioraMLP, D 16, against the restatements on the device's scores):
# what -> (max |log_prob - fp64|, max |log_z_c - fp64|, samples left out, the restatement's smallest margin); the lists of
# cliora_kbest_spans_constrained are equal bit for bit, so they have no figure.
MEASURED = {'L <= 13, S 64': (4.756e-7, 3.347e-7, 0, 8.152e-6), 'L 65, S 16': (1.872e-6, 9.486e-8, 0, 2.655e-5),
            'L 128, S 8, M 256': (3.398e-6, 1.503e-7, 0, 4.473e-6), 'padded L 14': (2.304e-8, 6.763e-9, 0, 9.551e-3),
            'TreeLSTM L 5': (1.121e-7, 1.450e-8, 0, 3.804e-4)}


def nested(n, B, forbidden=()):
    """Per sentence of a chart of B: constrained_cases.nested_required as required rows, then the forbidden spans that lie in it."""
    return [[(s, e, 1) for s, e in CC.nested_required(n, b)] + [(s, e, 0) for s, e in forbidden if e < n] for b in range(B)]


def cases(L, B):
    """Bracket sets of a chart of B <= 3 sentences of L words, by name -> (B, M, 3) rows.  From L 6 on every set but the last leaves
    every sentence a tree and takes some away; the last leaves its second sentence none (a crossing required pair)."""
    if L < 3:
        return {'leaf / root': CC.pack_rows([[(0, 0, 1)], [(0, L - 1, 1)], []][:B], 2)}
    mid = L // 2
    return {'nested': CC.pack_rows(nested(L, B)),
            'nested + forbidden': CC.pack_rows(nested(L, B, forbidden=[(1, 2), (4, 5), (L - 2, L - 1)])),
            'forbidden only': CC.pack_rows([[(0, 1, 0), (1, 2, 0)], [(mid - 1, mid, 0)], [(0, L - 2, 0), (1, L - 1, 0)]][:B]),
            'one infeasible': CC.pack_rows([[(0, mid, 1)], [(0, mid, 1), (mid, L - 1, 1)], [(1, L - 1, 1)]][:B])}
