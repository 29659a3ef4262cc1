"""Span posteriors, log-partition and MBR (cliora_amd/posterior.py, cliora_span_posteriors) without a GPU: the fp64 restatement against
enumeration of every binary tree, the fp32 MBR restatement against the best enumerated tree, the closed-form use lists against the
plan's pair tables, the MBR seeds against the fp64 oracle, and the symbol's declaration, export and binding."""
import ctypes
import os

import numpy as np
import pytest

import posterior_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_exported_and_bound():
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert 'int cliora_span_posteriors(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, float* marginals, float* log_z,' in header
    assert 'size_t cliora_span_posteriors_scratch_bytes(const cliora_plan* plan);' in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'cliora_span_posteriors') and hasattr(raw, 'cliora_span_posteriors_scratch_bytes')
    bound = _lib.lib().cliora_span_posteriors
    assert len(bound.argtypes) == 10 and bound.restype is ctypes.c_int


@pytest.mark.parametrize('n', range(1, 8))
def test_posterior_numpy_is_the_enumeration(n):
    """mu and log_z to 1e-12 for every binary tree of n = 1 .. 7 words (132 trees at 7), alone (L = n) and in a padded table."""
    from cliora_amd.posterior import cell_id, posterior_numpy
    assert len(PC.all_trees(n)) == [1, 1, 2, 5, 14, 42, 132][n - 1]
    for L in (n, n + 3):
        B = 3
        pair_s = PC.random_scores(B, L, seed=100 * n + L)
        mu, log_z = posterior_numpy(pair_s, [n] * B, L)
        assert mu.shape == (B, L * (L + 1) // 2) and mu.dtype == np.float64
        for b in range(B):
            want, want_z, _, _ = PC.enumerate_posteriors(pair_s, b, n)
            own = np.zeros(mu.shape[1], dtype=bool)
            for (level, pos), w in want.items():
                c = cell_id(L, level, pos)
                own[c] = True
                assert abs(mu[b, c] - w) <= 1e-12, (n, L, b, level, pos)
            assert abs(log_z[b] - want_z) <= 1e-12
            assert (mu[b, ~own] == 0).all()                                   # outside the triangle: exactly 0
            for p in range(n):
                assert abs(mu[b, cell_id(L, 0, p)] - 1) <= 1e-12              # the leaves
            assert abs(mu[b, cell_id(L, n - 1, 0)] - 1) <= 1e-12              # the root
            internal = sum(mu[b, cell_id(L, level, pos)] for level in range(1, n) for pos in range(n - level))
            assert abs(internal - (n - 1)) <= 1e-12 * max(1, n)
        if L > n:                                                             # inside the triangle: the values of the exact-length table
            alone, alone_z = posterior_numpy({lv: s[:, :n - lv] for lv, s in pair_s.items() if lv < n}, [n] * B, n)
            for level in range(n):
                a0, p0 = cell_id(n, level, 0), cell_id(L, level, 0)
                assert np.array_equal(alone[:, a0:a0 + n - level], mu[:, p0:p0 + n - level])
            assert np.array_equal(alone_z, log_z)


def _seed_with_a_gap(n, L, first):
    """The first seed from `first` on whose best and second-best enumerated totals differ by at least 1e-6 in fp64."""
    for seed in range(first, first + 50):
        pair_s = PC.random_scores(1, L, seed)
        mu, _, trees, _ = PC.enumerate_posteriors(pair_s, 0, n)
        totals = np.sort([sum(mu[(lv, p)] for lv, p, _ in t) for t in trees])[::-1]
        if len(totals) < 2 or totals[0] - totals[1] >= 1e-6:
            return pair_s, mu, trees
    raise AssertionError('no seed with a gap')


@pytest.mark.parametrize('n', range(1, 8))
def test_mbr_numpy_is_the_best_enumerated_tree(n):
    from cliora_amd.posterior import cell_id, mbr_numpy, posterior_numpy
    for L in (n, n + 2):
        pair_s, mu, trees = _seed_with_a_gap(n, L, 300 + 10 * n + L)
        best = max(trees, key=lambda t: sum(mu[(lv, p)] for lv, p, _ in t))
        marg, _ = posterior_numpy(pair_s, [n], L)
        spans, split = mbr_numpy(marg.astype(np.float32), [n], L)
        assert spans[0] == PC.tree_spans(best)
        assert len(spans[0]) == n - 1 and (n < 2 or spans[0][-1] == (0, n - 1))
        chosen = {cell_id(L, lv, p): k for lv, p, k in best}
        internal = {cell_id(L, lv, p) for lv in range(1, n) for p in range(n - lv)}
        for c in range(split.shape[1]):                                   # a split for every cell of the triangle, the tree's on its cells
            assert (split[0, c] >= 0) == (c in internal)
            assert c not in chosen or split[0, c] == chosen[c]
        assert PC.mbr_fp64(marg[0], n, L)[0] == spans[0]


@pytest.mark.parametrize('L', range(2, 41))
def test_closed_form_uses_are_the_pair_tables_uses(L):
    """Brute force: every (parent, split) of the plan's inside pair tables that reads a cell as its left or right child, against
    cell_uses -- for the whole chart (n = L) and for a shorter sentence's triangle in it."""
    from cliora_amd import _lib
    from cliora_amd.posterior import cell_id, cell_uses
    plan = _lib.Plan(1, L, 16)
    pa, pb, base = plan.table('pair_a_in'), plan.table('pair_b_in'), plan.table('pair_lvl_base_in')
    uses = {}
    for plevel in range(1, L):
        for ppos in range(L - plevel):
            for k in range(plevel):
                i = int(base[plevel]) + ppos * plevel + k
                uses.setdefault(int(pa[i]), set()).add((plevel, ppos, k, int(pb[i])))
                uses.setdefault(int(pb[i]), set()).add((plevel, ppos, k, int(pa[i])))
    for n in sorted({L, L // 2 + 1}):
        for level in range(n):
            for pos in range(n - level):
                want = {u for u in uses.get(cell_id(L, level, pos), ()) if u[1] + u[0] < n}
                got = [(pl, pp, k, cell_id(L, sl, sp)) for pl, pp, k, sl, sp in cell_uses(n, level, pos)]
                assert len(got) == n - 1 - level and len(set(got)) == len(got)
                assert set(got) == want, (n, level, pos)


def test_mbr_seeds_keep_the_gap_on_the_oracle():
    """Every seeded sentence of the end-to-end MBR test: in fp64 on the oracle's scores the two best candidates of every cell differ
    by at least 2 (n - 1) * 1e-4; the seeds are the first four of 0 .. 99 that do."""
    gaps = [PC.mbr_oracle(s)[1] for s in PC.MBR_SEEDS]
    print('fp64 MBR candidate gaps %s (needed %.3e)' % (['%.3e' % g for g in gaps], PC.MBR_GAP))
    assert len(PC.MBR_SEEDS) == 4 and min(gaps) >= PC.MBR_GAP
    assert abs(min(gaps) - PC.MBR_MEASURED_MIN_GAP) <= 1e-6
    assert PC.mbr_seed_search(count=4, first=max(PC.MBR_SEEDS) + 1) == PC.MBR_SEEDS


def test_ragged_seed_keeps_the_gap_on_the_oracle():
    assert PC.ragged_seed_keeps_the_gap(PC.RAGGED_SEED)
    assert not any(PC.ragged_seed_keeps_the_gap(s) for s in range(PC.RAGGED_SEED))


def test_marginal_table_is_indexed_by_start_and_end():
    from cliora_amd.posterior import cell_id, marginal_table
    L = 6
    marg = np.arange(2 * L * (L + 1) // 2, dtype=np.float32).reshape(2, -1) + 1
    table = marginal_table(marg, L)
    assert table.shape == (2, L, L)
    for s in range(L):
        for e in range(L):
            want = marg[:, cell_id(L, e - s, s)] if e >= s else 0
            assert (table[:, s, e] == want).all()
