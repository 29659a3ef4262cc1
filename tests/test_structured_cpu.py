"""``bracket_grad_numpy`` (cliora_amd/structured.py), the fp64 restatement of cliora_bracket_grad that the device tests measure the
kernel against: pinned here to central differences of ``constrained_numpy``'s fp64 log_prob and to enumeration of every binary tree.
Cases and bounds: structured_cases.py."""
import numpy as np
import pytest

import constrained_cases as CC
import posterior_cases as PC
import structured_cases as SC

from cliora_amd.constrained import constrained_numpy
from cliora_amd.structured import bracket_grad_numpy


def _log_prob(scores, n, rows):
    return float(constrained_numpy(scores, [n], CC.pack_rows([rows]), L=n).log_prob[0])


@pytest.mark.parametrize('n', SC.FD_NS)
def test_against_central_differences(n):
    scores = SC.gapped_scores(n, 900 + n)
    worst = 0.0
    for name, rows in SC.bracket_sets(n).items():
        assert np.isfinite(_log_prob(scores, n, rows)), (n, name)
        G = bracket_grad_numpy(scores, [n], CC.pack_rows([rows]))
        for level in range(1, n):
            for pos in range(n - level):
                for k in range(level):
                    hi = {lv: s.copy() for lv, s in scores.items()}
                    lo = {lv: s.copy() for lv, s in scores.items()}
                    hi[level][0, pos, k] += SC.FD_H
                    lo[level][0, pos, k] -= SC.FD_H
                    fd = (_log_prob(hi, n, rows) - _log_prob(lo, n, rows)) / (2 * SC.FD_H)
                    worst = max(worst, abs(fd - G[level][0, pos, k]))
                    assert abs(fd - G[level][0, pos, k]) <= SC.FD_TOL, (n, name, level, pos, k, fd, G[level][0, pos, k])
        assert any(np.abs(g).max() > 1e-3 for g in G.values()) or n == 3, (n, name)        # a gradient, not zeros
    print('n %d: max |G - central difference| = %.3e' % (n, worst))


def _enumerated_gradient(n, seed, rows):
    """d/ds of log sum exp(weight) over the qualifying trees minus that over all trees, summed tree by tree: a tree's weight is the
    sum of r = s - rowmax over its nodes, so it adds its probability at (cell, k) and takes it from (cell, argmax)."""
    pair_s, trees, w, member = CC.enumeration(n, seed)
    ok = np.ones(len(trees), dtype=bool)
    for s, e, kind in rows:
        ok &= member[:, s, e] if kind == 1 else ~member[:, s, e]
    G = {level: np.zeros((n - level, level)) for level in range(1, n)}
    if not ok.any():
        return G
    pc = np.where(ok, np.exp(w - CC.logsumexp(w[ok])), 0.0)
    pu = np.exp(w - CC.logsumexp(w))
    for t, tree in enumerate(trees):
        for level, pos, k in tree:
            kstar = int(np.argmax(pair_s[level][0, pos]))
            G[level][pos, k] += pc[t] - pu[t]
            G[level][pos, kstar] -= pc[t] - pu[t]
    return G


@pytest.mark.parametrize('n', range(2, 7))
def test_against_enumeration(n):
    for seed in CC.ENUM_SEEDS:
        pair_s = CC.enum_scores(n, seed)
        sets = list(SC.bracket_sets(n, seed).values()) if n >= 3 else [[(0, 1, 1)], [(0, 0, 0)]]
        sets += CC.bracket_sets(n, seed)[-CC.RANDOM_SETS:]
        for rows in sets:
            rows = [r for r in rows if r[1] < n]
            got = bracket_grad_numpy(pair_s, [n], CC.pack_rows([rows]) if rows else None)
            want = _enumerated_gradient(n, seed, rows)
            for level in range(1, n):
                np.testing.assert_allclose(got[level][0], want[level], rtol=SC.ENUM_RTOL, atol=SC.ENUM_RTOL, err_msg=str((n, seed, rows)))


def test_row_sums_no_constraint_infeasible_and_weights():
    n, B = 7, 5
    scores = PC.random_scores(B, n, 31)
    sets = [[(1, 4, 1), (2, 3, 0)], [], [(0, 3, 1), (2, 5, 1)], [(0, 6, 1), (3, 3, 1)], [(1, 4, 1), (2, 3, 0)]]
    G = bracket_grad_numpy(scores, [n] * B, CC.pack_rows(sets))
    for level in range(1, n):
        assert np.abs(G[level].sum(axis=2)).max() <= SC.ROW_SUM_TOL
        assert not G[level][1].any()            # no bracket at all
        assert not G[level][2].any()            # crossing required brackets: no qualifying tree
        assert not G[level][3].any()            # a required root and a required leaf disallow nothing
    assert any(G[level][0].any() for level in range(1, n))
    w = np.array([2.5, 1.0, 3.0, 1.0, -0.5])
    Gw = bracket_grad_numpy(scores, [n] * B, CC.pack_rows(sets), weights=w)
    for level in range(1, n):
        np.testing.assert_allclose(Gw[level], G[level] * w[:, None, None], rtol=1e-15, atol=0)
    # a bad row and a bad length: zero, the neighbours unaffected; a shorter sentence: zero beyond its triangle
    sets[1] = [(3, 9, 1)]
    Gb = bracket_grad_numpy(scores, [n, n, n, n, 4], CC.pack_rows(sets))
    for level in range(1, n):
        assert not Gb[level][1].any() and np.array_equal(Gb[level][0], G[level][0])
        assert not Gb[level][4, max(0, 4 - level):].any()
