"""``tree_expectation_numpy`` and ``span_costs`` (cliora_amd/structured.py): the fp64 restatement of cliora_tree_expectation that the
device tests measure the kernel against, pinned here to enumeration of every binary tree, to central differences of the enumerated
objective, to closed forms and to ``posterior_numpy``.  Cases and bounds: expectation_cases.py."""
import numpy as np
import pytest

import constrained_cases as CC
import expectation_cases as EC
import posterior_cases as PC
import structured_cases as SC

from cliora_amd.posterior import posterior_numpy
from cliora_amd.structured import span_costs, tree_expectation_numpy


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=EC.ENUM_RTOL, atol=EC.ENUM_RTOL, err_msg=str(what))


@pytest.mark.parametrize('n', CC.ENUM_NS)
def test_against_enumeration(n):
    for seed in CC.ENUM_SEEDS:
        pair_s = CC.enumeration(n, seed)[0]
        L = max(n, 2)
        cost = EC.random_costs(1, L, 300 + 10 * n + seed)
        for wc, we in EC.WEIGHTS:
            want = EC.enumerated(pair_s, n, cost[0], L, wc, we)
            G, risk, entropy, log_z = tree_expectation_numpy(pair_s, [n], cost, [wc], [we])
            _close(risk[0], want['risk'], (n, seed, 'risk'))
            _close(entropy[0], want['entropy'], (n, seed, 'entropy'))
            _close(log_z[0], want['log_z'], (n, seed, 'log_z'))
            for level in range(1, L):
                _close(G[level][0, :max(0, n - level)], want['G'].get(level, np.zeros((0, level))), (n, seed, wc, we, level))
                assert not G[level][0, max(0, n - level):].any()
        if n >= 3:
            assert any(np.abs(g).max() > 1e-3 for g in G.values()), (n, seed)               # a gradient, not zeros


@pytest.mark.parametrize('n', EC.FD_NS)
def test_against_central_differences_of_the_enumerated_objective(n):
    scores = SC.gapped_scores(n, 900 + n)
    cost = EC.random_costs(1, n, 77 + n)
    wc, we = EC.WEIGHTS[2]
    G = tree_expectation_numpy(scores, [n], cost, [wc], [we])[0]
    worst = 0.0
    for level in range(1, n):
        for pos in range(n - level):
            for k in range(level):
                hi = {lv: s.copy() for lv, s in scores.items()}
                lo = {lv: s.copy() for lv, s in scores.items()}
                hi[level][0, pos, k] += EC.FD_H
                lo[level][0, pos, k] -= EC.FD_H
                fd = (EC.enumerated(hi, n, cost[0], n, wc, we)['J'] - EC.enumerated(lo, n, cost[0], n, wc, we)['J']) / (2 * EC.FD_H)
                worst = max(worst, abs(fd - G[level][0, pos, k]))
                assert abs(fd - G[level][0, pos, k]) <= EC.FD_TOL, (n, level, pos, k, fd, G[level][0, pos, k])
    print('n %d: max |G - central difference| = %.3e' % (n, worst))
    assert any(np.abs(g).max() > 1e-3 for g in G.values())


@pytest.mark.parametrize('n', range(2, 11))
def test_uniform_scores_give_log_catalan_and_the_average_cost(n):
    rs = np.random.RandomState(n)
    scores = {level: np.repeat(rs.randn(1, n - level, 1), level, axis=2) for level in range(1, n)}       # every row ties
    cost = EC.random_costs(1, n, 50 + n)
    G, risk, entropy, log_z = tree_expectation_numpy(scores, [n], cost, [1.0], [1.0])
    trees = PC.all_trees(n)
    assert len(trees) == EC.catalan(n - 1)
    average = np.mean([sum(cost[0, EC.cell_id(n, lv, p)] for lv, p in EC.tree_cells(t, n)) for t in trees])
    _close(entropy[0], np.log(EC.catalan(n - 1)), n)
    _close(log_z[0], np.log(EC.catalan(n - 1)), n)
    _close(risk[0], average, n)


def test_row_sums_linearity_padding_and_bad_lengths():
    L, lengths = 7, [7, 3, 1, 5, 2]
    B = len(lengths)
    scores = PC.random_scores(B, L, 31)
    cost = EC.random_costs(B, L, 32)
    wa, wb = np.array([0.7, 1.0, -2.0, 0.3, 1.5]), np.array([-1.3, 0.5, 1.0, 2.0, -0.5])
    G, risk, entropy, log_z = tree_expectation_numpy(scores, lengths, cost, wa, wb)
    Gc, risk_c, entropy_c, _ = tree_expectation_numpy(scores, lengths, cost)                              # wc 1, we 0
    Ge = tree_expectation_numpy(scores, lengths, cost, np.zeros(B), np.ones(B))[0]
    np.testing.assert_array_equal(risk, risk_c)                                                          # no scalar depends on the weights
    np.testing.assert_array_equal(entropy, entropy_c)
    for level in range(1, L):
        assert np.abs(G[level].sum(axis=2)).max() <= EC.ROW_SUM_TOL
        np.testing.assert_allclose(G[level], wa[:, None, None] * Gc[level] + wb[:, None, None] * Ge[level], rtol=0, atol=1e-13)
        for b, n in enumerate(lengths):
            assert not G[level][b, max(0, n - level):].any(), (b, level)                                 # beyond the triangle
    assert any(np.abs(Gc[level][0]).max() > 1e-3 for level in range(1, L)) and any(np.abs(Ge[level][0]).max() > 1e-3 for level in range(1, L))
    for b, n in enumerate(lengths):                                                                      # each sentence alone at its own L
        alone_s = {level: scores[level][b:b + 1, :n - level] for level in range(1, n)}
        alone_c = np.zeros((1, n * (n + 1) // 2))
        for level in range(n):
            alone_c[0, EC.cell_id(n, level, 0):EC.cell_id(n, level, 0) + n - level] = cost[b, EC.cell_id(L, level, 0):EC.cell_id(L, level, 0) + n - level]
        g1, r1, e1, z1 = tree_expectation_numpy(alone_s, [n], alone_c, wa[b:b + 1], wb[b:b + 1])
        assert (r1[0], e1[0], z1[0]) == (risk[b], entropy[b], log_z[b])
        for level in range(1, n):
            np.testing.assert_array_equal(g1[level][0], G[level][b, :n - level])
    # the closed forms: one word, two words
    assert risk[2] == cost[2, 0] and entropy[2] == 0.0 and log_z[2] == 0.0
    three = cost[4, 0] + cost[4, 1] + cost[4, EC.cell_id(L, 1, 0)]
    assert abs(risk[4] - three) <= 1e-15 and entropy[4] == 0.0 and not any(G[level][4].any() for level in range(1, L))
    # a bad length: zeros, the neighbours unaffected, NaN weights and costs unread
    bad = list(lengths)
    bad[1], bad[3] = 0, L + 1
    cost_b, wa_b = cost.copy(), wa.copy()
    cost_b[1], wa_b[3] = np.nan, np.nan
    Gb, risk_b, entropy_b, log_z_b = tree_expectation_numpy(scores, bad, cost_b, wa_b, wb)
    for b in (1, 3):
        assert risk_b[b] == entropy_b[b] == log_z_b[b] == 0.0 and not any(Gb[level][b].any() for level in range(1, L))
    for b in (0, 2, 4):
        assert (risk_b[b], entropy_b[b], log_z_b[b]) == (risk[b], entropy[b], log_z[b])
        for level in range(1, L):
            np.testing.assert_array_equal(Gb[level][b], G[level][b])


def test_risk_is_the_posterior_weighted_cost():
    L, lengths = 9, [9, 4, 6]
    scores = PC.random_scores(3, L, 41)
    cost = EC.random_costs(3, L, 42)
    mu, log_z64 = posterior_numpy(scores, lengths, L)
    _, risk, entropy, log_z = tree_expectation_numpy(scores, lengths, cost)
    _close(risk, (mu * cost).sum(axis=1), 'risk')
    _close(log_z, log_z64, 'log_z')
    for b, n in enumerate(lengths):                                          # H = log_z - E[R] with R <= 0, and at most log of the number of trees
        assert log_z[b] - 1e-12 <= entropy[b] <= np.log(EC.catalan(n - 1)) + 1e-12


def test_span_costs_against_the_per_cell_definition():
    from cliora_amd.constrained import brackets_from_entity_labels, crosses
    L = 8
    labels = [[('np', 1, 3), ('np', 2, 4), ('np', 1, 3), None, ('x', 7, 1)], [('np', 0, 2), ('vp', 5, 6), ('np', 6, 2)], []]
    req = brackets_from_entity_labels(labels, drop_crossing=False)
    assert crosses(req[0][0], req[0][1])                                     # a crossing pair is kept
    forb = [[(0, 7), (1, 3)], [(3, 3), (-1, 2), (4, 9)], [(2, 5)]]
    got = span_costs(req, forb, L=L).numpy()
    assert got.shape == (3, L * (L + 1) // 2) and got.dtype == np.float32
    for b in range(3):
        for level in range(L):
            for pos in range(L - level):
                span = (pos, pos + level)
                want = float(span in forb[b]) - float(span in req[b])
                assert got[b, EC.cell_id(L, level, pos)] == want, (b, span)
    assert got[0, EC.cell_id(L, 3, 2)] == -1 and got[0, EC.cell_id(L, 2, 1)] == 0       # required and forbidden at once: 0
    assert got[1].sum() == -2 + 1                                            # (5, 10) and (4, 9) leave the chart, (-1, 2) too: ignored
    assert not span_costs(req, None, L=L).numpy()[2].any()
    with pytest.raises(ValueError):
        span_costs(req)
