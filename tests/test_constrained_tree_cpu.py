"""The K best trees and sampled trees under brackets on the host (cliora_amd/constrained.py): ``constrained_kbest_numpy`` and
``constrained_sample_numpy`` against enumeration of every binary tree (n <= 7) over constrained_cases.bracket_sets, their equality
with ``kbest_numpy`` / ``sample_numpy`` without brackets, and the clamp rule of the draw.  Cases: constrained_cases.py."""
import numpy as np
import pytest

import constrained_cases as CC
import posterior_cases as PC
import sample_cases as SC
from cliora_amd import constrained as CN
from cliora_amd.kbest import kbest_numpy
from cliora_amd.sample import sample_numpy, split_weights

KS = (1, 4, 16)
# An fp32 list may order two trees otherwise than fp64 only where their fp64 weights are closer than the rounding of the fp32
# recurrence, which constrained_cases.py bounds by 5e-5 for these scores (13 additions of magnitudes below 64); BEST_GAP is twice that.
F32_SUM_BOUND = 5e-5


def _qualifying(n, seed, rows):
    """-> (the qualifying trees' spans, best first by fp64 weight (stable), their weights)."""
    _, trees, w, member = CC.enumeration(n, seed)
    ok = np.ones(len(trees), dtype=bool)
    for s, e, kind in rows:
        ok &= member[:, s, e] if kind == 1 else ~member[:, s, e]
    idx = np.flatnonzero(ok)
    idx = idx[np.argsort(-w[idx], kind='stable')]
    return [tuple(PC.tree_spans(trees[i])) for i in idx], w[idx]


# ---- 1. the K best ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', CC.ENUM_NS)
@pytest.mark.parametrize('seed', CC.ENUM_SEEDS)
def test_constrained_kbest_numpy_is_the_enumeration(n, seed):
    """Every bracket set of the case: the qualifying trees sorted by fp64 weight, the first K -- the same trees in the same order,
    count = min(K, the number that qualify), nothing where none does.  Where two of the first K + 1 weights lie within BEST_GAP the
    fp32 order between them is not decided by fp64: there the ranks must still hold distinct qualifying trees, each within the fp32
    bound of the enumerated weight of its rank; the number of such sets is printed."""
    pair_s = CC.enumeration(n, seed)[0]
    sets = CC.bracket_sets(n, seed)
    L = max(n, 2)
    want = [_qualifying(n, seed, rows) for rows in sets]
    index = {}
    for spans, w in want:
        index.update(zip(spans, w))
    for K in KS:
        got = CN.constrained_kbest_numpy(CC.repeat_scores(pair_s, len(sets)), [n] * len(sets), CC.pack_rows(sets), K, L=L)
        assert got.status == 0
        close = 0
        for b, rows in enumerate(sets):
            spans, w = want[b]
            cnt = min(K, len(spans))
            assert got.count[b] == cnt and got.feasible[b] == (cnt > 0), rows
            assert (got.spans[b, cnt:] == -1).all() and (got.scores[b, cnt:] == -np.inf).all(), rows
            trees = [CC.span_key(got.spans[b, t].tolist()) for t in range(cnt)]
            assert len(set(trees)) == cnt and set(trees) <= set(spans), (rows, K)
            assert all(abs(float(got.scores[b, r]) - index[t]) <= F32_SUM_BOUND for r, t in enumerate(trees)), (rows, K)
            if np.diff(-w[:cnt + 1]).min(initial=np.inf) > CC.BEST_GAP:
                assert trees == spans[:cnt], (rows, K)
            else:                                     # two fp32 scores, each within the bound of its weight, may swap: twice the bound
                close += 1
                assert all(abs(index[t] - w[r]) <= 2 * F32_SUM_BOUND for r, t in enumerate(trees)), (rows, K)
        print('n %d seed %d K %d: %d bracket sets, %d with two of the first K + 1 within %.0e' % (n, seed, K, len(sets), close, CC.BEST_GAP))
        if K == 1:
            assert close == 0                         # constrained_cases.ENUM_MIN_GAP: the two best always differ by more


def test_constrained_kbest_numpy_rank_0_is_constrained_numpy():
    n, seed = 6, 1
    pair_s = CC.enumeration(n, seed)[0]
    sets = CC.bracket_sets(n, seed)
    scores, brackets = CC.repeat_scores(pair_s, len(sets)), CC.pack_rows(sets)
    best = CN.constrained_numpy(scores, [n] * len(sets), brackets, L=n)
    got = CN.constrained_kbest_numpy(scores, [n] * len(sets), brackets, 16, L=n)
    assert np.array_equal(got.feasible, best.feasible)
    assert np.array_equal(got.spans[:, 0], best.spans)
    assert np.array_equal(got.scores[:, 0].view(np.int32), best.score.view(np.int32))


# ---- 2. the draws -----------------------------------------------------------------------------------------------------------------------
def _sample_sets(n, seed):
    """The single brackets, every seventh pair and the random sets of the case."""
    sets = CC.bracket_sets(n, seed)
    singles = 2 * len(CC.cells(n))
    return sets[:singles] + sets[singles:-CC.RANDOM_SETS:7] + sets[-CC.RANDOM_SETS:]


@pytest.mark.parametrize('n', CC.ENUM_NS)
@pytest.mark.parametrize('seed', CC.ENUM_SEEDS)
def test_constrained_sample_numpy_is_the_enumeration(n, seed):
    """Every draw is a qualifying tree with log_prob = beta * (its weight) - log_z_c; exp of that formula over the enumerated
    qualifying trees sums to 1; log_z is the unconstrained one; at beta = 1 log_z_c - log_z is constrained_numpy's log_prob."""
    pair_s = CC.enumeration(n, seed)[0]
    sets = _sample_sets(n, seed)
    L, S = max(n, 2), 6
    scores, brackets = CC.repeat_scores(pair_s, len(sets)), CC.pack_rows(sets)
    for beta in SC.BETAS:
        got = CN.constrained_sample_numpy(scores, [n] * len(sets), brackets, S, 77 + seed, beta=beta, L=L)
        assert got.status == 0
        log_z = SC.enumerate_trees(pair_s, 0, n, beta)[2]
        parse = CN.constrained_numpy(scores, [n] * len(sets), brackets, L=L) if beta == 1.0 else None
        infeasible = 0
        for b, rows in enumerate(sets):
            spans, w = _qualifying(n, seed, rows)
            assert bool(got.feasible[b]) == bool(spans), rows
            assert abs(got.log_z[b] - log_z) <= SC.ENUM_RTOL * max(1.0, abs(log_z)), rows
            if not spans:
                infeasible += 1
                assert (got.spans[b] == -1).all() and (got.log_prob[b] == -np.inf).all() and got.log_z_c[b] == -np.inf, rows
                continue
            weight = dict(zip(spans, w))
            assert abs(np.exp(beta * w - got.log_z_c[b]).sum() - 1.0) <= SC.ENUM_RTOL, (rows, beta)
            for s in range(S):
                tree = CC.span_key(got.spans[b, s].tolist())
                assert tree in weight, (rows, beta, s)                         # the draw qualifies
                assert (got.spans[b, s, n - 1:] == -1).all()
                want = beta * weight[tree] - got.log_z_c[b]
                assert abs(got.log_prob[b, s] - want) <= SC.ENUM_RTOL * max(1.0, abs(want)), (rows, beta, s)
            if parse is not None:
                assert abs((got.log_z_c[b] - got.log_z[b]) - parse.log_prob[b]) <= SC.ENUM_RTOL * max(1.0, abs(parse.log_prob[b])), rows
        if n > 1:
            assert 0 < infeasible < len(sets)


@pytest.mark.parametrize('rows,trees', [([(0, 1, 0)], 9), ([(1, 3, 1)], 4), ([(0, 2, 1), (3, 4, 0)], 2)])
def test_at_beta_0_every_qualifying_tree_is_drawn(rows, trees):
    """n 5, beta 0: uniform over the qualifying trees, so 4096 draws miss one of at most 9 with probability below 9 (8/9)^4096."""
    n, seed, S = 5, 0, 4096
    pair_s = CC.enumeration(n, seed)[0]
    spans, _ = _qualifying(n, seed, rows)
    assert len(spans) == trees
    got = CN.constrained_sample_numpy(pair_s, [n], CC.pack_rows([rows]), S, 12345, beta=0.0)
    drawn = set(CC.span_key(r) for r in got.spans[0].tolist())
    assert drawn == set(spans)
    assert np.allclose(got.log_prob[0], -np.log(trees), rtol=0, atol=1e-12)


def test_without_brackets_the_restatements_are_the_unconstrained_ones():
    """No bracket, unused rows, a required leaf and a required root: sample_numpy's and kbest_numpy's outputs exactly."""
    lengths, L = [6, 1, 4], 6
    pair_s = PC.random_scores(len(lengths), L, SC.DRAW_SCORE_SEED)
    for brackets in (None, np.full((3, 2, 3), -1, dtype=np.int32), CC.pack_rows([[(2, 2, 1), (0, 5, 1)], [(0, 0, 1)], [(0, 3, 1)]])):
        for K in KS:
            spans, scores, count = kbest_numpy(pair_s, lengths, K, L=L)
            got = CN.constrained_kbest_numpy(pair_s, lengths, brackets, K, L=L)
            assert got.status == 0 and got.feasible.tolist() == [1, 1, 1]
            assert np.array_equal(got.spans, spans) and np.array_equal(got.count, count)
            assert np.array_equal(got.scores.view(np.int32), scores.view(np.int32))
        for beta in SC.BETAS:
            spans, log_prob, log_z, margin = sample_numpy(pair_s, lengths, 8, SC.DRAW_SEED, ids=[5, 9, 2], first_sample=3, beta=beta, L=L)
            got = CN.constrained_sample_numpy(pair_s, lengths, brackets, 8, SC.DRAW_SEED, ids=[5, 9, 2], first_sample=3, beta=beta, L=L)
            assert got.status == 0 and got.feasible.tolist() == [1, 1, 1]
            assert np.array_equal(got.spans, spans) and np.array_equal(got.log_prob, log_prob) and np.array_equal(got.margin, margin)
            assert np.array_equal(got.log_z, log_z) and np.array_equal(got.log_z_c, log_z)


def test_bad_rows_and_lengths_count_once_and_write_nothing():
    L = 5
    pair_s = CC.repeat_scores(CC.enum_scores(L, 2), 4)
    brackets = CC.pack_rows([[(1, 3, 1)], [(1, 5, 1), (0, 1, 2)], [(0, 1, 1)], [(0, 3, 1)]])
    lengths = [5, 5, 0, 3]                            # fine; two bad rows; a bad length; end >= n
    kb = CN.constrained_kbest_numpy(pair_s, lengths, brackets, 4, L=L)
    ts = CN.constrained_sample_numpy(pair_s, lengths, brackets, 3, 1, L=L)
    assert kb.status == 3 and ts.status == 3
    assert kb.feasible.tolist() == [1, 0, 0, 0] and ts.feasible.tolist() == [1, 0, 0, 0]
    for b in (1, 2, 3):
        assert kb.count[b] == 0 and (kb.spans[b] == -1).all() and (kb.scores[b] == -np.inf).all()
        assert (ts.spans[b] == -1).all() and (ts.log_prob[b] == -np.inf).all() and ts.log_z_c[b] == -np.inf and ts.log_z[b] == 0
    with pytest.raises(ValueError):
        CN.constrained_kbest_numpy(pair_s, lengths, brackets, 17, L=L)
    with pytest.raises(ValueError):
        CN.constrained_sample_numpy(pair_s, lengths, brackets, 0, 1, L=L)
    with pytest.raises(ValueError):
        CN.constrained_sample_numpy(pair_s, lengths, brackets, 1, 1, beta=-1.0, L=L)


def test_the_device_seed_keeps_the_margin_on_the_oracles_scores():
    """The device tests draw with constrained_cases.GPU_SAMPLE_SEED and may leave a sample out only below sample_cases.MARGIN.  On
    the fp64 oracle's scores of the same sentences and parameters (the device's differ from them by fp32 rounding), under every
    bracket set of constrained_tree_cases.cases, no sample comes near it: the seed stands."""
    import torch
    from oracle import diora_ref as R
    import constrained_tree_cases as TC
    B, D = PC.GPU_B, PC.GPU_D
    P = {k: v.double() for k, v in PC.params(D, PC.GPU_SEED).items()}
    smallest = np.inf
    for L in TC.LENGTHS:
        if L < 2:
            continue
        with torch.no_grad():
            o = R.diora_forward(P, PC.batch(D, L, B, PC.GPU_SEED + L).double(), outside=False, normalize='unit', share=True, keep_pairs=True)
        pair_s = {lv: s.numpy()[..., 0] for lv, s in o['pair_s_in'].items()}
        for name, brackets in TC.cases(L, B).items():
            for beta in ((1.0, 0.5) if L == 13 else (1.0,)):
                got = CN.constrained_sample_numpy(pair_s, [L] * B, brackets, SC.GPU_S, CC.GPU_SAMPLE_SEED, beta=beta, L=L)
                smallest = min(smallest, float(got.margin.min()))
    print('smallest margin of the device cases on the oracle\'s scores: %.3e' % smallest)
    assert smallest >= TC.ORACLE_MIN_MARGIN * (1 - 1e-3) > SC.MARGIN


# ---- 3. the clamp -----------------------------------------------------------------------------------------------------------------------
def test_the_clamp_goes_to_the_last_split_with_finite_children():
    """n 3 with [0, 1] forbidden: the root's last split (left child [0, 1]) weighs exactly 0.  A uniform of 1.0 -- which the scan
    answers with N, the clamp's only case -- picks split 0, the last one a qualifying tree can take, not N - 1."""
    n = 3
    pair_s = CC.enum_scores(n, 0)
    from cliora_amd.posterior import inside_numpy
    r, al = inside_numpy(pair_s, 0, n)
    allowed, _ = CN.allowed_cells(n, [(0, 1, 0)])
    assert not allowed[1, 0] and allowed[1, 1]
    al[1, 0] = -np.inf
    al[2, 0] = al[0, 0] + al[1, 1] + r[2, 0, 0]       # the one term left
    w = split_weights(r, al, 2, 0, 1.0)
    assert w[1] == 0.0 and abs(w[0] - 1.0) <= 1e-15
    finite = np.array([True, False])
    assert CN.choose_split(w, 1.0, finite)[0] == 0
    assert CN.choose_split(w, 0.25, finite)[0] == 0 and CN.choose_split(w, 1.0 - 2.0 ** -53, finite)[0] == 0
    # every child finite: sample_numpy's clamp, N - 1; and a zero weight in the middle is never chosen by the scan
    assert CN.choose_split(np.array([0.5, 0.5]), 1.0, np.array([True, True]))[0] == 1
    assert CN.choose_split(np.array([0.5, 0.0, 0.5]), 0.5, np.array([True, False, True]))[0] == 2
    assert CN.choose_split(np.array([0.5, 0.0, 0.5]), 0.4999, np.array([True, False, True]))[0] == 0
    # through the restatement: every draw of the sentence is the one qualifying tree
    got = CN.constrained_sample_numpy(pair_s, [n], CC.pack_rows([[(0, 1, 0)]]), 16, 3)
    assert all(CC.span_key(rows) == ((1, 2), (0, 2)) for rows in got.spans[0].tolist()) and np.abs(got.log_prob).max() <= 1e-15
