"""cliora_amd/constrained.py on the host: ``constrained_numpy`` against enumeration of every binary tree (n <= 7) -- log_z_c, the
feasibility, the best qualifying tree and the conditional span posteriors, for every single bracket, every pair of brackets of either
kind and three larger random sets per case -- and the host helpers (pack_brackets, brackets_from_entity_labels, the refusals that need
no device).  Cases: constrained_cases.py."""
import numpy as np
import pytest
import torch

import constrained_cases as CC
from cliora_amd import constrained as CN
from cliora_amd.posterior import cell_id


@pytest.mark.parametrize('n', CC.ENUM_NS)
@pytest.mark.parametrize('seed', CC.ENUM_SEEDS)
def test_constrained_numpy_is_the_enumeration(n, seed):
    pair_s = CC.enumeration(n, seed)[0]
    sets = CC.bracket_sets(n, seed)
    L = max(n, 2)
    got = CN.constrained_numpy(CC.repeat_scores(pair_s, len(sets)), [n] * len(sets), CC.pack_rows(sets), L=L)
    assert got.status == 0
    min_gap, infeasible = np.inf, 0
    for b, rows in enumerate(sets):
        want = CC.enumerate_constrained(n, seed, rows)
        assert abs(got.log_z[b] - want['log_z']) <= CC.ENUM_RTOL * max(1.0, abs(want['log_z'])), rows
        assert bool(got.feasible[b]) == (want['best'] is not None), rows                     # infeasible exactly when no tree qualifies
        if want['best'] is None:
            infeasible += 1
            assert got.log_z_c[b] == -np.inf and got.log_prob[b] == -np.inf and got.score[b] == -np.inf, rows
            assert (got.spans[b] == -1).all() and (got.marginals[b] == 0).all(), rows
            continue
        assert abs(got.log_z_c[b] - want['log_zc']) <= CC.ENUM_RTOL * max(1.0, abs(want['log_zc'])), rows
        assert abs(got.log_prob[b] - (want['log_zc'] - want['log_z'])) <= 2 * CC.ENUM_RTOL * max(1.0, abs(want['log_z'])), rows
        assert got.log_prob[b] <= 1e-15, rows
        assert want['gap'] > CC.BEST_GAP, (rows, want['gap'])                                 # fp32 cannot flip the best tree
        min_gap = min(min_gap, want['gap'])
        assert CC.span_key(got.spans[b].tolist()) == tuple(want['best']), rows
        assert (got.spans[b, n - 1:] == -1).all()
        allowed, required = CN.allowed_cells(n, rows)
        for s, e in CC.cells(n):
            mu = got.marginals[b, cell_id(L, e - s, s)]
            assert abs(mu - want['mu'][s, e]) <= CC.ENUM_RTOL, (rows, s, e)
            if not allowed[e - s, s]:
                assert mu == 0.0, (rows, s, e)
            if required[e - s, s]:
                assert mu == 1.0, (rows, s, e)
    print('n %d seed %d: %d bracket sets, %d infeasible, smallest gap %.3e' % (n, seed, len(sets), infeasible, min_gap))
    assert min_gap >= CC.ENUM_MIN_GAP * (1 - 1e-3)                            # the recorded figure, four digits
    if n > 1:
        assert 0 < infeasible < len(sets)


def test_score_of_the_best_tree_is_the_sum_of_its_potentials():
    """n 7: the fp32 score against the enumerated weight of the best qualifying tree -- at most 2 n fp32 additions of magnitudes
    below 64, so within 2 * 7 * 64 * 6e-8 = 5.4e-5."""
    n, seed = 7, 0
    pair_s, _, w, member = CC.enumeration(n, seed)
    sets = CC.bracket_sets(n, seed)[:2 * len(CC.cells(n))]                    # the single brackets
    got = CN.constrained_numpy(CC.repeat_scores(pair_s, len(sets)), [n] * len(sets), CC.pack_rows(sets), L=n)
    for b, rows in enumerate(sets):
        (s, e, kind), = rows
        ok = member[:, s, e] if kind == 1 else ~member[:, s, e]
        if ok.any():
            assert abs(float(got.score[b]) - w[ok].max()) <= 5.4e-5, rows
        else:
            assert got.score[b] == -np.inf


def test_brackets_without_effect_and_no_brackets():
    """No row, unused rows, a required leaf and a required root: the unconstrained parse, log_prob exactly 0."""
    from cliora_amd.posterior import posterior_numpy
    n = 6
    pair_s = CC.enum_scores(n, 1)
    mu, log_z = posterior_numpy(pair_s, [n], n)
    base = CN.constrained_numpy(pair_s, [n], None)
    for rows in ([], [(-1, 5, 7)], [(2, 2, 1)], [(0, n - 1, 1)], [(0, n - 1, 1), (4, 4, 1), (-1, -1, -1)]):
        got = CN.constrained_numpy(pair_s, [n], CC.pack_rows([rows], M=max(len(rows), 1)))
        assert got.status == 0 and got.feasible[0] == 1 and got.log_prob[0] == 0.0
        assert got.log_z[0] == log_z[0] and got.log_z_c[0] == log_z[0]
        assert np.array_equal(got.spans, base.spans) and got.score[0] == base.score[0]
        assert np.abs(got.marginals - mu).max() <= CC.ENUM_RTOL


def test_bad_rows_and_lengths_count_once_per_sentence():
    L = 6
    pair_s = CC.repeat_scores(CC.enum_scores(L, 2), 6)
    sets = [[(1, 3, 1)],                             # fine
            [(1, 6, 1), (7, 2, 0), (0, 1, 2)],       # three bad rows: one count
            [(0, 4, 1)],                             # end >= n = 4, inside the padding
            [(2, 1, 0)],                             # start > end
            [(0, 1, 2)],                             # kind
            [(-2, 1, 1)]]                            # a negative start that is not the unused mark
    lengths = [6, 6, 4, 6, 6, 6]
    got = CN.constrained_numpy(pair_s, lengths, CC.pack_rows(sets), L=L)
    assert got.status == 5
    assert got.feasible.tolist() == [1, 0, 0, 0, 0, 0]
    for b in range(1, 6):
        assert (got.spans[b] == -1).all() and got.log_z[b] == 0 and (got.marginals[b] == 0).all()
        assert got.score[b] == -np.inf and got.log_z_c[b] == -np.inf and got.log_prob[b] == -np.inf
    assert CN.constrained_numpy(pair_s, [0, 7, 6, 6, 6, 6], None, L=L).status == 2
    alone = CN.constrained_numpy(CC.enum_scores(L, 2), [6], CC.pack_rows(sets[:1]), L=L)
    assert np.array_equal(alone.spans[0], got.spans[0]) and alone.log_z_c[0] == got.log_z_c[0]


def test_padded_sentence_is_the_sentence_alone():
    """A sentence of 4 words in a chart of 7 under its brackets: what it gives alone in a chart of 4 from the same rows of scores."""
    L, n = 7, 4
    pair_s = CC.enum_scores(L, 0)
    own = {level: pair_s[level][:, :n - level] for level in range(1, n)}
    rows = CC.pack_rows([[(1, 2, 1), (0, 1, 0)]])
    a, b = CN.constrained_numpy(pair_s, [n], rows, L=L), CN.constrained_numpy(own, [n], rows, L=n)
    assert np.array_equal(a.spans[0, :n - 1], b.spans[0]) and (a.spans[0, n - 1:] == -1).all()
    assert a.score[0] == b.score[0] and a.log_z_c[0] == b.log_z_c[0] and a.log_prob[0] == b.log_prob[0]
    for level in range(n):
        for pos in range(n - level):
            assert a.marginals[0, cell_id(L, level, pos)] == b.marginals[0, cell_id(n, level, pos)]
    assert a.marginals[0].sum() == b.marginals[0].sum()                       # nothing outside the triangle


def test_pack_brackets_pads_with_unused_rows():
    t = CN.pack_brackets([[(0, 2), (1, 2)], [], [(3, 4)]], [[(0, 1)], [], []])
    assert t.dtype == torch.int32 and tuple(t.shape) == (3, 3, 3)
    assert t.tolist() == [[[0, 2, 1], [1, 2, 1], [0, 1, 0]], [[-1, -1, -1]] * 3, [[3, 4, 1], [-1, -1, -1], [-1, -1, -1]]]
    assert tuple(CN.pack_brackets([[], []]).shape) == (2, 0, 3)
    wide = CN.pack_brackets([[(0, 1)]], M=4)
    assert tuple(wide.shape) == (1, 4, 3) and (wide[0, 1:] == -1).all()
    assert tuple(CN.pack_brackets([[(0, 1)] * 256]).shape) == (1, 256, 3)


def test_refusals_on_the_host():
    with pytest.raises(ValueError, match='M must be in 0..256'):
        CN.pack_brackets([[(0, 1)] * 257])
    with pytest.raises(ValueError, match='M must be in 0..256'):
        CN.pack_brackets([[]], M=257)
    with pytest.raises(ValueError, match='a sentence has 2 brackets'):
        CN.pack_brackets([[(0, 1), (0, 2)]], M=1)
    with pytest.raises(ValueError, match='forbidden 1'):
        CN.pack_brackets([[], []], [[]])
    from cliora_amd import ragged

    class Net(object):
        diora = None

    with pytest.raises(ValueError, match='one list of spans per sentence'):
        ragged.parse_ragged_constrained(Net(), [[1, 2]], [[], []])
    with pytest.raises(ValueError, match='at most 256 brackets'):
        ragged.parse_ragged_constrained(Net(), [[1, 2]], [[(0, 1)] * 257])


def test_brackets_from_entity_labels():
    labels = [[('people', 0, 3), None, ('hat', 4, 1), ('other', 2, 3), ('people', 0, 3), ('scene', 0, 6), ('bodyparts', 1, 2)],
              [None], []]
    assert CN.brackets_from_entity_labels(labels) == [[(0, 2), (0, 5), (1, 2)], [], []]       # (2, 4) crosses (0, 2); size 1 dropped
    assert CN.brackets_from_entity_labels(labels, drop_crossing=False)[0] == [(0, 2), (2, 4), (0, 5), (1, 2)]
    assert CN.brackets_from_entity_labels(labels, min_size=1)[0] == [(0, 2), (4, 4), (0, 5), (1, 2)]
    assert CN.brackets_from_entity_labels(labels, min_size=3)[0] == [(0, 2), (0, 5)]
    from cliora_amd.phrases import entity_rows
    kept = CN.brackets_from_entity_labels(labels, drop_crossing=False)
    assert sorted(set((i, pos, pos + size - 1) for i, pos, size, _ in entity_rows(labels))) == \
        sorted((i, s, e) for i, spans in enumerate(kept) for s, e in spans)
    # the laminar subset is feasible as a required set
    got = CN.constrained_numpy(CC.enum_scores(6, 0), [6], CN.pack_brackets(CN.brackets_from_entity_labels(labels[:1])).numpy())
    assert got.feasible[0] == 1 and got.status == 0
    crossing = CN.constrained_numpy(CC.enum_scores(6, 0), [6], CN.pack_brackets(kept[:1]).numpy())
    assert crossing.feasible[0] == 0 and crossing.status == 0
