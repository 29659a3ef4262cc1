"""``tree_kl_numpy`` (cliora_amd/structured.py): the fp64 restatement of cliora_tree_kl that the device tests measure the kernel
against, pinned here to enumeration of every binary tree over BOTH score tables, to central differences of the enumerated objective, to
closed forms and to ``tree_expectation_numpy``; the ABI table's entry and the refusals that need no device.  Cases and bounds:
kl_cases.py."""
import types

import numpy as np
import pytest
import torch

import constrained_cases as CC
import expectation_cases as EC
import kl_cases as KC
import posterior_cases as PC
import structured_cases as SC

from cliora_amd import _lib, structured
from cliora_amd.query import ChartQuery
from cliora_amd.structured import tree_expectation_numpy, tree_kl_numpy


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=KC.ENUM_RTOL, atol=KC.ENUM_RTOL, err_msg=str(what))


def _pair(n, seed):
    """Two random score tables of one sentence of n words (a chart of length max(n, 2))."""
    return CC.enumeration(n, seed)[0], PC.random_scores(1, max(n, 2), 7000 + 100 * n + seed)


@pytest.mark.parametrize('n', CC.ENUM_NS)
def test_against_enumeration(n):
    for seed in CC.ENUM_SEEDS:
        pair_p, pair_q = _pair(n, seed)
        L = max(n, 2)
        for wk, wc in KC.WEIGHTS:
            want = KC.enumerated(pair_p, pair_q, n, wk, wc)
            got = tree_kl_numpy(pair_p, pair_q, [n], [wk], [wc])
            assert got.status == 0
            for name in ('kl', 'cross_entropy', 'entropy_p', 'log_z_p', 'log_z_q'):
                _close(getattr(got, name)[0], want[name], (n, seed, name))
            for level in range(1, L):
                for G, key in ((got.d_split_p, 'Gp'), (got.d_split_q, 'Gq')):
                    _close(G[level][0, :max(0, n - level)], want[key].get(level, np.zeros((0, level))), (n, seed, wk, wc, level, key))
                    assert not G[level][0, max(0, n - level):].any()
            assert got.kl[0] >= -1e-12
            _close(got.cross_entropy[0] - got.entropy_p[0], got.kl[0], (n, seed))
        if n >= 3:
            assert any(np.abs(g).max() > 1e-3 for g in got.d_split_p.values()) and any(np.abs(g).max() > 1e-3 for g in got.d_split_q.values())


@pytest.mark.parametrize('n', KC.FD_NS)
def test_against_central_differences_of_the_enumerated_objective(n):
    tables = [SC.gapped_scores(n, 900 + n), SC.gapped_scores(n, 1900 + n)]
    wk, wc = KC.FD_WEIGHTS
    got = tree_kl_numpy(tables[0], tables[1], [n], [wk], [wc])
    worst = 0.0
    for which, G in enumerate((got.d_split_p, got.d_split_q)):
        for level in range(1, n):
            for pos in range(n - level):
                for k in range(level):
                    J = []
                    for sign in (1.0, -1.0):
                        moved = [{lv: s.copy() for lv, s in t.items()} for t in tables]
                        moved[which][level][0, pos, k] += sign * KC.FD_H
                        J.append(KC.enumerated(moved[0], moved[1], n, wk, wc)['J'])
                    fd = (J[0] - J[1]) / (2 * KC.FD_H)
                    worst = max(worst, abs(fd - G[level][0, pos, k]))
                    assert abs(fd - G[level][0, pos, k]) <= KC.FD_TOL, (n, which, level, pos, k, fd, G[level][0, pos, k])
    print('n %d: max |G - central difference| over both gradients = %.3e' % (n, worst))
    assert any(np.abs(g).max() > 1e-3 for g in got.d_split_p.values()) and any(np.abs(g).max() > 1e-3 for g in got.d_split_q.values())


def test_equal_tables_give_zero():
    L, lengths = 7, [7, 3, 1, 5, 2]
    scores = PC.random_scores(len(lengths), L, 31)
    got = tree_kl_numpy(scores, scores, lengths)                               # KL alone: at p == q the divergence is stationary in both
    mixed = tree_kl_numpy(scores, scores, lengths, [0.7] * 5, [-0.4] * 5)      # (the cross-entropy term is not: d_split_p is -0.4 dH / ds there)
    assert np.abs(got.kl).max() <= 1e-12
    for level in range(1, L):
        assert not got.d_split_q[level].any() and not mixed.d_split_q[level].any()      # exactly: nu^q - nu^p of equal tables
        assert np.abs(got.d_split_p[level]).max() <= 1e-12
    Gh = tree_expectation_numpy(scores, lengths, None, np.zeros(5), np.full(5, -0.4))[0]
    for level in range(1, L):
        np.testing.assert_allclose(mixed.d_split_p[level], Gh[level], rtol=0, atol=1e-12)


def test_entropy_is_the_expectation_restatements_and_kl_is_not_negative():
    L, lengths = 7, [7, 3, 1, 5, 2]
    B = len(lengths)
    sp, sq = PC.random_scores(B, L, 31), PC.random_scores(B, L, 32)
    got = tree_kl_numpy(sp, sq, lengths)
    _, _, entropy, log_z = tree_expectation_numpy(sp, lengths, None, None, np.ones(B))
    _close(got.entropy_p, entropy, 'entropy_p')
    _close(got.log_z_p, log_z, 'log_z_p')
    _close(got.log_z_q, tree_expectation_numpy(sq, lengths, None)[3], 'log_z_q')
    assert (got.kl >= 0).all() and (got.kl[[0, 1, 3]] > 1e-3).all()
    _close(got.cross_entropy - got.entropy_p, got.kl, 'kl')
    assert got.kl[2] == 0 and got.kl[4] == 0 and got.cross_entropy[4] == 0 and got.entropy_p[4] == 0       # one word, two words
    for level in range(1, L):
        assert not got.d_split_p[level][[2, 4]].any() and not got.d_split_q[level][[2, 4]].any()


@pytest.mark.parametrize('n', range(2, 11))
def test_tied_student_scores_give_log_catalan(n):
    rs = np.random.RandomState(n)
    tied = {level: np.repeat(rs.randn(1, n - level, 1), level, axis=2) for level in range(1, n)}          # every row ties: q is uniform
    got = tree_kl_numpy(PC.random_scores(1, n, 40 + n), tied, [n])
    _close(got.cross_entropy[0], np.log(EC.catalan(n - 1)), n)
    _close(got.log_z_q[0], np.log(EC.catalan(n - 1)), n)
    _close(got.kl[0], np.log(EC.catalan(n - 1)) - got.entropy_p[0], n)


def test_row_sums_padding_and_bad_lengths():
    L, lengths = KC.RAGGED_L, list(KC.RAGGED_LENGTHS)
    B = len(lengths)
    sp, sq = PC.random_scores(B, L, 51), PC.random_scores(B, L, 52)
    wk, wc = np.array([0.7, 1.0, -2.0, 0.3]), np.array([-0.4, 0.5, 1.0, 2.0])
    got = tree_kl_numpy(sp, sq, lengths, wk, wc)
    for G in (got.d_split_p, got.d_split_q):
        for level in range(1, L):
            assert np.abs(G[level].sum(axis=2)).max() <= KC.ROW_SUM_TOL, level
    for b, n in enumerate(lengths):                                            # a padded batch is each sentence alone
        cut = lambda t: {lv: t[lv][b:b + 1, :n - lv] for lv in range(1, n)}
        one = tree_kl_numpy(cut(sp), cut(sq), [n], wk[b:b + 1], wc[b:b + 1]) if n > 1 else None
        for name in ('kl', 'cross_entropy', 'entropy_p', 'log_z_p', 'log_z_q'):
            assert getattr(got, name)[b] == (getattr(one, name)[0] if one else 0.0), (b, name)
        for level in range(1, L):
            for G, G1 in ((got.d_split_p, one.d_split_p if one else {}), (got.d_split_q, one.d_split_q if one else {})):
                assert not G[level][b, max(0, n - level):].any()
                if level < n:
                    assert np.array_equal(G[level][b, :n - level], G1[level][0])
    bad = tree_kl_numpy(sp, sq, [5, 0, 8, 7], wk, wc)
    assert bad.status == 2 and not bad.kl[1:3].any() and not bad.log_z_q[1:3].any()
    for level in range(1, L):
        assert not bad.d_split_p[level][1:3].any() and not bad.d_split_q[level][1:3].any()
        assert np.array_equal(bad.d_split_q[level][[0, 3]], got.d_split_q[level][[0, 3]])


def test_torch_restatement_agrees_with_enumeration():
    """kl_cases.torch_kl, the yardstick of the gradients through the chart, against enumeration: values and both gradients."""
    n = 5
    wk, wc = KC.FD_WEIGHTS
    tables = [SC.gapped_scores(n, 905), SC.gapped_scores(n, 1905)]
    tt = [{lv: torch.tensor(s[0], dtype=torch.float64, requires_grad=True) for lv, s in t.items()} for t in tables]
    kl, ce = KC.torch_kl(tt[0], tt[1], n)
    want = KC.enumerated(tables[0], tables[1], n, wk, wc)
    _close(float(kl.detach()), want['kl'], 'kl')
    _close(float(ce.detach()), want['cross_entropy'], 'cross_entropy')
    (wk * kl + wc * ce).backward()
    for level in range(1, n):
        np.testing.assert_allclose(tt[0][level].grad.numpy(), want['Gp'][level], rtol=0, atol=1e-10)
        np.testing.assert_allclose(tt[1][level].grad.numpy(), want['Gq'][level], rtol=0, atol=1e-10)


def test_abi_entry_and_symbol():
    restype, argtypes = _lib.ABI['cliora_tree_kl']
    assert len(argtypes) == 16 and all(a is _lib.ABI['cliora_tree_expectation'][1][0] for a in argtypes)
    f = _lib.fn('cliora_tree_kl')                                              # exported by the built library
    assert f.restype is restype and list(f.argtypes) == list(argtypes)


def _stub(B, L, nws=1):
    return types.SimpleNamespace(_plan=types.SimpleNamespace(B=B, L=L, C=L * (L + 1) // 2, handle=None), _wss=[torch.zeros(1)] * nws)


def test_refusals_that_need_no_device():
    never = types.SimpleNamespace(_plan=None)
    for args in ((never, _stub(2, 5)), (_stub(2, 5), never)):
        with pytest.raises(_lib.ChartLibError, match='has run no forward'):
            structured.tree_kl(*args)
    with pytest.raises(_lib.ChartLibError, match='has run no forward'):
        structured.parse_kl(_stub(2, 5), never)
    with pytest.raises(_lib.ChartLibError, match='has run no forward'):
        structured.parse_divergence(never, _stub(2, 5))
    for other in (_stub(3, 5), _stub(2, 6), _stub(2, 5, nws=2)):               # B, L, the number of workspaces
        with pytest.raises(ValueError, match='the two charts differ'):
            structured.tree_kl(_stub(2, 5), other)
        with pytest.raises(ValueError, match='the two charts differ'):
            ChartQuery(_stub(2, 5)).second(ChartQuery(other), 'tree_kl')
    with pytest.raises(ValueError, match='lengths must be int32'):
        structured.tree_kl(_stub(2, 5), _stub(2, 5), lengths=torch.zeros(2))
    with pytest.raises(ValueError, match='w_kl must hold one value per sentence'):
        structured.tree_kl(_stub(2, 5), _stub(2, 5), w_kl=torch.zeros(3))
    with pytest.raises(ValueError, match='direction'):
        structured.parse_divergence(_stub(2, 5), _stub(2, 5), direction='sideways')
    with pytest.raises(ValueError, match='reduction'):
        structured.parse_divergence(_stub(2, 5), _stub(2, 5), reduction='max')
