"""``bracket_margin_numpy`` (cliora_amd/structured.py), the restatement of cliora_bracket_margin that the device tests hold the kernel
to: pinned here to enumeration of every binary tree from the definitions and to central differences of its own loss; its ties to
``constrained_numpy`` and to the CKY restatement; and the entry's refusals through the C ABI on a plan made without a device.
Cases and bounds: margin_cases.py."""
import ctypes

import numpy as np
import pytest

import constrained_cases as CC
import margin_cases as MC

from cliora_amd.structured import bracket_margin_numpy


def _rows(rows):
    return CC.pack_rows([rows]) if rows else None


def _cells(res, field, n):
    return MC.tree_of(getattr(res, field)[0][:max(n - 1, 0)])


# ---- 1. against enumeration -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', MC.ENUM_NS)
def test_against_enumeration(n):
    cases, infeasible, positive = 0, 0, 0
    for seed in MC.ENUM_SEEDS:
        scores = MC.enum_scores(n, seed)
        for name, rows in MC.enum_sets(n, seed).items():
            for margin, penalty in MC.PARAMS:
                what = (n, seed, name, margin, penalty)
                want = MC.enumerate_margin(scores, n, rows, margin, penalty)
                assert want['gap'] >= MC.MIN_GAP, what
                got = bracket_margin_numpy(scores, [n], _rows(rows), margin, penalty)
                assert got.status == 0 and got.loss[0] >= 0, what
                assert bool(got.feasible[0]) == want['feasible'], what
                assert abs(got.aug_score[0] - want['aug']) <= MC.ENUM_TOL, what
                assert got.violations[0] == want['violations'], what
                assert _cells(got, 'spans_aug', n) == set((p, p + lv) for lv, p, _ in want['tree_a']), what
                assert abs(got.loss[0] - want['loss']) <= MC.ENUM_TOL, what
                if want['feasible']:
                    assert abs(got.ref_score[0] - want['ref']) <= MC.ENUM_TOL, what
                    assert _cells(got, 'spans_ref', n) == set((p, p + lv) for lv, p, _ in want['tree_b']), what
                else:
                    assert got.ref_score[0] == -np.inf and (got.spans_ref[0] == -1).all(), what
                    assert not any(g.any() for g in got.d_split.values()), what
                    infeasible += 1
                cases += 1
                positive += int(got.loss[0] > 0)
    if n >= 3:
        assert infeasible >= len(MC.ENUM_SEEDS) * 2 and positive > 0, (infeasible, positive)     # the crossing pair under an infinite penalty
    print('n %d: %d cases, %d infeasible, %d with a positive loss' % (n, cases, infeasible, positive))


# ---- 2. the gradient --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (3, 5, 7))
def test_gradient_against_central_differences(n):
    worst, moved = 0.0, 0
    for seed in MC.ENUM_SEEDS:
        scores = MC.enum_scores(n, seed)
        for name, rows in MC.enum_sets(n, seed).items():
            for margin, penalty in MC.PARAMS:
                loss = lambda sc: float(bracket_margin_numpy(sc, [n], _rows(rows), margin, penalty).loss[0])
                G = bracket_margin_numpy(scores, [n], _rows(rows), margin, penalty).d_split
                for level in range(1, n):
                    assert not G[level].sum(axis=2).any(), (n, seed, name)              # row sums: exactly 0
                    for pos in range(n - level):
                        for k in range(level):
                            hi = {lv: s.copy() for lv, s in scores.items()}
                            lo = {lv: s.copy() for lv, s in scores.items()}
                            hi[level][0, pos, k] += MC.FD_H
                            lo[level][0, pos, k] -= MC.FD_H
                            fd = (loss(hi) - loss(lo)) / (2 * MC.FD_H)
                            worst = max(worst, abs(fd - G[level][0, pos, k]))
                            assert abs(fd - G[level][0, pos, k]) <= MC.FD_TOL, (n, seed, name, margin, penalty, level, pos, k, fd)
                moved += int(any(g.any() for g in G.values()))
    print('n %d: max |G - central difference| = %.3e, %d cases with a gradient' % (n, worst, moved))
    assert moved > 0


def test_weights_scale_and_neighbours():
    n, B = 7, 5
    import posterior_cases as PC
    scores = PC.random_scores(B, n, 31)
    sets = [[(1, 4, 1), (2, 3, 0)], [], [(0, 3, 1), (2, 5, 1)], [(0, 6, 1), (3, 3, 1)], [(1, 4, 1), (2, 3, 0)]]
    a = bracket_margin_numpy(scores, [n] * B, CC.pack_rows(sets), 1.0, MC.INF)
    assert a.feasible.tolist() == [1, 1, 0, 1, 1] and a.status == 0
    for level in range(1, n):
        assert not a.d_split[level][1].any() and not a.d_split[level][2].any() and not a.d_split[level][3].any()
    assert a.loss[1] == 0 and a.loss[2] == 0 and a.loss[3] == 0 and a.violations[1] == 0
    assert (a.spans_ref[2] == -1).all() and (a.spans_aug[2, :n - 1] >= 0).all()      # infeasible: the augmented tree is still given
    w = np.array([2.5, 1.0, np.nan, 1.0, -0.5])
    b = bracket_margin_numpy(scores, [n] * B, CC.pack_rows(sets), 1.0, MC.INF, weights=w)
    for level in range(1, n):
        assert np.array_equal(b.d_split[level][0], 2.5 * a.d_split[level][0]) and not b.d_split[level][2].any()
        assert np.array_equal(b.d_split[level][4], -0.5 * a.d_split[level][4]) and not np.signbit(b.d_split[level][4][b.d_split[level][4] == 0]).any()
    # the ramp takes the crossing pair
    c = bracket_margin_numpy(scores, [n] * B, CC.pack_rows(sets), 1.0, 1.0)
    assert c.feasible.tolist() == [1] * B and c.loss[2] > 0 and np.isfinite(c.ref_score[2])
    # a bad row and a bad length: zeros, counted once each, the neighbours unaffected; a shorter sentence: zero beyond its triangle
    sets[1], sets[4] = [(3, 9, 1), (2, 2, 5)], [(1, 2, 1), (0, 1, 0)]
    d =bracket_margin_numpy(scores, [n, n, 0, n, 4], CC.pack_rows(sets), 1.0, MC.INF)
    assert d.status == 2 and d.feasible.tolist()[1:3] == [0, 0] and d.loss[1] == 0 and d.aug_score[1] == 0
    for level in range(1, n):
        assert not d.d_split[level][1].any() and np.array_equal(d.d_split[level][0], a.d_split[level][0])
        assert not d.d_split[level][4, max(0, 4 - level):].any()


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (2, 5, 7))
def test_identities(n):
    from cliora_amd.constrained import constrained_numpy
    from cliora_amd.ragged import decode_ragged_numpy
    import structured_cases as SC
    for seed in MC.ENUM_SEEDS:
        scores = MC.enum_scores(n, seed)
        cky = decode_ragged_numpy(scores, [n])[0]
        # brackets the CKY tree already satisfies, perceptron: loss 0 and a zero gradient
        own = SC.spans_as_required(cky, n)
        got = bracket_margin_numpy(scores, [n], _rows(own), 0.0, MC.INF)
        assert got.loss[0] == 0 and not np.signbit(got.loss[0]) and got.feasible[0] == 1 and got.violations[0] == 0
        assert not any(g.any() for g in got.d_split.values())
        assert _cells(got, 'spans_aug', n) == _cells(got, 'spans_ref', n) == set(cky)
        for name, rows in MC.enum_sets(n, seed).items():
            cp = constrained_numpy(scores, [n], CC.pack_rows([rows]) if rows else None, L=n)
            for margin, penalty in MC.PARAMS:
                got = bracket_margin_numpy(scores, [n], _rows(rows), margin, penalty)
                if penalty == MC.INF:                   # the reference tree is constrained_numpy's, row by row
                    assert np.array_equal(got.spans_ref, cp.spans) and np.array_equal(got.feasible, cp.feasible), (n, seed, name)
                if margin == 0:                         # the augmented tree is the CKY restatement's, row by row
                    assert [tuple(r) for r in got.spans_aug[0][:n - 1].tolist()] == cky, (n, seed, name)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    """Every refusal comes before any launch (there is no GPU here), with CLIORA_EINVAL and a message that starts with the entry's name."""
    from cliora_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    err = lambda: _lib.fn('cliora_last_error')().decode()
    # (plan, ws, lengths, brackets, M, margin, penalty, weights, d_split, loss, aug, ref, violations, feasible, spans_aug, spans_ref, status)
    good = lambda h: [h, p, None, p, 2, 1.0, MC.INF, None, p, p, p, p, p, p, None, None, p]
    call = lambda a: lib.cliora_bracket_margin(*(a + [None]))
    text = _lib.Plan(2, 5, 16)

    def refused(words, **change):
        a = good(text.handle)
        for i, v in change.items():
            a[int(i[1:])] = v
        rc = call(a)
        assert rc == -1 and err().startswith('cliora_bracket_margin') and words in err(), (rc, err(), words)
    for M in (-1, 257):
        refused('M outside 0..256', _4=M)
    for margin in (-0.5, float('nan'), MC.INF):
        refused('margin', _5=margin)
    for penalty in (-1.0, float('nan')):
        refused('penalty', _6=penalty)
    for i in (0, 1, 8, 9, 10, 11, 12, 13, 16):          # plan, workspace, d_split, the three scores, violations, feasible, status
        refused('NULL argument', **{'_%d' % i: None})
    refused('NULL brackets', _3=None)
    a = good(_lib.Plan(2, 70, 16, forward_only=True).handle)
    assert call(a) == -1 and err().startswith('cliora_bracket_margin') and 'the backward stops at 64 words' in err()
    for plan in (text, _lib.Plan(2, 5, 16, arch=1)):     # past every refusal of its own (a TreeLSTM plan too): no forward has run
        assert call(good(plan.handle)) == -1 and err().startswith('cliora_bracket_margin') and 'before forward' in err()
    assert not buf.any()


def test_python_side_value_errors():
    import torch
    from cliora_amd import _lib, structured

    class NoForward(object):
        _plan = None
    for f in (structured.bracket_margin, structured.bracket_margin_loss, structured.bracket_hinge):
        with pytest.raises(_lib.ChartLibError, match='has run no forward'):
            f(NoForward(), None)

    class Chart(object):                                 # what the checks read before any device call
        _plan = _lib.Plan(2, 5, 16)
        _wss = [torch.zeros(4)]
    for kw in (dict(margin=-1.0), dict(margin=float('nan')), dict(margin=MC.INF), dict(penalty=-0.5), dict(penalty=float('nan'))):
        with pytest.raises(ValueError, match='margin|penalty'):
            structured.bracket_margin(Chart(), None, **kw)
        with pytest.raises(ValueError, match='margin|penalty'):
            structured.bracket_hinge(Chart(), None, **kw)
        with pytest.raises(ValueError, match='margin|penalty'):
            bracket_margin_numpy({}, [1], None, kw.get('margin', 1.0), kw.get('penalty', MC.INF))
    with pytest.raises(ValueError, match='brackets must be int32'):
        structured.bracket_margin(Chart(), torch.zeros((3, 2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match='brackets must be int32'):
        structured.bracket_margin(Chart(), torch.zeros((2, 2, 3), dtype=torch.int64))
    with pytest.raises(ValueError, match='lengths must be int32'):
        structured.bracket_margin(Chart(), None, lengths=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='weights must hold'):
        structured.bracket_margin(Chart(), None, weights=torch.zeros(5))
    with pytest.raises(ValueError, match='reduction'):
        structured.bracket_hinge(Chart(), None, reduction='max')
