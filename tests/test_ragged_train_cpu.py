"""Training through a padded chart of mixed lengths, the facts it rests on, on the CPU in fp64: the schedule
of cliora_chart_forward_ragged_train differentiated by torch autograd gives, for a loss on the own triangles, the sum of the
oracle's per-sentence exact-length gradients; and which rows the two new kernels touch, against brute force."""
import numpy as np
import pytest
import torch

import ragged_outside_cases as ROC
import ragged_train_cases as TC
from oracle import chart_layout as CL


@pytest.mark.parametrize('normalize,share', [('unit', True), ('unit', False), ('none', True), ('none', False)])
@pytest.mark.parametrize('D,lengths', TC.CPU_CASES)
def test_masked_schedule_differentiates_to_the_per_sentence_gradients(D, lengths, normalize, share):
    L = max(lengths)
    assert {1, 2, L} <= set(lengths) and len(set(lengths)) < len(lengths)
    P, xs, _ = ROC.small_case(D, lengths, seed=31 + D, share=share, scale=1.0 if normalize == 'unit' else 0.25)
    W = TC.weights(L, lengths, D, seed=7)
    want_loss, want, want_dx, _ = TC.oracle_sum(P, xs, lengths, W, normalize, share)
    xp = ROC.padded(xs, L)
    loss, got, dx = TC.padded_autograd(P, xp, lengths, W, normalize, share)
    assert abs(loss - want_loss) <= TC.CPU_BOUND * max(1.0, abs(want_loss))
    worst = 0.0
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        worst = max(worst, TC.rel_err(got[k], want[k]))
    for b, n in enumerate(lengths):
        assert bool(torch.isfinite(dx[b]).all())
        worst = max(worst, TC.rel_err(dx[b, :n], want_dx[b]))
        assert not dx[b, n:].any()                      # d x of every padded position: exactly 0
    print('D %d %s share=%s: worst relative error %.3e' % (D, normalize, share, worst))
    assert worst <= TC.CPU_BOUND


@pytest.mark.parametrize('L', range(2, 13))
def test_rows_the_kernels_touch_by_brute_force(L):
    """ragged_mask_cotangents zeroes exactly the cells whose span [pos, pos + level] does not end inside the sentence;
    ragged_root_cut(level) and root_bwd address exactly the cell that spans the whole sentence."""
    off = CL.level_offsets(L)
    rs = np.random.RandomState(L)
    lengths = list(range(1, L + 1)) + [int(rs.randint(1, L + 1)) for _ in range(4)]
    C = L * (L + 1) // 2
    span_of = {}
    for level in range(L):
        for pos in range(L - level):
            span_of[int(off[level]) + pos] = (pos, pos + level)
    assert sorted(span_of) == list(range(C))
    masked = TC.masked_rows(L, lengths)
    for b, n in enumerate(lengths):
        brute = np.array([span_of[c][1] >= n for c in range(C)])
        assert (masked[b] == brute).all(), (b, n)
        assert int((~masked[b]).sum()) == n * (n + 1) // 2
        assert span_of[TC.root_cell(L, n)] == (0, n - 1)
    assert TC.root_cell(L, L) == C - 1
    cut = [TC.root_cut_rows(L, lengths, level) for level in range(L)]
    assert cut[L - 1] == []                              # level L - 1 is the padded chart's own root: root_bwd's, never cut
    for level in range(L - 1):
        want = [(b, c) for b, n in enumerate(lengths) for c in range(C) if n < L and span_of[c] == (0, n - 1) and n - 1 == level]
        assert cut[level] == want
    # every sentence shorter than L is cut exactly once, none of length L
    assert sorted(b for rows in cut for b, _ in rows) == [b for b, n in enumerate(lengths) if n < L]


def test_refusals_on_the_cpu():
    """What needs no device: the module state is there, the inference state keeps its refusal, and the training entry refuses a net
    it cannot take before any launch."""
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import ChartWorkspaces, DioraMLP
    from cliora_amd.harness import build_net
    m = DioraMLP(8)
    assert m._ragged is None and m._ragged_train is None
    assert ChartWorkspaces().lengths is None
    for name in ('cliora_chart_forward_ragged_train', 'cliora_chart_backward_ragged'):
        assert name in _lib.ABI
    net = build_net(16, torch.nn.Embedding(11, 16), obj_feats=True, img_dim=16)
    with pytest.raises(NotImplementedError, match='text-only'):
        next(ragged.forward_ragged_train(net, [[1, 2, 3]]))
    net = build_net(16, torch.nn.Embedding(11, 16))
    with pytest.raises(_lib.ChartLibError, match='L > 64'):
        next(ragged.forward_ragged_train(net, [[1] * 65]))
    with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='gradients enabled'):
        next(ragged.forward_ragged_train(net, [[1, 2]]))
