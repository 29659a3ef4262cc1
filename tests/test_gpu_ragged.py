"""Mixed-length batches on the device (cliora_amd/ragged.py, cliora_cky_spans_ragged).

The yardstick is the existing path -- forward + cky_spans() on a batch of the sentence's exact length, itself pinned to the
reference's goldens -- never the new code.  The padded chart's own-triangle cells were measured against the exact-length charts on
the MI355X (ragged_cases.MEASURED_INSIDE_S_DIFF): they agree to rounding, not bitwise, so the tree test excuses
a sentence only on a near-tie of the existing path's own candidates, and at most 2 % of them.
"""
import numpy as np
import pytest
import torch

import ragged_cases as RC

pytestmark = pytest.mark.gpu


def _module(P, D):
    from cliora_amd.diora import DioraMLP
    m = DioraMLP(D, outside=True, normalize='unit', compress=False, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P['inside_' + k[len('outside_'):] if k.startswith('outside_') else k].detach().clone()
    m.load_state_dict(sd)
    return m.cuda().eval()


def _exact(m, xs):
    """The existing path, one sentence at a time at its own length: spans, inside_s, inside_h per sentence."""
    res = []
    with torch.no_grad():
        for x in xs:
            xg = x[None].cuda()
            m(xg, xg)
            res.append((m.cky_spans()[0].tolist(), m.chart.inside_s[0, :, 0].cpu().numpy().copy(), m.chart.inside_h[0].cpu().numpy().copy(),
                        _split_scores(m)))
    return res


def _split_scores(m):
    """Per-split inside scores of the chart the module just computed (B = 1), read from the forward workspace where the CKY kernels
    read them: {level: (1, Lc, N, 1)} as the oracle's pair_s_in."""
    from cliora_amd import _lib
    plan = m._plan
    assert plan.B == 1
    sp = _lib.lib().cliora_plan_fwd_offset(plan.handle, b'sp')
    base = plan.table('pair_lvl_base_in')
    ws = m._wss[0].view(torch.float32).cpu()
    return {lv: ws[sp + int(base[lv]):sp + int(base[lv]) + (plan.L - lv) * lv].view(1, plan.L - lv, lv, 1).clone() for lv in range(1, plan.L)}


def _own_cells(L, n):
    """Cell ids, in a chart of length L, of the triangle of a sentence of length n, in the order of a chart of length n."""
    ids = []
    for level in range(n):
        off = L * (L + 1) // 2 - (L - level) * (L - level + 1) // 2
        ids.extend(range(off, off + n - level))
    return np.array(ids)


def _padded_run(m, xs, outside=False):
    xp = RC.padded(xs).cuda()
    m.outside = outside
    with torch.no_grad():
        m(xp, xp)
    return xp


@pytest.mark.parametrize('D', sorted(RC.CASES))
def test_padded_chart_decodes_to_the_exact_length_trees(D):
    """Ragged spans of the padded chart == cky_spans() of the existing path at the sentence's exact length, for every sentence; the
    rows beyond n - 1 are (-1, -1), split_out is -1 outside each triangle and at the leaves."""
    from cliora_amd import ragged
    P, xs, lengths = RC.case(D)
    m = _module(P, D)
    want = _exact(m, xs)
    _padded_run(m, xs)
    L, Cc = RC.LMAX, RC.LMAX * (RC.LMAX + 1) // 2
    spans, status, split = ragged.cky_spans_ragged(m, torch.tensor(lengths, dtype=torch.int32).cuda(), split_out=True)
    spans, split = spans.cpu().numpy(), split.cpu().numpy()
    assert status.cpu().tolist() == [0]
    ins_s = m.chart.inside_s[:, :, 0].cpu().numpy()
    diff = max(float(np.abs(ins_s[b, _own_cells(L, n)] - want[b][1]).max()) for b, n in enumerate(lengths))
    scale = max(1.0, max(float(np.abs(w[1]).max()) for w in want))
    print('D %d: max |inside_s(padded) - inside_s(exact)| = %.3e (scale %.3e)' % (D, diff, scale))
    assert diff <= 1e-4 * scale                                             # the project's forward bound
    # Not bitwise (the level kernels' tiles depend on a level's row count), so a sentence may differ ONLY where the existing path's
    # own chart has a cell whose two best candidates are within NEAR_TIE, and at most 2 % of the sentences may.  The CPU test shows
    # that the fp64 oracle has no such cell on these inputs: the cap is met by the yardstick alone.
    same = [spans[b, :n - 1].tolist() == want[b][0] for b, n in enumerate(lengths)]
    gaps = [RC.cky_margin(w[3], n) for w, n in zip(want, lengths)]
    print('D %d: %d of %d sentences decode to the exact-length tree; smallest candidate gap of the existing path %.3e'
          % (D, sum(same), len(same), min(gaps)))
    excused = [b for b, ok in enumerate(same) if not ok and gaps[b] < RC.NEAR_TIE]
    wrong = [lengths[b] for b, ok in enumerate(same) if not ok and gaps[b] >= RC.NEAR_TIE]
    assert not wrong, 'sentences of these lengths differ without a near-tie: %s' % wrong
    assert len(excused) <= 0.02 * len(lengths), 'near-tie sentences %s' % excused
    for b, n in enumerate(lengths):
        assert (spans[b, max(n - 1, 0):] == -1).all()
        if n > 1:
            assert spans[b, n - 2].tolist() == [0, n - 1]                   # the sentence's own root, last
        own = _own_cells(L, n)
        outside_triangle = np.setdiff1d(np.arange(Cc), own[n:])
        assert (split[b, outside_triangle] == -1).all()
        assert (split[b, own[n:]] >= 0).all()


def test_bad_lengths_are_counted_and_harm_no_other_sentence():
    from cliora_amd import ragged
    D = 50
    P, xs, lengths = RC.case(D)
    m = _module(P, D)
    _padded_run(m, xs)
    good = torch.tensor(lengths, dtype=torch.int32).cuda()
    ref_spans, _, ref_split = ragged.cky_spans_ragged(m, good, split_out=True)
    bad = good.clone()
    bad[3], bad[10], bad[17] = 0, RC.LMAX + 1, -5
    spans, status, split = ragged.cky_spans_ragged(m, bad, split_out=True)
    assert status.cpu().tolist() == [3]
    for b in range(len(lengths)):
        if b in (3, 10, 17):
            assert bool((spans[b] == -1).all()) and bool((split[b] == -1).all())
        else:
            assert torch.equal(spans[b], ref_spans[b]) and torch.equal(split[b], ref_split[b])


@pytest.mark.parametrize('D,B,L', [(50, 9, 14), (400, 5, 23), (50, 3, 2), (50, 4, 1), (50, 2, 65), (50, 2, 128)])
def test_all_equal_lengths_are_bitwise_cky_spans(D, B, L):
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import _ptr, _stream
    P, _, _ = RC.case(D)
    m = _module(P, D)
    x = torch.randn(B, L, D, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        m(x, x)
    spans, status, split = ragged.cky_spans_ragged(m, torch.full((B,), L, dtype=torch.int32).cuda(), split_out=True)
    assert status.cpu().tolist() == [0]
    assert spans.cpu().numpy().tolist() == m.cky_spans().tolist()
    want_split = torch.empty((B, m._plan.C), dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().cliora_cky_decode(m._plan.handle, _ptr(m._wss[0]), _ptr(want_split), _stream()), 'cliora_cky_decode')
    assert torch.equal(split, want_split)


def _net(D, V=97, E=32, seed=11):
    from cliora_amd.harness import build_net
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(V, E)
    return build_net(D, emb, obj_feats=False).cuda()


def _sentences(lengths, V=97, seed=5):
    rs = np.random.RandomState(seed)
    return [rs.randint(1, V, size=n).tolist() for n in lengths]


@pytest.mark.parametrize('max_waste', [0.0, 1.0, float('inf')])
def test_parse_ragged_returns_the_callers_order(max_waste):
    """parse_ragged == the existing path (net on a batch of one exact-length sentence, then cky()), sentence by sentence, in the
    order the caller gave -- whatever the packer did with them."""
    from cliora_amd import ragged
    net = _net(50)
    lengths = [9, 1, 30, 2, 17, 9, 40, 3, 25, 12, 6, 33, 2, 21, 9, 1, 38, 14]
    sents = _sentences(lengths)
    net.train()
    had_outside = net.diora.outside
    got = ragged.parse_ragged(net, sents, max_batch=7, max_waste=max_waste)
    assert net.training and net.diora.outside == had_outside          # both restored
    net.eval()
    want = []
    with torch.no_grad():
        for s in sents:
            net(torch.tensor([s]).cuda(), compute_loss=False)
            want.append(net.diora.cky()[0])
    assert [str(t) for t in got] == [str(t) for t in want]
    assert got[1] == 0 and got[3] == (0, 1)


def test_encode_ragged_rows_are_the_exact_length_roots():
    from cliora_amd import ragged
    net = _net(50)
    lengths = [9, 1, 30, 2, 17, 9, 40, 3, 25, 12, 6, 33]
    sents = _sentences(lengths, seed=6)
    got = ragged.encode_ragged(net, sents, max_batch=5).cpu().numpy()
    assert got.shape == (len(sents), 50)
    net.eval()
    with torch.no_grad():
        for i, s in enumerate(sents):
            net(torch.tensor([s]).cuda(), compute_loss=False)
            want = net.diora.chart.inside_h[0, -1].cpu().numpy()
            err = float(np.abs(got[i] - want).max())
            assert err <= 1e-4 * max(1.0, float(np.abs(want).max())), (i, lengths[i], err)      # the project's forward bound


def test_refusals():
    from cliora_amd import _lib, ragged
    from cliora_amd.harness import build_net
    net = _net(50)
    with pytest.raises(_lib.ChartLibError, match='L > 64'):
        ragged.parse_ragged(net, _sentences([5, 65]))
    with pytest.raises(ValueError):
        ragged.parse_ragged(net, [[1, 2], []])
    assert ragged.parse_ragged(net, []) == []
    vl = build_net(50, torch.nn.Embedding(97, 32), obj_feats=True, img_dim=64).cuda()
    with pytest.raises(NotImplementedError, match='outside'):
        ragged.parse_ragged(vl, _sentences([3, 4]))
