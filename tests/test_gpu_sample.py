"""cliora_sample_trees on the GPU (cliora_amd/sample.py): trees drawn from the chart's posterior, their log-probabilities and log_z.

The yardstick, never the code under test: ``sample_numpy`` (pinned to enumeration of every binary tree by test_sample_cpu.py) on the
device's OWN per-split scores, read through cliora_inside_pair_states, so that the comparison isolates this kernel.  Spans bit for
bit -- a sample may be left out only where the restatement's margin for it is below 1e-9, at most one per test, the count printed;
log_prob and log_z within the project's bound.  Cases and measured figures: sample_cases.py.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import posterior_cases as PC
import sample_cases as SC

pytestmark = pytest.mark.gpu


def _scores(m):
    """Per-split inside scores of the chart the module just computed, through cliora_inside_pair_states: {level: (B, L - level, level)}."""
    from cliora_amd import _lib
    plan, ws = m._plan, m._wss[0]
    assert len(m._wss) == 1
    wsf = ws.view(torch.float32)
    out = {}
    for level in range(1, plan.L):
        ps, ph, rows, ldh = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.call('cliora_inside_pair_states', plan.handle, C.c_void_p(ws.data_ptr()), level, C.byref(ps), C.byref(ph), C.byref(rows),
                  C.byref(ldh))
        so = (ps.value - ws.data_ptr()) // 4
        out[level] = wsf[so:so + rows.value].view(plan.B, plan.L - level, level).cpu().numpy()
    return out


def _forward(m, x):
    with torch.no_grad():
        m(x, x)


def _host(ts):
    return dict(spans=ts.spans.cpu().numpy(), log_prob=ts.log_prob.cpu().numpy(), log_z=ts.log_z.cpu().numpy(),
                status=ts.status.cpu().tolist())


def _same_bits(got, want, what=''):
    for k in ('spans', 'log_prob', 'log_z'):
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), (what, k)


def _against_numpy(got, want, what):
    """got: _host() of the device; want: sample_numpy's tuple on the device's scores.  -> (max |log_prob - fp64|, max |log_z - fp64|,
    samples left out)."""
    spans, log_prob, log_z, margin = want
    assert got['spans'].shape == spans.shape and got['spans'].dtype == np.int32
    differ = (got['spans'] != spans).reshape(spans.shape[0], spans.shape[1], -1).any(axis=2)
    excused = differ & (margin < SC.MARGIN)
    assert not (differ & ~excused).any(), (what, np.argwhere(differ & ~excused).tolist(), margin[differ].tolist())
    assert excused.sum() <= SC.MAX_EXCUSED, what
    keep = ~excused
    e_lp = float(np.abs(got['log_prob'].astype(np.float64) - log_prob)[keep].max())
    e_lz = float(np.abs(got['log_z'].astype(np.float64) - log_z).max())
    print('%s: max |log_prob - fp64| = %.3e, max |log_z - fp64| = %.3e, left out %d (smallest margin %.3e)'
          % (what, e_lp, e_lz, int(excused.sum()), float(margin.min())))
    assert e_lp <= SC.BOUND and e_lz <= SC.BOUND, what
    return e_lp, e_lz, int(excused.sum())


@functools.lru_cache(maxsize=None)
def _uniform(L):
    """One eval forward of a text-only DioraMLP (D 16, B 3, random weights) at length L and the device's scores -- once per length."""
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, L, PC.GPU_B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m))


def _check_uniform(L, S, beta=1.0):
    from cliora_amd.sample import sample_numpy, sample_spans
    r = _uniform(L)
    got = _host(sample_spans(r['m'], S, SC.GPU_SEED, beta=beta))
    assert got['status'] == [0]
    assert got['spans'].shape == (PC.GPU_B, S, L - 1, 2) and got['log_prob'].shape == (PC.GPU_B, S)
    _against_numpy(got, sample_numpy(r['scores'], [L] * PC.GPU_B, S, SC.GPU_SEED, beta=beta, L=L), 'L %d, S %d, beta %g' % (L, S, beta))
    if L > 1:
        assert (got['spans'][:, :, -1] == (0, L - 1)).all()                  # the root last
        assert (got['log_prob'] <= 0).all()
    return got


@pytest.mark.parametrize('L', SC.GPU_LENGTHS)
def test_uniform_lengths_are_sample_numpy(L):
    """L in {1, 2, 3, 7, 13}, S 64."""
    got = _check_uniform(L, SC.GPU_S)
    if L <= 2:
        assert (got['log_prob'] == 0).all() and (got['log_z'] == 0).all()     # one tree: probability 1


@pytest.mark.parametrize('L,S', SC.GPU_LONG)
def test_long_instances(L, S):
    """L 65 / S 16 and L 128 / S 8: two splits per lane, the second half of the scan offset by the first half's total."""
    _check_uniform(L, S)


@pytest.mark.parametrize('beta', [1.0, 0.5])
def test_inverse_temperature(beta):
    """L 13: beta scales the potentials in the inside table and in the draw alike."""
    _check_uniform(13, SC.GPU_S, beta)


@pytest.mark.parametrize('L', [5, 13, 65])
def test_log_z_at_beta_one_is_span_posteriors_bit_for_bit(L):
    from cliora_amd.sample import sample_spans
    m = _uniform(L)['m']
    assert torch.equal(sample_spans(m, 2, 1).log_z.view(torch.int32), m.span_posteriors().log_z.view(torch.int32))


def test_beta_zero_is_uniform_over_the_42_trees():
    """L 6, beta 0: every log_prob is -log 42 and log_z is log 42, within the bound; the draws are sample_numpy's."""
    got = _check_uniform(6, SC.GPU_S, 0.0)
    assert np.abs(got['log_prob'] + math.log(42)).max() <= SC.BOUND
    assert np.abs(got['log_z'] - math.log(42)).max() <= SC.BOUND
    assert len(set(SC.span_key(r) for r in got['spans'][0].tolist())) > 20    # 64 uniform draws of 42 trees: no handful


def test_samples_are_among_the_fourteen_trees_with_their_log_probability():
    """L 5, S 64: every sampled tree is one of the 14 that kbest_spans(m, 16) lists, and its log_prob is that tree's KBest.log_prob
    within the bound."""
    from cliora_amd.kbest import kbest_spans
    from cliora_amd.sample import sample_spans
    m = _uniform(5)['m']
    kb = kbest_spans(m, 16)
    assert kb.count.cpu().tolist() == [14] * PC.GPU_B
    ts = sample_spans(m, SC.GPU_S, SC.GPU_SEED)
    klp = kb.log_prob(ts.log_z).cpu().numpy()
    kspans = kb.spans.cpu().numpy()
    got = _host(ts)
    worst = 0.0
    for b in range(PC.GPU_B):
        index = {SC.span_key(kspans[b, t].tolist()): t for t in range(14)}
        assert len(index) == 14
        for s in range(SC.GPU_S):
            t = index[SC.span_key(got['spans'][b, s].tolist())]
            worst = max(worst, abs(float(got['log_prob'][b, s]) - float(klp[b, t])))
    print('L 5: max |log_prob - KBest.log_prob| = %.3e' % worst)
    assert worst <= SC.BOUND


def _padded_module(extra):
    """The L 14 chart of posterior_cases' mixed lengths, with `extra` more sentences of L words behind them."""
    xs = PC.ragged_sentences() + [PC.sentence(PC.GPU_D, PC.RAGGED_L, 9100 + i) for i in range(extra)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.padded(xs, PC.RAGGED_L).cuda())
    return m


def test_padded_chart_with_two_bad_lengths():
    """L 14, lengths [1, 2, 14, 9, 5] plus one 0 and one 15: each sentence samples from its own triangle, the two bad ones are counted
    and empty, rows beyond n - 1 are (-1, -1)."""
    from cliora_amd.sample import sample_numpy, sample_spans
    L, lengths, S = PC.RAGGED_L, PC.RAGGED_LENGTHS + [0, PC.RAGGED_L + 1], 16
    m = _padded_module(2)
    got = _host(sample_spans(m, S, SC.GPU_SEED, torch.tensor(lengths, dtype=torch.int32).cuda()))
    assert got['status'] == [2]
    _against_numpy(got, sample_numpy(_scores(m), lengths, S, SC.GPU_SEED, L=L), 'padded L 14')
    for b in (5, 6):
        assert (got['spans'][b] == -1).all() and (got['log_prob'][b] == 0).all() and got['log_z'][b] == 0
    for b, n in enumerate(PC.RAGGED_LENGTHS):
        assert (got['spans'][b, :, max(n - 1, 0):] == -1).all()
        assert (got['spans'][b, :, :n - 1] >= 0).all() and (got['spans'][b, :, :n - 1] < n).all()
        if n > 1:
            assert (got['spans'][b, :, n - 2] == (0, n - 1)).all()


def test_every_length_equal_to_L_is_the_call_without_lengths():
    from cliora_amd.sample import sample_spans
    m = _uniform(13)['m']
    full = _host(sample_spans(m, 16, SC.GPU_SEED, torch.full((PC.GPU_B,), 13, dtype=torch.int32).cuda()))
    assert full['status'] == [0]
    _same_bits(full, _host(sample_spans(m, 16, SC.GPU_SEED)))


def test_chunked_calls_are_one_call():
    """S = 8 is first_sample 0 and 4 with S = 4 each, at L 13 and in the long instance."""
    from cliora_amd.sample import sample_spans
    for L in (13, 65):
        m = _uniform(L)['m']
        whole = _host(sample_spans(m, 8, SC.GPU_SEED))
        lo, hi = _host(sample_spans(m, 4, SC.GPU_SEED)), _host(sample_spans(m, 4, SC.GPU_SEED, first_sample=4))
        joined = dict(spans=np.concatenate([lo['spans'], hi['spans']], axis=1),
                      log_prob=np.concatenate([lo['log_prob'], hi['log_prob']], axis=1), log_z=lo['log_z'])
        _same_bits(whole, joined, L)
        assert np.array_equal(hi['log_z'].view(np.int32), lo['log_z'].view(np.int32))
        assert not np.array_equal(lo['spans'], hi['spans'])


def test_permuting_sentences_with_their_ids_permutes_the_rows():
    """The same three sentences in another order with their ids: the same samples per sentence (the inside pass of a sentence does
    not depend on its row: the scores are compared first)."""
    from cliora_amd.sample import sample_numpy, sample_spans
    L, S, perm, ids = 13, 16, [2, 0, 1], [40, 7, 1 << 20]
    x = PC.batch(PC.GPU_D, L, PC.GPU_B, PC.GPU_SEED + L)
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, x.cuda())
    base_scores = _scores(m)
    base = _host(sample_spans(m, S, SC.GPU_SEED, ids=torch.tensor(ids, dtype=torch.int32)))
    _against_numpy(base, sample_numpy(base_scores, [L] * 3, S, SC.GPU_SEED, ids=ids, L=L), 'ids')
    _forward(m, x[perm].cuda())
    moved_scores = _scores(m)
    assert all(np.array_equal(base_scores[lv][perm], moved_scores[lv]) for lv in base_scores)
    moved = _host(sample_spans(m, S, SC.GPU_SEED, ids=torch.tensor([ids[i] for i in perm], dtype=torch.int32)))
    _same_bits(moved, {k: base[k][perm] for k in ('spans', 'log_prob', 'log_z')})
    assert not np.array_equal(base['spans'], _host(sample_spans(m, S, SC.GPU_SEED))['spans'])      # the ids reach the draw


@pytest.mark.parametrize('L,S', [(13, 64), (65, 16), (128, 8)])
def test_two_calls_give_equal_bits(L, S):
    from cliora_amd.sample import sample_spans
    m = _uniform(L)['m']
    _same_bits(_host(sample_spans(m, S, SC.GPU_SEED)), _host(sample_spans(m, S, SC.GPU_SEED)))


def test_treelstm_plan():
    """A TreeLSTM plan (L 5): the same score rows, the same draws."""
    from cliora_amd.sample import sample_numpy, sample_spans
    from cliora_amd.treelstm import DioraTreeLSTM
    from oracle import diora_ref as R
    B, L, D = PC.GPU_B, 5, PC.GPU_D
    P = R.init_params_treelstm(D, seed=6, share=True)
    m = DioraTreeLSTM(D, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    m = m.cuda().eval()
    _forward(m, PC.batch(D, L, B, 515).cuda())
    got = _host(sample_spans(m, SC.GPU_S, SC.GPU_SEED))
    _against_numpy(got, sample_numpy(_scores(m), [L] * B, SC.GPU_S, SC.GPU_SEED, L=L), 'TreeLSTM L 5')


def test_module_entry_returns_trees_and_log_probs():
    """DioraBase.sample_trees(5, seed) at L 7: per sentence [(tree, log_prob)], the trees trees_from_spans builds from the device rows."""
    m = _uniform(7)['m']
    ts = _host(m.sample_spans_device(5, 21))
    got = m.sample_trees(5, 21)
    assert len(got) == PC.GPU_B
    for b in range(PC.GPU_B):
        assert len(got[b]) == 5
        assert [str(t) for t, _ in got[b]] == [str(t) for t in m.trees_from_spans(ts['spans'][b])]
        assert [p for _, p in got[b]] == ts['log_prob'][b].tolist()
    half = _host(m.sample_spans_device(5, 21, beta=0.5))
    assert not np.array_equal(half['log_prob'], ts['log_prob'])
    assert [p for _, p in m.sample_trees(5, 21, beta=0.5)[0]] == half['log_prob'][0].tolist()


def _chart_error():
    from cliora_amd._lib import ChartLibError
    return ChartLibError


def test_parse_ragged_samples_returns_the_callers_order():
    """Sentences of 9, 70, 3, 1, 3, 70 and 9 words, max_batch 3: what sample_spans gives on each pack's padded chart with the caller's
    indices as ids, back in the caller's order."""
    from cliora_amd import ragged
    from cliora_amd.harness import build_net
    from cliora_amd.sample import sample_spans
    torch.manual_seed(11)
    net = build_net(50, torch.nn.Embedding(97, 32), obj_feats=False).cuda()
    rs = np.random.RandomState(5)
    sents = [rs.randint(1, 97, size=n).tolist() for n in [9, 70, 3, 1, 3, 70, 9]]
    S, seed = 4, 77
    got = ragged.parse_ragged_samples(net, sents, S, seed, max_batch=3)
    want = [None] * len(sents)

    def per_pack(idx, lens):
        ts = _host(sample_spans(net.diora, S, seed, lens, ids=torch.tensor(idx, dtype=torch.int32)))
        assert ts['status'] == [0]
        for b, i in enumerate(idx):
            trees = net.diora.trees_from_spans(ts['spans'][b, :, :len(sents[i]) - 1])
            want[i] = list(zip(trees, ts['log_prob'][b].tolist()))

    ragged._run_packs(net, sents, 3, ragged.DEFAULT_MAX_WASTE, 0, per_pack, max_len=128)
    assert [len(g) for g in got] == [S] * len(sents)
    assert [[(str(t), p) for t, p in g] for g in got] == [[(str(t), p) for t, p in w] for w in want]
    assert got[3] == [(0, 0.0)] * S
    assert got[0] != got[6] or sents[0] == sents[6]                           # equal lengths, their own ids and words
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError):
            ragged.parse_ragged_samples(net, sents, bad, seed)
    with pytest.raises(_chart_error()):
        ragged.parse_ragged_samples(net, sents, 2, seed, max_len=64)


def test_refusals():
    from cliora_amd import _lib
    from cliora_amd.sample import sample_spans
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    call = lambda h, ws, lengths, ids, S, beta, spans, lp, lz, status: lib.cliora_sample_trees(h, ws, lengths, ids, S, 1, 0, beta, spans, lp,
                                                                                             lz, status, st)
    fresh = _lib.Plan(2, 5, 16)                                               # never ran a forward
    assert call(fresh.handle, p(0), None, None, 4, 1.0, p(100), p(200), p(300), None) != 0
    assert 'before forward' in err()
    m = _uniform(3)['m']
    h, ws = m._plan.handle, C.c_void_p(m._wss[0].data_ptr())
    for S in (0, -1, (1 << 20) + 1):
        assert call(h, ws, None, None, S, 1.0, p(100), p(200), p(300), None) != 0
        assert 'S outside 1..1048576' in err()
    for beta in (-0.5, float('inf'), float('nan')):
        assert call(h, ws, None, None, 4, beta, p(100), p(200), p(300), None) != 0
        assert 'beta negative or not finite' in err()
    for args in [(None, ws, None, None, 4, 1.0, p(100), p(200), p(300)), (h, None, None, None, 4, 1.0, p(100), p(200), p(300)),
                 (h, ws, None, None, 4, 1.0, None, p(200), p(300)), (h, ws, None, None, 4, 1.0, p(100), None, p(300)),
                 (h, ws, None, None, 4, 1.0, p(100), p(200), None)]:
        assert call(*(args + (None,))) != 0
        assert 'NULL argument' in err()
    assert call(h, ws, p(400), None, 4, 1.0, p(100), p(200), p(300), None) != 0
    assert 'without status' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                      # nothing was launched
    with pytest.raises(_lib.ChartLibError, match='S outside 1..1048576'):     # through the Python entry: the library's reason
        sample_spans(m, 0, 1)
    with pytest.raises(_lib.ChartLibError, match='beta negative or not finite'):
        sample_spans(m, 4, 1, beta=-1.0)
    with pytest.raises(ValueError):
        sample_spans(m, 4, 1, torch.zeros(PC.GPU_B, dtype=torch.int64))
    with pytest.raises(ValueError):
        sample_spans(m, 4, 1, ids=torch.zeros(PC.GPU_B + 1, dtype=torch.int32))
