"""cliora_kbest_spans on the GPU (cliora_amd/kbest.py): the K best trees, their scores and their number.

The yardstick, never the code under test: ``kbest_numpy`` (pinned to enumeration of every binary tree by test_kbest_cpu.py) on the
device's OWN per-split scores, read through cliora_inside_pair_states, so that the comparison isolates this kernel -- spans, scores
and counts bit for bit.  Cases and measured figures: kbest_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kbest_cases as KC
import posterior_cases as PC

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


def _host(kb):
    return dict(spans=kb.spans.cpu().numpy(), scores=kb.scores.cpu().numpy(), count=kb.count.cpu().numpy(), status=kb.status.cpu().tolist())


def _same_bits(got, want, what=''):
    """want: kbest_numpy's (spans, scores, count), or another _host() dict."""
    if isinstance(want, dict):
        want = (want['spans'], want['scores'], want['count'])
    assert np.array_equal(got['count'], want[2]), what
    assert np.array_equal(got['scores'].view(np.int32), want[1].view(np.int32)), what
    assert got['spans'].shape == want[0].shape and np.array_equal(got['spans'], want[0]), what


@functools.lru_cache(maxsize=None)
def _uniform(L):
    """One eval forward of a text-only DioraMLP (D 16, B 3, random weights) at length L and the device's scores -- once per length."""
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, L, PC.GPU_B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m))


def _check_uniform(L, K):
    from cliora_amd.kbest import kbest_numpy, kbest_spans, tree_count
    r = _uniform(L)
    got = _host(kbest_spans(r['m'], K))
    assert got['status'] == [0]
    assert got['count'].tolist() == [tree_count(L, K)] * PC.GPU_B
    _same_bits(got, kbest_numpy(r['scores'], [L] * PC.GPU_B, K, L), (L, K))
    if L > 1:
        assert np.array_equal(got['spans'][:, 0], r['m'].cky_spans_device().cpu().numpy())       # rank 0: cliora_cky_spans' tree
        assert (got['scores'][:, 0] >= got['scores'][:, -1]).all() and (got['scores'][:, 0] <= 0).all()
    return got


@pytest.mark.parametrize('K', KC.KS)
@pytest.mark.parametrize('L', KC.GPU_LENGTHS)
def test_uniform_lengths_are_kbest_numpy_bit_for_bit(L, K):
    """L in {1, 2, 3, 7, 13}, K in {1, 3, 8, 16}: spans, scores and counts; at K = 1 (and at every K, rank 0) cky_spans_device()'s rows."""
    _check_uniform(L, K)


@pytest.mark.parametrize('L,K', KC.GPU_LONG)
def test_long_instances(L, K):
    """L 65 / K 4: two splits per lane, the lists in LDS.  L 128 / K 8: the lists in the caller's scratch."""
    from cliora_amd import _lib
    need = _lib.fn('cliora_kbest_scratch_bytes')(_uniform(L)['m']._plan.handle, K)
    assert need == (0 if L == 65 else PC.GPU_B * (L * (L + 1) // 2) * K * 8)
    _check_uniform(L, K)


def _padded_module(extra):
    """The L 14 chart of posterior_cases' mixed lengths, with `extra` more sentences of L words behind them."""
    xs = PC.ragged_sentences() + [PC.sentence(PC.GPU_D, PC.RAGGED_L, 9100 + i) for i in range(extra)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.padded(xs, PC.RAGGED_L).cuda())
    return m


@pytest.mark.parametrize('K', [3, 16])
def test_padded_chart_with_two_bad_lengths(K):
    """L 14, lengths [1, 2, 14, 9, 5] plus one 0 and one 15: each sentence from its own triangle, the two bad ones counted and empty."""
    from cliora_amd.kbest import kbest_numpy, kbest_spans
    L, lengths = PC.RAGGED_L, PC.RAGGED_LENGTHS + [0, PC.RAGGED_L + 1]
    m = _padded_module(2)
    got = _host(kbest_spans(m, K, torch.tensor(lengths, dtype=torch.int32).cuda()))
    assert got['status'] == [2]
    _same_bits(got, kbest_numpy(_scores(m), lengths, K, L))
    for b in (5, 6):
        assert got['count'][b] == 0 and np.isneginf(got['scores'][b]).all() and (got['spans'][b] == -1).all()
    for b, n in enumerate(PC.RAGGED_LENGTHS):
        assert (got['spans'][b, :, max(n - 1, 0):] == -1).all()
        assert (got['spans'][b, :got['count'][b], :n - 1] >= 0).all()


def test_every_length_equal_to_L_is_the_call_without_lengths():
    from cliora_amd.kbest import kbest_spans
    m = _uniform(13)['m']
    for K in (1, 8):
        full = _host(kbest_spans(m, K, torch.full((PC.GPU_B,), 13, dtype=torch.int32).cuda()))
        assert full['status'] == [0]
        _same_bits(full, _host(kbest_spans(m, K)))


def test_exact_ties_give_sixteen_distinct_trees_in_key_order():
    """A module whose parameters are all zero, L 6, K 16: every per-split score is 0, so every candidate of a cell ties and the order
    is that of the keys alone (kbest_cases.key_order_spans, from the definition); every tree's score is 0."""
    from cliora_amd.kbest import kbest_numpy, kbest_spans
    L, K = 6, 16
    P = {k: torch.zeros_like(v) for k, v in PC.params(PC.GPU_D, PC.GPU_SEED).items()}
    m = PC.text_module(P, PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, L, PC.GPU_B, 31).cuda())
    scores = _scores(m)
    assert all((s == 0).all() for s in scores.values())
    got = _host(kbest_spans(m, K))
    _same_bits(got, kbest_numpy(scores, [L] * PC.GPU_B, K, L))
    want = KC.key_order_spans(L, K)
    for b in range(PC.GPU_B):
        assert got['count'][b] == 16 and (got['scores'][b] == 0).all()
        trees = [tuple(map(tuple, got['spans'][b, t].tolist())) for t in range(K)]
        assert len(set(trees)) == 16
        assert [list(t) for t in trees] == want


def test_all_fourteen_trees_hold_the_whole_posterior_mass():
    """L 5, K 16: count 14 = Catalan(4), and sum over the trees of exp(score - log_z) is 1 within the project's bound, log_z from
    cliora_span_posteriors on the same chart.  Measured: kbest_cases.MEASURED['mass']."""
    from cliora_amd.kbest import kbest_spans
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, 5, PC.GPU_B, PC.GPU_SEED + 5).cuda())
    kb = kbest_spans(m, 16)
    assert kb.count.cpu().tolist() == [14] * PC.GPU_B
    lp = kb.log_prob(m.span_posteriors().log_z)
    assert torch.equal(lp, kb.scores - m.span_posteriors().log_z[:, None])
    mass = lp[:, :14].double().exp().sum(1).cpu().numpy()
    err = float(np.abs(mass - 1).max())
    print('L 5, K 16: max |sum exp(score - log_z) - 1| = %.3e' % err)
    assert err <= KC.MASS_BOUND
    assert np.isneginf(lp[:, 14:].cpu().numpy()).all()


@pytest.mark.parametrize('L,K', [(13, 16), (65, 4), (128, 8)])
def test_two_calls_give_equal_bits(L, K):
    from cliora_amd.kbest import kbest_spans
    m = _uniform(L)['m']
    _same_bits(_host(kbest_spans(m, K)), _host(kbest_spans(m, K)))


def test_treelstm_plan():
    """A TreeLSTM plan (L 5): the same score rows, the same lists."""
    from cliora_amd.kbest import kbest_numpy, kbest_spans
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
    got = _host(kbest_spans(m, 16))
    _same_bits(got, kbest_numpy(_scores(m), [L] * B, 16, L))
    assert got['count'].tolist() == [14] * B
    assert np.array_equal(got['spans'][:, 0], m.cky_spans_device().cpu().numpy())


def test_module_entry_returns_trees_and_scores():
    """DioraBase.kbest(3) at L 7: per sentence [(tree, score)], the trees trees_from_spans builds from the device's spans."""
    r = _uniform(7)
    m = r['m']
    kb = _host(m.kbest_spans_device(3))
    got = m.kbest(3)
    assert len(got) == PC.GPU_B
    for b in range(PC.GPU_B):
        assert len(got[b]) == 3
        assert [str(t) for t, _ in got[b]] == [str(t) for t in m.trees_from_spans(kb['spans'][b])]
        assert [s for _, s in got[b]] == kb['scores'][b].tolist()
    assert [str(g[0][0]) for g in got] == [str(t) for t in m.cky()]


def test_parse_ragged_kbest_returns_the_callers_order():
    """Sentences of 3, 9 and 70 words (and a single word), two of each, shuffled: what kbest_spans gives on each pack's padded chart,
    back in the caller's order."""
    from cliora_amd import ragged
    from cliora_amd.harness import build_net
    from cliora_amd.kbest import kbest_spans
    torch.manual_seed(11)
    net = build_net(50, torch.nn.Embedding(97, 32), obj_feats=False).cuda()
    rs = np.random.RandomState(5)
    sents = [rs.randint(1, 97, size=n).tolist() for n in [9, 70, 3, 1, 3, 70, 9]]
    K = 4
    got = ragged.parse_ragged_kbest(net, sents, K, max_batch=3)
    want = [None] * len(sents)

    def per_pack(idx, lens):
        kb = _host(kbest_spans(net.diora, K, lens))
        assert kb['status'] == [0]
        for b, i in enumerate(idx):
            c = kb['count'][b]
            trees = net.diora.trees_from_spans(kb['spans'][b, :c, :len(sents[i]) - 1])
            want[i] = list(zip(trees, kb['scores'][b, :c].tolist()))

    ragged._run_packs(net, sents, 3, ragged.DEFAULT_MAX_WASTE, 0, per_pack, max_len=128)
    assert [len(g) for g in got] == [4, 4, 2, 1, 2, 4, 4]
    assert [[(str(t), s) for t, s in g] for g in got] == [[(str(t), s) for t, s in w] for w in want]
    assert got[3] == [(0, 0.0)]
    assert [g[0][0] for g in got] == ragged.parse_ragged(net, sents, max_batch=3, max_len=128)      # rank 0: the parser's own tree
    with pytest.raises(ValueError):
        ragged.parse_ragged_kbest(net, sents, 17)
    with pytest.raises(_chart_error()):
        ragged.parse_ragged_kbest(net, sents, 2, max_len=64)


def _chart_error():
    from cliora_amd._lib import ChartLibError
    return ChartLibError


def test_refusals():
    from cliora_amd import _lib
    from cliora_amd.kbest import kbest_spans
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    fresh = _lib.Plan(2, 5, 16)                                               # never ran a forward
    assert lib.cliora_kbest_spans(fresh.handle, p(0), None, 4, p(100), p(200), p(300), None, None, st) != 0
    assert 'before forward' in err()
    m = _uniform(3)['m']
    h, ws = m._plan.handle, C.c_void_p(m._wss[0].data_ptr())
    for K in (0, 17, -1):
        assert lib.cliora_kbest_spans(h, ws, None, K, p(100), p(200), p(300), None, None, st) != 0
        assert 'K outside 1..16' in err()
    for args in [(None, ws, None, 4, p(100), p(200), p(300)), (h, None, None, 4, p(100), p(200), p(300)),
                 (h, ws, None, 4, None, p(200), p(300)), (h, ws, None, 4, p(100), None, p(300)), (h, ws, None, 4, p(100), p(200), None)]:
        assert lib.cliora_kbest_spans(*(args + (None, None, st))) != 0
        assert 'NULL argument' in err()
    assert lib.cliora_kbest_spans(h, ws, p(400), 4, p(100), p(200), p(300), None, None, st) != 0
    assert 'without status' in err()
    long_m = _uniform(128)['m']
    assert _lib.fn('cliora_kbest_scratch_bytes')(long_m._plan.handle, 8) > 0
    assert lib.cliora_kbest_spans(long_m._plan.handle, C.c_void_p(long_m._wss[0].data_ptr()), None, 8, p(100), p(200), p(300), None, None,
                                  st) != 0
    assert 'NULL scratch' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                      # nothing was launched
    with pytest.raises(_lib.ChartLibError, match='K outside 1..16'):          # through the Python entry: the library's reason
        kbest_spans(m, 17)
    with pytest.raises(_lib.ChartLibError, match='K outside 1..16'):
        kbest_spans(m, 0)
    with pytest.raises(ValueError):
        kbest_spans(m, 4, torch.zeros(PC.GPU_B, dtype=torch.int64))
