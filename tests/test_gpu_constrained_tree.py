"""cliora_kbest_spans_constrained and cliora_sample_trees_constrained on the GPU (cliora_amd/constrained.py): the K best trees and
sampled trees among those that keep required brackets and hold no forbidden one.

The yardsticks, never the code under test: ``constrained_kbest_numpy`` and ``constrained_sample_numpy`` (pinned to enumeration of every
binary tree by test_constrained_tree_cpu.py) on the device's OWN per-split scores, read through cliora_inside_pair_states -- lists bit
for bit; draws bit for bit, a sample left out only where the restatement's margin is below sample_cases.MARGIN, at most one per test,
the count printed; log_prob within the project's bound -- and the entries they extend on the same chart: cliora_kbest_spans,
cliora_sample_trees and cliora_constrained_parse, bit for bit.  Cases and measured figures: constrained_tree_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import constrained_cases as CC
import constrained_tree_cases as TC
import posterior_cases as PC
import sample_cases as SC

pytestmark = pytest.mark.gpu

KS, LENGTHS = TC.KS, TC.LENGTHS
SEED = CC.GPU_SAMPLE_SEED
KB_KEYS, TS_KEYS = ('spans', 'scores', 'count', 'feasible'), ('spans', 'log_prob', 'log_z', 'log_z_c', 'feasible')


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


@functools.lru_cache(maxsize=None)
def _uniform(L, B=PC.GPU_B):
    """One eval forward of a text-only DioraMLP (D 16, random weights) at length L and the device's scores -- once per (L, B)."""
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, L, B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m))


def _t(a):
    """Host rows, lengths or ids -> an int32 tensor (None stays None)."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))


def _host(res, keys):
    out = {k: getattr(res, k).cpu().numpy() for k in keys}
    out['status'] = res.status.cpu().tolist()
    return out


def _kbest(m, brackets, K, lengths=None):
    from cliora_amd.constrained import constrained_kbest
    return _host(constrained_kbest(m, _t(brackets), K, _t(lengths)), KB_KEYS)


def _samples(m, brackets, S, lengths=None, ids=None, first_sample=0, beta=1.0, seed=SEED):
    from cliora_amd.constrained import constrained_samples
    return _host(constrained_samples(m, _t(brackets), S, seed, _t(lengths), _t(ids), first_sample, beta), TS_KEYS)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want, keys, what='', rows=None):
    for k in keys:
        a, b = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, k)


def _kbest_is_numpy(got, scores, lengths, brackets, K, L, what):
    """Spans, count and feasible equal, scores bit for bit, status the restatement's.  -> the restatement."""
    from cliora_amd.constrained import constrained_kbest_numpy
    want = constrained_kbest_numpy(scores, lengths, brackets, K, L=L)
    assert got['status'] == [want.status], what
    assert np.array_equal(got['count'], want.count) and np.array_equal(got['feasible'], want.feasible), (what, got['count'], want.count)
    assert got['spans'].dtype == np.int32 and got['spans'].shape == want.spans.shape and np.array_equal(got['spans'], want.spans), what
    assert np.array_equal(_bits(got['scores']), _bits(want.scores)), what
    return want


def _samples_are_numpy(got, scores, lengths, brackets, S, L, what, **kw):
    """Spans equal but for at most one sample of a margin below sample_cases.MARGIN; log_prob, log_z_c and log_z within the bound.
    -> the restatement."""
    from cliora_amd.constrained import constrained_sample_numpy
    want = constrained_sample_numpy(scores, lengths, brackets, S, SEED, L=L, **kw)
    assert got['status'] == [want.status], what
    assert np.array_equal(got['feasible'], want.feasible), what
    assert got['spans'].dtype == np.int32 and got['spans'].shape == want.spans.shape
    differ = (got['spans'] != want.spans).reshape(want.spans.shape[0], S, -1).any(axis=2)
    excused = differ & (want.margin < SC.MARGIN)
    assert not (differ & ~excused).any(), (what, np.argwhere(differ & ~excused).tolist(), want.margin[differ].tolist())
    assert excused.sum() <= SC.MAX_EXCUSED, what
    fin = np.isfinite(want.log_prob)
    assert np.array_equal(np.isneginf(got['log_prob']), ~fin) and np.array_equal(np.isneginf(got['log_z_c']), np.isneginf(want.log_z_c)), what
    keep = fin & ~excused
    e_lp = float(np.abs(got['log_prob'].astype(np.float64)[keep] - want.log_prob[keep]).max(initial=0.0))
    ok = np.isfinite(want.log_z_c)
    e_lzc = float(np.abs(got['log_z_c'].astype(np.float64)[ok] - want.log_z_c[ok]).max(initial=0.0))
    e_lz = float(np.abs(got['log_z'].astype(np.float64) - want.log_z).max())
    print('%s: max |log_prob - fp64| = %.3e, |log_z_c - fp64| = %.3e, |log_z - fp64| = %.3e, left out %d (smallest margin %.3e)'
          % (what, e_lp, e_lzc, e_lz, int(excused.sum()), float(want.margin.min())))
    assert e_lp <= CC.BOUND and e_lzc <= CC.BOUND and e_lz <= CC.BOUND, what
    return want


# ---- 1. the K best against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('L', LENGTHS)
def test_kbest_is_constrained_kbest_numpy_bit_for_bit(L, K):
    """L in {1, 2, 3, 6, 7, 13}, K in {1, 4, 16}.  At L 6 the counts saturate from the brackets and from K in one chart."""
    r, B = _uniform(L), PC.GPU_B
    for name, brackets in TC.cases(L, B).items():
        got = _kbest(r['m'], brackets, K)
        want = _kbest_is_numpy(got, r['scores'], [L] * B, brackets, K, L, 'L %d, K %d, %s' % (L, K, name))
        if name == 'one infeasible':
            assert want.feasible.tolist() == [1, 0, 1] and want.count[1] == 0
        if L == 6 and K == 16 and name == 'nested':                           # below K by the brackets, and at K
            assert 0 < want.count.min() < 16 and _kbest(r['m'], None, K)['count'].tolist() == [16] * B
        assert (got['scores'][:, :-1] >= got['scores'][:, 1:]).all()           # best first, -inf beyond count


@pytest.mark.parametrize('K', [1, 16])
@pytest.mark.parametrize('L', CC.LONG_LENGTHS)
def test_kbest_long_instance(L, K):
    """L 65 and 128 at B 2, two splits per lane: K 1 keeps its lists in LDS, K 16 in the caller's scratch (at L 128: 1 MiB a
    sentence).  Nested required brackets plus two forbidden spans."""
    from cliora_amd import _lib
    B = 2
    r = _uniform(L, B)
    brackets = CC.pack_rows(TC.nested(L, B, forbidden=[(1, 2), (L - 3, L - 1)]))
    need = _lib.fn('cliora_kbest_constrained_scratch_bytes')(r['m']._plan.handle, K, brackets.shape[1])
    assert need == (0 if K == 1 else B * (L * (L + 1) // 2) * K * 8)
    got = _kbest(r['m'], brackets, K)
    want = _kbest_is_numpy(got, r['scores'], [L] * B, brackets, K, L, 'L %d, K %d' % (L, K))
    assert want.count.tolist() == [K] * B


# ---- 2. the links to the entries they extend ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS + (65,))
def test_without_a_disallowed_cell_the_outputs_are_the_unconstrained_entries(L):
    """No bracket, unused rows, a required root and required leaves: cliora_kbest_spans' and cliora_sample_trees' bits."""
    from cliora_amd.kbest import kbest_spans
    from cliora_amd.sample import sample_spans
    B = PC.GPU_B if L < 65 else 2
    m = _uniform(L, B)['m']
    sets = {'M 0': None, 'unused rows': np.full((B, 3, 3), -1, dtype=np.int32),
            'root and leaves': CC.pack_rows([[(0, L - 1, 1), (0, 0, 1), (L - 1, L - 1, 1)]] * B)}
    for K in (1, 16):
        kb = kbest_spans(m, K)
        want = dict(spans=kb.spans.cpu().numpy(), scores=kb.scores.cpu().numpy(), count=kb.count.cpu().numpy())
        for name, brackets in sets.items():
            got = _kbest(m, brackets, K)
            assert got['status'] == [0] and got['feasible'].tolist() == [1] * B
            _same_bits(got, want, ('spans', 'scores', 'count'), (L, K, name))
    for beta in (1.0, 0.5):
        ts = sample_spans(m, 16, SEED, first_sample=5, beta=beta)
        want = dict(spans=ts.spans.cpu().numpy(), log_prob=ts.log_prob.cpu().numpy(), log_z=ts.log_z.cpu().numpy())
        for name, brackets in sets.items():
            got = _samples(m, brackets, 16, first_sample=5, beta=beta)
            assert got['status'] == [0] and got['feasible'].tolist() == [1] * B
            _same_bits(got, want, ('spans', 'log_prob', 'log_z'), (L, beta, name))
            assert np.array_equal(_bits(got['log_z_c']), _bits(got['log_z']))


@pytest.mark.parametrize('L,B', [(L, PC.GPU_B) for L in LENGTHS] + [(L, 2) for L in CC.LONG_LENGTHS])
def test_rank_0_and_the_log_partitions_are_constrained_parse_bit_for_bit(L, B):
    from cliora_amd.constrained import constrained_parse
    m = _uniform(L, B)['m']
    for name, brackets in TC.cases(L, B).items():
        cp = constrained_parse(m, _t(brackets))
        for K in (1, 16):
            got = _kbest(m, brackets, K)
            assert np.array_equal(got['feasible'], cp.feasible.cpu().numpy()), (L, name)
            assert np.array_equal(got['spans'][:, 0], cp.spans.cpu().numpy()), (L, K, name)
            assert np.array_equal(_bits(got['scores'][:, 0]), _bits(cp.score.cpu().numpy())), (L, K, name)
        ts = _samples(m, brackets, 2)
        assert np.array_equal(ts['feasible'], cp.feasible.cpu().numpy()), (L, name)
        assert np.array_equal(_bits(ts['log_z_c']), _bits(cp.log_z_c.cpu().numpy())), (L, name)
        assert np.array_equal(_bits(ts['log_z']), _bits(cp.log_z.cpu().numpy())), (L, name)


# ---- 3. the draws against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', LENGTHS)
def test_samples_are_constrained_sample_numpy(L):
    """L in {1, 2, 3, 6, 7, 13}, S 64, beta 1 and (L 13) 0.5."""
    r, B = _uniform(L), PC.GPU_B
    for name, brackets in TC.cases(L, B).items():
        for beta in ((1.0, 0.5) if L == 13 else (1.0,)):
            got = _samples(r['m'], brackets, SC.GPU_S, beta=beta)
            want = _samples_are_numpy(got, r['scores'], [L] * B, brackets, SC.GPU_S, L, 'L %d, %s, beta %g' % (L, name, beta), beta=beta)
            if L >= 6 and name != 'one infeasible':
                assert want.feasible.all() and (want.log_z_c < want.log_z).all()                  # the set binds


@pytest.mark.parametrize('L,S', SC.GPU_LONG)
def test_samples_long_instance(L, S):
    """L 65 / S 16 and L 128 / S 8 at B 2: two splits per lane, both fp64 tables resident; M padded to 256 at L 128, the most LDS a
    call takes."""
    B = 2
    r = _uniform(L, B)
    brackets = CC.pack_rows(TC.nested(L, B, forbidden=[(1, 2), (L - 3, L - 1)]), 256 if L == 128 else None)
    got = _samples(r['m'], brackets, S)
    _samples_are_numpy(got, r['scores'], [L] * B, brackets, S, L, 'L %d, S %d' % (L, S))


@pytest.mark.parametrize('L,B', [(13, PC.GPU_B), (128, 2)])
def test_every_drawn_tree_keeps_the_brackets(L, B):
    """S 256: each draw holds every required span, none of the forbidden ones, n - 1 spans with the root last; and its log_prob is
    at most 0."""
    m = _uniform(L, B)['m']
    sets = TC.nested(L, B, forbidden=[(1, 2), (4, 5), (L - 3, L - 1)])
    got = _samples(m, CC.pack_rows(sets), 256)
    assert got['status'] == [0] and got['feasible'].tolist() == [1] * B
    for b, rows in enumerate(sets):
        for s in range(256):
            tree = set(CC.span_key(got['spans'][b, s].tolist()))
            assert len(tree) == L - 1 and tuple(got['spans'][b, s, -1]) == (0, L - 1)
            assert all(((s0, e0) in tree or s0 == e0) == bool(kind) for s0, e0, kind in rows), (b, s)
    assert (got['log_prob'] <= 0).all()
    assert len(set(CC.span_key(r) for r in got['spans'][0].tolist())) > 1      # not one tree over and over


# ---- 4. infeasible sentences and bad input ------------------------------------------------------------------------------------------
def test_infeasible_sentences_are_no_error():
    """L 7: a crossing required pair, a span both required and forbidden, a forbidden leaf, a forbidden root."""
    L, B = 7, PC.GPU_B
    r = _uniform(L)
    m = r['m']
    log_z = m.span_posteriors().log_z.cpu().numpy()
    first = [(s, e, 1) for s, e in CC.nested_required(L, 0)]
    clean_kb, clean_ts = _kbest(m, CC.pack_rows([first, [], []], 2), 4), _samples(m, CC.pack_rows([first, [], []], 2), 8)
    for pair in ([[(1, 4, 1), (3, 5, 1)], [(2, 4, 1), (2, 4, 0)]], [[(3, 3, 0)], [(0, L - 1, 0)]]):
        brackets = CC.pack_rows([first] + pair, 2)
        kb, ts = _kbest(m, brackets, 4), _samples(m, brackets, 8)
        assert kb['status'] == [0] and ts['status'] == [0]
        assert kb['feasible'].tolist() == [1, 0, 0] and ts['feasible'].tolist() == [1, 0, 0]
        for b in (1, 2):
            assert kb['count'][b] == 0 and (kb['spans'][b] == -1).all() and np.isneginf(kb['scores'][b]).all()
            assert (ts['spans'][b] == -1).all() and np.isneginf(ts['log_prob'][b]).all() and np.isneginf(ts['log_z_c'][b])
        assert np.array_equal(_bits(ts['log_z']), _bits(log_z))                # still the real value
        _same_bits(kb, clean_kb, KB_KEYS, 'neighbour', rows=[0])
        _same_bits(ts, clean_ts, TS_KEYS, 'neighbour', rows=[0])
        _kbest_is_numpy(kb, r['scores'], [L] * B, brackets, 4, L, 'infeasible')
        _samples_are_numpy(ts, r['scores'], [L] * B, brackets, 8, L, 'infeasible')


def _padded(lengths, L, seed0):
    xs = [PC.sentence(PC.GPU_D, n, seed0 + b) for b, n in enumerate(lengths)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, L).cuda())
    return m, xs


def test_padded_chart_of_four_with_an_infeasible_sentence_a_bad_row_and_a_bad_length():
    """L 14, lengths [9, 14, 15, 5]: sentence 0 infeasible (not counted), sentence 1 with a row that ends past its last word
    (counted), sentence 2 with a bad length (counted); sentence 3 as in its own call on the same chart bit for bit, and as in a chart
    of its own length: the same trees, the sums within the bound (another forward)."""
    L, lengths = 14, [9, 14, 15, 5]
    m, xs = _padded([9, 14, 14, 5], L, 4100)
    sets = [[(0, 4, 1), (3, 7, 1)], [(2, 5, 1), (3, 14, 1)], [(0, 1, 1)], [(1, 3, 1), (0, 1, 0)]]
    brackets = CC.pack_rows(sets)
    kb, ts = _kbest(m, brackets, 16, lengths), _samples(m, brackets, 16, lengths, ids=[7, 8, 9, 10])
    assert kb['status'] == [2] and ts['status'] == [2]
    assert kb['feasible'].tolist() == [0, 0, 0, 1] and ts['feasible'].tolist() == [0, 0, 0, 1]
    for b in (0, 1, 2):
        assert kb['count'][b] == 0 and (kb['spans'][b] == -1).all() and np.isneginf(kb['scores'][b]).all()
        assert (ts['spans'][b] == -1).all() and np.isneginf(ts['log_prob'][b]).all() and np.isneginf(ts['log_z_c'][b])
    assert ts['log_z'][0] != 0 and ts['log_z'][1] == 0 and ts['log_z'][2] == 0
    scores = _scores(m)
    _kbest_is_numpy(kb, scores, lengths, brackets, 16, L, 'padded L 14')
    _samples_are_numpy(ts, scores, lengths, brackets, 16, L, 'padded L 14', ids=[7, 8, 9, 10])
    # the fourth sentence: the same chart with only its own brackets gives the same bits
    alone = CC.pack_rows([[], [], [], sets[3]], brackets.shape[1])
    _same_bits(_kbest(m, alone, 16, [9, 14, 14, 5]), kb, KB_KEYS, 'own call', rows=[3])
    _same_bits(_samples(m, alone, 16, [9, 14, 14, 5], ids=[7, 8, 9, 10]), ts, TS_KEYS, 'own call', rows=[3])
    # and a chart of its own length gives the same trees
    one = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    one.outside = False
    _forward(one, xs[3][None].cuda())
    kb1, ts1 = _kbest(one, brackets[3:4], 16), _samples(one, brackets[3:4], 16, ids=[10])
    assert kb1['count'][0] == kb['count'][3] and np.array_equal(kb1['spans'][0], kb['spans'][3, :, :4])
    assert np.array_equal(ts1['spans'][0], ts['spans'][3, :, :4])
    cnt = kb1['count'][0]
    assert (np.abs(kb1['scores'][0, :cnt] - kb['scores'][3, :cnt]) <= CC.BOUND * np.maximum(1.0, np.abs(kb1['scores'][0, :cnt]))).all()
    assert (np.abs(ts1['log_prob'][0] - ts['log_prob'][3]) <= CC.BOUND * np.maximum(1.0, np.abs(ts1['log_prob'][0]))).all()


# ---- 5. invariances -------------------------------------------------------------------------------------------------------------------
def test_every_length_equal_to_L_is_the_call_without_lengths():
    L, B = 13, PC.GPU_B
    m = _uniform(L)['m']
    brackets = CC.pack_rows(TC.nested(L, B, forbidden=[(1, 2)]))
    kb = _kbest(m, brackets, 8, [L] * B)
    assert kb['status'] == [0]
    _same_bits(kb, _kbest(m, brackets, 8), KB_KEYS, 'lengths == L')
    _same_bits(_samples(m, brackets, 16, [L] * B), _samples(m, brackets, 16), TS_KEYS, 'lengths == L')


def test_chunks_of_S_are_one_call_and_two_calls_give_equal_bits():
    L, B, S = 13, PC.GPU_B, 24
    m = _uniform(L)['m']
    brackets = CC.pack_rows(TC.nested(L, B, forbidden=[(1, 2), (3, 5)]))
    whole = _samples(m, brackets, S, first_sample=3)
    _same_bits(_samples(m, brackets, S, first_sample=3), whole, TS_KEYS, 'two calls')
    a, b = _samples(m, brackets, 10, first_sample=3), _samples(m, brackets, S - 10, first_sample=13)
    assert np.array_equal(np.concatenate([a['spans'], b['spans']], axis=1), whole['spans'])
    assert np.array_equal(_bits(np.concatenate([a['log_prob'], b['log_prob']], axis=1)), _bits(whole['log_prob']))
    for K in (4, 16):
        _same_bits(_kbest(m, brackets, K), _kbest(m, brackets, K), KB_KEYS, 'two calls')
    long = _uniform(65, 2)['m']
    lb = CC.pack_rows(TC.nested(65, 2, forbidden=[(1, 2)]))
    _same_bits(_kbest(long, lb, 16), _kbest(long, lb, 16), KB_KEYS, 'two calls, scratch')
    _same_bits(_samples(long, lb, 8), _samples(long, lb, 8), TS_KEYS, 'two calls, long')


def test_permuting_sentences_with_their_ids_and_brackets_permutes_the_rows():
    L, B = 7, PC.GPU_B
    x = PC.batch(PC.GPU_D, L, B, PC.GPU_SEED + L)
    brackets = CC.pack_rows(TC.nested(L, B, forbidden=[(4, 5)]))
    perm = [2, 0, 1]
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, x.cuda())
    kb, ts = _kbest(m, brackets, 8), _samples(m, brackets, 16, ids=[0, 1, 2])
    _same_bits(ts, _samples(m, brackets, 16), TS_KEYS, 'ids = rows')
    _forward(m, x[perm].cuda())
    kbp, tsp = _kbest(m, brackets[perm], 8), _samples(m, brackets[perm], 16, ids=perm)
    for keys, got, want in ((KB_KEYS, kbp, kb), (TS_KEYS, tsp, ts)):
        for k in keys:
            assert np.array_equal(_bits(got[k]), _bits(want[k][perm])), k


def test_outputs_and_scratch_filled_with_nan_change_nothing():
    """Poisoned outputs (0x7f bytes: NaN floats, large ints) and scratch before the call: every element is written, nothing is read."""
    from cliora_amd import _lib
    L, B, K, S = 65, 2, 16, 8
    m = _uniform(L, B)['m']
    brackets = CC.pack_rows(TC.nested(L, B, forbidden=[(1, 2)]))
    want_kb, want_ts = _kbest(m, brackets, K), _samples(m, brackets, S)
    plan, ws = m._plan, m._wss[0]
    bt = torch.from_numpy(brackets).cuda()
    Mr = brackets.shape[1]
    fill = lambda *shape: torch.full(shape, 0x7f, dtype=torch.uint8, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = _lib.fn('cliora_kbest_constrained_scratch_bytes')(plan.handle, K, Mr)
    assert need > 0
    spans, scores, count, feas, status = fill(B, K, L - 1, 2, 4), fill(B, K, 4), fill(B, 4), fill(B, 4), fill(4)
    _lib.call('cliora_kbest_spans_constrained', plan.handle, p(ws), None, p(bt), Mr, K, p(spans), p(scores), p(count), p(feas),
              p(fill(need)), p(status), st)
    got = dict(spans=spans.view(torch.int32).reshape(B, K, L - 1, 2), scores=scores.view(torch.float32).reshape(B, K),
               count=count.view(torch.int32).reshape(B), feasible=feas.view(torch.int32).reshape(B))
    assert status.view(torch.int32).item() == 0
    _same_bits({k: v.cpu().numpy() for k, v in got.items()}, want_kb, KB_KEYS, 'poisoned k-best')
    spans, lp, lzc, lz, feas, status = fill(B, S, L - 1, 2, 4), fill(B, S, 4), fill(B, 4), fill(B, 4), fill(B, 4), fill(4)
    _lib.call('cliora_sample_trees_constrained', plan.handle, p(ws), None, None, p(bt), Mr, S, SEED, 0, 1.0, p(spans), p(lp), p(lzc),
              p(lz), p(feas), p(status), st)
    got = dict(spans=spans.view(torch.int32).reshape(B, S, L - 1, 2), log_prob=lp.view(torch.float32).reshape(B, S),
               log_z_c=lzc.view(torch.float32).reshape(B), log_z=lz.view(torch.float32).reshape(B), feasible=feas.view(torch.int32).reshape(B))
    assert status.view(torch.int32).item() == 0
    _same_bits({k: v.cpu().numpy() for k, v in got.items()}, want_ts, TS_KEYS, 'poisoned samples')


# ---- 6. plans -----------------------------------------------------------------------------------------------------------------------
def test_treelstm_plan():
    """A TreeLSTM plan (L 5): the same score rows, the same results."""
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
    brackets = CC.pack_rows([[(1, 3, 1)], [(0, 2, 1), (3, 4, 0)], [(2, 3, 0), (0, 1, 0)]])
    scores = _scores(m)
    _kbest_is_numpy(_kbest(m, brackets, 16), scores, [L] * B, brackets, 16, L, 'TreeLSTM L 5')
    _samples_are_numpy(_samples(m, brackets, 32), scores, [L] * B, brackets, 32, L, 'TreeLSTM L 5')


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from cliora_amd import _lib
    from cliora_amd.constrained import constrained_kbest, constrained_samples
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    # (plan, ws, lengths, brackets, M, K, spans, scores, count, feasible, scratch, status)
    kcall = lambda *a: lib.cliora_kbest_spans_constrained(*(a + (st,)))
    kgood = lambda h, ws: [h, ws, None, p(0), 2, 4, p(100), p(2000), p(2100), p(2200), None, p(2300)]
    # (plan, ws, lengths, ids, brackets, M, S, seed, first_sample, beta, spans, log_prob, log_zc, log_z, feasible, status)
    scall = lambda *a: lib.cliora_sample_trees_constrained(*(a + (st,)))
    sgood = lambda h, ws: [h, ws, None, None, p(0), 2, 4, 1, 0, 1.0, p(100), p(2000), p(2100), p(2200), p(2300), p(2400)]
    fresh = _lib.Plan(2, 5, 16)                                               # never ran a forward
    assert kcall(*kgood(fresh.handle, p(4000))) != 0
    assert 'kbest_spans_constrained called before forward' in err()
    assert scall(*sgood(fresh.handle, p(4000))) != 0
    assert 'sample_trees_constrained called before forward' in err()
    m = _uniform(3)['m']
    h, ws = m._plan.handle, C.c_void_p(m._wss[0].data_ptr())

    def refused(call, good, changes, message):
        a = good(h, ws)
        for i, v in changes.items():
            a[i] = v
        assert call(*a) != 0, (changes, message)
        assert message in err(), (changes, err())

    for K in (0, 17):
        refused(kcall, kgood, {5: K}, 'cliora_kbest_spans_constrained: K outside 1..16')
    for M in (-1, 257):
        refused(kcall, kgood, {4: M}, 'cliora_kbest_spans_constrained: M outside 0..256')
        refused(scall, sgood, {5: M}, 'cliora_sample_trees_constrained: M outside 0..256')
    for S in (0, (1 << 20) + 1):
        refused(scall, sgood, {6: S}, 'cliora_sample_trees_constrained: S outside 1..1048576')
    for beta in (-0.5, float('nan'), float('inf')):
        refused(scall, sgood, {9: beta}, 'cliora_sample_trees_constrained: beta negative or not finite')
    for i in (0, 1, 7, 8, 9, 11):                                             # plan, workspace, scores, count, feasible, status
        refused(kcall, kgood, {i: None}, 'cliora_kbest_spans_constrained: NULL argument')
    for i in (0, 1, 11, 12, 13, 14, 15):                                      # plan, workspace, the three sums, feasible, status
        refused(scall, sgood, {i: None}, 'cliora_sample_trees_constrained: NULL argument')
    refused(kcall, kgood, {6: None}, 'cliora_kbest_spans_constrained: NULL spans_out')
    refused(scall, sgood, {10: None}, 'cliora_sample_trees_constrained: NULL spans_out')
    refused(kcall, kgood, {3: None}, 'cliora_kbest_spans_constrained: NULL brackets')
    refused(scall, sgood, {4: None}, 'cliora_sample_trees_constrained: NULL brackets')
    long = _uniform(128, 2)['m']                                              # K 16 at L 128 asks for scratch
    assert _lib.fn('cliora_kbest_constrained_scratch_bytes')(long._plan.handle, 16, 2) > 0
    a = kgood(long._plan.handle, C.c_void_p(long._wss[0].data_ptr()))
    a[5] = 16
    assert kcall(*a) != 0
    assert 'cliora_kbest_spans_constrained: NULL scratch' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                      # nothing was launched
    for call, good, bi in ((kcall, kgood, 3), (scall, sgood, 4)):             # M = 0 with NULL brackets is a call
        a = good(h, ws)
        a[bi], a[bi + 1] = None, 0
        assert call(*a) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.ChartLibError, match='K outside 1..16'):           # through the Python entries: the library's reasons
        constrained_kbest(m, None, 17)
    with pytest.raises(_lib.ChartLibError, match='M outside 0..256'):
        constrained_samples(m, torch.full((PC.GPU_B, 257, 3), -1, dtype=torch.int32), 4, 1)
    with pytest.raises(ValueError):
        constrained_kbest(m, torch.full((PC.GPU_B, 2, 3), -1, dtype=torch.int64), 4)
    with pytest.raises(ValueError):
        constrained_samples(m, None, 4, 1, ids=torch.zeros(PC.GPU_B + 1, dtype=torch.int32))


# ---- 8. the module and ragged entries -----------------------------------------------------------------------------------------------
def test_module_entries_return_trees():
    from cliora_amd import _lib
    L = 7
    m = _uniform(L)['m']
    required, forbidden = [[(1, 3), (1, 2)], [(0, 3), (2, 5)], []], [[(4, 5)], [], [(0, 5), (1, 6)]]
    kb = m.kbest_constrained(4, required, forbidden)
    ts = m.sample_trees_constrained(8, 11, required, forbidden)
    assert kb[1] == [] and ts[1] == [] and len(kb[0]) == 4 and len(ts[0]) == 8 and len(ts[2]) == 8
    best = m.cky_constrained(required, forbidden)
    for b in (0, 2):
        assert str(kb[b][0][0]) == str(best[b]) and kb[b][0][1] >= kb[b][-1][1]
        listed = {str(t): s for t, s in m.kbest_constrained(16, required, forbidden)[b]}
        assert all(str(t) in listed or len(listed) == 16 for t, _ in ts[b]) and all(lp <= 0 for _, lp in ts[b])
    assert [[(str(t), s) for t, s in row] for row in m.kbest_constrained(4, [[], [], []])] == \
           [[(str(t), s) for t, s in row] for row in m.kbest(4)]
    assert [[(str(t), s) for t, s in row] for row in m.sample_trees_constrained(8, 11, [[], [], []])] == \
           [[(str(t), s) for t, s in row] for row in m.sample_trees(8, 11)]
    with pytest.raises(_lib.ChartLibError, match='cliora_kbest_spans_constrained rejected 1 sentence'):
        m.kbest_constrained(4, [[(0, L)], [], []])
    with pytest.raises(_lib.ChartLibError, match='cliora_sample_trees_constrained rejected 2 sentence'):
        m.sample_trees_constrained(4, 1, [[(0, L)], [], [(3, 2)]])


def test_ragged_entries_keep_the_callers_order_and_a_sentences_draws():
    """Sentences of 9, 70, 3, 1, 3, 12 and 9 words (lengths on both sides of 64), one of them infeasible: max_batch 3 against
    max_batch 2 -- other packs, the same trees and draws, in the caller's order -- and against the per-pack device entries."""
    from cliora_amd import _lib, ragged
    from cliora_amd.harness import build_net
    torch.manual_seed(11)
    net = build_net(50, torch.nn.Embedding(97, 32), obj_feats=False).cuda()
    rs = np.random.RandomState(5)
    lens = [9, 70, 3, 1, 3, 12, 9]
    sents = [rs.randint(1, 97, size=n).tolist() for n in lens]
    required = [CC.nested_required(n, i) if n >= 3 else [] for i, n in enumerate(lens)]
    required[5] = [(0, 5), (3, 8)]                                            # crossing
    forbidden = [[(n - 2, n - 1)] if n >= 5 else [] for n in lens]
    kb = ragged.parse_ragged_kbest_constrained(net, sents, 4, required, forbidden, max_batch=3)
    ts = ragged.parse_ragged_samples_constrained(net, sents, 6, 21, required, forbidden, max_batch=3)
    best = ragged.parse_ragged_constrained(net, sents, required, forbidden, max_batch=3)
    assert kb[3] == [(0, 0.0)] and ts[3] == [(0, 0.0)] * 6 and kb[5] == [] and ts[5] == []
    for i, n in enumerate(lens):
        if i in (3, 5):
            continue
        assert str(kb[i][0][0]) == str(best[i][0]) and len(ts[i]) == 6 and 1 <= len(kb[i]) <= 4
        for tree, _ in kb[i] + ts[i]:                                         # every tree keeps the sentence's brackets
            spans = _tree_spans(tree)
            assert all(tuple(s) in spans for s in required[i]) and not any(tuple(s) in spans for s in forbidden[i]), i
    kb2 = ragged.parse_ragged_kbest_constrained(net, sents, 4, required, forbidden, max_batch=2)
    ts2 = ragged.parse_ragged_samples_constrained(net, sents, 6, 21, required, forbidden, max_batch=2)
    assert [[str(t) for t, _ in row] for row in kb2] == [[str(t) for t, _ in row] for row in kb]
    assert [[str(t) for t, _ in row] for row in ts2] == [[str(t) for t, _ in row] for row in ts]      # the same draws in another pack
    for a, b in zip(kb2 + ts2, kb + ts):
        for (_, p), (_, q) in zip(a, b):
            assert p == q or abs(p - q) <= CC.BOUND * max(1.0, abs(q))
    with pytest.raises(_lib.ChartLibError, match='rejected 1 sentence'):
        ragged.parse_ragged_kbest_constrained(net, sents, 4, [[(0, 9)]] + [[]] * 6)
    with pytest.raises(ValueError):
        ragged.parse_ragged_samples_constrained(net, sents, 0, 1, required)
    with pytest.raises(_lib.ChartLibError):
        ragged.parse_ragged_samples_constrained(net, sents, 2, 1, required, max_len=64)


def _tree_spans(tree):
    """Nested tuples of word positions -> the set of its constituents (start, end), leaves excluded."""
    out = set()

    def walk(t):
        if not isinstance(t, tuple):
            return t, t
        (ls, _), (_, re) = walk(t[0]), walk(t[1])
        out.add((ls, re))
        return ls, re
    walk(tree)
    return out


def test_oracle_f1_given_brackets_is_at_least_oracle_f1():
    """L 13, K 8, the gold phrases = the brackets: four spans of a tree drawn uniformly per sentence.  Every tree that keeps them
    holds all four among its eleven spans, F1 = 2 * 4 / (11 + 4), which no tree can exceed: at least what the k best trees reach."""
    from cliora_amd.evaluate import oracle_f1, oracle_f1_given_brackets
    from cliora_amd.kbest import kbest_spans
    from cliora_amd.sample import sample_spans
    L, B, K = 13, PC.GPU_B, 8
    m = _uniform(L)['m']
    drawn = sample_spans(m, 1, 99, beta=0.0).spans.cpu().numpy()[:, 0]        # uniform draws: far from the model's best trees
    gold = [[tuple(r) for r in drawn[b].tolist()[:-1]][-4:] for b in range(B)]
    entity_labels = [[('np', s, e - s + 1) for s, e in g] + [None] for g in gold]
    given = oracle_f1_given_brackets(m, entity_labels, gold, K)
    kb = kbest_spans(m, K)
    free = oracle_f1(kb.spans, kb.count, gold)
    print('oracle F1 at K %d: %.4f given the phrases, %.4f without' % (K, given['oracle_sent_f1'], free['oracle_sent_f1']))
    assert all(g >= f for g, f in zip(given['best_f1'], free['best_f1']))
    assert given['oracle_sent_f1'] >= free['oracle_sent_f1'] and given['sent_f1'] >= free['sent_f1']
    assert all(abs(f - 8.0 / 15) <= 1e-6 for f in given['best_f1'])    # SpanF1's sentence figure carries 1e-8 in its denominators
