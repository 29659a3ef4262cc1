"""The bracket loss on the GPU (cliora_amd/structured.py): cliora_bracket_grad alone, cliora_chart_backward_split, and the loss
through the chart's autograd node.

The yardsticks, never the code under test: ``bracket_grad_numpy`` (pinned to central differences and to enumeration by
test_structured_cpu.py) on the device's OWN per-split scores for the kernel; cliora_constrained_parse for log_prob (bitwise); the fp64
oracle with a torch restatement of the two inside recurrences, differentiated by autograd, for the gradients through the chart.
Cases, bounds and measured figures: structured_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import constrained_cases as CC
import posterior_cases as PC
import structured_cases as SC
from test_gpu_constrained import _forward, _scores

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _chart(B, L, D):
    """One eval forward of a text-only DioraMLP (random weights) and the device's scores -- once per shape."""
    m = PC.text_module(PC.params(D, PC.GPU_SEED), D).cuda().eval()
    _forward(m, PC.batch(D, L, B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m) if L > 1 else {})


def _tensor(rows):
    return None if rows is None else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32))


def _grad(m, rows=None, weights=None, lengths=None):
    """structured.bracket_grad with host inputs -> dict: G {level: (B, L - level, level)} numpy, flat, log_prob, feasible, status."""
    from cliora_amd.structured import bracket_grad, split_rows_by_level
    wt = None if weights is None else torch.tensor(weights, dtype=torch.float32)
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    res = bracket_grad(m, _tensor(rows), wt, lt)
    G = {lv: g.cpu().numpy() for lv, g in split_rows_by_level(m._plan, res.d_split).items()}
    return dict(G=G, flat=res.d_split.cpu().numpy(), log_prob=res.log_prob.cpu().numpy(), feasible=res.feasible.cpu().numpy(),
                status=res.status.cpu().tolist())


def _log_prob_of_the_parser(m, rows, lengths=None):
    from cliora_amd.constrained import constrained_parse
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    cp = constrained_parse(m, _tensor(rows), lt)
    return cp.log_prob.cpu().numpy(), cp.feasible.cpu().numpy()


def _sets(m, B, L):
    """name -> per-sentence rows: single required, nested required, required plus forbidden, the CKY tree, a sampled tree."""
    single = [[(b % (L - 1), b % (L - 1) + 1, 1)] if L == 3 else [(1 + b % 2, L - 2, 1)] for b in range(B)]
    nested = [[(s, e, 1) for s, e in CC.nested_required(L, b)] for b in range(B)]
    forb = (L // 2, L // 2 + 1)
    mixed = [rows + [forb + (0,)] for rows in nested]
    cky = m.cky_spans_device().cpu().numpy()
    sampled = m.sample_spans_device(1, CC.GPU_SAMPLE_SEED).spans.cpu().numpy()[:, 0]
    return {'single': single, 'nested': nested, 'required+forbidden': mixed,
            'cky tree': [SC.spans_as_required(cky[b], L) for b in range(B)],
            'sampled tree': [SC.spans_as_required(sampled[b], L) for b in range(B)]}


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', SC.GPU_SHAPES)
def test_kernel_against_the_fp64_restatement(B, L, D):
    from cliora_amd.structured import bracket_grad_numpy
    c = _chart(B, L, D)
    m, scores = c['m'], c['scores']
    worst, moved = 0.0, 0
    for name, sets in _sets(m, B, L).items():
        rows = CC.pack_rows(sets)
        got = _grad(m, rows)
        want = bracket_grad_numpy(scores, [L] * B, rows)
        lp, feas = _log_prob_of_the_parser(m, rows)
        assert got['status'] == [0], name
        assert np.array_equal(_bits(got['log_prob']), _bits(lp)), (name, got['log_prob'], lp)
        assert np.array_equal(got['feasible'], feas), name
        for level in range(1, L):
            err = float(np.abs(got['G'][level].astype(np.float64) - want[level]).max())
            worst = max(worst, err)
            assert err <= SC.BOUND, (name, level, err)
            assert float(np.abs(got['G'][level].astype(np.float64).sum(axis=2)).max()) <= 1e-6, (name, level)
            for b in range(B):
                if not feas[b]:
                    assert not got['G'][level][b].any(), (name, b)
        moved += int(any(np.abs(got['G'][level]).max() > 1e-3 for level in range(1, L)))
    print('L %d: max |G - fp64| = %.3e (measured before: %s)' % (L, worst, SC.MEASURED.get('L %d' % L)))
    assert moved >= 3                                  # gradients, not zeros


def test_two_words_and_no_brackets_give_zeros():
    m = _chart(3, 2, 16)['m']                          # one cell, one split
    got = _grad(m, CC.pack_rows([[(0, 1, 1)], [(0, 0, 0)], [(1, 1, 1)]]))
    assert not got['flat'].any() and got['flat'].size == 3
    assert got['feasible'].tolist() == [1, 0, 1] and got['log_prob'].tolist() == [0.0, -np.inf, 0.0] and got['status'] == [0]
    B, L = 3, 7
    m = _chart(B, L, 16)['m']
    for rows in (None, np.full((B, 4, 3), -1, dtype=np.int32), CC.pack_rows([[(0, L - 1, 1)], [(2, 2, 1)], []])):
        got = _grad(m, rows, weights=[3.0, -2.0, 0.5])
        assert not got['flat'].any() and got['log_prob'].tolist() == [0.0] * B and got['feasible'].tolist() == [1] * B


def test_weights_scale_and_two_calls_give_equal_bits():
    B, L = 2, 13
    m = _chart(B, L, 48)['m']
    rows = CC.pack_rows(_sets(m, B, L)['required+forbidden'])
    a, b = _grad(m, rows), _grad(m, rows)
    assert a['flat'].any() and np.array_equal(_bits(a['flat']), _bits(b['flat'])) and np.array_equal(_bits(a['log_prob']), _bits(b['log_prob']))
    w = _grad(m, rows, weights=[2.0, -0.25])           # powers of two: the scaled fp64 value rounds to the scaled fp32 value
    for level in range(1, L):
        assert np.array_equal(w['G'][level][0], 2.0 * a['G'][level][0]) and np.array_equal(w['G'][level][1], -0.25 * a['G'][level][1])
    assert np.array_equal(_bits(w['log_prob']), _bits(a['log_prob']))


# ---- 2. padded charts -------------------------------------------------------------------------------------------------------------
RAGGED_L, RAGGED_LENGTHS = 7, (7, 3, 1, 5)


@functools.lru_cache(maxsize=None)
def _padded():
    xs = [PC.sentence(PC.GPU_D, n, 4100 + b) for b, n in enumerate(RAGGED_LENGTHS)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, RAGGED_L).cuda())
    sets = [[(1, 4, 1), (2, 3, 1), (5, 6, 0)], [(1, 2, 1)], [], [(0, 2, 1), (3, 4, 0)]]
    return m, xs, sets


def test_padded_chart_is_each_sentence_alone():
    """lengths (7, 3, 1, 5) at L 7: each sentence's rows are bitwise those of the sentence run alone at its own L (the kernel's
    arithmetic depends on the sentence's words alone), and every element beyond a triangle is zero."""
    from cliora_amd.structured import bracket_grad_numpy
    m, xs, sets = _padded()
    L, lengths = RAGGED_L, list(RAGGED_LENGTHS)
    rows = CC.pack_rows(sets)
    got = _grad(m, rows, lengths=lengths)
    lp, feas = _log_prob_of_the_parser(m, rows, lengths)
    assert got['status'] == [0] and np.array_equal(_bits(got['log_prob']), _bits(lp)) and np.array_equal(got['feasible'], feas)
    want = bracket_grad_numpy(_scores(m), lengths, rows)
    for level in range(1, L):
        assert float(np.abs(got['G'][level] - want[level]).max()) <= SC.BOUND
    alone = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    alone.outside = False
    for b, n in enumerate(lengths):
        for level in range(1, L):
            assert not got['G'][level][b, max(0, n - level):].any(), (b, level)          # beyond the triangle
        if n < 2:
            continue
        _forward(alone, xs[b][None].cuda())
        one = _grad(alone, rows[b:b + 1])
        assert one['status'] == [0] and np.array_equal(_bits(one['log_prob']), _bits(got['log_prob'][b:b + 1]))
        for level in range(1, n):
            assert np.array_equal(_bits(one['G'][level][0]), _bits(got['G'][level][b, :n - level])), (b, level)
    assert any(got['G'][level][0].any() for level in range(1, L)) and any(got['G'][level][3].any() for level in range(1, L))


def test_every_length_equal_to_L_is_the_call_without_lengths():
    B, L = 2, 13
    m = _chart(B, L, 48)['m']
    rows = CC.pack_rows(_sets(m, B, L)['nested'])
    a, b = _grad(m, rows, lengths=[L] * B), _grad(m, rows)
    assert a['status'] == [0] and a['flat'].any()
    for k in ('flat', 'log_prob', 'feasible'):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_bad_rows_lengths_and_infeasible_sets_leave_their_neighbours_alone():
    m, _, sets = _padded()
    L, lengths = RAGGED_L, list(RAGGED_LENGTHS)
    clean = _grad(m, CC.pack_rows(sets, 4), lengths=lengths)
    bad_sets = [list(s) for s in sets]
    bad_sets[1] = [(1, 2, 1), (1, 3, 1), (2, 2, 7)]                # two bad rows in one sentence (an end in the padding, a bad kind): one count
    bad_sets[3] = [(0, 2, 1), (1, 3, 1)]                           # crossing required brackets: infeasible, not counted
    bad_lengths = list(lengths)
    bad_lengths[2] = 0                                             # a bad length
    got = _grad(m, CC.pack_rows(bad_sets, 4), weights=[1.0, float('nan'), float('nan'), float('nan')], lengths=bad_lengths)
    assert got['status'] == [2]
    assert got['feasible'].tolist() == [1, 0, 0, 0] and np.isneginf(got['log_prob'][1:]).all()
    for level in range(1, L):
        assert not got['G'][level][1:].any()                       # zeros, whatever the weight
        assert np.array_equal(_bits(got['G'][level][0]), _bits(clean['G'][level][0]))
    assert got['log_prob'][0] == clean['log_prob'][0]


def test_the_buffer_is_fully_overwritten():
    """Pre-filled with NaN, through the C entry: no NaN may remain (feasible, infeasible, rejected and short sentences alike)."""
    from cliora_amd import _lib
    m, _, sets = _padded()
    sets = [list(s) for s in sets]
    sets[1] = [(0, 1, 1), (1, 2, 1)]                               # infeasible
    rows = _tensor(CC.pack_rows(sets)).cuda()
    lengths = torch.tensor([7, 3, 9, 5], dtype=torch.int32).cuda()  # one bad length
    count = _lib.fn('cliora_plan_split_score_count')(m._plan.handle)
    assert count == 4 * sum(lv * (RAGGED_L - lv) for lv in range(1, RAGGED_L))
    buf = torch.full((count + 64,), float('nan'), device='cuda')
    lp, feas, status = torch.empty(4, device='cuda'), torch.empty(4, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.call('cliora_bracket_grad', m._plan.handle, p(m._wss[0]), p(lengths), p(rows), rows.shape[1], None, p(buf), p(lp), p(feas), p(status),
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    host = buf.cpu().numpy()
    assert not np.isnan(host[:count]).any() and np.isnan(host[count:]).all()          # all of it, and nothing beyond it
    assert status.item() == 1 and feas.cpu().tolist() == [1, 0, 0, 1] and host[:count].any()


def test_refusals():
    from cliora_amd import _lib, structured
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    # (plan, ws, lengths, brackets, M, weights, d_split, log_prob, feasible, status)
    call = lambda *a: lib.cliora_bracket_grad(*(a + (st,)))
    good = lambda h, ws: [h, ws, None, p(0), 2, None, p(100), p(500), p(600), p(700)]
    fresh = _lib.Plan(2, 5, 16)                                    # never ran a forward
    assert call(*good(fresh.handle, p(1000))) != 0
    assert 'before forward' in err()
    m = _chart(3, 3, 16)['m']
    h, ws = m._plan.handle, C.c_void_p(m._wss[0].data_ptr())
    for M in (-1, 257):
        a = good(h, ws)
        a[4] = M
        assert call(*a) != 0
        assert 'M outside 0..256' in err()
    for i in (0, 1, 6, 7, 8, 9):                                   # plan, workspace, d_split, log_prob, feasible, status
        a = good(h, ws)
        a[i] = None
        assert call(*a) != 0
        assert 'NULL argument' in err(), i
    a = good(h, ws)
    a[3] = None
    assert call(*a) != 0
    assert 'NULL brackets' in err()
    long_plan = _lib.Plan(2, 70, 16, forward_only=True)
    assert call(*good(long_plan.handle, p(1000))) != 0
    assert 'the backward stops at 64 words' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                           # nothing was launched
    with pytest.raises(_lib.ChartLibError, match='M outside 0..256'):
        structured.bracket_grad(m, torch.full((3, 257, 3), -1, dtype=torch.int32))
    with pytest.raises(ValueError):
        structured.bracket_grad(m, torch.full((4, 2, 3), -1, dtype=torch.int32))
    # the loss needs a forward that kept its backward state, on a plan with a backward
    with pytest.raises(_lib.ChartLibError, match='kept no backward state'):
        structured.bracket_log_prob(m, None)                       # _chart ran under no_grad
    lm = PC.text_module(PC.params(16, PC.GPU_SEED), 16).cuda().eval()
    _forward(lm, PC.batch(16, 65, 1, 5).cuda())
    with pytest.raises(_lib.ChartLibError, match='the backward stops at 64 words'):
        structured.bracket_log_prob(lm, None)
    with pytest.raises(_lib.ChartLibError, match='the backward stops at 64 words'):
        structured.bracket_grad(lm, None)


# ---- 3. through the chart ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def exact_mode():
    from cliora_amd import _lib
    prev = _lib.set_mfma_mode('f32')
    yield
    _lib.set_mfma_mode(prev)


def _case_sets(B, L):
    """Feasible sets: a nested required set, with a forbidden bracket inside it in every other sentence."""
    out = []
    for b in range(B):
        rows = [(s, e, 1) for s, e in CC.nested_required(L, b)]
        if b % 2 == 0:
            rows.append((rows[-1][0], rows[-1][0] + 1, 0))          # the first two words of the innermost bracket
        out.append(rows)
    return out


def _lists(sets):
    return [[(s, e) for s, e, k in rows if k == 1] for rows in sets], [[(s, e) for s, e, k in rows if k == 0] for rows in sets]


def _text_module(P, D, share):
    from test_gpu_parity import _module_from_params
    return _module_from_params(P, D, share, 'unit')


def _vl_module(P, D):
    from cliora_amd.cliora import DioraMLP
    m = DioraMLP(D, share=True, compress=False)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].clone()
    m.load_state_dict(sd)
    return m.cuda().eval()


def _oracle(P, inputs, sets, share):
    """fp64: the oracle's per-split inside scores -> mean over the sentences of -(log_z_c - log_z), differentiated by autograd.
    -> (nll, {name: gradient or None} over the parameters and the inputs)."""
    from oracle import diora_ref as R
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    t64 = [v.detach().double().requires_grad_(True) for v in inputs]
    o = R.diora_forward(P64, *t64, outside=True, normalize='unit', share=share, training=False, keep_pairs=True)
    B, L = t64[0].shape[:2]
    lps = [SC.torch_log_prob({lv: s[b, :, :, 0] for lv, s in o['pair_s_in'].items()}, L, sets[b]) for b in range(B)]
    nll = -torch.stack(lps).mean()
    nll.backward()
    grads = {k: v.grad for k, v in P64.items()}
    grads.update({name: v.grad for name, v in zip(('x_span', 'x_word', 'obj_span', 'obj_word'), t64)})
    return float(nll.detach()), grads


def _device(m, inputs, sets, resident=None):
    """bracket_nll alone through the module -> (nll, gradients by the oracle's names)."""
    from cliora_amd import _lib
    for p in m.parameters():
        p.grad = None
    tg = [v.clone().cuda().requires_grad_(True) for v in inputs]
    prev = _lib.set_resident(resident) if resident else None
    try:
        m(*((tg[0], tg[0]) if len(tg) == 1 else tg))
        nll = m.bracket_nll(*_lists(sets))
        nll.backward()
        torch.cuda.synchronize()
    finally:
        if resident:
            _lib.set_resident(prev)
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads.update({name: v.grad for name, v in zip(('x_span', 'x_word', 'obj_span', 'obj_word'), tg)})
    return float(nll.detach()), grads


def _check(got, want, what):
    from conftest import grad_check
    moved = 0
    for k, ref in want.items():
        if ref is None:                                 # the loss does not depend on it (the outside pass, the word branch)
            assert got.get(k) is None or not got[k].any(), (what, k)
            continue
        assert got[k] is not None, (what, k)
        grad_check(got[k], ref, 'f32', SC.GRAD_BOUND, '%s %s' % (what, k))
        moved += int(float(ref.abs().max()) > 1e-2)
    assert moved >= 3, what                             # a reference that would show a cotangent lost on its way to DS


@pytest.mark.parametrize('B,L,D,share', [(3, 6, 16, True), (2, 12, 80, True), (2, 6, 32, False)])
def test_bracket_nll_alone_against_the_oracle(B, L, D, share, exact_mode):
    from oracle import diora_ref as R
    P = R.init_params(D, share=share, seed=11)
    x = PC.batch(D, L, B, 700 + L)
    sets = _case_sets(B, L)
    ref_nll, want = _oracle(P, [x], sets, share)
    m = _text_module(P, D, share).train()
    nll, got = _device(m, [x], sets)
    assert abs(nll - ref_nll) <= PC.BOUND * max(1.0, abs(ref_nll))
    _check(got, want, 'B %d L %d D %d' % (B, L, D))
    if (B, L, D) == (3, 6, 16):                         # the resident schedule would take this plan: its forward, then the launch path's
        nll_off, off = _device(m, [x], sets, resident='off')        # backward -- against the launch path alone, within the bound the
        for k, g in got.items():                                    # two paths are held to (test_gpu_resident.py: 3e-5 of scale)
            if g is not None:
                sc = max(1.0, float(off[k].abs().max()))
                assert float((g - off[k]).abs().max()) <= 3e-5 * sc, k
        assert abs(nll - nll_off) <= 1e-5 * max(1.0, abs(nll_off))


def test_bracket_nll_alone_against_the_oracle_cliora(exact_mode):
    from oracle import diora_ref as R
    B, L, D, Rg = 2, 8, 32, 5
    P = R.init_params(D, share=True, seed=12)
    gen = torch.Generator().manual_seed(13)
    inputs = [torch.randn(B, L, D, generator=gen), torch.randn(B, L, D, generator=gen), 0.3 * torch.randn(B, Rg, D, generator=gen),
              0.3 * torch.randn(B, Rg, D, generator=gen)]
    sets = _case_sets(B, L)
    ref_nll, want = _oracle(P, inputs, sets, True)
    nll, got = _device(_vl_module(P, D), inputs, sets)
    assert abs(nll - ref_nll) <= PC.BOUND * max(1.0, abs(ref_nll))
    _check(got, want, 'CLIORA')


def _grads_of(m, x, loss_of):
    for p in m.parameters():
        p.grad = None
    xg = x.clone().cuda().requires_grad_(True)
    m(xg, xg)
    loss_of(m).backward()
    torch.cuda.synchronize()
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    g['x_span'] = xg.grad.detach().clone()
    return g


def test_sums_with_another_loss_two_calls_and_no_stale_cotangent(exact_mode):
    from cliora_amd import structured
    from cliora_amd.constrained import pack_brackets
    from oracle import diora_ref as R
    B, L, D = 2, 12, 80
    P = R.init_params(D, share=True, seed=11)
    x = PC.batch(D, L, B, 700 + L)
    m = _text_module(P, D, True).train()
    req, forb = _lists(_case_sets(B, L))
    gen = torch.Generator().manual_seed(3)
    cot = {k: torch.randn(B, L * (L + 1) // 2, w, generator=gen).cuda() for k, w in (('inside_h', D), ('inside_s', 1), ('outside_h', D), ('outside_s', 1))}
    loss_a = lambda mm: sum((getattr(mm, k) * v).sum() for k, v in cot.items())
    nll = lambda mm: mm.bracket_nll(req, forb)
    ga, gb, gsum = _grads_of(m, x, loss_a), _grads_of(m, x, nll), _grads_of(m, x, lambda mm: loss_a(mm) + nll(mm))
    assert set(ga) == set(gb) == set(gsum)
    for k in gsum:
        want = ga[k].double() + gb[k].double()
        sc = max(1.0, float(want.abs().max()))
        assert float((gsum[k].double() - want).abs().max()) <= SC.SUM_TOL * sc, k
    # two bracket_log_prob calls on one forward: their cotangents add in the slot -- one call with the summed weights
    br = pack_brackets(req, forb)
    w1, w2 = torch.tensor([0.5, -1.0]).cuda(), torch.tensor([0.25, 3.0]).cuda()
    two = _grads_of(m, x, lambda mm: (structured.bracket_log_prob(mm, br) * w1).sum() + (structured.bracket_log_prob(mm, br) * w2).sum())
    one = _grads_of(m, x, lambda mm: (structured.bracket_log_prob(mm, br) * (w1 + w2)).sum())
    for k in one:
        sc = max(1.0, float(one[k].abs().max()))
        assert float((two[k] - one[k]).abs().max()) <= SC.SUM_TOL * sc, k
    # a cotangent left behind (a backward that stops at inside_s) does not reach the next forward
    xg = x.clone().cuda().requires_grad_(True)
    m(xg, xg)
    torch.autograd.grad(m.bracket_nll(req, forb), [m.chart.inside_s])
    assert m._wss.split_cot[0] is not None
    again = _grads_of(m, x, loss_a)
    for k in ga:
        assert torch.equal(again[k], ga[k]), k


def test_a_zero_cotangent_gives_the_bits_of_the_plain_backward(exact_mode):
    """cliora_chart_backward_split with a buffer of zeros against cliora_chart_backward, at a shape of the launch path (the same
    schedule in both calls): every output bit for bit."""
    from cliora_amd import structured
    from oracle import diora_ref as R
    B, L, D = 2, 12, 80
    m = _text_module(R.init_params(D, share=True, seed=11), D, True).train()
    x = PC.batch(D, L, B, 700 + L)
    gen = torch.Generator().manual_seed(3)
    cot = {k: torch.randn(B, L * (L + 1) // 2, w, generator=gen).cuda() for k, w in (('inside_h', D), ('inside_s', 1), ('outside_h', D), ('outside_s', 1))}
    loss_a = lambda mm: sum((getattr(mm, k) * v).sum() for k, v in cot.items())
    plain = _grads_of(m, x, loss_a)

    def with_zeros(mm):
        mm._wss.split_cot[0] = torch.zeros(structured.split_score_count(mm._plan), device='cuda')
        return loss_a(mm)
    zeros = _grads_of(m, x, with_zeros)
    assert m._wss.split_cot[0] is None                  # taken
    assert set(plain) == set(zeros)
    for k in plain:
        assert torch.equal(plain[k], zeros[k]), k


# ---- 4. training use --------------------------------------------------------------------------------------------------------------
def _net(weight=None):
    from cliora_amd import harness as H
    torch.manual_seed(21)
    kw = {} if weight is None else dict(bracket_loss_weight=weight)
    return H.build_net(32, torch.nn.Embedding(100, 32), k_neg=20, **kw).cuda()


def _train_batch():
    g = torch.Generator().manual_seed(22)
    labels = [[('np', 1, 3), ('np', 5, 2)], [('np', 0, 2), ('vp', 2, 5), None], [('np', 3, 4)], [('np', 0, 3), ('np', 1, 2), ('x', 7, 1)]] * 2
    return dict(sentences=torch.randint(0, 100, (8, 8), generator=g).cuda(), neg_samples=torch.randperm(100, generator=g)[:20].cuda(),
                entity_labels=labels)


def test_training_lowers_the_bracket_loss():
    from cliora_amd import harness as H
    from cliora_amd.constrained import brackets_from_entity_labels
    net, bm = _net(1.0), _train_batch()
    req = brackets_from_entity_labels(bm['entity_labels'])

    def nll_now():
        net.train()
        out = net(bm['sentences'], None, bm['neg_samples'])
        assert 'bracket_nll' not in out                 # the labels were not passed: the plain step's losses
        return float(net.diora.bracket_nll(req))
    tr = H.Trainer(net)
    first = nll_now()
    for _ in range(10):
        tr.step(bm)
    last = nll_now()
    print('bracket_nll over ten steps: %.4f -> %.4f' % (first, last))
    assert first > 0 and last < first


def test_weight_zero_is_the_plain_step_bit_for_bit():
    from cliora_amd import harness as H
    bm = _train_batch()
    runs = []
    for weight in (None, 0.0):
        net = _net(weight)
        tr = H.Trainer(net)
        losses = [tr.step(bm)['total_loss'] for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k
