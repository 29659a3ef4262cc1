"""The expected cost and the entropy of the parse distribution on the GPU (cliora_amd/structured.py): cliora_tree_expectation alone,
its links to cliora_span_posteriors, and the objective through the chart's autograd node.

The yardsticks, never the code under test: ``tree_expectation_numpy`` (pinned to enumeration and to central differences by
test_expectation_cpu.py) on the device's OWN per-split scores for the kernel; cliora_span_posteriors for log_z and risk; the fp64
oracle with a torch restatement of J (expectation_cases.torch_objective), differentiated by autograd, for the gradients through the
chart.  Cases, bounds and measured figures: expectation_cases.py.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import constrained_cases as CC
import expectation_cases as EC
import posterior_cases as PC
import structured_cases as SC
from test_gpu_constrained import _forward, _scores
from test_gpu_structured import _check, _grads_of, _lists, _case_sets, _text_module, _vl_module, exact_mode     # noqa: F401

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _chart(B, L, D):
    """One eval forward of a text-only DioraMLP (random weights) and the device's scores -- once per shape."""
    m = PC.text_module(PC.params(D, PC.GPU_SEED), D).cuda().eval()
    _forward(m, PC.batch(D, L, B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m) if L > 1 else {})


def _expect(m, cost=None, wc=None, we=None, lengths=None):
    """structured.tree_expectation with host inputs -> dict of numpy arrays: G {level: (B, L - level, level)}, flat, the scalars, status."""
    from cliora_amd.structured import split_rows_by_level, tree_expectation
    t32 = lambda v: None if v is None else torch.as_tensor(np.asarray(v, dtype=np.float32))
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    res = tree_expectation(m, t32(cost), t32(wc), t32(we), lt)
    G = {lv: g.cpu().numpy() for lv, g in split_rows_by_level(m._plan, res.d_split).items()}
    return dict(G=G, flat=res.d_split.cpu().numpy(), risk=res.risk.cpu().numpy(), entropy=res.entropy.cpu().numpy(),
                log_z=res.log_z.cpu().numpy(), status=res.status.cpu().tolist())


def _costs(B, L):
    """name -> (B, C) fp32 costs: -1 on the inner brackets of a gold tree; -1 / +1 on random spans with a crossing pair."""
    from cliora_amd.structured import span_costs
    gold = [[(s, e) for s, e, _ in SC.gold_tree_rows(L, 60 + b)] for b in range(B)]
    lists = [EC.crossing_spans(L, b) for b in range(B)]
    return {'gold tree': span_costs(gold, L=L).numpy(), 'crossing spans': span_costs([r for r, _ in lists], [f for _, f in lists], L=L).numpy()}


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))))


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', EC.GPU_SHAPES)
def test_kernel_against_the_fp64_restatement(B, L, D):
    from cliora_amd.structured import tree_expectation_numpy
    c = _chart(B, L, D)
    m, scores = c['m'], c['scores']
    worst, moved = [0.0] * 4, 0
    for name, cost in _costs(B, L).items():
        for wc, we in EC.WEIGHTS:
            got = _expect(m, cost, [wc] * B, [we] * B)
            G64, risk, entropy, log_z = tree_expectation_numpy(scores, [L] * B, cost, [wc] * B, [we] * B)
            assert got['status'] == [0], name
            scale = max(1.0, max(float(np.abs(g).max()) for g in G64.values()))
            for level in range(1, L):
                err = float(np.abs(got['G'][level].astype(np.float64) - G64[level]).max()) / scale
                worst[0] = max(worst[0], err)
                assert err <= EC.BOUND, (name, wc, we, level, err)
                assert float(np.abs(got['G'][level].astype(np.float64).sum(axis=2)).max()) <= 1e-6, (name, level)
            for i, (g, w) in enumerate(((got['risk'], risk), (got['entropy'], entropy), (got['log_z'], log_z))):
                worst[1 + i] = max(worst[1 + i], _rel(g, w))
                assert _rel(g, w) <= EC.BOUND, (name, wc, we, i, g, w)
            moved += int(any(np.abs(got['G'][level]).max() > 1e-3 for level in range(1, L)))
    print('L %d: max |G - fp64| / scale = %.3e, risk %.3e, entropy %.3e, log_z %.3e relative (measured before: %s)'
          % ((L,) + tuple(worst) + (EC.MEASURED.get('L %d' % L),)))
    assert moved >= 4                                  # gradients, not zeros


def test_one_and_two_words_are_the_closed_forms():
    from cliora_amd.structured import span_costs
    m = _chart(3, 2, 16)['m']                          # one cell, one split
    cost = np.array([[0.25, -1.0, 2.0], [1.0, 1.0, 1.0], [0.0, 0.5, -0.125]], dtype=np.float32)
    got = _expect(m, cost, [3.0, -2.0, 0.5], [1.0, 1.0, -4.0])
    assert got['flat'].size == 3 and not got['flat'].any() and got['status'] == [0]
    assert got['risk'].tolist() == cost.sum(axis=1).tolist() and not got['entropy'].any() and not got['log_z'].any()
    one = PC.text_module(PC.params(16, PC.GPU_SEED), 16).cuda().eval()
    _forward(one, PC.batch(16, 1, 2, 9).cuda())
    got = _expect(one, np.array([[0.75], [-3.0]], dtype=np.float32))
    assert got['flat'].size == 0 and got['risk'].tolist() == [0.75, -3.0] and got['entropy'].tolist() == [0.0, 0.0] and got['status'] == [0]
    # in a padded chart too
    m7 = _chart(3, 7, 16)['m']
    cost = span_costs([[(0, 1)], [(0, 0)], [(1, 1), (0, 1)]], L=7).numpy()
    got = _expect(m7, cost, lengths=[2, 1, 2])
    assert got['risk'].tolist() == [-1.0, -1.0, -2.0] and not got['entropy'].any() and not got['flat'].any() and got['status'] == [0]


# ---- 2. the links to cliora_span_posteriors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', EC.GPU_SHAPES)
def test_log_z_and_risk_are_those_of_the_span_posteriors(B, L, D):
    from cliora_amd.posterior import span_posteriors
    m = _chart(B, L, D)['m']
    post = span_posteriors(m)
    mu, log_z = post.marginals.cpu().numpy().astype(np.float64), post.log_z.cpu().numpy()
    for name, cost in _costs(B, L).items():
        got = _expect(m, cost)
        assert _rel(got['log_z'], log_z) <= EC.BOUND and _rel(got['risk'], (mu * cost).sum(axis=1)) <= EC.BOUND, name
        assert np.array_equal(_bits(got['log_z']), _bits(log_z)), name       # one inside reduction (posterior_kernels.hpp: inside_lse)


# ---- 3. bitwise and robustness properties -----------------------------------------------------------------------------------------
RAGGED_L, RAGGED_LENGTHS = 7, (5, 1, 2, 7)
KEYS = ('flat', 'risk', 'entropy', 'log_z')


@functools.lru_cache(maxsize=None)
def _padded():
    xs = [PC.sentence(PC.GPU_D, n, 5100 + b) for b, n in enumerate(RAGGED_LENGTHS)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, RAGGED_L).cuda())
    cost = EC.random_costs(len(xs), RAGGED_L, 8).astype(np.float32)
    return m, xs, cost


PADDED_W = ([0.7, 1.0, -2.0, 0.5], [-1.3, 0.5, 1.0, 2.0])


def test_two_calls_give_equal_bits():
    B, L = 2, 64
    m = _chart(B, L, 32)['m']
    cost = _costs(B, L)['crossing spans']
    a, b = _expect(m, cost, [0.7] * B, [-1.3] * B), _expect(m, cost, [0.7] * B, [-1.3] * B)
    assert a['flat'].any()
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_padded_chart_is_each_sentence_alone():
    """lengths (5, 1, 2, 7) at L 7: each sentence gets the bits it gets alone at its own L, and every element beyond a triangle is zero."""
    from cliora_amd.structured import tree_expectation_numpy
    m, xs, cost = _padded()
    L, lengths = RAGGED_L, list(RAGGED_LENGTHS)
    got = _expect(m, cost, *PADDED_W, lengths=lengths)
    assert got['status'] == [0]
    G64, risk, entropy, log_z = tree_expectation_numpy(_scores(m), lengths, cost, *PADDED_W)
    for level in range(1, L):
        assert float(np.abs(got['G'][level] - G64[level]).max()) <= EC.BOUND * max(1.0, max(float(np.abs(g).max()) for g in G64.values()))
    assert max(_rel(got['risk'], risk), _rel(got['entropy'], entropy), _rel(got['log_z'], log_z)) <= EC.BOUND
    alone = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    alone.outside = False
    for b, n in enumerate(lengths):
        for level in range(1, L):
            assert not got['G'][level][b, max(0, n - level):].any(), (b, level)          # beyond the triangle
        own = np.zeros((1, n * (n + 1) // 2), dtype=np.float32)
        for level in range(n):
            own[0, EC.cell_id(n, level, 0):EC.cell_id(n, level, 0) + n - level] = cost[b, EC.cell_id(L, level, 0):EC.cell_id(L, level, 0) + n - level]
        _forward(alone, xs[b][None].cuda())
        one = _expect(alone, own, PADDED_W[0][b:b + 1], PADDED_W[1][b:b + 1])
        assert one['status'] == [0]
        for k in KEYS[1:]:
            assert np.array_equal(_bits(one[k]), _bits(got[k][b:b + 1])), (b, k)
        for level in range(1, n):
            assert np.array_equal(_bits(one['G'][level][0]), _bits(got['G'][level][b, :n - level])), (b, level)
    assert any(got['G'][level][0].any() for level in range(1, L)) and any(got['G'][level][3].any() for level in range(1, L))


def test_every_length_equal_to_L_is_the_call_without_lengths():
    B, L = 2, 13
    m = _chart(B, L, 48)['m']
    cost = _costs(B, L)['gold tree']
    a, b = _expect(m, cost, [0.7] * B, [-1.3] * B, lengths=[L] * B), _expect(m, cost, [0.7] * B, [-1.3] * B)
    assert a['status'] == [0] and a['flat'].any()
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_bad_lengths_leave_their_neighbours_alone():
    m, _, cost = _padded()
    L, lengths = RAGGED_L, list(RAGGED_LENGTHS)
    clean = _expect(m, cost, *PADDED_W, lengths=lengths)
    bad_lengths = [5, 0, 8, 7]
    nan = float('nan')
    bad_cost = cost.copy()
    bad_cost[1:3] = nan                                            # the costs and the weights of a bad-length sentence are not read
    got = _expect(m, bad_cost, [0.7, nan, nan, 0.5], [-1.3, nan, nan, 2.0], lengths=bad_lengths)
    assert got['status'] == [2]
    for k in KEYS[1:]:
        assert got[k][1:3].tolist() == [0.0, 0.0], k
        assert np.array_equal(_bits(got[k][[0, 3]]), _bits(clean[k][[0, 3]])), k
    for level in range(1, L):
        assert not got['G'][level][1:3].any()
        for b in (0, 3):
            assert np.array_equal(_bits(got['G'][level][b]), _bits(clean['G'][level][b])), (level, b)


def test_the_buffer_is_fully_overwritten():
    """Pre-filled with NaN, through the C entry: no NaN may remain (full, short, one-word and rejected sentences alike)."""
    from cliora_amd import _lib
    m, _, cost = _padded()
    lengths = torch.tensor([5, 1, 9, 7], dtype=torch.int32).cuda()  # one bad length
    count = _lib.fn('cliora_plan_split_score_count')(m._plan.handle)
    assert count == 4 * sum(lv * (RAGGED_L - lv) for lv in range(1, RAGGED_L))
    buf = torch.full((count + 64,), float('nan'), device='cuda')
    ct = torch.from_numpy(cost).cuda()
    out = torch.full((3, 4), float('nan'), device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.call('cliora_tree_expectation', m._plan.handle, p(m._wss[0]), p(lengths), p(ct), None, None, p(buf), p(out[0]), p(out[1]), p(out[2]),
              p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    host = buf.cpu().numpy()
    assert not np.isnan(host[:count]).any() and np.isnan(host[count:]).all()          # all of it, and nothing beyond it
    assert status.item() == 1 and host[:count].any() and not torch.isnan(out).any()


def test_refusals():
    from cliora_amd import _lib, structured
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    # (plan, ws, lengths, cost, w_cost, w_entropy, d_split, risk, entropy, log_z, status)
    call = lambda *a: lib.cliora_tree_expectation(*(a + (st,)))
    good = lambda h, ws: [h, ws, None, None, None, None, p(100), p(500), p(600), p(700), p(800)]
    fresh = _lib.Plan(2, 5, 16)                                    # never ran a forward
    assert call(*good(fresh.handle, p(1000))) != 0
    assert 'before forward' in err()
    m = _chart(3, 3, 16)['m']
    h, ws = m._plan.handle, C.c_void_p(m._wss[0].data_ptr())
    for i in (0, 1, 6, 7, 8, 9, 10):                               # plan, workspace, d_split, risk, entropy, log_z, status
        a = good(h, ws)
        a[i] = None
        assert call(*a) != 0
        assert 'NULL argument' in err(), i
    long_plan = _lib.Plan(2, 65, 16, forward_only=True)
    assert call(*good(long_plan.handle, p(1000))) != 0
    assert 'the backward stops at 64 words' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                           # nothing was launched
    with pytest.raises(ValueError):
        structured.tree_expectation(m, torch.zeros(3, 5))          # not (B, C)
    # the objective needs a forward that kept its backward state, on a plan with a backward, of a module with one chart node
    with pytest.raises(_lib.ChartLibError, match='has run no forward'):
        structured.tree_objective(PC.text_module(PC.params(16, PC.GPU_SEED), 16))
    with pytest.raises(_lib.ChartLibError, match='kept no backward state'):
        structured.tree_objective(m)                               # _chart ran under no_grad
    lm = PC.text_module(PC.params(16, PC.GPU_SEED), 16).cuda().eval()
    _forward(lm, PC.batch(16, 65, 1, 5).cuda())
    with pytest.raises(_lib.ChartLibError, match='the backward stops at 64 words'):
        structured.tree_objective(lm)
    with pytest.raises(_lib.ChartLibError, match='the backward stops at 64 words'):
        structured.tree_expectation(lm)
    with pytest.raises(_lib.ChartLibError, match='TreeLSTM'):
        structured.tree_objective(types.SimpleNamespace(_plan=m._plan, plan_arch=1))
    with pytest.raises(_lib.ChartLibError, match='2 workspaces'):
        structured.tree_objective(types.SimpleNamespace(_plan=m._plan, _wss=[m._wss[0], m._wss[0]]))


# ---- 4. through the chart ---------------------------------------------------------------------------------------------------------
A_RISK, B_ENTROPY = 0.7, -1.3


def _case_costs(B, L):
    from cliora_amd.structured import span_costs
    lists = [EC.crossing_spans(L, b) for b in range(B)]
    return span_costs([r for r, _ in lists], [f for _, f in lists], L=L)


def _oracle(P, inputs, cost, share):
    """fp64: the oracle's per-split inside scores -> J = a mean risk + b mean entropy by expectation_cases.torch_objective,
    differentiated by autograd.  -> (J, {name: gradient or None} over the parameters and the inputs)."""
    from oracle import diora_ref as R
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    t64 = [v.detach().double().requires_grad_(True) for v in inputs]
    o = R.diora_forward(P64, *t64, outside=True, normalize='unit', share=share, training=False, keep_pairs=True)
    B, L = t64[0].shape[:2]
    c64 = cost.double().numpy()
    vals = [EC.torch_objective({lv: s[b, :, :, 0] for lv, s in o['pair_s_in'].items()}, L, c64[b], L) for b in range(B)]
    J = A_RISK * torch.stack([r for r, _ in vals]).mean() + B_ENTROPY * torch.stack([h for _, h in vals]).mean()
    J.backward()
    grads = {k: v.grad for k, v in P64.items()}
    grads.update({name: v.grad for name, v in zip(('x_span', 'x_word', 'obj_span', 'obj_word'), t64)})
    return float(J.detach()), grads


def _device(m, inputs, cost):
    """(a risk.mean() + b entropy.mean()).backward() alone through the module -> (J, gradients by the oracle's names)."""
    for p in m.parameters():
        p.grad = None
    tg = [v.clone().cuda().requires_grad_(True) for v in inputs]
    m(*((tg[0], tg[0]) if len(tg) == 1 else tg))
    risk, entropy = m.tree_objective(cost.cuda())
    J = A_RISK * risk.mean() + B_ENTROPY * entropy.mean()
    J.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads.update({name: v.grad for name, v in zip(('x_span', 'x_word', 'obj_span', 'obj_word'), tg)})
    return float(J.detach()), grads


@pytest.mark.parametrize('B,L,D,share', [(3, 6, 16, True), (2, 12, 80, True), (2, 6, 32, False)])
def test_objective_alone_against_the_oracle(B, L, D, share, exact_mode):
    from oracle import diora_ref as R
    P = R.init_params(D, share=share, seed=11)
    x = PC.batch(D, L, B, 700 + L)
    cost = _case_costs(B, L)
    ref, want = _oracle(P, [x], cost, share)
    J, got = _device(_text_module(P, D, share).train(), [x], cost)
    print('B %d L %d D %d: J %.6f, fp64 %.6f' % (B, L, D, J, ref))
    assert abs(J - ref) <= EC.BOUND * max(1.0, abs(ref))
    _check(got, want, 'B %d L %d D %d' % (B, L, D))


def test_objective_alone_against_the_oracle_cliora(exact_mode):
    from oracle import diora_ref as R
    B, L, D, Rg = 2, 8, 32, 5
    P = R.init_params(D, share=True, seed=12)
    gen = torch.Generator().manual_seed(13)
    inputs = [torch.randn(B, L, D, generator=gen), torch.randn(B, L, D, generator=gen), 0.3 * torch.randn(B, Rg, D, generator=gen),
              0.3 * torch.randn(B, Rg, D, generator=gen)]
    cost = _case_costs(B, L)
    ref, want = _oracle(P, inputs, cost, True)
    J, got = _device(_vl_module(P, D), inputs, cost)
    assert abs(J - ref) <= EC.BOUND * max(1.0, abs(ref))
    _check(got, want, 'CLIORA')


def test_sums_with_other_losses_and_with_a_second_call(exact_mode):
    """On one forward: a loss on the four chart outputs (what the reconstruction loss reads; a fixed linear one here), bracket_nll and
    the objective together give the sum of the three separate backward results; two tree_objective calls add up in the slot."""
    from cliora_amd import structured
    from oracle import diora_ref as R
    B, L, D = 2, 12, 80
    P = R.init_params(D, share=True, seed=11)
    x = PC.batch(D, L, B, 700 + L)
    m = _text_module(P, D, True).train()
    req, forb = _lists(_case_sets(B, L))
    cost = _case_costs(B, L).cuda()
    gen = torch.Generator().manual_seed(3)
    cot = {k: torch.randn(B, L * (L + 1) // 2, w, generator=gen).cuda() for k, w in (('inside_h', D), ('inside_s', 1), ('outside_h', D), ('outside_s', 1))}
    loss_a = lambda mm: sum((getattr(mm, k) * v).sum() for k, v in cot.items())
    nll = lambda mm: mm.bracket_nll(req, forb)

    def obj(mm):
        risk, entropy = mm.tree_objective(cost)
        return A_RISK * risk.mean() + B_ENTROPY * entropy.mean()
    ga, gb, gc = _grads_of(m, x, loss_a), _grads_of(m, x, nll), _grads_of(m, x, obj)
    gsum = _grads_of(m, x, lambda mm: loss_a(mm) + nll(mm) + obj(mm))
    assert set(ga) == set(gb) == set(gc) == set(gsum)
    assert sum(int(float(g.abs().max()) > 1e-2) for g in gc.values()) >= 3
    for k in gsum:
        want = ga[k].double() + gb[k].double() + gc[k].double()
        sc = max(1.0, float(want.abs().max()))
        assert float((gsum[k].double() - want).abs().max()) <= EC.SUM_TOL * sc, k
    w1, w2 = torch.tensor([0.5, -1.0]).cuda(), torch.tensor([0.25, 3.0]).cuda()

    def twice(mm):
        r1, h1 = structured.tree_objective(mm, cost)
        r2, h2 = structured.tree_objective(mm, cost)
        return (r1 * w1).sum() + (h2 * w2).sum() + (r2 * w2).sum() + (h1 * w1).sum()

    def once(mm):
        r, h = structured.tree_objective(mm, cost)
        return (r * (w1 + w2)).sum() + (h * (w1 + w2)).sum()
    two, one = _grads_of(m, x, twice), _grads_of(m, x, once)
    for k in one:
        sc = max(1.0, float(one[k].abs().max()))
        assert float((two[k] - one[k]).abs().max()) <= EC.SUM_TOL * sc, k
    # one cotangent alone: the other one is taken as zeros
    only = _grads_of(m, x, lambda mm: mm.parse_entropy())
    both = _grads_of(m, x, lambda mm: 0.0 * mm.tree_objective(cost)[0].mean() + mm.tree_objective(None)[1].mean())
    for k in only:
        sc = max(1.0, float(only[k].abs().max()))
        assert float((only[k] - both[k]).abs().max()) <= EC.SUM_TOL * sc, k


# ---- 5. training use --------------------------------------------------------------------------------------------------------------
def _net(**kw):
    from cliora_amd import harness as H
    torch.manual_seed(21)
    return H.build_net(32, torch.nn.Embedding(100, 32), k_neg=20, **kw).cuda()


def _train_batch():
    g = torch.Generator().manual_seed(22)
    labels = [[('np', 1, 3), ('np', 2, 4)], [('np', 0, 2), ('vp', 2, 5), None], [('np', 3, 4)], [('np', 0, 3), ('np', 1, 2), ('x', 7, 1)]] * 2
    return dict(sentences=torch.randint(0, 100, (8, 8), generator=g).cuda(), neg_samples=torch.randperm(100, generator=g)[:20].cuda(),
                entity_labels=labels)


def test_zero_weights_are_the_plain_step_bit_for_bit():
    from cliora_amd import harness as H
    bm = _train_batch()
    runs = []
    for kw in ({}, dict(risk_loss_weight=0.0, entropy_loss_weight=0.0)):
        net = _net(**kw)
        tr = H.Trainer(net)
        losses = [tr.step(bm)['total_loss'] for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k


@pytest.mark.parametrize('which', ['risk', 'entropy'])
def test_training_lowers_the_risk_and_the_entropy(which):
    from cliora_amd import harness as H
    from cliora_amd.constrained import brackets_from_entity_labels, crosses
    from cliora_amd.structured import span_costs
    net = _net(**{which + '_loss_weight': 1.0})
    bm = _train_batch()
    phrases = brackets_from_entity_labels(bm['entity_labels'], drop_crossing=False)
    assert crosses(*phrases[0])                             # the batch holds a crossing pair
    cost = span_costs(phrases, L=8, device='cuda')

    def now():
        net.train()
        net(bm['sentences'], None, bm['neg_samples'])
        risk, entropy = net.diora.tree_objective(cost)
        return float(risk.detach().mean()) if which == 'risk' else float(entropy.detach().mean())
    tr = H.Trainer(net)
    first = now()
    for _ in range(10):
        tr.step(bm)
    net.train()
    assert which in net(bm['sentences'], None, bm['neg_samples'], entity_labels=bm['entity_labels'])      # the step's loss has the term
    last = now()
    print('mean %s over ten steps: %.4f -> %.4f' % (which, first, last))
    assert last < first
