"""The divergence between two charts' parse distributions on the GPU (cliora_amd/structured.py): cliora_tree_kl alone, its links to
cliora_span_posteriors and cliora_tree_expectation, both gradients through the two charts' autograd nodes, and its use in training.

The yardsticks, never the code under test: ``tree_kl_numpy`` (pinned to enumeration and to central differences by test_kl_cpu.py) on
the device's OWN per-split scores of both charts for the kernel; cliora_span_posteriors for the two log_z and
cliora_tree_expectation for entropy_p; the fp64 oracle with a torch restatement of J (kl_cases.torch_kl), differentiated by autograd,
for the gradients through the charts.  Cases, bounds and measured figures: kl_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kl_cases as KC
import posterior_cases as PC
from test_gpu_constrained import _forward, _scores
from test_gpu_structured import _check, _grads_of, _lists, _case_sets, _text_module, _vl_module, exact_mode     # noqa: F401

pytestmark = pytest.mark.gpu

SCALARS = ('kl', 'cross_entropy', 'entropy_p', 'log_z_p', 'log_z_q')
KEYS = ('flat_p', 'flat_q') + SCALARS


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _module(D, seed):
    return PC.text_module(PC.params(D, seed), D).cuda().eval()


@functools.lru_cache(maxsize=None)
def _pair(B, L, D, Dt=None):
    """One eval forward each of a teacher (width Dt, default D) and a student, two text-only DioraMLPs of different seeds, on batches
    of the same B and L, and the device's scores of both -- once per shape."""
    Dt = D if Dt is None else Dt
    t, s = _module(Dt, KC.TEACHER_SEED), _module(D, KC.STUDENT_SEED)
    _forward(t, PC.batch(Dt, L, B, PC.GPU_SEED + L).cuda())
    _forward(s, PC.batch(D, L, B, PC.GPU_SEED + L).cuda())
    return dict(t=t, s=s, sp=_scores(t) if L > 1 else {}, sq=_scores(s) if L > 1 else {})


def _kl(t, s, wk=None, wc=None, lengths=None, teacher_grad=True):
    """structured.tree_kl with host inputs -> dict of numpy arrays: Gp (None without teacher_grad), Gq {level: (B, L - level, level)},
    flat_p, flat_q, the five scalars, status."""
    from cliora_amd.structured import split_rows_by_level, tree_kl
    t32 = lambda v: None if v is None else torch.as_tensor(np.asarray(v, dtype=np.float32))
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    res = tree_kl(t, s, t32(wk), t32(wc), lt, teacher_grad=teacher_grad)
    rows = lambda d: {lv: g.cpu().numpy() for lv, g in split_rows_by_level(t._plan, d).items()}
    out = dict(Gp=rows(res.d_split_p) if teacher_grad else None, Gq=rows(res.d_split_q),
               flat_p=res.d_split_p.cpu().numpy() if teacher_grad else np.zeros(0, dtype=np.float32), flat_q=res.d_split_q.cpu().numpy(),
               status=res.status.cpu().tolist())
    out.update({k: getattr(res, k).cpu().numpy() for k in SCALARS})
    return out


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))))


def _against(got, want, L, what, worst=None):
    """One device result against a tree_kl_numpy result: the bounds of kl_cases.py; -> the worst errors (Gp, Gq, the five scalars)."""
    worst = [0.0] * 7 if worst is None else worst
    for i, (G, G64) in enumerate(((got['Gp'], want.d_split_p), (got['Gq'], want.d_split_q))):
        if G is None:
            continue
        scale = max(1.0, max([float(np.abs(g).max()) for g in G64.values()] + [0.0]))
        for level in range(1, L):
            err = float(np.abs(G[level].astype(np.float64) - G64[level]).max()) / scale
            worst[i] = max(worst[i], err)
            assert err <= KC.BOUND, (what, 'pq'[i], level, err)
            assert float(np.abs(G[level].astype(np.float64).sum(axis=2)).max()) <= KC.GPU_ROW_SUM_TOL, (what, 'pq'[i], level)
    for i, k in enumerate(SCALARS):
        worst[2 + i] = max(worst[2 + i], _rel(got[k], getattr(want, k)))
        assert _rel(got[k], getattr(want, k)) <= KC.BOUND, (what, k, got[k], getattr(want, k))
    return worst


# ---- 1. the kernel against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', KC.GPU_SHAPES)
def test_kernel_against_the_fp64_restatement(B, L, D):
    from cliora_amd.structured import tree_kl_numpy
    c = _pair(B, L, D)
    worst, moved = None, 0
    for wk, wc in KC.WEIGHTS:
        want = tree_kl_numpy(c['sp'], c['sq'], [L] * B, [wk] * B, [wc] * B)
        for tg in (True, False):
            got = _kl(c['t'], c['s'], [wk] * B, [wc] * B, teacher_grad=tg)
            assert got['status'] == [0]
            worst = _against(got, want, L, (wk, wc, tg), worst)
            moved += int(any(np.abs(got['Gq'][level]).max() > 1e-3 for level in range(1, L)))
            moved += int(tg and any(np.abs(got['Gp'][level]).max() > 1e-3 for level in range(1, L)))
        assert (want.kl > 1e-3).all()                  # two different distributions
    print('L %d: max |d_split_p - fp64| / scale = %.3e, d_split_q %.3e; kl %.3e, cross_entropy %.3e, entropy_p %.3e, log_z_p %.3e, '
          'log_z_q %.3e relative (measured before: %s)' % ((L,) + tuple(worst) + (KC.MEASURED.get('L %d' % L),)))
    assert moved >= 6                                  # gradients, not zeros (the cross-entropy alone leaves some d_split_p rows small)


def test_one_and_two_words_are_zeros():
    c = _pair(3, 2, 16)                                # one cell, one split
    got = _kl(c['t'], c['s'], [3.0, -2.0, 0.5], [1.0, 1.0, -4.0])
    assert got['flat_p'].size == 3 and not got['flat_p'].any() and not got['flat_q'].any() and got['status'] == [0]
    for k in SCALARS:
        assert not got[k].any(), k
    t, s = _module(16, KC.TEACHER_SEED), _module(16, KC.STUDENT_SEED)
    for m in (t, s):
        _forward(m, PC.batch(16, 1, 2, 9).cuda())
    got = _kl(t, s)
    assert got['flat_q'].size == 0 and got['status'] == [0] and all(not got[k].any() for k in SCALARS)
    c7 = _pair(3, 7, 16)                               # in a padded chart too
    got = _kl(c7['t'], c7['s'], lengths=[2, 1, 2])
    assert got['status'] == [0] and not got['flat_p'].any() and not got['flat_q'].any() and all(not got[k].any() for k in SCALARS)


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', KC.GPU_SHAPES)
def test_log_z_and_entropy_have_the_siblings_bits(B, L, D):
    from cliora_amd.posterior import span_posteriors
    from cliora_amd.structured import tree_expectation
    c = _pair(B, L, D)
    got = _kl(c['t'], c['s'])
    assert np.array_equal(_bits(got['log_z_p']), _bits(span_posteriors(c['t']).log_z.cpu().numpy()))      # one inside reduction
    assert np.array_equal(_bits(got['log_z_q']), _bits(span_posteriors(c['s']).log_z.cpu().numpy()))
    ex = tree_expectation(c['t'], None, torch.zeros(B), torch.ones(B))
    assert np.array_equal(_bits(got['entropy_p']), _bits(ex.entropy.cpu().numpy()))                       # one sum of nu r, in one order
    assert np.array_equal(_bits(got['log_z_p']), _bits(ex.log_z.cpu().numpy()))


def test_two_calls_give_equal_bits_with_or_without_the_teachers_gradient():
    B, L = 2, 64
    c = _pair(B, L, 32)
    a, b = (_kl(c['t'], c['s'], [0.7] * B, [-0.4] * B) for _ in range(2))
    only_q = _kl(c['t'], c['s'], [0.7] * B, [-0.4] * B, teacher_grad=False)
    assert a['flat_p'].any() and a['flat_q'].any()
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    for k in KEYS[1:]:
        assert np.array_equal(_bits(a[k]), _bits(only_q[k])), k


def _padded_modules(seed):
    xs = [PC.sentence(PC.GPU_D, n, 5100 + b) for b, n in enumerate(KC.RAGGED_LENGTHS)]
    m = _module(PC.GPU_D, seed)
    m.outside = False
    _forward(m, PC.padded(xs, KC.RAGGED_L).cuda())
    return m, xs


@functools.lru_cache(maxsize=None)
def _padded():
    t, xs = _padded_modules(PC.MBR_PARAM_SEED)
    return t, _padded_modules(PC.MBR_PARAM_SEED + 3)[0], xs


def _raw(t, s, lengths, with_p=True, with_q=True, wk=None, wc=None):
    """The C entry itself with NaN-filled outputs -> (d_split_p, d_split_q with 64 floats beyond each, the (5, B) scalars, status)."""
    from cliora_amd import _lib
    B = t._plan.B
    count = _lib.fn('cliora_plan_split_score_count')(t._plan.handle)
    bufs = [torch.full((count + 64,), float('nan'), device='cuda') for _ in range(2)]
    out = torch.full((5, B), float('nan'), device='cuda')
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    _lib.call('cliora_tree_kl', t._plan.handle, p(t._wss[0]), s._plan.handle, p(s._wss[0]), p(lengths), p(wk), p(wc),
              p(bufs[0]) if with_p else None, p(bufs[1]) if with_q else None, *(p(out[i]) for i in range(5)), p(status),
              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return bufs[0].cpu().numpy(), bufs[1].cpu().numpy(), out.cpu().numpy(), int(status.item()), count


def test_every_output_is_fully_overwritten():
    """Pre-filled with NaN, through the C entry: no NaN may remain (full, short, one-word and rejected sentences alike), with both
    gradients, with the student's alone and with none."""
    t, s, _ = _padded()
    lengths = torch.tensor([5, 1, 9, 7], dtype=torch.int32).cuda()  # one bad length
    assert _raw(t, s, lengths)[4] == 4 * sum(lv * (KC.RAGGED_L - lv) for lv in range(1, KC.RAGGED_L))
    full = None
    for with_p, with_q in ((True, True), (False, True), (False, False)):
        gp, gq, out, status, count = _raw(t, s, lengths, with_p, with_q)
        assert status == 1 and not np.isnan(out).any()
        for g, given in ((gp, with_p), (gq, with_q)):
            assert np.isnan(g[count:]).all()                                   # nothing beyond it
            assert (not np.isnan(g[:count]).any() and g[:count].any()) if given else np.isnan(g).all()
        full = out if full is None else full
        assert np.array_equal(_bits(out), _bits(full))                         # the scalars do not depend on which gradients are asked for


# ---- 3. the same chart as both ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', KC.GPU_SHAPES[1:])
def test_a_chart_against_itself(B, L, D):
    t = _pair(B, L, D)['t']
    got = _kl(t, t)                                    # KL alone: stationary in both charts
    assert got['status'] == [0] and not got['flat_q'].any()                    # nu^q == nu^p bit for bit: one expression forms both
    assert float(np.abs(got['kl']).max()) <= KC.SAME_TOL
    assert float(np.abs(got['flat_p']).max()) <= KC.SAME_TOL                   # of scale 1: a difference of probabilities at rounding level
    mixed = _kl(t, t, [0.7] * B, [-0.4] * B)
    assert not mixed['flat_q'].any() and np.array_equal(_bits(mixed['cross_entropy']), _bits(mixed['entropy_p']))


# ---- 4. roles and shapes ----------------------------------------------------------------------------------------------------------
def test_teacher_of_another_width():
    from cliora_amd.structured import tree_kl_numpy
    B, L = 3, 7
    c = _pair(B, L, 16, 32)
    assert c['t']._plan.D == 32 and c['s']._plan.D == 16
    got = _kl(c['t'], c['s'], [0.7] * B, [-0.4] * B)
    _against(got, tree_kl_numpy(c['sp'], c['sq'], [L] * B, [0.7] * B, [-0.4] * B), L, 'D 32 against D 16')
    # swapped roles agree with the restatement's swapped call
    got = _kl(c['s'], c['t'], [0.7] * B, [-0.4] * B)
    _against(got, tree_kl_numpy(c['sq'], c['sp'], [L] * B, [0.7] * B, [-0.4] * B), L, 'swapped')


def test_cliora_student_and_hard_student():
    from cliora_amd.diora import DioraMLP
    from cliora_amd.structured import tree_kl_numpy
    from oracle import diora_ref as R
    B, L, D, Rg = 2, 8, 32, 5
    gen = torch.Generator().manual_seed(13)
    x, obj = torch.randn(B, L, D, generator=gen).cuda(), (0.3 * torch.randn(B, Rg, D, generator=gen)).cuda()
    t = _module(D, KC.TEACHER_SEED)
    _forward(t, x)
    vl = _vl_module(R.init_params(D, share=True, seed=12), D)
    with torch.no_grad():
        vl(x, x, obj, obj)
    assert vl._plan is not t._plan
    hard = DioraMLP(D, hard=True).cuda().eval()
    hard.load_state_dict(_module(D, KC.STUDENT_SEED).state_dict())
    _forward(hard, x)
    assert hard.selection is not None
    for name, s in (('CLIORA', vl), ('hard', hard)):
        got = _kl(t, s, [0.7] * B, [-0.4] * B)
        assert got['status'] == [0] and got['flat_q'].any()
        _against(got, tree_kl_numpy(_scores(t), _scores(s), [L] * B, [0.7] * B, [-0.4] * B), L, name)


def test_refusals():
    from cliora_amd import _lib, structured
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(8192, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    # (plan_p, ws_p, plan_q, ws_q, lengths, w_kl, w_ce, d_split_p, d_split_q, kl, ce, entropy_p, log_z_p, log_z_q, status)
    call = lambda *a: lib.cliora_tree_kl(*(a + (st,)))
    good = lambda hp, wp, hq, wq: [hp, wp, hq, wq, None, None, None, p(100), p(300), p(500), p(600), p(700), p(800), p(900), p(1000)]
    c3, c7 = _pair(3, 3, 16), _pair(3, 7, 16)
    h = lambda m: (m._plan.handle, C.c_void_p(m._wss[0].data_ptr()))
    fresh = _lib.Plan(3, 3, 16)                                    # never ran a forward
    for a in (good(fresh.handle, p(2000), *h(c3['s'])), good(*h(c3['t']), fresh.handle, p(2000))):
        assert call(*a) != 0
        assert err().startswith('cliora_tree_kl') and 'before forward' in err()
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14):                  # the plans, the workspaces, the five scalars, status
        a = good(*h(c3['t']), *h(c3['s']))
        a[i] = None
        assert call(*a) != 0
        assert err().startswith('cliora_tree_kl') and 'NULL argument' in err(), i
    for a in (good(*h(c3['t']), *h(c7['s'])), good(*h(c3['t']), *h(_pair(2, 3, 16)['s']))):       # L, B
        assert call(*a) != 0
        assert err().startswith('cliora_tree_kl') and 'differ in B or L' in err()
    long_plan = _lib.Plan(3, 65, 16, forward_only=True)
    for a in (good(long_plan.handle, p(2000), long_plan.handle, p(2000)), good(*h(c3['t']), long_plan.handle, p(2000))):
        assert call(*a) != 0
        assert err().startswith('cliora_tree_kl') and 'the backward stops at 64 words' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                           # nothing was launched
    with pytest.raises(ValueError, match='the two charts differ'):
        structured.tree_kl(c3['t'], c7['s'])
    with pytest.raises(_lib.ChartLibError, match='kept no backward state'):
        structured.parse_kl(c3['t'], c3['s'])                      # _pair ran under no_grad
    with pytest.raises(_lib.ChartLibError, match='has run no forward'):
        structured.parse_kl(PC.text_module(PC.params(16, 1), 16), c3['s'])


# ---- 5. lengths -------------------------------------------------------------------------------------------------------------------
PADDED_W = ([0.7, 1.0, -2.0, 0.5], [-0.4, 0.5, 1.0, 2.0])


def test_padded_chart_is_each_sentence_alone():
    """lengths (5, 1, 2, 7) at L 7: each sentence gets the bits it gets alone at its own L, and every element beyond a triangle is zero."""
    from cliora_amd.structured import tree_kl_numpy
    t, s, xs = _padded()
    L, lengths = KC.RAGGED_L, list(KC.RAGGED_LENGTHS)
    got = _kl(t, s, *PADDED_W, lengths=lengths)
    assert got['status'] == [0]
    _against(got, tree_kl_numpy(_scores(t), _scores(s), lengths, *PADDED_W), L, 'padded')
    alone = [_module(PC.GPU_D, PC.MBR_PARAM_SEED), _module(PC.GPU_D, PC.MBR_PARAM_SEED + 3)]
    for b, n in enumerate(lengths):
        for G in (got['Gp'], got['Gq']):
            for level in range(1, L):
                assert not G[level][b, max(0, n - level):].any(), (b, level)  # beyond the triangle
        for m in alone:
            m.outside = False
            _forward(m, xs[b][None].cuda())
        one = _kl(alone[0], alone[1], PADDED_W[0][b:b + 1], PADDED_W[1][b:b + 1])
        assert one['status'] == [0]
        for k in SCALARS:
            assert np.array_equal(_bits(one[k]), _bits(got[k][b:b + 1])), (b, k)
        for key in ('Gp', 'Gq'):
            for level in range(1, n):
                assert np.array_equal(_bits(one[key][level][0]), _bits(got[key][level][b, :n - level])), (b, key, level)
    for key in ('Gp', 'Gq'):
        assert any(got[key][level][0].any() for level in range(1, L)) and any(got[key][level][3].any() for level in range(1, L))


def test_every_length_equal_to_L_is_the_call_without_lengths():
    B, L = 2, 13
    c = _pair(B, L, 48)
    a, b = _kl(c['t'], c['s'], [0.7] * B, [-0.4] * B, lengths=[L] * B), _kl(c['t'], c['s'], [0.7] * B, [-0.4] * B)
    assert a['status'] == [0] and a['flat_p'].any() and a['flat_q'].any()
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _poison(m, rows):
    """NaN into every per-split score of sentences `rows` in the module's forward workspace."""
    from cliora_amd import _lib
    plan, ws = m._plan, m._wss[0]
    wsf = ws.view(torch.float32)
    for level in range(1, plan.L):
        ps, ph, n, ldh = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.call('cliora_inside_pair_states', plan.handle, C.c_void_p(ws.data_ptr()), level, C.byref(ps), C.byref(ph), C.byref(n), C.byref(ldh))
        so = (ps.value - ws.data_ptr()) // 4
        wsf[so:so + n.value].view(plan.B, plan.L - level, level)[rows] = float('nan')


def test_bad_lengths_leave_their_neighbours_alone():
    t, xs = _padded_modules(PC.MBR_PARAM_SEED)         # this test's own charts: it writes NaN into them
    s, _ = _padded_modules(PC.MBR_PARAM_SEED + 3)
    L, lengths = KC.RAGGED_L, list(KC.RAGGED_LENGTHS)
    clean = _kl(t, s, *PADDED_W, lengths=lengths)
    nan = float('nan')
    _poison(t, [1, 2])
    _poison(s, [1, 2])                                 # the scores and the weights of a bad-length sentence are not read
    got = _kl(t, s, [0.7, nan, nan, 0.5], [-0.4, nan, nan, 2.0], lengths=[5, 0, 8, 7])
    assert got['status'] == [2]
    for k in SCALARS:
        assert got[k][1:3].tolist() == [0.0, 0.0], k
        assert np.array_equal(_bits(got[k][[0, 3]]), _bits(clean[k][[0, 3]])), k
    for key in ('Gp', 'Gq'):
        for level in range(1, L):
            assert not got[key][level][1:3].any()
            for b in (0, 3):
                assert np.array_equal(_bits(got[key][level][b]), _bits(clean[key][level][b])), (key, level, b)


# ---- 6. through the charts --------------------------------------------------------------------------------------------------------
NAMES = ('x_span', 'x_word', 'obj_span', 'obj_word')


def _oracle(Pt, t_inputs, Ps, s_inputs, share):
    """fp64: the oracle's per-split inside scores of both nets -> J = a mean kl + b mean cross_entropy by kl_cases.torch_kl,
    differentiated by autograd.  -> (J, the teacher's gradients, the student's), each {name: gradient or None}."""
    from oracle import diora_ref as R
    sides = []
    for P, inputs in ((Pt, t_inputs), (Ps, s_inputs)):
        P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
        t64 = [v.detach().double().requires_grad_(True) for v in inputs]
        o = R.diora_forward(P64, *t64, outside=True, normalize='unit', share=share, training=False, keep_pairs=True)
        sides.append((P64, t64, o['pair_s_in']))
    B, L = s_inputs[0].shape[:2]
    vals = [KC.torch_kl({lv: s[b, :, :, 0] for lv, s in sides[0][2].items()}, {lv: s[b, :, :, 0] for lv, s in sides[1][2].items()}, L)
            for b in range(B)]
    J = KC.A_KL * torch.stack([k for k, _ in vals]).mean() + KC.B_CE * torch.stack([c for _, c in vals]).mean()
    J.backward()
    out = []
    for P64, t64, _ in sides:
        grads = {k: v.grad for k, v in P64.items()}
        grads.update({name: v.grad for name, v in zip(NAMES, t64)})
        out.append(grads)
    return float(J.detach()), out[0], out[1]


def _run(m, inputs, grad=True):
    """One forward of `m` on fresh leaves of `inputs` (under no_grad without `grad`) -> the leaves."""
    for p in m.parameters():
        p.grad = None
    tg = [v.clone().cuda().requires_grad_(grad) for v in inputs]
    with torch.set_grad_enabled(grad):
        m(*((tg[0], tg[0]) if len(tg) == 1 else tg))
    return tg


def _grads(m, leaves):
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads.update({name: v.grad for name, v in zip(NAMES, leaves)})
    return grads


def _objective(t, s):
    kl, ce = s.parse_kl(t)
    return KC.A_KL * kl.mean() + KC.B_CE * ce.mean()


@pytest.mark.parametrize('B,L,D,share,teacher_trains', [(3, 6, 16, True, True), (2, 12, 80, True, False), (2, 6, 32, False, True)])
def test_objective_alone_against_the_oracle(B, L, D, share, teacher_trains, exact_mode):
    from oracle import diora_ref as R
    Pt, Ps = R.init_params(D, share=share, seed=21), R.init_params(D, share=share, seed=11)
    x = PC.batch(D, L, B, 700 + L)
    ref, want_t, want_s = _oracle(Pt, [x], Ps, [x], share)
    t, s = _text_module(Pt, D, share).train(), _text_module(Ps, D, share).train()
    lt, ls = _run(t, [x], grad=teacher_trains), _run(s, [x])
    J = _objective(t, s)
    J.backward()
    torch.cuda.synchronize()
    print('B %d L %d D %d: J %.6f, fp64 %.6f' % (B, L, D, float(J.detach()), ref))
    assert abs(float(J.detach()) - ref) <= KC.BOUND * max(1.0, abs(ref))
    _check(_grads(s, ls), want_s, 'student B %d L %d D %d' % (B, L, D))
    if teacher_trains:
        _check(_grads(t, lt), want_t, 'teacher B %d L %d D %d' % (B, L, D))
    else:
        assert all(p.grad is None for p in t.parameters()) and lt[0].grad is None
    assert t._wss.split_cot[0] is None and s._wss.split_cot[0] is None        # each chart node took its cotangent


def test_objective_alone_against_the_oracle_cliora_student(exact_mode):
    from oracle import diora_ref as R
    B, L, D, Rg = 2, 8, 32, 5
    Pt, Ps = R.init_params(D, share=True, seed=21), R.init_params(D, share=True, seed=12)
    gen = torch.Generator().manual_seed(13)
    inputs = [torch.randn(B, L, D, generator=gen), torch.randn(B, L, D, generator=gen), 0.3 * torch.randn(B, Rg, D, generator=gen),
              0.3 * torch.randn(B, Rg, D, generator=gen)]
    ref, _, want_s = _oracle(Pt, inputs[:1], Ps, inputs, True)
    t, s = _text_module(Pt, D, True).eval(), _vl_module(Ps, D)
    _run(t, inputs[:1], grad=False)
    ls = _run(s, inputs)
    J = _objective(t, s)
    J.backward()
    torch.cuda.synchronize()
    assert abs(float(J.detach()) - ref) <= KC.BOUND * max(1.0, abs(ref))
    _check(_grads(s, ls), want_s, 'CLIORA student')


def test_sums_with_other_losses_and_with_a_second_call(exact_mode):
    """On one forward of the student: a loss on the four chart outputs, bracket_nll, tree_objective and the divergence together give
    the sum of the four separate backward results; two parse_kl calls add up in the slot; the directions of parse_divergence."""
    from cliora_amd import structured
    from oracle import diora_ref as R
    B, L, D = 2, 12, 80
    x = PC.batch(D, L, B, 700 + L)
    t = _text_module(R.init_params(D, share=True, seed=21), D, True).eval()
    _run(t, [x], grad=False)
    m = _text_module(R.init_params(D, share=True, seed=11), D, True).train()
    req, forb = _lists(_case_sets(B, L))
    gen = torch.Generator().manual_seed(3)
    cot = {k: torch.randn(B, L * (L + 1) // 2, w, generator=gen).cuda() for k, w in (('inside_h', D), ('inside_s', 1), ('outside_h', D), ('outside_s', 1))}
    loss_a = lambda mm: sum((getattr(mm, k) * v).sum() for k, v in cot.items())
    nll = lambda mm: mm.bracket_nll(req, forb)
    ent = lambda mm: -1.3 * mm.parse_entropy()
    div = lambda mm: _objective(t, mm)
    parts = [_grads_of(m, x, f) for f in (loss_a, nll, ent, div)]
    gsum = _grads_of(m, x, lambda mm: loss_a(mm) + nll(mm) + ent(mm) + div(mm))
    assert all(set(g) == set(gsum) for g in parts)
    assert sum(int(float(g.abs().max()) > 1e-2) for g in parts[3].values()) >= 3
    for k in gsum:
        want = sum(g[k].double() for g in parts)
        sc = max(1.0, float(want.abs().max()))
        assert float((gsum[k].double() - want).abs().max()) <= KC.SUM_TOL * sc, k
    w1, w2 = torch.tensor([0.5, -1.0]).cuda(), torch.tensor([0.25, 3.0]).cuda()

    def twice(mm):
        k1, c1 = structured.parse_kl(t, mm)
        k2, c2 = structured.parse_kl(t, mm)
        return (k1 * w1).sum() + (c2 * w2).sum() + (k2 * w2).sum() + (c1 * w1).sum()

    def once(mm):
        k, c = structured.parse_kl(t, mm)
        return (k * (w1 + w2)).sum() + (c * (w1 + w2)).sum()
    same = lambda a, b: all(float((a[k] - b[k]).abs().max()) <= KC.SUM_TOL * max(1.0, float(b[k].abs().max())) for k in b)
    assert same(_grads_of(m, x, twice), _grads_of(m, x, once))
    # one cotangent alone: the other one is taken as zeros; the wrapper's directions
    fwd = _grads_of(m, x, lambda mm: mm.parse_divergence(t))
    assert same(_grads_of(m, x, lambda mm: mm.parse_kl(t)[0].mean() + 0.0 * mm.parse_kl(t)[1].mean()), fwd)
    rev = _grads_of(m, x, lambda mm: mm.parse_divergence(t, direction='reverse'))
    assert same(_grads_of(m, x, lambda mm: structured._kl_node(mm, t)[0].mean()), rev) and not same(rev, fwd)
    sym = _grads_of(m, x, lambda mm: mm.parse_divergence(t, direction='symmetric', reduction='sum'))
    assert same({k: (sym[k] / B) for k in sym}, {k: fwd[k] + rev[k] for k in fwd})


# ---- 7. training use --------------------------------------------------------------------------------------------------------------
def _teacher(hard=False):
    from cliora_amd.diora import DioraMLP
    torch.manual_seed(77)
    return DioraMLP(32, outside=True, hard=hard).cuda().eval()


def _net(**kw):
    from cliora_amd import harness as H
    torch.manual_seed(21)
    return H.build_net(32, torch.nn.Embedding(100, 32), k_neg=20, **kw).cuda()


def _train_batch():
    g = torch.Generator().manual_seed(22)
    return dict(sentences=torch.randint(0, 100, (8, 8), generator=g).cuda(), neg_samples=torch.randperm(100, generator=g)[:20].cuda())


def test_training_lowers_the_divergence_and_leaves_the_teacher_alone():
    from cliora_amd import harness as H
    from cliora_amd.structured import tree_kl
    teacher = _teacher()
    frozen = {k: v.detach().clone() for k, v in teacher.state_dict().items()}
    net = _net(teacher=teacher, kl_loss_weight=1.0)
    assert not any(k.startswith('teacher') for k in net.state_dict()) and teacher not in list(net.modules())
    ids = {id(p) for p in teacher.parameters()}
    assert not any(id(p) in ids for p in net.parameters())
    bm = _train_batch()

    def now():
        net.train()
        out = net(bm['sentences'], None, bm['neg_samples'])                    # runs the teacher on the same x_span
        assert 'kl' in out
        return float(tree_kl(teacher, net.diora).kl.mean())
    tr = H.Trainer(net)
    first = now()
    for _ in range(10):
        tr.step(bm)
    last = now()
    print('mean KL(teacher || student) over ten steps: %.4f -> %.4f' % (first, last))
    assert last < first
    assert not teacher.training and teacher.outside
    for k, v in teacher.state_dict().items():
        assert torch.equal(v, frozen[k]), k
    assert all(p.grad is None for p in teacher.parameters())


def test_weight_zero_is_the_plain_step_bit_for_bit():
    from cliora_amd import harness as H
    bm = _train_batch()
    runs = []
    for kw in ({}, dict(teacher=_teacher(), kl_loss_weight=0.0), dict(teacher=None, kl_loss_weight=1.0)):
        net = _net(**kw)
        tr = H.Trainer(net)
        losses = [tr.step(bm)['total_loss'] for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    for other in runs[1:]:
        assert runs[0][0] == other[0]
        for k, v in runs[0][1].items():
            assert torch.equal(v, other[1][k]), k


def test_step_ragged_reads_each_sentences_own_chart(exact_mode):
    """Lengths 5, 3, 8, 1 through padded packs: the kl the step's loss reads is tree_kl of each sentence's own chart; one step runs."""
    from cliora_amd import harness as H, ragged
    from cliora_amd.structured import tree_kl
    lengths = [5, 3, 8, 1]
    rs = np.random.RandomState(9)
    sentences = [rs.randint(1, 97, size=n).tolist() for n in lengths]
    neg = torch.from_numpy(rs.randint(1, 97, size=5)).cuda()
    teacher = _teacher()
    torch.manual_seed(31)
    net = H.build_net(32, torch.nn.Embedding(97, 32), k_neg=5, teacher=teacher, kl_loss_weight=1.0).cuda()
    net.train()
    packed, seen = {}, []
    hook = net.diora.register_forward_pre_hook(lambda _, args: seen.append(args))
    try:
        for idx, lens, diora in ragged.forward_ragged_train(net, sentences):
            net.run_teacher(*seen[-1])
            terms = dict(net.structured_losses(None, diora._plan.L, lens.device))
            res = tree_kl(teacher, diora)                                      # the lengths of the student's padded chart
            assert int(res.status.sum()) == 0
            assert abs(float(terms['kl'].detach()) - float(res.kl.mean())) <= 1e-6 * max(1.0, float(res.kl.mean()))
            packed.update(zip(idx, res.kl.cpu().tolist()))
    finally:
        hook.remove()
    assert sorted(packed) == [0, 1, 2, 3]
    net.eval()
    for i, sent in enumerate(sentences):                                       # each sentence alone at its own length
        with torch.no_grad():
            x_span, x_word = net.embed(torch.tensor([sent]).cuda())
            net.diora(x_span, x_word)
            teacher(x_span, x_word)
        want = float(tree_kl(teacher, net.diora).kl[0])
        assert abs(packed[i] - want) <= KC.BOUND * max(1.0, abs(want)), (i, packed[i], want)
    assert packed[3] == 0.0 and packed[2] > 1e-3
    loss = H.Trainer(net, lr=2e-3).step_ragged(sentences, neg_samples=neg)['total_loss']
    assert np.isfinite(loss) and all(bool(torch.isfinite(p).all()) for p in net.parameters())
    assert all(p.grad is None for p in teacher.parameters())


def test_a_hard_student_is_moved_by_the_divergence_alone():
    """Under the reconstruction loss alone a hard chart's score matrix gets an exactly zero gradient; with the KL term it moves."""
    from cliora_amd import harness as H
    bm = _train_batch()
    moved = {}
    for weight in (0.0, 1.0):
        net = _net(hard=True, teacher=_teacher(), kl_loss_weight=weight)
        before = net.diora.inside_score_func.mat.detach().clone()
        loss = H.Trainer(net).step(bm)['total_loss']
        assert np.isfinite(loss)
        moved[weight] = not torch.equal(before, net.diora.inside_score_func.mat.detach())
    assert moved == {0.0: False, 1.0: True}


# ---- 8. evaluation ----------------------------------------------------------------------------------------------------------------
def test_chart_divergence_is_the_mean_of_the_raw_calls():
    from cliora_amd import evaluate
    from cliora_amd.structured import tree_kl
    torch.manual_seed(5)
    from cliora_amd import harness as H
    a = H.build_net(32, torch.nn.Embedding(100, 32), k_neg=20).cuda()
    b = H.build_net(16, torch.nn.Embedding(100, 32), k_neg=20, hard=True).cuda()                 # another width, a hard chart
    g = torch.Generator().manual_seed(6)
    batches = [dict(sentences=torch.randint(0, 100, (4, 6), generator=g)), dict(sentences=torch.randint(0, 100, (3, 9), generator=g))]
    a.train()
    res = evaluate.chart_divergence(a, b, batches)
    assert a.training and a.diora.outside and b.diora.outside                  # modes and flags restored
    ab, ba = [], []
    for bm in batches:
        with torch.no_grad():
            for net in (a.eval(), b.eval()):
                net(bm['sentences'].cuda(), None, None, compute_loss=False)
        ab.append(tree_kl(a.diora, b.diora).kl.cpu().numpy())
        ba.append(tree_kl(b.diora, a.diora).kl.cpu().numpy())
    ab, ba = np.concatenate(ab), np.concatenate(ba)
    assert res['per_sentence_ab'].shape == (7,) and (ab > 1e-3).all()
    np.testing.assert_allclose(res['per_sentence_ab'], ab, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res['per_sentence_ba'], ba, rtol=1e-5, atol=1e-6)
    assert abs(res['kl_ab'] - ab.mean()) <= 1e-5 * max(1.0, ab.mean()) and abs(res['kl_ba'] - ba.mean()) <= 1e-5 * max(1.0, ba.mean())
    # the ragged variant: the same sentences in one call, in the caller's order
    sents = [row.tolist() for bm in batches for row in bm['sentences']]
    rag = evaluate.chart_divergence_ragged(a, b, sents)
    np.testing.assert_allclose(rag['per_sentence_ab'], ab, rtol=KC.BOUND, atol=KC.BOUND)
    np.testing.assert_allclose(rag['per_sentence_ba'], ba, rtol=KC.BOUND, atol=KC.BOUND)
