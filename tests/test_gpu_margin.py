"""The max-margin bracket losses on the GPU (cliora_amd/structured.py): cliora_bracket_margin alone, its ties
to cliora_cky_spans and cliora_constrained_parse, the loss through the chart's autograd node, and training steps.

The yardsticks, never the code under test: ``bracket_margin_numpy`` (pinned to enumeration and to central differences by
test_margin_cpu.py) on the device's OWN per-split scores for the kernel -- trees, violations, feasible and d_split exactly, the three
scalars to the rounding of one fp32 store; the existing entries, bitwise, for the two trees; the fp64 oracle with a torch restatement
of the tree score difference, teacher-forced by the device's two span lists, for the gradients through the chart.
Cases, bounds and measured figures: margin_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import constrained_cases as CC
import margin_cases as MC
import posterior_cases as PC
import structured_cases as SC
from test_gpu_constrained import _forward, _scores
from test_gpu_structured import _case_sets, _check, _grads_of, _lists, _sets, _tensor, _text_module, _vl_module, exact_mode  # noqa: F401

pytestmark = pytest.mark.gpu
INF = MC.INF


@functools.lru_cache(maxsize=None)
def _chart(B, L, D, mode):
    """One eval forward of a text-only DioraMLP (random weights) under the arithmetic mode and the device's scores -- once per shape."""
    m = PC.text_module(PC.params(D, PC.GPU_SEED), D).cuda().eval()
    _forward(m, PC.batch(D, L, B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m) if L > 1 else {})


def _margin(m, rows=None, margin=1.0, penalty=INF, weights=None, lengths=None, spans=True):
    """structured.bracket_margin with host inputs -> dict of numpy arrays: G {level: (B, L - level, level)}, flat, the scalars, spans."""
    from cliora_amd.structured import bracket_margin, split_rows_by_level
    wt = None if weights is None else torch.tensor(weights, dtype=torch.float32)
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    res = bracket_margin(m, _tensor(rows), margin, penalty, wt, lt, spans=spans)
    out = {k: getattr(res, k).cpu().numpy() for k in ('loss', 'aug_score', 'ref_score', 'violations', 'feasible')}
    out.update(G={lv: g.cpu().numpy() for lv, g in split_rows_by_level(m._plan, res.d_split).items()}, flat=res.d_split.cpu().numpy(),
               status=res.status.cpu().tolist(), spans_aug=res.spans_aug.cpu().numpy() if spans else None,
               spans_ref=res.spans_ref.cpu().numpy() if spans else None)
    return out


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, keys=('flat', 'loss', 'aug_score', 'ref_score', 'violations', 'feasible', 'spans_aug', 'spans_ref')):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _small_sets(B, L):
    """The bracket sets of one and two words: nothing, a forbidden leaf, a required leaf, and the root either way."""
    sets = {'none': [[]] * B, 'forbidden leaf': [[(0, 0, 0)]] * B, 'required leaf': [[(L - 1, L - 1, 1)]] * B}
    if L == 2:
        sets.update({'required root': [[(0, 1, 1)]] * B, 'forbidden root': [[(0, 1, 0)]] * B})
    return sets


def _against_the_restatement(m, scores, lengths, sets, what, worst):
    """Every set under every parameter pair: trees, violations, feasible and d_split exactly, the scalars to one fp32 rounding."""
    from cliora_amd.structured import bracket_margin_numpy
    L = m._plan.L
    positive = 0
    for name, per_sentence in sets.items():
        rows = CC.pack_rows(per_sentence)
        for margin, penalty in MC.PARAMS:
            got = _margin(m, rows, margin, penalty, lengths=None if lengths is None else list(lengths))
            want = bracket_margin_numpy(scores, [L] * len(per_sentence) if lengths is None else lengths, rows, margin, penalty)
            tag = (what, name, margin, penalty)
            assert got['status'] == [want.status] == [0], tag
            assert np.array_equal(got['spans_aug'], want.spans_aug) and np.array_equal(got['spans_ref'], want.spans_ref), tag
            assert np.array_equal(got['violations'], want.violations) and np.array_equal(got['feasible'], want.feasible), tag
            for level in range(1, L):
                assert torch.equal(torch.from_numpy(got['G'][level]), torch.from_numpy(want.d_split[level].astype(np.float32))), tag + (level,)
            for k, ref in (('loss', want.loss), ('aug_score', want.aug_score), ('ref_score', want.ref_score)):
                fin = np.isfinite(ref)
                assert np.array_equal(got[k][~fin], ref[~fin].astype(np.float32)), tag + (k,)
                err = float((np.abs(got[k][fin].astype(np.float64) - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()) if fin.any() else 0.0
                worst[k] = max(worst[k], err)
            assert (got['loss'] >= 0).all() and not np.signbit(got['loss']).any(), tag
            positive += int((got['loss'] > 0).any())
    return positive


# ---- 5. the kernel against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', MC.GPU_SHAPES)
def test_kernel_against_the_restatement(B, L, D, mfma_mode):
    c = _chart(B, L, D, mfma_mode)
    m, scores = c['m'], c['scores']
    sets = _sets(m, B, L) if L >= 3 else _small_sets(B, L)
    if L >= 3:                                          # structured_cases.bracket_sets, a seed per sentence, and the crossing pair
        per_seed = [SC.bracket_sets(L, b) for b in range(B)]
        sets.update({'cases: ' + name: [per_seed[b][name] for b in range(B)] for name in per_seed[0]})
        sets['crossing'] = [MC.crossing_pair(L)] * B
    worst =dict(loss=0.0, aug_score=0.0, ref_score=0.0)
    positive = _against_the_restatement(m, scores, None, sets, 'L %d' % L, worst)
    print('L %d %s: max relative |loss - fp64| %.3e, |aug - fp64| %.3e, |ref - fp64| %.3e (measured before: %s)'
          % (L, mfma_mode, worst['loss'], worst['aug_score'], worst['ref_score'], MC.MEASURED.get('L %d' % L)))
    for k, err in worst.items():
        assert err <= MC.SCALAR_RTOL, (k, err)
    assert positive >= 3 or L < 3                      # losses, not zeros


@functools.lru_cache(maxsize=None)
def _padded(mode):
    xs = [PC.sentence(PC.GPU_D, n, 5200 + b) for b, n in enumerate(MC.PADDED_LENGTHS)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, MC.PADDED_L).cuda())
    return m, _scores(m)


PADDED_SETS = {'mixed': [[], [(0, 1, 1)], [(1, 2, 1)], [(1, 3, 1), (1, 2, 0)], [(0, 2, 1), (3, 4, 1)]],
               'crossing and leaves': [[(0, 0, 0)], [(1, 1, 1)], [(0, 1, 1), (1, 2, 1)], [(0, 2, 1), (1, 3, 1)], [(2, 3, 0), (1, 4, 1)]]}


def test_padded_chart_against_the_restatement(mfma_mode):
    m, scores = _padded(mfma_mode)
    lengths = list(MC.PADDED_LENGTHS)
    worst = dict(loss=0.0, aug_score=0.0, ref_score=0.0)
    positive = _against_the_restatement(m, scores, lengths, PADDED_SETS, 'padded', worst)
    print('padded L %d %s: max relative errors %s' % (MC.PADDED_L, mfma_mode, worst))
    assert max(worst.values()) <= MC.SCALAR_RTOL and positive >= 2
    got = _margin(m, CC.pack_rows(PADDED_SETS['mixed']), 1.0, 1.0, lengths=lengths)
    for b, n in enumerate(lengths):
        for level in range(1, MC.PADDED_L):
            assert not got['G'][level][b, max(0, n - level):].any(), (b, level)          # beyond the triangle
        assert (got['spans_aug'][b, max(n - 1, 0):] == -1).all()


# ---- 6. bitwise ties to the existing entries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,L,D', SC.GPU_SHAPES)
def test_trees_are_those_of_the_existing_entries(B, L, D):
    from cliora_amd.constrained import constrained_parse
    m = _chart(B, L, D, 'bf16x3')['m']
    cky = m.cky_spans_device().cpu().numpy()
    sets = _sets(m, B, L)
    if L >= 4:
        sets['crossing'] = [MC.crossing_pair(L)] * B
    infeasible = 0
    for name, per_sentence in sets.items():
        rows = CC.pack_rows(per_sentence)
        cp = constrained_parse(m, _tensor(rows))
        for penalty in (INF, 1.0):
            got = _margin(m, rows, 0.0, penalty)
            assert np.array_equal(got['spans_aug'], cky), (name, penalty)            # margin 0: the CKY tree
        for margin in (0.0, 1.0):
            got = _margin(m, rows, margin, INF)
            assert np.array_equal(got['spans_ref'], cp.spans.cpu().numpy()) and np.array_equal(got['feasible'], cp.feasible.cpu().numpy()), name
            infeasible += int((got['feasible'] == 0).sum())
    assert infeasible > 0 or L < 4


def test_ragged_cky_tie_and_lengths_equal_to_L():
    from cliora_amd.ragged import cky_spans_ragged
    m, _ = _padded('bf16x3')
    lengths = list(MC.PADDED_LENGTHS)
    lt = torch.tensor(lengths, dtype=torch.int32)
    want = cky_spans_ragged(m, lt)
    want = (want[0] if isinstance(want, tuple) else want).cpu().numpy()
    from cliora_amd.constrained import constrained_parse
    for per_sentence in PADDED_SETS.values():
        rows = CC.pack_rows(per_sentence)
        got = _margin(m, rows, 0.0, INF, lengths=lengths)
        cp = constrained_parse(m, _tensor(rows), lt)
        assert np.array_equal(got['spans_aug'], want)
        assert np.array_equal(got['spans_ref'], cp.spans.cpu().numpy()) and np.array_equal(got['feasible'], cp.feasible.cpu().numpy())
    B, L = 2, 13
    m = _chart(B, L, 48, 'bf16x3')['m']
    rows = CC.pack_rows(_sets(m, B, L)['required+forbidden'])
    for margin, penalty in MC.PARAMS:
        a, b = _margin(m, rows, margin, penalty, lengths=[L] * B), _margin(m, rows, margin, penalty)
        assert a['status'] == [0]
        _same(a, b)
        _same(b, _margin(m, rows, margin, penalty))                                   # a second call
    assert a['flat'].any()


def test_zero_paths():
    B, L = 3, 7
    m = _chart(B, L, 16, 'bf16x3')['m']
    cky = m.cky_spans_device().cpu().numpy()
    for rows in (None, np.full((B, 4, 3), -1, dtype=np.int32), CC.pack_rows([[(0, L - 1, 1)], [(2, 2, 1)], [(0, 0, 1), (0, L - 1, 1)]])):
        for margin, penalty in MC.PARAMS:
            got = _margin(m, rows, margin, penalty, weights=[3.0, -2.0, float('nan')])
            assert not got['flat'].any() and not np.signbit(got['flat']).any()
            assert got['loss'].tolist() == [0.0] * B and not np.signbit(got['loss']).any()
            assert got['feasible'].tolist() == [1] * B and got['violations'].tolist() == [0] * B and got['status'] == [0]
            assert np.array_equal(got['spans_aug'], cky) and np.array_equal(got['spans_ref'], cky)
            assert np.array_equal(_bits(got['aug_score']), _bits(got['ref_score']))
    # the scalars without the span outputs are the same
    rows = CC.pack_rows(_sets(m, B, L)['nested'])
    _same(_margin(m, rows, spans=False), _margin(m, rows), keys=('flat', 'loss', 'aug_score', 'ref_score', 'violations', 'feasible'))


def test_nan_prefill_nan_weights_bad_rows_and_bad_lengths():
    """Through the C entry on a NaN-filled buffer: every element is written, nothing beyond it; an infeasible, a rejected and a short
    sentence get zeros whatever their weight; bad rows and bad lengths are counted once each; the neighbours keep their bits."""
    from cliora_amd import _lib
    m, _ = _padded('bf16x3')
    L, lengths = MC.PADDED_L, [1, 2, 3, 5, 5]
    sets = [[], [(0, 1, 1)], [(0, 1, 1), (1, 2, 1)], [(1, 3, 1), (1, 2, 0)], [(0, 2, 1), (3, 4, 1)]]
    clean = _margin(m, CC.pack_rows(sets, 3), 1.0, INF, lengths=lengths)
    assert clean['feasible'].tolist() == [1, 1, 0, 1, 1] and clean['status'] == [0]
    bad_sets = [list(s) for s in sets]
    bad_sets[1] = [(0, 1, 1), (1, 3, 1), (0, 0, 7)]                 # two bad rows in one sentence (an end in the padding, a bad kind): one count
    bad_lengths = list(lengths)
    bad_lengths[0] = 9                                              # a bad length
    rows = _tensor(CC.pack_rows(bad_sets, 3)).cuda()
    count = _lib.fn('cliora_plan_split_score_count')(m._plan.handle)
    assert count == 5 * sum(lv * (L - lv) for lv in range(1, L))
    buf = torch.full((count + 64,), float('nan'), device='cuda')
    w = torch.tensor([float('nan'), float('nan'), float('nan'), 1.0, 1.0], device='cuda')
    f = [torch.full((5,), float('nan'), device='cuda') for _ in range(3)]
    i = [torch.full((5,), -7, dtype=torch.int32, device='cuda') for _ in range(2)]
    status = torch.full((1,), 5, dtype=torch.int32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.call('cliora_bracket_margin', m._plan.handle, p(m._wss[0]), p(torch.tensor(bad_lengths, dtype=torch.int32).cuda()), p(rows), 3, 1.0, INF,
              p(w), p(buf), p(f[0]), p(f[1]), p(f[2]), p(i[0]), p(i[1]), None, None, p(status), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    host = buf.cpu().numpy()
    assert not np.isnan(host[:count]).any() and np.isnan(host[count:]).all()          # all of it, and nothing beyond it
    assert status.item() == 2 and i[1].cpu().tolist() == [0, 0, 0, 1, 1]
    assert f[0].cpu().tolist()[:3] == [0.0, 0.0, 0.0] and f[1].cpu().tolist()[:2] == [0.0, 0.0] and f[2].cpu().tolist()[:2] == [0.0, 0.0]
    assert np.isneginf(f[2].cpu().numpy()[2])
    from cliora_amd.structured import split_rows_by_level
    G = {lv: g.cpu().numpy() for lv, g in split_rows_by_level(m._plan, buf[:count]).items()}
    for level in range(1, L):
        assert not G[level][:3].any()
        assert np.array_equal(_bits(G[level][3:]), _bits(clean['G'][level][3:]))
    assert np.array_equal(_bits(f[0].cpu().numpy()[3:]), _bits(clean['loss'][3:])) and host[:count].any()


def test_256_rows_at_64_words():
    from cliora_amd.structured import bracket_margin_numpy
    B, L = 2, 64
    c = _chart(B, L, 32, 'bf16x3')
    m = c['m']
    per_sentence = []
    for b in range(B):                                  # 256 rows: nested required, forbidden pairs, repeats
        rows = [(s, e, 1) for s, e in CC.nested_required(L, b)] + [(p, p + 1, 0) for p in range(2, 60)]
        per_sentence.append((rows * 8)[:256])
    rows = CC.pack_rows(per_sentence)
    assert rows.shape[1] == 256
    for margin, penalty in ((1.0, INF), (0.5, 2.0)):
        got = _margin(m, rows, margin, penalty)
        want = bracket_margin_numpy(c['scores'], [L] * B, rows, margin, penalty)
        assert got['status'] == [0] and np.array_equal(got['spans_aug'], want.spans_aug) and np.array_equal(got['spans_ref'], want.spans_ref)
        assert np.array_equal(got['violations'], want.violations) and np.array_equal(got['feasible'], want.feasible)
        for level in range(1, L):
            assert np.array_equal(got['G'][level], want.d_split[level].astype(np.float32)), level
    assert got['flat'].any()


def test_refusals_on_the_device():
    from cliora_amd import _lib, structured
    m = _chart(3, 3, 16, 'bf16x3')['m']
    with pytest.raises(_lib.ChartLibError, match='cliora_bracket_margin: M outside 0..256'):
        structured.bracket_margin(m, torch.full((3, 257, 3), -1, dtype=torch.int32))
    with pytest.raises(_lib.ChartLibError, match='kept no backward state'):
        structured.bracket_margin_loss(m, None)          # _chart ran under no_grad
    lm = PC.text_module(PC.params(16, PC.GPU_SEED), 16).cuda().eval()
    _forward(lm, PC.batch(16, 65, 1, 5).cuda())
    for f in (structured.bracket_margin, structured.bracket_hinge):
        with pytest.raises(_lib.ChartLibError, match='the backward stops at 64 words'):
            f(lm, None)
    assert structured.bracket_violations(m, _tensor(CC.pack_rows([[(0, 1, 1)], [(1, 2, 1)], []]))).dtype == np.int32


# ---- 7. through the chart ---------------------------------------------------------------------------------------------------------
def _tree_splits(spans_row, n):
    """A span list of one sentence -> [(level, pos, split)]: the split of a constituent is where its two children meet."""
    have = set((int(s), int(e)) for s, e in spans_row if s >= 0) | set((p, p) for p in range(n))
    out = []
    for s, e in sorted(have):
        if e > s:
            ks = [k for k in range(e - s) if (s, s + k) in have and (s + k + 1, e) in have]
            assert len(ks) == 1, (s, e, ks)
            out.append((e - s, s, ks[0]))
    assert len(out) == n - 1
    return out


def _oracle_hinge(P, inputs, trees, share):
    """fp64: the oracle's per-split inside scores -> the mean over the feasible sentences of sum_{aug} r - sum_{ref} r + the constant
    cost terms, teacher-forced by the device's two trees, differentiated by autograd.  trees: per sentence (aug splits, ref splits or
    None, the constant)."""
    from oracle import diora_ref as R
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
    t64 = [v.detach().double().requires_grad_(True) for v in inputs]
    o = R.diora_forward(P64, *t64, outside=True, normalize='unit', share=share, training=False, keep_pairs=True)
    total, feasible = 0.0, 0
    for b, (aug, ref, const) in enumerate(trees):
        if ref is None:
            continue
        feasible += 1
        r = {lv: s[b, :, :, 0] - s[b, :, :, 0].max(dim=1, keepdim=True).values for lv, s in o['pair_s_in'].items()}
        total = total + sum(r[lv][pos, k] for lv, pos, k in aug) - sum(r[lv][pos, k] for lv, pos, k in ref) + const
    loss = total / max(feasible, 1)
    loss.backward()
    grads = {k: v.grad for k, v in P64.items()}
    grads.update({name: v.grad for name, v in zip(('x_span', 'x_word', 'obj_span', 'obj_word'), t64)})
    return float(loss.detach()), grads


def _device_hinge(m, inputs, sets, margin, penalty):
    """bracket_hinge alone through the module -> (loss, gradients by the oracle's names, the device's trees for _oracle_hinge)."""
    from cliora_amd import structured
    from cliora_amd.constrained import pack_brackets
    for p in m.parameters():
        p.grad = None
    tg = [v.clone().cuda().requires_grad_(True) for v in inputs]
    m(*((tg[0], tg[0]) if len(tg) == 1 else tg))
    req, forb = _lists(sets)
    raw = structured.bracket_margin(m, pack_brackets(req, forb), margin, penalty, spans=True)
    loss = m.bracket_hinge(req, forb, margin=margin, penalty=penalty)
    loss.backward()
    torch.cuda.synchronize()
    n = inputs[0].shape[1]
    sa, sr, feas, viol, each = (t.cpu().numpy() for t in (raw.spans_aug, raw.spans_ref, raw.feasible, raw.violations, raw.loss))
    trees = []
    for b in range(len(sets)):
        if not feas[b]:
            trees.append((None, None, 0.0))
            continue
        aug, ref = _tree_splits(sa[b], n), _tree_splits(sr[b], n)
        d_ref = sum(MC.disallowed((p, p + lv), sets[b]) for lv, p, _ in ref if 1 <= lv <= n - 2)
        trees.append((aug, ref, margin * float(viol[b]) + (penalty * d_ref if d_ref else 0.0)))
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads.update({name: v.grad for name, v in zip(('x_span', 'x_word', 'obj_span', 'obj_word'), tg)})
    return float(loss.detach()), grads, trees, each


def _through_the_chart(P, m, inputs, sets, share, what):
    moved = 0
    for margin, penalty in ((1.0, INF), (0.5, 2.0)):
        loss, got, trees, each = _device_hinge(m, inputs, sets, margin, penalty)
        ref_loss, want = _oracle_hinge(P, inputs, trees, share)
        print('%s margin %g penalty %g: hinge %.6f (fp64 %.6f), per sentence %s' % (what, margin, penalty, loss, ref_loss, each.tolist()))
        assert abs(loss - ref_loss) <= PC.BOUND * max(1.0, abs(ref_loss))
        if (each > 0).any():
            _check(got, want, '%s %g %g' % (what, margin, penalty))
            moved += 1
    assert moved >= 1, what


@pytest.mark.parametrize('B,L,D,share', [(3, 6, 16, True), (2, 12, 80, True), (2, 6, 32, False)])
def test_hinge_alone_against_the_oracle(B, L, D, share, exact_mode):
    from oracle import diora_ref as R
    P = R.init_params(D, share=share, seed=11)
    _through_the_chart(P, _text_module(P, D, share).train(), [PC.batch(D, L, B, 700 + L)], _case_sets(B, L), share, 'B %d L %d D %d' % (B, L, D))


def test_hinge_alone_against_the_oracle_cliora(exact_mode):
    from oracle import diora_ref as R
    B, L, D, Rg = 2, 8, 32, 5
    P = R.init_params(D, share=True, seed=12)
    gen = torch.Generator().manual_seed(13)
    inputs = [torch.randn(B, L, D, generator=gen), torch.randn(B, L, D, generator=gen), 0.3 * torch.randn(B, Rg, D, generator=gen),
              0.3 * torch.randn(B, Rg, D, generator=gen)]
    _through_the_chart(P, _vl_module(P, D), inputs, _case_sets(B, L), True, 'CLIORA')


def test_sums_with_another_loss(exact_mode):
    from oracle import diora_ref as R
    B, L, D = 2, 12, 80
    P = R.init_params(D, share=True, seed=11)
    x = PC.batch(D, L, B, 700 + L)
    m = _text_module(P, D, True).train()
    req, forb = _lists(_case_sets(B, L))
    gen = torch.Generator().manual_seed(3)
    cot = {k: torch.randn(B, L * (L + 1) // 2, w, generator=gen).cuda() for k, w in (('inside_h', D), ('inside_s', 1), ('outside_h', D), ('outside_s', 1))}
    loss_a = lambda mm: sum((getattr(mm, k) * v).sum() for k, v in cot.items())
    hinge = lambda mm: mm.bracket_hinge(req, forb, margin=1.0)
    both = lambda mm: loss_a(mm) + hinge(mm) + mm.bracket_nll(req, forb)               # the slot sums the two bracket losses too
    nll = lambda mm: mm.bracket_nll(req, forb)
    ga, gb, gc, gsum = _grads_of(m, x, loss_a), _grads_of(m, x, hinge), _grads_of(m, x, nll), _grads_of(m, x, both)
    assert set(ga) == set(gb) == set(gsum) and any(float(g.abs().max()) > 1e-2 for g in gb.values())
    for k in gsum:
        want = ga[k].double() + gb[k].double() + gc[k].double()
        sc = max(1.0, float(want.abs().max()))
        assert float((gsum[k].double() - want).abs().max()) <= MC.SUM_TOL * sc, k


def test_a_hard_chart_is_moved_by_the_hinge_alone(exact_mode):
    from cliora_amd.diora import DioraMLP
    from oracle import diora_ref as R
    B, L, D = 3, 6, 16
    P = R.init_params(D, share=True, seed=11)
    m = DioraMLP(D, share=True, normalize='unit', outside=True, hard=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    m = m.cuda().train()
    x = PC.batch(D, L, B, 700 + L)
    req, forb = _lists(_case_sets(B, L))
    cot = torch.randn(B, L * (L + 1) // 2, D, generator=torch.Generator().manual_seed(3)).cuda()
    recon = lambda mm: (mm.outside_h * cot).sum()          # what the reconstruction loss reads
    without = _grads_of(m, x, recon)
    with_hinge = _grads_of(m, x, lambda mm: recon(mm) + mm.bracket_hinge(req, forb, margin=1.0))
    key = 'inside_score_func.mat'
    assert key not in without or not without[key].any()    # exactly zero
    assert float(with_hinge[key].abs().max()) > 1e-3


def test_a_padded_training_chart_keeps_the_padding_at_zero(mfma_mode):
    import ragged_outside_cases as ROC
    from test_gpu_parity import _module_from_params
    from test_gpu_ragged_train import _forward as ragged_forward
    lengths = [2, 3, 4, 5, 6]
    P, xs, _ = ROC.small_case(32, lengths, seed=941)
    m = _module_from_params(P, 32, True, 'unit').train()
    x = ROC.padded(xs, max(lengths)).clone().cuda().requires_grad_(True)
    ragged_forward(m, x, lengths)
    req = [[], [(0, 1)], [(1, 2)], [(1, 3)], [(1, 4), (2, 3)]]
    forb = [[], [], [], [(1, 2)], [(3, 4)]]
    loss = m.bracket_hinge(req, forb, margin=1.0, penalty=2.0)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) > 0 and float(x.grad.abs().max()) > 1e-3
    for b, n in enumerate(lengths):
        assert not x.grad[b, n:].any(), b


# ---- 8. training use --------------------------------------------------------------------------------------------------------------
def _net(**kw):
    from cliora_amd import harness as H
    torch.manual_seed(21)
    return H.build_net(32, torch.nn.Embedding(100, 32), k_neg=20, **kw).cuda()


def _train_batch():
    g = torch.Generator().manual_seed(22)
    labels = [[('np', 1, 3), ('np', 5, 2)], [('np', 0, 2), ('vp', 2, 5), None], [('np', 3, 4)], [('np', 0, 3), ('np', 1, 2), ('x', 7, 1)]] * 2
    return dict(sentences=torch.randint(0, 100, (8, 8), generator=g).cuda(), neg_samples=torch.randperm(100, generator=g)[:20].cuda(),
                entity_labels=labels)


@pytest.mark.parametrize('penalty', [INF, 2.0])
def test_training_lowers_the_hinge(penalty):
    from cliora_amd import harness as H
    from cliora_amd.constrained import brackets_from_entity_labels
    net, bm = _net(hinge_loss_weight=1.0, hinge_penalty=penalty), _train_batch()
    req = brackets_from_entity_labels(bm['entity_labels'], drop_crossing=penalty == INF)

    def hinge_now():
        net.train()
        out = net(bm['sentences'], None, bm['neg_samples'])
        assert 'hinge' not in out                       # the labels were not passed: the plain step's losses
        return float(net.diora.bracket_hinge(req, penalty=penalty).detach())
    tr = H.Trainer(net)
    first = hinge_now()
    for _ in range(10):
        tr.step(bm)
    last = hinge_now()
    print('mean hinge over ten steps (penalty %g): %.4f -> %.4f (measured before: %s)' % (penalty, first, last, MC.MEASURED_TRAINING))
    assert first > 0 and last < first


@pytest.mark.parametrize('hard', [False, True])
def test_step_ragged_takes_the_hinge(hard):
    """Mixed lengths through one padded chart: the hinge joins the pack's loss, and on a hard net it alone moves the score matrix."""
    from cliora_amd import harness as H
    lengths = [7, 1, 3, 2, 6, 3, 5, 4, 7]
    rs = np.random.RandomState(9)
    sentences = [rs.randint(1, 97, size=n).tolist() for n in lengths]
    labels = [[('np', 0, 2), ('np', 1, n - 1)] if n >= 4 else [] for n in lengths]      # crossing from five words on: the ramp keeps both
    neg = torch.from_numpy(rs.randint(1, 97, size=5)).cuda()
    losses, moved = {}, {}
    for weight in (0.0, 1.0):
        torch.manual_seed(31)
        net = H.build_net(32, torch.nn.Embedding(97, 32), k_neg=5, hard=hard, hinge_loss_weight=weight, hinge_penalty=2.0).cuda()
        before = net.diora.inside_score_func.mat.detach().clone()
        losses[weight] = H.Trainer(net, lr=2e-3).step_ragged(sentences, neg_samples=neg, entity_labels=labels)['total_loss']
        assert np.isfinite(losses[weight]) and all(bool(torch.isfinite(p).all()) for p in net.parameters())
        moved[weight] = not torch.equal(before, net.diora.inside_score_func.mat.detach())
    assert losses[1.0] > losses[0.0] and moved[1.0]
    assert moved[0.0] == (not hard)                      # a hard chart's selection carries no gradient: only a loss on the scores moves M


def test_weight_zero_is_the_plain_step_bit_for_bit():
    from cliora_amd import harness as H
    bm = _train_batch()
    runs = []
    for kw in ({}, dict(hinge_loss_weight=0.0, hinge_margin=2.0, hinge_penalty=1.0)):
        net = _net(**kw)
        tr = H.Trainer(net)
        losses = [tr.step(bm)['total_loss'] for _ in range(3)]
        runs.append((losses, {k: v.detach().clone() for k, v in net.state_dict().items()}))
    assert runs[0][0] == runs[1][0]
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k
