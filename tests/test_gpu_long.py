"""Sentences of 65 .. 128 words on the device: forward-only plans (include/cliora_chart.h), checked against the fp64 oracle.

Cases, bounds and the measured figures live in long_cases.py.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

import long_cases as LC
import ragged_cases as RC

pytestmark = pytest.mark.gpu


def _run(m, x, vl=None):
    with torch.no_grad():
        if vl is None:
            xg = x.cuda()
            m(xg, xg)
        else:
            m(x.cuda(), vl[0].cuda(), vl[1].cuda(), vl[2].cuda())


def _charts(m, vl):
    keys = ('inside_h', 'inside_s', 'outside_h', 'outside_s') + (('atten_score',) if vl else ())
    out = {}
    for k in keys:
        a = getattr(m, k).detach().float().cpu().numpy()
        out[k] = a
    return out


@pytest.mark.parametrize('L', LC.LENGTHS)
@pytest.mark.parametrize('D', [50, 400])
@pytest.mark.parametrize('variant', ['text', 'cliora'])
def test_forward_parity_against_fp64(mfma_mode, variant, D, L):
    """All four charts (and atten_score of the CLIORA module) within the project's forward bound of the fp64 oracle.

    Measured on the MI355X: see long_cases.MEASURED_FWD_FRACTION and DESIGN.md section 14."""
    P, x, vl = LC.forward_case(variant, D, L)
    want = LC.forward_oracle(variant, D, L)
    m = (LC.vl_module(P, D) if vl is not None else LC.text_module(P, D)).cuda().eval()
    _run(m, x, vl)
    got = _charts(m, vl is not None)
    worst = {}
    for k, w in want.items():
        g = got[k].reshape(w.shape)
        assert np.isfinite(g).all(), k
        scale = max(1.0, float(np.abs(w).max()))
        worst[k] = float(np.abs(g - w).max()) / scale
    print('LONG_FWD variant=%s D=%d L=%d mode=%s %s' % (variant, D, L, mfma_mode, ' '.join('%s=%.3e' % kv for kv in sorted(worst.items()))))
    for k, e in worst.items():
        assert e <= LC.FORWARD_BOUND, (k, e)


def test_normalize_none_is_finite_and_shaped():
    """normalize = 'none' on a long chart: the reference's own fp32 run is 2e-3 from fp64 there (tools/regimes.py), so finiteness and
    shapes only."""
    D, L, B = 50, 65, 2
    P = LC.params(D, 4401, scale=0.05)
    x = torch.stack([LC.sentence(D, L, 4402 + b) for b in range(B)])
    m = LC.text_module(P, D, normalize='none').cuda().eval()
    _run(m, x)
    C = L * (L + 1) // 2
    for k, shape in (('inside_h', (B, C, D)), ('inside_s', (B, C, 1)), ('outside_h', (B, C, D)), ('outside_s', (B, C, 1))):
        a = getattr(m, k)
        assert tuple(a.shape) == shape and bool(torch.isfinite(a).all()), k
    assert len(m.cky()) == B


def _device_gap(pair_s, b, L):
    return RC.cky_margin({lv: s[b:b + 1] for lv, s in pair_s.items()}, L)


@pytest.mark.parametrize('L', LC.LENGTHS)
def test_trees_equal_the_oracles(L):
    """cky() == the oracle's CKY on its fp64 per-split scores, sentence by sentence; cky_spans_device() and cliora_cky_decode agree
    with cky().  A sentence is excused only if the DEVICE's own candidates tie within NEAR_TIE[L] in some cell; at most 2 %."""
    from cliora_amd import _lib
    from cliora_amd.diora import _ptr, _stream
    assert LC.TREE_SEEDS[L], 'no seeded sentences for L = %d' % L
    P, x = LC.tree_case(L)
    want = LC.tree_oracle(L)
    m = LC.text_module(P, LC.TREE_D).cuda().eval()
    prev = _lib.set_mfma_mode(LC.TREE_MODE)          # the exact-product mode: long_cases.py says why
    try:
        _run(m, x)
    finally:
        _lib.set_mfma_mode(prev)
    got = m.cky()
    err = float(np.abs(m.chart.inside_s[:, :, 0].cpu().numpy() - want['inside_s']).max())
    print('LONG_TREES L=%d inside_s_err=%.3e min_fp64_gap=%.3e near_tie=%.3e' % (L, err, min(want['gaps']), LC.NEAR_TIE[L]))
    assert 4 * err <= min(want['gaps']), 'the seeds no longer clear four times the device error'
    spans = m.cky_spans_device()
    assert spans.shape == (x.shape[0], L - 1, 2) and spans.dtype == torch.int32
    assert [str(t) for t in m.trees_from_spans(spans.cpu().numpy())] == [str(t) for t in got]
    split = torch.empty((x.shape[0], m._plan.C), dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().cliora_cky_decode(m._plan.handle, _ptr(m._wss[0]), _ptr(split), _stream()), 'cliora_cky_decode')
    split = split.cpu().numpy()
    assert (split[:, :L] == -1).all() and (split[:, L:] >= 0).all()
    pair_s = LC.device_split_scores(m)
    excused = 0
    for b in range(x.shape[0]):
        if str(got[b]) == str(want['trees'][b]):
            continue
        assert _device_gap(pair_s, b, L) < LC.NEAR_TIE[L], (L, b)
        excused += 1
    assert excused <= LC.MAX_EXCUSED * x.shape[0], excused


def test_length_64_is_bitwise_on_both_cky_entry_points():
    """L = 64, the largest plan with a backward: the uniform entry points and the ragged decode (every length 64) agree bit for bit,
    spans and splits; the forward of an eval call equals the forward of a training-mode call (the two flag sets of one plan)."""
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import _ptr, _stream
    D, B, L = 50, 3, 64
    P = LC.params(D, 6601)
    x = torch.stack([LC.sentence(D, L, 6602 + b) for b in range(B)])
    m = LC.text_module(P, D).cuda().eval()
    _run(m, x)
    assert m._plan.bwd_bytes > 0
    keys = ('inside_h', 'inside_s', 'outside_h', 'outside_s')
    ev = {k: getattr(m, k).clone() for k in keys}
    want = m.cky_spans_device().clone()
    want_split = torch.empty((B, m._plan.C), dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().cliora_cky_decode(m._plan.handle, _ptr(m._wss[0]), _ptr(want_split), _stream()), 'cliora_cky_decode')
    spans, status, split = ragged.cky_spans_ragged(m, torch.full((B,), L, dtype=torch.int32).cuda(), split_out=True)
    assert status.cpu().tolist() == [0]
    assert torch.equal(spans, want) and torch.equal(split, want_split)
    m.train()
    xg = x.cuda()
    m(xg, xg)
    for k in keys:
        assert torch.equal(getattr(m, k).detach(), ev[k]), k
    assert torch.equal(m.cky_spans_device(), want)


def _net(D, V=97, E=32, seed=11):
    from cliora_amd.harness import build_net
    torch.manual_seed(seed)
    return build_net(D, torch.nn.Embedding(V, E), obj_feats=False).cuda()


def _sentences(lengths, V=97, seed=5):
    rs = np.random.RandomState(seed)
    return [rs.randint(1, V, size=n).tolist() for n in lengths]


def test_parse_ragged_max_len_128_equals_the_uniform_trees():
    """Every tree of parse_ragged(max_len=128) equals cky() of the same sentence on a batch of one at its exact length; a sentence may
    differ only on a near-tie of the uniform path's own candidates (the rule of test_gpu_ragged.py), at most 2 %."""
    from cliora_amd import ragged
    net = _net(50)
    sents = _sentences(LC.RAGGED_LENGTHS)
    got = ragged.parse_ragged(net, sents, max_batch=4, max_len=128)
    net.eval()
    excused = 0
    with torch.no_grad():
        for i, s in enumerate(sents):
            net(torch.tensor([s]).cuda(), compute_loss=False)
            want = net.diora.cky()[0]
            if str(got[i]) == str(want):
                continue
            n = len(s)
            tie = 4 * (LC.MEASURED_INSIDE_S_ERR[128] if n > 64 else RC.MEASURED_INSIDE_S_DIFF)
            assert _device_gap(LC.device_split_scores(net.diora), 0, n) < tie, (i, n)
            excused += 1
    print('LONG_RAGGED excused=%d of %d' % (excused, len(sents)))
    assert excused <= LC.MAX_EXCUSED * len(sents)


def test_encode_ragged_max_len_128_rows_are_the_exact_length_roots():
    from cliora_amd import ragged
    net = _net(50)
    sents = _sentences(LC.RAGGED_LENGTHS, seed=6)
    got = ragged.encode_ragged(net, sents, max_batch=4, max_len=128).cpu().numpy()
    assert got.shape == (len(sents), 50)
    net.eval()
    worst = 0.0
    with torch.no_grad():
        for i, s in enumerate(sents):
            net(torch.tensor([s]).cuda(), compute_loss=False)
            want = net.diora.chart.inside_h[0, -1].cpu().numpy()
            err = float(np.abs(got[i] - want).max()) / max(1.0, float(np.abs(want).max()))
            worst = max(worst, err)
            assert err <= LC.FORWARD_BOUND, (i, len(s), err)
    print('LONG_ENCODE worst=%.3e' % worst)


def test_device_refusals_on_a_long_plan():
    """Each refusal of include/cliora_chart.h for 64 < L <= 128 reaches Python as a ChartLibError that says why, before any launch."""
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import DioraMLP
    D, L = 16, 65
    x = torch.randn(2, L, D).cuda()
    m = DioraMLP(D).cuda()
    with pytest.raises(_lib.ChartLibError, match='inference only'):
        m(x, x)                                     # training mode
    m.eval()
    with pytest.raises(_lib.ChartLibError, match='inference only'):
        m(x, x)                                     # eval mode, but the parameters still want gradients
    with torch.no_grad():
        m(x, x)
    assert m._plan.bwd_bytes == 0 and m._plan.pair_bytes == 0
    c = DioraMLP(D, compress=True).cuda().eval()
    with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='compress'):
        c(x, x)
    h = DioraMLP(D).cuda().eval()
    h.inside_hook = lambda level, hh, cc, ss: None
    with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='per-pair'):
        h(x, x)
    prev = _lib.set_resident('on')
    try:
        with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='resident'):
            m(x, x)
    finally:
        _lib.set_resident(prev)
    net = _net(50)
    with pytest.raises(_lib.ChartLibError, match='L > 64'):
        ragged.forward_ragged(net, _sentences([5, 65]))
    with pytest.raises(_lib.ChartLibError, match='L > 128'):
        ragged.parse_ragged(net, _sentences([5, 129]), max_len=128)


def _e2e_batch(L=80, B=3):
    import ragged_outside_cases as RO
    ex = RO.examples([L] * B, seed=17)
    bm = dict(sentences=torch.tensor([e['sentence'] for e in ex]), obj_feats=torch.stack([e['obj_feats'] for e in ex]),
              boxes=torch.stack([e['boxes'] for e in ex]), neg_samples=torch.randint(1, 97, (100,), generator=torch.Generator().manual_seed(3)),
              VG_GT=[e['VG_GT'] for e in ex], GT=[e['GT'] for e in ex], example_ids=[e['example_id'] for e in ex])
    return RO.vl_net().cuda(), bm


def test_evaluate_end_to_end_at_length_80():
    """evaluate.evaluate on one batch of 80-word sentences: the four metrics equal those of the torch restatement of the selection
    rule (tests/test_gpu_eval.py's helpers) applied to the module's own attention scores and spans."""
    from test_gpu_eval import _torch_iou, _torch_select
    from cliora_amd.evaluate import Evaluator, METRICS, Targets, evaluate
    net, bm = _e2e_batch()
    B, L = bm['sentences'].shape
    got = evaluate(net, [bm], {i: 'w%d' % i for i in range(97)})
    assert all(np.isfinite(got[k]) for k in METRICS)
    d = net.diora
    att, spans = d.atten_score, d.cky_spans()
    boxes = bm['boxes'].cuda()
    tg = Targets(bm['VG_GT'], bm['GT'], B, L)
    want = Evaluator()
    hits, ccrs = [], []
    for k, (b, s, e) in enumerate(tg.phrases):
        w, box = _torch_select(att[b], s, e)
        hit = int(bool(_torch_iou(boxes[b, box], torch.tensor(tg.phr_box[k]).cuda()) > 0.5))
        pred = set(map(tuple, spans[b][:-1].tolist()))
        hits.append(hit)
        ccrs.append(int(bool(hit) and (e - 1 == s or (s, e - 1) in pred)))
    sent = []
    for b in range(B):
        pred, gold = set(map(tuple, spans[b][:-1].tolist())), set(tg.gold[b])
        sent.append((len(pred & gold), len(pred), len(gold)))
    want.add_counts(sent, hits, ccrs)
    wr = want.result()
    for k in METRICS[:4]:
        assert got[k] == wr[k], (k, got[k], wr[k])


def test_embed_phrases_at_length_80():
    """phrases.embed_phrases ('all-spans') on one batch of 80-word sentences: every row is [inside_h | outside_h] of its cell, by
    torch indexing of the module's charts (tests/test_gpu_phrases.py's cell offset)."""
    from test_gpu_phrases import _offset
    from cliora_amd.phrases import embed_phrases
    net, bm = _e2e_batch()
    B, L = bm['sentences'].shape
    pset = embed_phrases(net, [bm], 'all-spans')
    d = net.diora
    assert len(pset) == B * (L * (L + 1) // 2)
    rs = np.random.RandomState(2)
    for i in rs.choice(len(pset), size=200, replace=False).tolist() + [len(pset) - 1]:
        b = bm['example_ids'].index(pset.example_ids[i])
        cell = _offset(L, pset.sizes[i]) + pset.positions[i]
        want = torch.cat([d.inside_h[b, cell], d.outside_h[b, cell]])
        assert torch.equal(pset.vectors[i], want), i
