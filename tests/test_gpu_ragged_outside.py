"""Both passes of mixed-length batches on the device (cliora_chart_forward_ragged, cliora_ground_eval_ragged and the Python built on
them).  The yardstick is the oracle run on one sentence at its exact length (ragged_outside_cases.exact), at the project's forward
bound; bitwise claims are against the existing entries of the library."""
import ctypes as C

import numpy as np
import pytest
import torch

import ragged_cases as RC
import ragged_outside_cases as ROC

pytestmark = pytest.mark.gpu


def _module(P, D, share=True, normalize='unit', vl=False):
    from cliora_amd import cliora, diora
    cls = cliora.DioraMLP if vl else diora.DioraMLP
    m = cls(D, outside=True, normalize=normalize, compress=False, share=share)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if (not share or not k.startswith('outside_')) else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    return m.cuda().eval()


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32).cuda()


def _ragged_run(m, xp, lengths, vl=None, mask=None):
    """The module's eval forward through cliora_chart_forward_ragged; -> status word on the host."""
    from cliora_amd import ragged
    m._ragged = (_lens(lengths), ragged.root_level_mask(lengths) if mask is None else mask)
    try:
        with torch.no_grad():
            if vl is None:
                m(xp, xp)
            else:
                m(xp, vl[0], vl[1], vl[2])
    finally:
        m._ragged = None
    return int(m._ragged_status.item())


def _charts(m):
    ch = m.chart
    return [t.clone() for t in (ch.inside_h, ch.inside_s, ch.outside_h, ch.outside_s)]


def _compare(m, P, xs, lengths, Lmax, normalize='unit', share=True, vl=None, what=''):
    """Every sentence, every cell of its triangle, inside_h / outside_h / outside_s (and atten_score[b, :n]) against the oracle at the
    exact length, at FORWARD_BOUND * max(1, |want|); prints the measured maxima first."""
    ih, _, oh, os_ = [t.cpu().double() for t in _charts(m)]
    att = m.atten_score.cpu().double() if vl is not None else None
    worst = dict(inside_h=0.0, outside_h=0.0, outside_s=0.0, atten_score=0.0)
    fails = []
    for b, n in enumerate(lengths):
        want = ROC.exact(P, xs[b], normalize, share, vl=vl[b] if vl is not None else None)
        own = torch.from_numpy(ROC.own_cells(Lmax, n))
        pairs = [('inside_h', ih[b, own], want['inside_h'][0]), ('outside_h', oh[b, own], want['outside_h'][0]),
                 ('outside_s', os_[b, own], want['outside_s'][0])]
        if vl is not None:
            pairs.append(('atten_score', att[b, :n], want['atten_score'][0]))
        for name, got, w in pairs:
            assert bool(torch.isfinite(got).all()), (name, b, n)
            err = float(((got - w).abs() / w.abs().clamp(min=1.0)).max())
            worst[name] = max(worst[name], err)
            if err > ROC.FORWARD_BOUND:
                fails.append((name, b, n, err))
    print('%s worst relative errors: %s' % (what, ', '.join('%s %.3e' % kv for kv in worst.items())))
    assert not fails, fails[:8]


@pytest.mark.parametrize('D', sorted(RC.CASES))
def test_forward_ragged_matches_the_oracle_at_the_exact_length(D, mfma_mode):
    from cliora_amd import ragged
    P, xs, lengths = RC.case(D)
    m = _module(P, D)
    xp = RC.padded(xs).cuda()
    # the inside-only forward of the padded batch first: its trees are what the new forward must leave unchanged
    m.outside = False
    with torch.no_grad():
        m(xp, xp)
    m.outside = True
    spans0, st0 = ragged.cky_spans_ragged(m, _lens(lengths))
    spans0 = spans0.clone()
    assert _ragged_run(m, xp, lengths) == 0
    first = _charts(m)
    spans1, st1 = ragged.cky_spans_ragged(m, _lens(lengths))
    assert st0.item() == 0 and st1.item() == 0 and torch.equal(spans0, spans1)          # the decode reads Sp, not inside_s
    _compare(m, P, xs, lengths, RC.LMAX, what='D %d %s' % (D, mfma_mode))
    own_masked = m.chart.inside_s[:, :, 0].cpu().numpy()
    for b, n in enumerate(lengths):                                                   # the documented state of inside_s
        beyond = np.setdiff1d(np.arange(own_masked.shape[1]), ROC.own_cells(RC.LMAX, n))
        assert (own_masked[b, beyond] == np.float32(ROC.MASKED)).all()
    assert _ragged_run(m, xp, lengths) == 0                                           # two runs, bitwise
    for a, b_ in zip(first, _charts(m)):
        assert torch.equal(a, b_)


@pytest.mark.parametrize('normalize,share,D,lengths,scale', [
    ('unit', False, 50, [14, 1, 2, 3, 5, 8, 9, 11, 13, 14, 6], 1.0),
    ('none', True, 16, [12, 1, 2, 3, 5, 8, 10, 12, 7], 0.25),
    ('none', False, 16, [9, 1, 2, 4, 9, 6], 0.25),
])
def test_forward_ragged_other_plans(normalize, share, D, lengths, scale):
    P, xs, _ = ROC.small_case(D, lengths, seed=211, share=share, scale=scale)
    Lmax = max(lengths)
    m = _module(P, D, share=share, normalize=normalize)
    assert _ragged_run(m, ROC.padded(xs, Lmax).cuda(), lengths) == 0
    _compare(m, P, xs, lengths, Lmax, normalize, share, what='%s share=%s' % (normalize, share))


@pytest.mark.parametrize('D,lengths', [(50, [20, 1, 2, 3, 5, 7, 9, 12, 15, 18, 20, 4]), (400, [16, 1, 2, 6, 11, 16, 9])])
def test_forward_ragged_cliora_plan(D, lengths, mfma_mode):
    Rn, Lmax = 36, max(lengths)
    P, xs, _ = ROC.small_case(D, lengths, seed=523)
    vl = ROC.vl_inputs(D, lengths, Rn, seed=523)
    m = _module(P, D, vl=True)
    xw = ROC.padded([v[0] for v in vl], Lmax, seed=98).cuda()
    obj_s, obj_w = torch.stack([v[1] for v in vl]).cuda(), torch.stack([v[2] for v in vl]).cuda()
    assert _ragged_run(m, ROC.padded(xs, Lmax).cuda(), lengths, vl=(xw, obj_s, obj_w)) == 0
    _compare(m, P, xs, lengths, Lmax, vl=vl, what='CLIORA D %d %s' % (D, mfma_mode))


@pytest.mark.parametrize('D,B,L,vl', [(50, 9, 14, False), (400, 5, 23, False), (50, 3, 2, False), (50, 4, 1, False), (50, 6, 9, True)])
def test_all_lengths_equal_are_bitwise_the_sequential_forward(D, B, L, vl):
    from cliora_amd import _lib
    P, _, _ = RC.case(D)
    m = _module(P, D, vl=vl)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, L, D, generator=g).cuda()
    extra = tuple(torch.randn(s, generator=g).cuda() for s in ((B, L, D), (B, 36, D), (B, 36, D))) if vl else None
    prev_w, prev_r = _lib.set_wavefront('off'), _lib.set_resident('off')
    try:
        with torch.no_grad():
            m(x, *(extra if vl else (x,)))
        want = _charts(m)
        want_att = m.atten_score.clone() if vl else None
        assert _ragged_run(m, x, [L] * B, vl=extra) == 0
    finally:
        _lib.set_wavefront(prev_w), _lib.set_resident(prev_r)
    for a, b_ in zip(want, _charts(m)):
        assert torch.equal(a, b_)
    if vl:
        assert torch.equal(want_att, m.atten_score)


def test_bad_lengths_are_counted_and_harm_no_other_sentence():
    from cliora_amd import ragged
    D = 50
    P, xs, lengths = RC.case(D)
    m = _module(P, D)
    xp = RC.padded(xs).cuda()
    assert _ragged_run(m, xp, lengths) == 0
    good = _charts(m)
    bad = list(lengths)
    bad[3], bad[10] = 0, RC.LMAX + 1
    # the same root levels as the good run: a re-scored level is the standalone scoring kernel's, equal to the riding scores to
    # rounding only, so the launches must be the same for the other sentences to come out bitwise
    assert _ragged_run(m, xp, bad, mask=ragged.root_level_mask(lengths)) == 2
    got = _charts(m)
    for b, n in enumerate(lengths):
        if b in (3, 10):
            continue
        own = torch.from_numpy(ROC.own_cells(RC.LMAX, n)).cuda()
        for a, c in zip(good, got):
            assert torch.equal(a[b, own], c[b, own]), b


def test_refusals():
    from cliora_amd import _lib
    from cliora_amd.diora import _param_struct, _ptr, _stream
    D, B, L = 32, 2, 5
    lib = _lib.lib()
    x = torch.randn(B, L, D).cuda()
    lens = _lens([5, 3])
    status = torch.zeros(1, dtype=torch.int32).cuda()

    def call(m, plan, flags, compress=False):
        names = dict(zip(_lib.PARAM_FIELDS, m._param_tensors()))
        if compress:
            names['root_mat'] = torch.randn(D, D).cuda()
        pst = _param_struct({k: (v.detach().contiguous() if v is not None else None) for k, v in names.items()})
        Cc = plan.C
        bufs = [torch.empty(B, Cc, D).cuda(), torch.empty(B, Cc, 1).cuda(), torch.empty(B, Cc, D).cuda(), torch.empty(B, Cc, 1).cuda()]
        ws = torch.empty(plan.fwd_bytes + plan.pair_bytes, dtype=torch.uint8).cuda()
        rc = lib.cliora_chart_forward_ragged(plan.handle, C.byref(pst), _ptr(x), None, None, *[_ptr(t) for t in bufs], None, _ptr(ws),
                                             ws.numel(), flags, _ptr(lens), 0b10100, _ptr(status), _stream())
        torch.cuda.synchronize()
        return rc, lib.cliora_last_error().decode()

    P = ROC.small_case(D, [5, 3], seed=1)[0]
    m = _module(P, D)
    plan = _lib.get_plan(B, L, D, True, 'unit', 0, 0)
    assert call(m, plan, 1 | _lib.FWD_NO_BACKWARD)[0] == 0
    for flags, compress, word in ((1, False, 'NO_BACKWARD'), (1 | _lib.FWD_NO_BACKWARD | _lib.FWD_PAIR_STATES, False, 'PAIR_STATES'),
                                  (1 | _lib.FWD_NO_BACKWARD, True, 'compress')):
        rc, msg = call(m, plan, flags, compress)
        assert rc != 0 and word in msg, (rc, msg)
    lstm_plan = _lib.get_plan(B, L, D, True, 'unit', 0, 0, arch=1)
    rc, msg = call(m, lstm_plan, 1 | _lib.FWD_NO_BACKWARD)
    assert rc != 0 and 'TreeLSTM' in msg
    # the module refuses what the entry cannot do before calling it
    m.train()
    m._ragged = (lens, 0b10100)
    try:
        with pytest.raises(_lib.ChartLibError, match='inference only'):
            m(x, x)
    finally:
        m._ragged = None


# ---- grounding over a padded batch ------------------------------------------------------------------------------------------
def _ground_inputs(B, L, Rn, lengths, seed):
    """Seeded attention with planted ties (duplicated regions, duplicated words), boxes, random trees of each sentence's own length
    in cliora_cky_spans_ragged's layout, phrases and gold spans inside each sentence."""
    gen = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed + 1)
    att = torch.softmax(torch.randn(B, L, Rn, generator=gen), -1)
    att[:, :, 20:30] = att[:, :, 0:10]
    att[:, 1] = att[:, 0]
    xy = torch.randint(0, 300, (B, Rn, 2), generator=gen).float()
    wh = torch.randint(0, 150, (B, Rn, 2), generator=gen).float()
    boxes = torch.cat([xy, xy + wh], -1)

    def tree(lo, hi, out):
        if hi - lo == 1:
            return
        k = rs.randint(lo + 1, hi)
        tree(lo, k, out), tree(k, hi, out)
        out.append((lo, hi - 1))
    spans = np.full((B, L - 1, 2), -1, dtype=np.int32)
    vg, gt = [], []
    for b, n in enumerate(lengths):
        sp = []
        tree(0, n, sp)
        spans[b, :n - 1] = np.array(sp, dtype=np.int32).reshape(-1, 2)
        target = {}
        for j in range(rs.randint(0, 8)):
            s = rs.randint(0, n)
            e = rs.randint(s + 1, n + 1)
            if sp and rs.rand() < 0.5:
                s, e = sp[rs.randint(0, len(sp))]
                e += 1
            bx = boxes[b, rs.randint(0, Rn)].tolist()
            target[j] = (s, e, [bx[0], bx[1], bx[2] + float(rs.randint(0, 40)), bx[3]])
        vg.append((target, None))
        gold = [tuple(sp[k]) for k in rs.choice(len(sp), size=rs.randint(0, n), replace=True)] if sp else []
        gt.append(gold + [(0, n - 1)])
    return att, boxes, spans, vg, gt


def _np_select(att, s, e):
    rows = att[s:e]
    rmax = rows.max(1)
    w = int(np.argmax(rmax))                 # numpy: the first maximum
    return s + w, int(np.argmax(rows[w]))


def _np_iou(a, g):
    f = np.float32
    a1 = f(f(a[2] - a[0]) * f(a[3] - a[1]))
    a2 = f(f(g[2] - g[0]) * f(g[3] - g[1]))
    w = max(f(min(a[2], g[2]) - max(a[0], g[0])), f(0))
    h = max(f(min(a[3], g[3]) - max(a[1], g[1])), f(0))
    inter = f(w * h)
    with np.errstate(invalid='ignore', divide='ignore'):
        return f(inter / f(f(a1 + a2) - inter))


def test_ground_eval_ragged_matches_the_rules_per_sentence():
    from cliora_amd.evaluate import Targets, ground
    B, L, Rn = 24, 20, 36
    lengths = [20, 3, 4, 5, 7, 9, 11, 13, 15, 17, 19, 20, 1, 6, 8, 10, 12, 14, 16, 18, 20, 2, 9, 1]
    att, boxes, spans, vg, gt = _ground_inputs(B, L, Rn, lengths, seed=17)
    tg = Targets(vg, gt, B, L, lengths=lengths)
    vgd = torch.randn(B, B, L, Rn)
    for i in range(B):
        vgd[i, i] = att[i]
    strided = torch.diagonal(vgd.cuda(), 0, 0, 1).permute(2, 0, 1)
    res = ground(strided, boxes.cuda(), tg, torch.from_numpy(spans).cuda(), lengths=_lens(lengths))
    a, bx = att.numpy(), boxes.numpy()
    assert tg.P == len(res.word) and tg.P > 40
    for k, (b, s, e) in enumerate(tg.phrases):
        n = lengths[b]
        w, box = _np_select(a[b, :n], s, e)
        hit = int(bool(_np_iou(bx[b, box], tg.phr_box[k]) > 0.5))
        pred = set(map(tuple, spans[b, :max(n - 2, 0)].tolist()))
        ccr = int(bool(hit) and (e - 1 == s or (s, e - 1) in pred))
        assert (res.word[k], res.box[k], res.hit[k], res.ccr[k]) == (w, box, hit, ccr), (k, b, s, e)
    for b, n in enumerate(lengths):
        pred, gold = set(map(tuple, spans[b, :max(n - 2, 0)].tolist())), set(gt[b][:-1])
        assert res.sent[b].tolist() == [len(pred & gold), len(pred), len(gold)], b
        for k in range(n - 1):
            s, e = spans[b, k]
            assert res.span_xyxy[b, k].tolist() == bx[b, _np_select(a[b, :n], s, e + 1)[1]].tolist(), (b, k)
        assert (res.span_xyxy[b, n - 1:] == 0).all()
    # span_box (ground() does not ask for it): the box id of every span of the sentence, -1 in the rows beyond
    from cliora_amd import _lib
    dev = strided.device
    tab = torch.from_numpy(tg.packed()).to(dev)
    o = np.cumsum([0, B + 1, tg.P * 2, tg.P * 4, B + 1, tg.G * 2]).tolist()
    t = [tab[o[i]:o[i + 1]] for i in range(5)]
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None and x.numel() else C.c_void_p(0)
    phr_out = torch.empty((tg.P, 4), dtype=torch.int32, device=dev)
    span_box = torch.full((B, L - 1), -7, dtype=torch.int32, device=dev)
    sent = torch.empty((B, 3), dtype=torch.int32, device=dev)
    status = torch.ones(1, dtype=torch.int32, device=dev)
    bxd, spd = boxes.cuda().contiguous(), torch.from_numpy(spans).cuda()
    _lib.check(_lib.lib().cliora_ground_eval_ragged(B, L, Rn, p(_lens(lengths)), p(strided), *strided.stride(), p(bxd), tg.P, p(t[0]), p(t[1]),
                                                    p(t[2]), p(spd), tg.G, p(t[3]), p(t[4]), p(phr_out), p(span_box), None, p(sent), p(status),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'cliora_ground_eval_ragged')
    assert status.item() == 0
    sb = span_box.cpu().numpy()
    for b, n in enumerate(lengths):
        assert sb[b, :n - 1].tolist() == [_np_select(a[b, :n], s_, e_ + 1)[1] for s_, e_ in spans[b, :n - 1]], b
        assert (sb[b, n - 1:] == -1).all(), b


def test_ground_eval_ragged_with_full_lengths_is_bitwise_ground_eval():
    from cliora_amd.evaluate import Targets, ground
    B, L, Rn = 16, 12, 36
    att, boxes, spans, vg, gt = _ground_inputs(B, L, Rn, [L] * B, seed=29)
    tg = Targets(vg, gt, B, L)
    args = (att.cuda(), boxes.cuda(), tg, torch.from_numpy(spans).cuda())
    a, b = ground(*args), ground(*args, lengths=_lens([L] * B))
    for f in ('spans', 'word', 'box', 'hit', 'ccr', 'sent', 'span_xyxy'):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_ground_eval_ragged_counts_bad_lengths():
    from cliora_amd import _lib
    from cliora_amd.evaluate import Targets, ground
    B, L, Rn = 6, 9, 36
    lengths = [9, 4, 5, 9, 3, 7]
    att, boxes, spans, vg, gt = _ground_inputs(B, L, Rn, lengths, seed=41)
    tg = Targets([({}, None)] * B, gt, B, L, lengths=lengths)
    bad = list(lengths)
    bad[2] = L + 1
    with pytest.raises(_lib.ChartLibError, match='rejected 1'):
        ground(att.cuda(), boxes.cuda(), tg, torch.from_numpy(spans).cuda(), lengths=_lens(bad))


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E_LENGTHS = ROC.E2E_LENGTHS


def _vl_net():
    return ROC.vl_net().cuda()


_examples = ROC.examples


def test_evaluate_ragged_matches_evaluate_example_by_example(tmp_path):
    """Example by example the spans, F1 counts and, per phrase, word / box / hit / ccr of `evaluate`'s pieces run on a batch of one at
    the exact length; a phrase is excused only where the exact-length atten_score has the two best entries of a decisive row within
    ROC.MEASURED_ATTEN_SCORE_DIFF, and the inputs are seeded so that none is (test_ragged_outside_cpu.py checks that on the oracle).
    parse.jsonl: every line equals the record `evaluate` writes for that example, in the caller's order; `pred_boxes` (one box per
    predicted span, each a selection of its own over up to 40 words) is compared by its length only."""
    import json
    from cliora_amd.evaluate import METRICS, batch_records, evaluate_ragged, ground_batch
    net = _vl_net()
    exs = _examples(E2E_LENGTHS)
    assert len(set(E2E_LENGTHS)) >= 10
    idx2word = {i: 'w%d' % i for i in range(97)}
    path = str(tmp_path / 'parse.jsonl')
    net.train()
    metrics, details = evaluate_ragged(net, exs, idx2word, out_path=path, max_batch=16, return_details=True)
    assert net.training
    assert set(metrics) == set(METRICS[:4])                     # the eval losses are left out for mixed lengths
    lines = open(path).read().splitlines()
    assert len(lines) == len(exs)
    net.eval()
    near, tot_hit, tot_ccr, tot = 0, 0, 0, 0
    with torch.no_grad():
        for i, ex in enumerate(exs):
            n = len(ex['sentence'])
            net(torch.tensor([ex['sentence']]).cuda(), ex['obj_feats'][None].cuda(), None, compute_loss=False)
            bm = dict(VG_GT=[ex['VG_GT']], GT=[ex['GT']], boxes=ex['boxes'][None].cuda())
            want = ground_batch(net.diora, bm)
            det = details[i]
            att = net.diora.atten_score[0].cpu().double().numpy()
            assert det['spans'].tolist() == want.spans[0].tolist(), (i, n)
            assert det['sent'].tolist() == want.sent[0].tolist(), (i, n)
            excused = set(ROC.near_tie_phrases(att, [(s, e) for _, s, e in want.phrases]))
            near += len(excused)
            for k in range(len(want.phrases)):
                if k not in excused:
                    for f in ('word', 'box', 'hit', 'ccr'):
                        assert det[f][k] == getattr(want, f)[k], (i, n, k, f)
            tot_hit, tot_ccr, tot = tot_hit + int(det['hit'].sum()), tot_ccr + int(det['ccr'].sum()), tot + len(det['hit'])
            rec = batch_records(want, net.diora.trees_from_spans(want.spans), [ex['sentence']], [ex['example_id']], idx2word, True)[0]
            ja, jb = json.loads(lines[i]), json.loads(rec)
            assert len(ja['pred_boxes']) == len(jb['pred_boxes'])
            ja.pop('pred_boxes'), jb.pop('pred_boxes')
            assert ja == jb, i
    print('phrases with a decisive near-tie of the exact-length scores: %d of %d' % (near, tot))
    assert near == 0
    assert metrics['ground_acc'] == tot_hit / (tot + 1e-8) and metrics['ccra'] == tot_ccr / (tot + 1e-8)


def test_embed_phrases_ragged_rows_are_the_exact_length_rows():
    from cliora_amd.phrases import embed_phrases, embed_phrases_ragged
    net = _vl_net()
    exs = _examples(E2E_LENGTHS[:14] + [2, 1], seed=9)
    sents = [ex['sentence'] for ex in exs]
    feats = torch.stack([ex['obj_feats'] for ex in exs])
    got = embed_phrases_ragged(net, sents, 'all-spans', example_ids=[ex['example_id'] for ex in exs], obj_feats=feats, max_batch=5)
    batches = [dict(sentences=torch.tensor([ex['sentence']]), obj_feats=ex['obj_feats'][None], example_ids=[ex['example_id']]) for ex in exs]
    want = embed_phrases(net, batches, 'all-spans')
    assert len(got) == len(want) == sum(n * (n + 1) // 2 for n in (len(s) for s in sents) if n > 2)
    assert got.example_ids == want.example_ids and got.positions == want.positions and got.sizes == want.sizes
    assert got.phrases == want.phrases
    g, w = got.vectors.cpu().double(), want.vectors.cpu().double()
    err = float(((g - w).abs() / w.abs().clamp(min=1.0)).max())
    print('embed_phrases_ragged: worst relative difference to the exact-length rows %.3e' % err)
    assert err <= ROC.FORWARD_BOUND
    lat = embed_phrases_ragged(net, sents, 'latent', obj_feats=feats, max_batch=5)
    assert len(lat) == sum(len(s) - 1 for s in sents if len(s) > 2)


def test_parse_ragged_takes_region_features():
    from cliora_amd import ragged
    net = _vl_net()
    exs = _examples([9, 1, 30, 2, 17, 9, 12], seed=13)
    sents = [ex['sentence'] for ex in exs]
    feats = torch.stack([ex['obj_feats'] for ex in exs])
    got = ragged.parse_ragged(net, sents, max_batch=3, obj_feats=feats)
    net.eval()
    with torch.no_grad():
        for i, ex in enumerate(exs):
            net(torch.tensor([ex['sentence']]).cuda(), ex['obj_feats'][None].cuda(), None, compute_loss=False)
            assert str(got[i]) == str(net.diora.cky()[0]), i
