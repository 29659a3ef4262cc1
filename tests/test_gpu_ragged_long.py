"""Both passes of mixed-length batches whose padded chart is longer than 64 words, on the device (cliora_chart_forward_ragged_wide and
the Python built on it with max_len = 128).  The yardstick is the oracle run in fp64 on one sentence at its exact
length (ragged_long_cases.parity_oracle), at the project's forward bound; bitwise claims are against the existing entries of the
library."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import ragged_long_cases as RL
import ragged_outside_cases as ROC

pytestmark = pytest.mark.gpu


def _module(P, D, vl=False):
    from cliora_amd import cliora, diora
    m = (cliora.DioraMLP if vl else diora.DioraMLP)(D, outside=True, normalize='unit', compress=False, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if not k.startswith('outside_') else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    return m.cuda().eval()


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32).cuda()


def _ragged_run(m, xp, lengths, vl=None, mask=None):
    """The module's eval forward through the ragged entry of its plan (L > 64: cliora_chart_forward_ragged_wide); -> the status word."""
    from cliora_amd import ragged
    m._ragged = (_lens(lengths), ragged.root_level_mask(lengths, max_len=128) if mask is None else mask)
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


def _vl_padded(vli, Lmax):
    """(x_word (B, Lmax, D), obj_span (B, R, D), obj_word (B, R, D)) on the device from ROC.vl_inputs."""
    return (ROC.padded([v[0] for v in vli], Lmax, seed=98).cuda(), torch.stack([v[1] for v in vli]).cuda(),
            torch.stack([v[2] for v in vli]).cuda())


# ---- 1, 2: parity with the fp64 oracle at the exact length, and the documented state -------------------------------------------------
@pytest.mark.parametrize('name', sorted(RL.PARITY))
def test_long_padded_chart_matches_the_oracle_at_the_exact_length(name, mfma_mode):
    from cliora_amd import ragged
    vl, D, P, xs, lengths, vli = RL.parity_case(name)
    Lmax = max(lengths)
    assert Lmax > 64
    m = _module(P, D, vl=vl)
    xp = ROC.padded(xs, Lmax).cuda()
    extra = _vl_padded(vli, Lmax) if vl else None
    # the inside-only forward of the same padded batch first: its trees are what the both-pass call must leave unchanged
    m.outside = False
    with torch.no_grad():
        m(xp, *(extra if vl else (xp,)))
    m.outside = True
    spans0, st0 = ragged.cky_spans_ragged(m, _lens(lengths))
    spans0 = spans0.clone()
    assert _ragged_run(m, xp, lengths, vl=extra) == 0
    assert m._plan.L == Lmax and m._plan.bwd_bytes == 0                  # a forward-only plan
    first = _charts(m)
    att = m.atten_score.cpu().double() if vl else None
    spans1, st1 = ragged.cky_spans_ragged(m, _lens(lengths))
    assert st0.item() == 0 and st1.item() == 0 and torch.equal(spans0, spans1)          # the decode reads the split scores, not inside_s
    ih, ins, oh, os_ = [t.cpu().double() for t in first]
    want = RL.parity_oracle(name)
    worst = {k: 0.0 for k in RL.CHARTS if vl or k != 'atten_score'}
    fails = []
    for b, n in enumerate(lengths):
        own = torch.from_numpy(ROC.own_cells(Lmax, n))
        got = dict(inside_h=ih[b, own], outside_h=oh[b, own], outside_s=os_[b, own])
        if vl:
            got['atten_score'] = att[b, :n]
        for k, g in got.items():
            w = want[b][k]
            assert g.shape == w.shape and bool(torch.isfinite(g).all()), (k, b, n)
            err = float(((g - w).abs() / w.abs().clamp(min=1.0)).max())
            worst[k] = max(worst[k], err)
            if err > RL.FORWARD_BOUND:
                fails.append((k, b, n, err))
        beyond = np.setdiff1d(np.arange(ins.shape[1]), ROC.own_cells(Lmax, n))             # the documented state of inside_s
        assert (first[1][b, :, 0].cpu().numpy()[beyond] == np.float32(ROC.MASKED)).all(), b
    print('\n%s %s worst errors: %s' % (name, mfma_mode, ', '.join('%s %.3e' % kv for kv in worst.items())))
    assert not fails, fails[:8]
    assert _ragged_run(m, xp, lengths, vl=extra) == 0                                       # two runs, bitwise
    for a, b_ in zip(first, _charts(m)):
        assert torch.equal(a, b_)
    if vl:
        assert torch.equal(att, m.atten_score.cpu().double())


# ---- 3: all lengths equal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vl', [False, True])
@pytest.mark.parametrize('D', [16, 50])
@pytest.mark.parametrize('L', RL.EQUAL_LENGTHS)
def test_all_lengths_equal_are_bitwise_the_sequential_forward(L, D, vl):
    from cliora_amd import _lib
    B = RL.EQUAL_B
    P = ROC.small_case(D, [1], seed=8130 + D)[0]
    m = _module(P, D, vl=vl)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, L, D, generator=g).cuda()
    extra = tuple(torch.randn(s, generator=g).cuda() for s in ((B, L, D), (B, RL.REGIONS, D), (B, RL.REGIONS, D))) if vl else None
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


# ---- 4: the wide entry on a short plan -------------------------------------------------------------------------------------------
def _direct(entry, m, x, lengths, mask):
    """One call of a ragged forward entry through ctypes -> (rc, status, the four charts)."""
    from cliora_amd import _lib
    from cliora_amd.diora import _param_struct, _ptr, _stream, split_root_levels
    B, L, D = x.shape
    plan = _lib.get_plan(B, L, D, True, 'unit', 0, x.device.index)
    names = dict(zip(_lib.PARAM_FIELDS, m._param_tensors()))
    keep = {k: (v.detach().contiguous() if v is not None else None) for k, v in names.items()}
    pst = _param_struct(keep)
    bufs = [torch.zeros(B, plan.C, w).cuda() for w in (D, 1, D, 1)]
    ws = torch.zeros(plan.fwd_bytes, dtype=torch.uint8).cuda()
    status = torch.ones(1, dtype=torch.int32).cuda()
    lens = _lens(lengths)
    arg = split_root_levels(mask) if entry.endswith('_wide') else mask
    rc = _lib.fn(entry)(plan.handle, C.byref(pst), _ptr(x), None, None, *[_ptr(t) for t in bufs], None, _ptr(ws), ws.numel(),
                        1 | _lib.FWD_NO_BACKWARD, _ptr(lens), arg, _ptr(status), _stream())
    torch.cuda.synchronize()
    return rc, int(status.item()), bufs


def test_wide_entry_on_a_short_plan_is_bitwise_the_entry_of_64_levels():
    from cliora_amd import ragged
    D, lengths, seed = RL.SHORT_CASE
    P, xs, lengths = ROC.small_case(D, lengths, seed=seed)
    m = _module(P, D)
    x = ROC.padded(xs, max(lengths)).cuda()
    mask = ragged.root_level_mask(lengths)
    rc0, st0, want = _direct('cliora_chart_forward_ragged', m, x, lengths, mask)
    rc1, st1, got = _direct('cliora_chart_forward_ragged_wide', m, x, lengths, mask)
    assert (rc0, st0, rc1, st1) == (0, 0, 0, 0)
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert float(want[2].abs().max()) > 0                                  # the outside pass ran


# ---- 5: bad lengths at L 65 ------------------------------------------------------------------------------------------------------
def test_bad_lengths_at_65_are_counted_and_harm_no_other_sentence():
    from cliora_amd import ragged
    D, lengths, seed = RL.BAD_CASE
    P, xs, lengths = ROC.small_case(D, lengths, seed=seed)
    Lmax = max(lengths)
    assert Lmax == 65
    m = _module(P, D)
    xp = ROC.padded(xs, Lmax).cuda()
    assert _ragged_run(m, xp, lengths) == 0
    good = _charts(m)
    bad = list(lengths)
    for b, n in RL.BAD_AT.items():
        bad[b] = n
    # the root levels of the good run: a re-scored level comes from the standalone scoring kernel, equal to the riding scores to
    # rounding only, so the launches must be the same for the other sentences to come out bitwise
    assert _ragged_run(m, xp, bad, mask=ragged.root_level_mask(lengths, max_len=128)) == len(RL.BAD_AT)
    got = _charts(m)
    for b, n in enumerate(lengths):
        if b in RL.BAD_AT:
            continue
        own = torch.from_numpy(ROC.own_cells(Lmax, n)).cuda()
        for a, c in zip(good, got):
            assert torch.equal(a[b, own], c[b, own]), b


# ---- 6: evaluate_ragged end to end -------------------------------------------------------------------------------------------------
def _tree_spans(tree):
    """(start, end) inclusive of every constituent of a nested-tuple tree."""
    out = []

    def walk(t):
        if not isinstance(t, tuple):
            return t, t
        (s, _), (_, e) = walk(t[0]), walk(t[1])
        out.append((s, e))
        return s, e
    walk(tree)
    return out


def test_evaluate_ragged_max_len_128_end_to_end(tmp_path):
    """Spans and F1 counts per example against parse_ragged (the same inside pass of the same packs: nothing is excused); per phrase
    word / box / hit / ccr against `evaluate`'s pieces on a batch of one at the exact length, no phrase excused
    (test_ragged_long_cpu.py checks on the fp64 oracle that none has a decisive near-tie); parse.jsonl line by line."""
    from cliora_amd import _lib, ragged
    from cliora_amd.evaluate import METRICS, batch_records, evaluate_ragged, ground_batch
    net = ROC.vl_net().cuda()
    exs = RL.e2e_examples()
    sents = [ex['sentence'] for ex in exs]
    feats = torch.stack([ex['obj_feats'] for ex in exs])
    idx2word = {i: 'w%d' % i for i in range(97)}
    path = str(tmp_path / 'parse.jsonl')
    with pytest.raises(_lib.ChartLibError, match='L > 64.*both-pass'):
        evaluate_ragged(net, exs, idx2word, max_batch=RL.E2E_MAX_BATCH)                  # the default still refuses
    net.train()
    metrics, details = evaluate_ragged(net, exs, idx2word, out_path=path, max_batch=RL.E2E_MAX_BATCH, return_details=True, max_len=128)
    assert net.training
    assert set(metrics) == set(METRICS[:4])
    trees = ragged.parse_ragged(net, sents, max_batch=RL.E2E_MAX_BATCH, obj_feats=feats, max_len=128, max_long_batch=8)
    assert net.training
    lines = open(path).read().splitlines()
    assert len(lines) == len(exs)
    net.eval()
    tot_hit = tot_ccr = tot = 0
    with torch.no_grad():
        for i, ex in enumerate(exs):
            n = len(ex['sentence'])
            det = details[i]
            assert str(net.diora.trees_from_spans(det['spans'][None])[0]) == str(trees[i]), (i, n)
            pred, gold = set(_tree_spans(trees[i])) - {(0, n - 1)}, set(map(tuple, ex['GT'][:-1]))
            assert det['sent'].tolist() == [len(pred & gold), len(pred), len(gold)], (i, n)
            net(torch.tensor([ex['sentence']]).cuda(), ex['obj_feats'][None].cuda(), None, compute_loss=False)
            want = ground_batch(net.diora, dict(VG_GT=[ex['VG_GT']], GT=[ex['GT']], boxes=ex['boxes'][None].cuda()))
            assert len(want.phrases) == len(det['hit'])
            for k in range(len(want.phrases)):                                           # no phrase is excused
                for f in ('word', 'box', 'hit', 'ccr'):
                    assert det[f][k] == getattr(want, f)[k], (i, n, k, f)
            tot_hit, tot_ccr, tot = tot_hit + int(det['hit'].sum()), tot_ccr + int(det['ccr'].sum()), tot + len(det['hit'])
            rec = batch_records(want, net.diora.trees_from_spans(want.spans), [ex['sentence']], [ex['example_id']], idx2word, True)[0]
            ja, jb = json.loads(lines[i]), json.loads(rec)
            assert len(ja['pred_boxes']) == len(jb['pred_boxes'])
            ja.pop('pred_boxes'), jb.pop('pred_boxes')
            assert ja == jb, i
    assert tot == RL.E2E_PHRASES
    assert metrics['ground_acc'] == tot_hit / (tot + 1e-8) and metrics['ccra'] == tot_ccr / (tot + 1e-8)
    m2 = evaluate_ragged(net, exs, idx2word, max_batch=RL.E2E_MAX_BATCH, max_len=128, decode='mbr')      # the other decode runs too
    assert set(m2) == set(METRICS[:4]) and m2['ground_acc'] == metrics['ground_acc']


# ---- 7: embed_phrases_ragged ---------------------------------------------------------------------------------------------------------
def test_embed_phrases_ragged_max_len_128_rows_are_the_exact_length_rows():
    from cliora_amd.phrases import embed_phrases, embed_phrases_ragged
    net = ROC.vl_net().cuda()
    exs = RL.e2e_examples(RL.EMBED_LENGTHS, seed=RL.EMBED_SEED)
    sents = [ex['sentence'] for ex in exs]
    feats = torch.stack([ex['obj_feats'] for ex in exs])
    got = embed_phrases_ragged(net, sents, 'all-spans', example_ids=[ex['example_id'] for ex in exs], obj_feats=feats, max_batch=4,
                               max_len=128)
    batches = [dict(sentences=torch.tensor([ex['sentence']]), obj_feats=ex['obj_feats'][None], example_ids=[ex['example_id']]) for ex in exs]
    want = embed_phrases(net, batches, 'all-spans')
    assert len(got) == len(want) == sum(n * (n + 1) // 2 for n in (len(s) for s in sents) if n > 2)
    assert got.example_ids == want.example_ids and got.positions == want.positions and got.sizes == want.sizes
    g, w = got.vectors.cpu().double(), want.vectors.cpu().double()
    err = float(((g - w).abs() / w.abs().clamp(min=1.0)).max())
    print('\nembed_phrases_ragged(max_len=128): worst relative difference to the exact-length rows %.3e' % err)
    assert err <= RL.FORWARD_BOUND
    lat = embed_phrases_ragged(net, sents, 'latent', obj_feats=feats, max_batch=4, max_len=128)
    assert len(lat) == sum(len(s) - 1 for s in sents if len(s) > 2)


# ---- 8: the memory cap ---------------------------------------------------------------------------------------------------------------
def test_max_long_batch_caps_the_long_packs_and_keeps_the_callers_order():
    from cliora_amd import ragged
    net = RL.text_net().cuda()
    rs = np.random.RandomState(21)
    lengths = RL.CAP_LENGTHS
    sents = [rs.randint(1, 97, size=n).tolist() for n in lengths]
    seen = []
    rows = torch.zeros(len(sents), net.diora.size).cuda()

    def per_pack(idx, lens, d):
        assert int(d._ragged_status.item()) == 0
        seen.append((len(idx), d._plan.L))
        assert lens.cpu().tolist() == [lengths[i] for i in idx]
        rows[torch.tensor(idx).cuda()] = ragged.root_rows(d, lens)

    packs = ragged.forward_ragged(net, sents, per_pack=per_pack, max_len=128, max_long_batch=RL.CAP)
    assert sorted(i for p in packs for i in p) == list(range(len(sents)))
    assert any(L > 64 for _, L in seen) and all(B <= RL.CAP for B, L in seen if L > 64)
    assert sum(B for B, L in seen if L > 64) >= 5 and len(seen) == len(packs)
    want = ragged.encode_ragged(net, sents, max_len=128)                # the inside-only entry, packed without the cap
    err = float(((rows - want).abs() / want.abs().clamp(min=1.0)).max())
    assert err <= RL.FORWARD_BOUND, err
