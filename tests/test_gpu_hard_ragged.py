"""Hard (S-DIORA) charts of mixed lengths in one padded chart on the device (cliora_chart_forward_ragged_hard, cliora_hard_spans_ragged,
the module's _ragged_hard / _ragged_hard_train slots, ragged.parse_ragged_hard, evaluate_ragged(decode='hard'), Trainer.step_ragged on
a hard net), in both arithmetic modes.  The yardstick is the fp64 hard chart of one sentence at its exact
length (cliora_amd.hard.hard_forward_ragged_torch), teacher-forced by the device's selection; bitwise claims are against the
library's existing entries and against a second run.  Cases and bounds: hard_ragged_cases.py."""
import numpy as np
import pytest
import torch

import hard_ragged_cases as RC
import ragged_train_cases as TC
from conftest import grad_check

pytestmark = pytest.mark.gpu


def _module(c):
    from test_gpu_parity import _module_from_params
    m = _module_from_params(c['P'], c['D'], c['share'], c['normalize'])
    m.hard = True
    return m


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32).cuda()


def _forward(m, x, lengths, train, expect_status=0):
    from cliora_amd import ragged
    slot = '_ragged_hard_train' if train else '_ragged_hard'
    m.__dict__[slot] = (_lens(lengths), ragged.root_level_mask(lengths, x.shape[1]))      # a length outside 1..L sets no bit
    try:
        m(x, x)
    finally:
        m.__dict__[slot] = None
    assert int(m._ragged_status.item()) == expect_status
    ch = m.chart
    return [ch.inside_h, ch.inside_s, ch.outside_h, ch.outside_s]


def _run(c, lengths=None, W=None, dense=False, fill=None, wavefront=None, uniform=False, monkeypatch=None, m=None):
    """One forward over the padded batch (+ backward with the cotangents W when the case trains) -> dict of host tensors: the charts,
    the selections, the gradients (or None), the per-split score / weight rows of the workspace, the device spans with their status."""
    from cliora_amd import _lib
    from cliora_amd import diora as DI
    lengths = c['lengths'] if lengths is None else lengths
    W = c['W'] if W is None else W
    m = _module(c) if m is None else m
    m.hard_dense = dense
    m.train(c['train'])
    for p in m.parameters():
        p.grad = None
    if fill is not None:
        orig = DI.chart_buffers

        def filled(*a, **k):
            outs, ws, n = orig(*a, **k)
            ws.fill_(fill)
            return outs, ws, n
        monkeypatch.setattr(DI, 'chart_buffers', filled)
    prev_w = _lib.set_wavefront(wavefront) if wavefront is not None else None
    try:
        with torch.set_grad_enabled(c['train']):
            xg = c['xp'].clone().cuda().requires_grad_(c['train'])
            if uniform:
                m(xg, xg)
                charts = [m.chart.inside_h, m.chart.inside_s, m.chart.outside_h, m.chart.outside_s]
            else:
                charts = _forward(m, xg, lengths, c['train'])
            if c['train']:
                torch.autograd.backward(charts, [w.float().cuda() for w in W])
            torch.cuda.synchronize()
    finally:
        if prev_w is not None:
            _lib.set_wavefront(prev_w)
        if fill is not None:
            monkeypatch.setattr(DI, 'chart_buffers', orig)
    out = dict(m=m, charts=[t.detach().cpu() for t in charts], grads=None, sel=tuple(s.cpu() for s in m.selection))
    if c['train']:
        out['grads'] = {k: v.grad.detach().cpu() for k, v in m.named_parameters() if v.grad is not None}
        out['grads']['x_span'] = xg.grad.detach().cpu()
    B, L = len(lengths), c['L']
    plan, ws = m._plan, m._wss[0].view(torch.float32)
    off = lambda n: _lib.fn('cliora_plan_fwd_offset')(plan.handle, n.encode())
    rows = sum(lv * (L - lv) for lv in range(L)) * B
    rows_out = sum((L - lv - 1) * (L - lv) for lv in range(L)) * B
    out['Sp'] = ws[off('sp'):off('sp') + rows + rows_out].cpu()
    out['Pp'] = ws[off('pp'):off('pp') + rows + rows_out].cpu()
    out['rows_in'] = rows
    return out


def _check_selections(c, r):
    """Exact, on the device's own numbers: on every cell of an own triangle the weight row is one-hot at the first maximum of the score
    row, which is a VALID pair; sel names it; the cell's score is that split's; -1 exactly where no cell of a sentence selects."""
    from cliora_amd.hard import level_offsets
    lengths, L = c['lengths'], c['L']
    B = len(lengths)
    off = level_offsets(L)
    n_b = torch.tensor(lengths).view(B, 1)
    base = {'in': 0, 'out': r['rows_in']}
    for which, sel, S in (('in', r['sel'][0], r['charts'][1]), ('out', r['sel'][1], r['charts'][3])):
        row = base[which]
        for level in range(L):
            Lc, N = L - level, (level if which == 'in' else L - level - 1)
            k = sel[:, off[level]:off[level] + Lc].long()
            own = torch.arange(Lc).view(1, Lc) + level < n_b
            chooses = own & (level >= 1 if which == 'in' else level < n_b - 1)          # above the leaves / other than the sentence's root
            assert bool((k[~chooses] == -1).all()), (which, level)
            if N == 0:
                continue
            sp = r['Sp'][row:row + B * Lc * N].view(B, Lc, N)
            pp = r['Pp'][row:row + B * Lc * N].view(B, Lc, N)
            row += B * Lc * N
            first = torch.where(sp == sp.max(-1, keepdim=True).values, torch.arange(N).expand_as(sp), torch.full(sp.shape, N)).min(-1).values
            assert torch.equal(k[chooses], first[chooses]), (which, level)
            assert torch.equal(pp[chooses], torch.nn.functional.one_hot(first, N).float()[chooses]), (which, level)
            assert torch.equal(S[:, off[level]:off[level] + Lc, 0][chooses], sp.gather(-1, first.unsqueeze(-1)).squeeze(-1)[chooses]), (which, level)
            if which == 'out':                           # a valid pair: among the first n_b - level - 1
                assert bool((k < (n_b - level - 1))[chooses].all()), level
                valid = torch.arange(N).view(1, 1, N) < (n_b - level - 1).view(B, 1, 1)
                first_valid = torch.where((sp == sp.masked_fill(~valid, -float('inf')).max(-1, keepdim=True).values) & valid,
                                          torch.arange(N).expand_as(sp), torch.full(sp.shape, N)).min(-1).values
                assert torch.equal(k[chooses], first_valid[chooses]), level
    own_all = RC.own(L, lengths)
    for t in r['charts']:
        assert bool(torch.isfinite(t[own_all]).all())


_TF = {}


def _teacher_forced(name, c, sel, dtype):
    key = (name, dtype, sel[0].numpy().tobytes(), sel[1].numpy().tobytes())
    if key not in _TF:
        _TF[key] = RC.teacher_forced(c, sel, dtype, c['train'])
    return _TF[key]


def _check_parity(name, c, r, mode):
    lengths, L = c['lengths'], c['L']
    own = RC.own(L, lengths)
    o64, g64 = _teacher_forced(name, c, r['sel'], torch.float64)
    for k, cname in enumerate(RC.CHARTS):
        have, want = r['charts'][k].double()[own], o64[cname][own]
        err = float(((have - want).abs() / want.abs().clamp(min=1.0)).max())
        print('%s %s %s: worst relative error %.3e' % (name, mode, cname, err))
        assert err <= RC.FORWARD_BOUND, (cname, err)
    if not c['train']:
        return
    have_dx = torch.cat([r['grads']['x_span'][b, :n].double().reshape(-1) for b, n in enumerate(lengths)])
    want_dx = torch.cat([g64['x_span'][b, :n].reshape(-1) for b, n in enumerate(lengths)])
    pairs = [(k, r['grads'][k].double(), g64[k]) for k in sorted(g64) if k != 'x_span'] + [('d x_span', have_dx, want_dx)]
    assert sorted(k for k in r['grads']) == sorted(g64)
    for k, have, want in pairs:                          # the figures first, then the bounds
        d = (have - want).abs().flatten()
        sc = max(1.0, float(want.abs().max()))
        print('%s %s grad %-40s max err %.3e median %.3e of scale %.3e' % (name, mode, k, float(d.max()) / sc, float(d.median()) / sc, sc))
    for k, have, want in pairs:
        assert bool(torch.isfinite(have).all()), k
        grad_check(have, want, mode, RC.GRAD_STRICT, '%s %s' % (name, k))
    for b, n in enumerate(lengths):                      # d x of the padded positions: exactly 0
        assert not r['grads']['x_span'][b, n:].any(), (b, n)


def _spans(m, lengths):
    from cliora_amd import ragged
    from cliora_amd.diora import host_copy
    spans, status = host_copy(*ragged.hard_spans_ragged(m, _lens(lengths)))
    assert status.tolist() == [0]
    return spans


@pytest.mark.parametrize('name', sorted(RC.GPU_CASES))
def test_hard_ragged_case(name, mfma_mode):
    from cliora_amd.hard import hard_spans_ragged_numpy
    c = RC.case(name)
    lengths, L = c['lengths'], c['L']
    r = _run(c)
    _check_selections(c, r)
    _check_parity(name, c, r, mfma_mode)
    spans = _spans(r['m'], lengths)
    assert np.array_equal(spans, hard_spans_ragged_numpy(r['sel'][0], lengths, L))
    trees = r['m'].hard_tree(_lens(lengths))
    if c['clear']:                                       # the device's selection is the fp64 selection, no cell exempt ...
        assert torch.equal(r['sel'][0].long(), c['ref']['sel_in']) and torch.equal(r['sel'][1].long(), c['ref']['sel_out'])
        for b, n in enumerate(lengths):
            m1 = _module(c).eval()
            with torch.no_grad():
                x1 = c['xp'][b:b + 1, :n].cuda()
                m1(x1, x1)
            assert m1.hard_tree() == [trees[b]], (b, n)      # ... and each tree is the sentence's exact-length hard tree
    if c['ties']:
        own = RC.own(L, lengths)
        assert int(r['sel'][0][own].max()) == 0 and int(r['sel'][1][own].max()) <= 0
        for b, n in enumerate(lengths):
            right = n - 1
            for w in range(n - 2, -1, -1):
                right = (w, right)
            assert trees[b] == right


def _same(a, b, what, own=None):
    for k, (u, v) in enumerate(zip(a['charts'], b['charts'])):
        assert torch.equal(u if own is None else u[own], v if own is None else v[own]), (what, RC.CHARTS[k])
    for s, t in zip(a['sel'], b['sel']):
        assert torch.equal(s, t), what
    if a['grads'] is not None:
        assert sorted(a['grads']) == sorted(b['grads'])
        for k in a['grads']:
            assert torch.equal(a['grads'][k], b['grads'][k]), (what, k)


@pytest.mark.parametrize('name', ['l5', 'd24', 'unshared', 'none', 'long'])
def test_every_length_equal_to_L_is_the_uniform_hard_chart_bit_for_bit(name, mfma_mode):
    from cliora_amd import _lib
    c = RC.case(name)
    full = [c['L']] * len(c['lengths'])
    W = TC.weights(c['L'], full, c['D'], seed=23)
    prev = _lib.set_resident('off')
    try:
        want, got = _run(c, full, W, uniform=True), _run(c, full, W)
    finally:
        _lib.set_resident(prev)
    # the padded entry specifies every entry of the selection arrays; the uniform one leaves -1 where it writes none: the same arrays
    _same(want, got, 'lengths = L')
    assert np.array_equal(_spans(got['m'], full), got['m'].hard_spans())      # one kernel, with and without lengths


@pytest.mark.parametrize('name', ['l5', 'd24', 'b17', 'd400', 'unshared', 'long'])
def test_dense_fill_cotangents_second_run_and_wavefront_change_no_bit(name, mfma_mode, monkeypatch):
    c = RC.case(name)
    own = RC.own(c['L'], c['lengths'])
    r = _run(c)
    _same(r, _run(c), 'second run')
    _same(r, _run(c, dense=True), 'CLIORA_FWD_HARD_DENSE')
    _same(r, _run(c, fill=0xFF, wavefront='off', monkeypatch=monkeypatch), '0xFF (NaN) workspace, wavefront off', own)
    _same(r, _run(c, fill=0, wavefront='on', monkeypatch=monkeypatch), 'zero workspace, wavefront on', own)
    if c['train']:
        Wn = TC.weights(c['L'], c['lengths'], c['D'], seed=17, beyond=float('nan'))
        assert any(bool(torch.isnan(w).any()) for w in Wn)
        _same(r, _run(c, W=Wn), 'NaN cotangents beyond the triangles')


def test_inference_route_is_the_training_route_without_the_backward_state(mfma_mode):
    c = RC.case('l5')
    _same(dict(_run(c), grads=None), _run(dict(c, train=False)), 'NO_BACKWARD')


def test_bad_lengths_are_counted_and_raise():
    from cliora_amd import _lib, ragged
    c = RC.case('l5')
    m = _module(c).eval()
    bad = [5, 0, 3, 6, 5]
    with torch.no_grad():
        x = c['xp'].cuda()
        _forward(m, x, bad, False, expect_status=2)
        _forward(m, x, c['lengths'], False)
    spans, status = ragged.hard_spans_ragged(m, _lens(bad))
    assert status.tolist() == [2] and bool((spans[1] == -1).all()) and bool((spans[3] == -1).all())
    assert spans[0, -1].tolist() == [0, 4]
    with pytest.raises(_lib.ChartLibError, match='cliora_hard_spans_ragged rejected 2'):
        m.hard_spans(_lens(bad))


def _net(**kw):
    from cliora_amd import harness as H
    torch.manual_seed(31)
    return H.build_net(32, torch.nn.Embedding(97, 32), k_neg=5, **kw).cuda()


SENTENCE_LENGTHS = [7, 1, 3, 2, 6, 3, 5, 4, 7]


def _sentences(seed=4, lengths=SENTENCE_LENGTHS):
    rs = np.random.RandomState(seed)
    return [rs.randint(1, 97, size=n).tolist() for n in lengths]


def test_parse_ragged_hard_returns_each_sentences_tree_in_the_callers_order():
    from cliora_amd import ragged
    net = _net(hard=True)
    sentences = _sentences(lengths=SENTENCE_LENGTHS + [70])
    trees = ragged.parse_ragged_hard(net, sentences)
    packed = ragged.parse_ragged_hard(net, sentences, max_waste=float('inf'))
    assert trees == packed
    net.eval()
    for i in (0, 1, 3, 4, 9):                            # ... against the sentence alone through the uniform hard forward
        with torch.no_grad():
            net.diora(*net.embed(torch.tensor([sentences[i]]).cuda()))
        assert net.diora.hard_tree() == [trees[i]], i
    # both passes on the hard net through forward_ragged, 128 words allowed: the trees of the packs' own selections are the same trees
    seen = {}

    def per_pack(idx, lens, d):
        assert int(d._ragged_status.item()) == 0 and d.selection is not None
        for i, t in zip(idx, d.hard_tree(lens)):
            seen[i] = t
    ragged.forward_ragged(net, sentences, per_pack=per_pack, max_len=128)
    assert [seen[i] for i in range(len(sentences))] == trees


def test_evaluate_ragged_decode_hard_reports_the_f1_of_hard_spans():
    from cliora_amd import ragged
    from cliora_amd.evaluate import SpanF1, evaluate_ragged
    rs = np.random.RandomState(6)
    lengths = [6, 4, 3, 6, 5, 2]
    examples = []
    for i, n in enumerate(lengths):
        gold = []
        for _ in range(rs.randint(1, n)):
            s = rs.randint(0, n - 1)
            gold.append((int(s), int(rs.randint(s + 1, n))))
        examples.append(dict(sentence=rs.randint(1, 97, size=n).tolist(), example_id='ex%d' % i, GT=gold + [(0, n - 1)]))
    net = _net(hard=True)
    got = evaluate_ragged(net, examples, [str(i) for i in range(97)], decode='hard')
    trees_spans = {}
    sents = [e['sentence'] for e in examples]

    def per_pack(idx, lens, d):
        spans = d.hard_spans(lens)
        for b, i in enumerate(idx):
            trees_spans[i] = spans[b, :len(sents[i]) - 1]
    ragged.forward_ragged(net, sents, per_pack=per_pack)
    f1 = SpanF1()
    for i, e in enumerate(examples):
        if len(e['sentence']) <= 2:
            continue
        pred, gd = set(map(tuple, trees_spans[i][:-1].tolist())), set(e['GT'][:-1])
        f1.add_counts(len(pred & gd), len(pred), len(gd))
    prec, rec = f1.tp / (f1.tp + f1.fp) if f1.tp + f1.fp else 0., f1.tp / (f1.tp + f1.fn) if f1.tp + f1.fn else 0.
    assert got['corpus_f1'] == (2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.)
    assert got['sent_f1'] == float(np.mean(np.array(f1.sentence)))
    with pytest.raises(ValueError, match="decode='hard'"):
        evaluate_ragged(_net(), examples, [str(i) for i in range(97)], decode='hard')


def test_step_ragged_on_a_hard_net_is_one_adam_step_on_the_teacher_forced_gradients(mfma_mode):
    """One pack (max_waste = inf), so that the module's selection after the step is the step's: the loss is the token-weighted sum of
    the per-sentence fp64 restatement under that selection, and the update one Adam step on its clipped gradients."""
    from cliora_amd import harness as H
    from cliora_amd import ragged
    from cliora_amd.hard import hard_forward_torch, own_rows
    from oracle import diora_ref as R
    D, V, K, lr = 32, 97, 5, 2e-3
    torch.manual_seed(41)
    net = H.build_net(D, torch.nn.Embedding(V, 32), k_neg=K, hard=True)
    rs = np.random.RandomState(4)
    sentences = [rs.randint(1, V, size=n).tolist() for n in SENTENCE_LENGTHS]
    neg = torch.from_numpy(rs.randint(1, V, size=K))
    sd = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in net.named_parameters()}
    start = {k: v.detach().clone() for k, v in leaves.items()}
    net = net.cuda()
    tr = H.Trainer(net, lr=lr)
    out = tr.step_ragged(sentences, neg_samples=neg.cuda(), max_waste=float('inf'))
    torch.cuda.synchronize()
    assert net.training and net.diora.selection is not None
    (idx,) = ragged.pack([len(s) for s in sentences], 64, float('inf'))
    sel, L = [s.cpu().long() for s in net.diora.selection], max(SENTENCE_LENGTHS)
    P = {k[len('diora.'):]: v for k, v in sd.items() if k.startswith('diora.')}
    n_tokens = float(sum(len(s) for s in sentences))
    want_loss = 0.0
    for b, i in enumerate(idx):
        s = sentences[i]
        tokens = torch.tensor([list(s)])
        x_span, _ = R.embed_forward(sd['embed.embeddings.weight'], sd['embed.mat'], sd['embed.mat1'], tokens)
        rows = own_rows(L, len(s))
        given = (sel[0][b:b + 1, rows], sel[1][b:b + 1, rows])
        assert int(given[1][0, -1]) == -1
        o = hard_forward_torch(P, x_span, True, 'unit', selection=given)
        loss = R.reconstruction_loss(sd['embed.embeddings.weight'], sd['reconstruct_softmax_loss.mat'], tokens, neg, o['outside_h'])
        want_loss = want_loss + loss * (len(s) / n_tokens)
    want_loss.backward()
    print('step_ragged hard %s: loss %.6f, restatement %.6f' % (mfma_mode, out['total_loss'], float(want_loss.detach())))
    assert abs(out['total_loss'] - float(want_loss.detach())) <= 1e-4 * max(1.0, abs(float(want_loss.detach())))
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    for k, v in leaves.items():
        v.grad = grads[k].clone()
    torch.nn.utils.clip_grad_norm_(list(leaves.values()), 5.0)
    clipped = {k: v.grad.clone() for k, v in leaves.items()}
    torch.optim.Adam(list(leaves.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8).step()
    for k, p in net.named_parameters():
        have, want = p.detach().cpu().double(), leaves[k].detach()
        # as test_gpu_ragged_train.py argues: where the gradient is no larger than the error the project accepts on it, Adam's first
        # step has no determined sign, and the element is held to the step's reach
        noise = clipped[k].abs() <= TC.GRAD_STRICT * max(1.0, float(clipped[k].abs().max()))
        noise &= clipped[k] != 0
        if noise.any():
            assert float((have - start[k])[noise].abs().max()) <= lr * (1 + 1e-3), k
        if (~noise).any():
            grad_check(have[~noise], want[~noise], mfma_mode, TC.GRAD_STRICT, k)
        assert float((have - start[k]).abs().max()) > 0 or not grads[k].any(), k
    assert not grads['diora.inside_score_func.mat'].any()        # the selection carries no gradient: only a loss on the scores moves M


def test_step_ragged_moves_the_score_matrix_under_the_bracket_loss():
    from cliora_amd import harness as H
    sentences = _sentences(9)
    labels = [[('np', 0, 2), ('np', 1, n - 1)] if n >= 4 else [] for n in SENTENCE_LENGTHS]
    neg = torch.from_numpy(np.random.RandomState(9).randint(1, 97, size=5)).cuda()
    moved = {}
    for weight in (0.0, 1.0):
        net = _net(hard=True, **(dict(bracket_loss_weight=weight) if weight else {}))
        before = net.diora.inside_score_func.mat.detach().clone()
        loss = H.Trainer(net, lr=2e-3).step_ragged(sentences, neg_samples=neg, entity_labels=labels)['total_loss']
        assert np.isfinite(loss) and all(bool(torch.isfinite(p).all()) for p in net.parameters())
        moved[weight] = not torch.equal(before, net.diora.inside_score_func.mat.detach())
    assert moved == {0.0: False, 1.0: True}
