"""Hard (single-tree, S-DIORA) charts on the device (cliora_chart_forward_hard, cliora_hard_spans), against the fp64
restatement cliora_amd.hard.hard_forward_torch, in both arithmetic modes.  Cases: hard_cases.py (the smallest shapes at which each part
of the path can go wrong).

Per case:
  exact, on the device's own numbers   each weight row one-hot at the first maximum of its score row; sel names it; the cell's score
                                       is that split's score, bit for bit; cliora_hard_spans is the host walk of sel_in
  teacher-forced parity                charts within OUT_TOL = 1e-4 of scale of the restatement run under the DEVICE's selection;
                                       gradients for random cotangents on the four charts: conftest.grad_check in split-bf16 mode, the
                                       exact-mode rule of test_gpu_dispatch.py in f32 mode (3x the fp32 restatement's own error + floors)
  selection parity (clear cases)       the device's selection is the fp64 selection, every cell of both passes
  sparse against dense                 CLIORA_FWD_HARD_DENSE: outputs, selections, gradients torch.equal; the launch record holds
                                       level_compose_hard in one run and level_compose_fwd in the other
  workspace fill, wavefront            a workspace of 0xFF bytes with the backward's wavefront off and one of zeros with it on: torch.equal
"""
import numpy as np
import pytest
import torch

import hard_cases as HC
from conftest import grad_check

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-4


def _module(c, P, hard=True, keyword=True):
    from cliora_amd.diora import DioraMLP
    kw = dict(hard=hard) if keyword else {}
    m = DioraMLP(c['D'], share=c['share'], normalize=c['normalize'], outside=c['outside'], **kw)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    return m.cuda()


def _run(c, dense=False, fill=None, wavefront=None, resident=None, hard=True, keyword=True, monkeypatch=None):
    """One forward (+ backward with the case's cotangents when it trains) -> dict of host tensors: the charts, the selections, the
    gradients (or None), the per-split score / weight rows of the workspace, the device spans and the launch record."""
    from cliora_amd import _lib
    from cliora_amd import diora as DI
    P, x, cot = HC.case_inputs(c)
    m = _module(c, P, hard, keyword)
    m.hard_dense = dense
    m.train(c['train'])
    if fill is not None:
        orig = DI.chart_buffers

        def filled(*a, **k):
            outs, ws, n = orig(*a, **k)
            ws.fill_(fill)
            return outs, ws, n
        monkeypatch.setattr(DI, 'chart_buffers', filled)
    prev_w = _lib.set_wavefront(wavefront) if wavefront is not None else None
    prev_r = _lib.set_resident(resident) if resident is not None else None
    try:
        with _lib.launch_record() as rec, torch.set_grad_enabled(c['train']):
            xg = x.clone().cuda().requires_grad_(c['train'])
            m(xg, xg)
            if c['train']:
                torch.autograd.backward([getattr(m, k) for k in HC.CHARTS], [cot[k].cuda() for k in HC.CHARTS])
            torch.cuda.synchronize()
    finally:
        if prev_w is not None:
            _lib.set_wavefront(prev_w)
        if prev_r is not None:
            _lib.set_resident(prev_r)
        if fill is not None:
            monkeypatch.setattr(DI, 'chart_buffers', orig)
    out = dict(rec=rec, m=m, charts={k: getattr(m, k).detach().cpu() for k in HC.CHARTS}, grads=None)
    if hard:
        out['sel'] = tuple(s.cpu() for s in m.selection)
        out['spans'] = m.hard_spans()
    if c['train']:
        named = dict(m.named_parameters())
        out['grads'] = {k: v.grad.detach().cpu() for k, v in named.items() if v.grad is not None}
        out['grads']['x_span'] = xg.grad.detach().cpu()
    plan, ws = m._plan, m._wss[0].view(torch.float32)
    off = lambda n: _lib.fn('cliora_plan_fwd_offset')(plan.handle, n.encode())
    rows = sum(lv * (c['L'] - lv) for lv in range(c['L'])) * c['B']
    rows_out = sum((c['L'] - lv - 1) * (c['L'] - lv) for lv in range(c['L'])) * c['B']
    out['Sp'] = ws[off('sp'):off('sp') + rows + rows_out].cpu()
    out['Pp'] = ws[off('pp'):off('pp') + rows + rows_out].cpu()
    out['rows_in'] = rows
    return out


def _check_device_properties(c, r):
    """Exact, on the device's own numbers."""
    from cliora_amd.hard import hard_spans_numpy, level_offsets
    B, L = c['B'], c['L']
    off = level_offsets(L)
    base = {'in': 0, 'out': r['rows_in']}
    for which, sel, S in (('in', r['sel'][0], r['charts']['inside_s']), ('out', r['sel'][1], r['charts']['outside_s'])):
        if which == 'out' and not c['outside']:
            assert int(sel.max()) == -1                     # nothing selected, nothing written
            continue
        row = base[which]
        for level in range(L):
            Lc, N = L - level, (level if which == 'in' else L - level - 1)
            k = sel[:, off[level]:off[level] + Lc].long()
            if N == 0:
                assert int(k.max()) == -1                   # leaves / the outside root: not written
                continue
            sp = r['Sp'][row:row + B * Lc * N].view(B, Lc, N)
            pp = r['Pp'][row:row + B * Lc * N].view(B, Lc, N)
            row += B * Lc * N
            first = torch.where(sp == sp.max(-1, keepdim=True).values, torch.arange(N).expand_as(sp), torch.full(sp.shape, N)).min(-1).values
            assert torch.equal(k, first), (which, level)
            assert torch.equal(pp, torch.nn.functional.one_hot(first, N).float()), (which, level)
            assert torch.equal(S[:, off[level]:off[level] + Lc, 0], sp.gather(-1, k.unsqueeze(-1)).squeeze(-1)), (which, level)
    assert np.array_equal(r['spans'], hard_spans_numpy(r['sel'][0], L))
    for k in HC.CHARTS:
        assert bool(torch.isfinite(r['charts'][k]).all()), k


_TF = {}


def _teacher_forced(name, c, sel, dtype):
    key = (name, dtype, sel[0].numpy().tobytes(), sel[1].numpy().tobytes())
    if key not in _TF:
        _TF[key] = HC.teacher_forced(c, sel, dtype, c['train'])
    return _TF[key]


def _check_parity(name, c, r, mode):
    from dispatch_cases import dist
    o64, g64 = _teacher_forced(name, c, r['sel'], torch.float64)
    for k in HC.CHARTS:
        err = float((r['charts'][k].double() - o64[k]).abs().max())
        scale = max(1.0, float(o64[k].abs().max()))
        print('%s %s %s: %.3g of scale %.3g' % (name, mode, k, err / scale, scale))
        assert err <= OUT_TOL * scale, (k, err, scale)
    if not c['train']:
        return
    if mode == 'f32':
        _, g32 = _teacher_forced(name, c, r['sel'], torch.float32)
    for k, ref in g64.items():
        if mode == 'f32':
            hip, o32 = dist(r['grads'][k], ref), dist(g32[k], ref)
            print('%s f32 %s: device %s fp32 restatement %s' % (name, k, {q: '%.2g' % v for q, v in hip.items()}, {q: '%.2g' % v for q, v in o32.items()}))
            for q, floor in (('q50', 2e-7), ('q99', 2e-6), ('max', 2e-5)):
                assert hip[q] <= 3.0 * o32[q] + floor, (k, q, hip[q], o32[q])
        else:
            grad_check(r['grads'][k], ref, mode, 2e-4, k, full_size=False)


def _same(a, b, what):
    for k in HC.CHARTS:
        assert torch.equal(a['charts'][k], b['charts'][k]), (what, k)
    for s, t in zip(a['sel'], b['sel']):
        assert torch.equal(s, t), what
    if a['grads'] is not None:
        for k in a['grads']:
            assert torch.equal(a['grads'][k], b['grads'][k]), (what, k)


@pytest.mark.parametrize('name', sorted(HC.CASES))
def test_hard_case(name, mfma_mode, monkeypatch):
    c = HC.CASES[name]
    r = _run(c)
    print('%s %s record: %s' % (name, mfma_mode, sorted(r['rec'])))
    _check_device_properties(c, r)
    _check_parity(name, c, r, mfma_mode)
    if c['clear']:
        ref = HC.reference(name)
        assert torch.equal(r['sel'][0].long(), ref['sel_in']) and torch.equal(r['sel'][1].long(), ref['sel_out'])
    if c['ties']:
        assert int(r['sel'][0].max()) == 0 and int(r['sel'][1].max()) == 0
        right = c['L'] - 1
        for w in range(c['L'] - 2, -1, -1):
            right = (w, right)
        assert r['m'].hard_tree() == [right] * c['B']
    # sparse against dense
    d = _run(c, dense=True)
    _same(r, d, 'dense')
    if c['L'] > 1:
        assert any(e.startswith('level_compose_hard<') for e in r['rec']) and not any(e.startswith('level_compose_fwd') for e in r['rec'])
        assert any(e.startswith('level_compose_fwd<') for e in d['rec']) and not any(e.startswith('level_compose_hard') for e in d['rec'])
    # workspace fill and the backward's wavefront
    _same(r, _run(c, fill=0xFF, wavefront='off', monkeypatch=monkeypatch), '0xFF workspace, wavefront off')
    _same(r, _run(c, fill=0, wavefront='on', monkeypatch=monkeypatch), 'zero workspace, wavefront on')


@pytest.mark.parametrize('resident', ['on', 'off'])
def test_plan_the_resident_kernels_would_take(resident, mfma_mode):
    """B 3 / L 5 / D 16 with cliora_set_resident forced: the hard forward runs its launch path either way (same charts, same
    selections); the backward is the resident or the launch one, each against fp64."""
    c = HC.CASES['b3l5']
    base, r = _run(c), _run(c, resident=resident)
    for k in HC.CHARTS:
        assert torch.equal(base['charts'][k], r['charts'][k]), k
    assert torch.equal(base['sel'][0], r['sel'][0]) and torch.equal(base['sel'][1], r['sel'][1])
    assert any(e.startswith('level_compose_hard<') for e in r['rec'])
    _check_device_properties(c, r)
    _check_parity('b3l5', c, r, mfma_mode)


def test_hard_false_is_the_module_without_the_keyword_and_the_flag_switches_paths():
    c = HC.CASES['b3l5']
    plain, off = _run(c, hard=False, keyword=False), _run(c, hard=False)
    for k in HC.CHARTS:
        assert torch.equal(plain['charts'][k], off['charts'][k]), k
    for k in plain['grads']:
        assert torch.equal(plain['grads'][k], off['grads'][k]), k
    assert plain['rec'] == off['rec'] and not any('hard' in e for e in off['rec'])
    m, (P, x, _) = off['m'], HC.case_inputs(c)
    assert m.selection is None
    with pytest.raises(Exception, match='not a hard chart'):
        m.hard_spans_device()
    from cliora_amd import _lib
    m.hard = True
    with _lib.launch_record() as rec, torch.no_grad():
        m(x.cuda(), x.cuda())
        torch.cuda.synchronize()
    assert any(e.startswith('level_compose_hard<') for e in rec) and m.selection is not None
    hard = _run(c)
    assert torch.equal(m.selection[0].cpu(), hard['sel'][0])
    # the decodes that read the split scores keep working on a hard chart: CKY picks, per cell, among the same scores
    assert len(m.cky()) == c['B'] and len(m.hard_tree()) == c['B']
    assert set(m.inside_tree) == {(b, 0) for b in range(c['B'])} and len(m.inside_tree[(0, 0)][(c['L'] - 1, 0)]) == c['L'] - 1
    m.hard = False
    with _lib.launch_record() as rec, torch.no_grad():
        m(x.cuda(), x.cuda())
        torch.cuda.synchronize()
    assert not any('hard' in e for e in rec) and m.selection is None


def _net(**kw):
    from cliora_amd import harness as H
    torch.manual_seed(31)
    return H.build_net(32, torch.nn.Embedding(100, 32), k_neg=20, **kw).cuda()


def test_build_net_hard_trains():
    from cliora_amd import harness as H
    g = torch.Generator().manual_seed(32)
    bm = dict(sentences=torch.randint(0, 100, (8, 8), generator=g).cuda(), neg_samples=torch.randperm(100, generator=g)[:20].cuda())
    net = _net(hard=True)
    assert net.diora.hard is True and _net().diora.hard is False
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    tr = H.Trainer(net)
    losses = [tr.step(bm)['total_loss'] for _ in range(2)]
    assert all(np.isfinite(v) for v in losses), losses
    assert net.diora.selection is not None and int(net.diora.selection[0].max()) >= 0
    moved = [k for k, v in net.state_dict().items() if not torch.equal(v, before[k])]
    for k in ('diora.inside_compose_func.h_fcs.2.weight', 'diora.inside_compose_func.leaf_fc.weight', 'diora.root_vector_out_h'):
        assert k in moved, (k, moved)
    # the reconstruction loss reads outside_h alone, and a hard cell's vector does not depend on its scores (the selection carries no
    # gradient): the score matrix moves only under a loss that reads the chart scores
    assert 'diora.inside_score_func.mat' not in moved


def test_evaluate_decode_hard_reports_the_f1_of_hard_spans():
    from cliora_amd.evaluate import SpanF1, evaluate, ground_batch
    g = torch.Generator().manual_seed(33)
    B, L = 4, 6
    gold = [[(0, 1), (2, 3), (0, 3), (4, 5), (0, 5)], [(1, 2), (0, 2), (3, 4), (3, 5), (0, 5)], [(4, 5), (3, 5), (2, 5), (1, 5), (0, 5)],
            [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5)]]
    bm = dict(sentences=torch.randint(0, 100, (B, L), generator=g), neg_samples=torch.randperm(100, generator=g)[:20], GT=gold,
              example_ids=list(range(B)))
    net = _net(hard=True)
    got = evaluate(net, [bm], [str(i) for i in range(100)], decode='hard')
    with torch.no_grad():
        net(bm['sentences'].cuda(), None, bm['neg_samples'].cuda(), compute_loss=True)
    spans = net.diora.hard_spans()
    f1 = SpanF1()
    for b in range(B):
        pred, gd = set(map(tuple, spans[b, :-1].tolist())), set(gold[b][:-1])
        f1.add_counts(len(pred & gd), len(pred), len(gd))
    prec, rec = f1.tp / (f1.tp + f1.fp) if f1.tp + f1.fp else 0., f1.tp / (f1.tp + f1.fn) if f1.tp + f1.fn else 0.
    assert got['corpus_f1'] == (2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.)
    assert got['sent_f1'] == float(np.mean(np.array(f1.sentence)))
    soft = _net()
    with pytest.raises(ValueError, match="decode='hard'"):
        evaluate(soft, [bm], [str(i) for i in range(100)], decode='hard')
    with torch.no_grad():
        soft(bm['sentences'].cuda(), None, bm['neg_samples'].cuda(), compute_loss=True)
    with pytest.raises(ValueError, match="decode='hard'"):
        ground_batch(soft.diora, bm, decode='hard')
    from cliora_amd import ragged
    with pytest.raises(ValueError):
        ragged.decode_entry('hard')            # the ragged evaluators keep refusing the name
