"""Training CLIORA through a padded chart of mixed lengths on the device (cliora_chart_forward_ragged_train_vl,
cliora_chart_backward_ragged_vl, cliora_vg_loss_ragged, cliora_contrastive_loss_ragged, ragged.forward_ragged_train(obj_feats=...),
Trainer.step_ragged(obj_feats=...)).  The yardsticks are the fp64 oracle on one sentence at its exact length
and the fp64 restatements of the two loss definitions (ragged_vl_train_cases); bitwise claims are against the library's existing
entries and against a second run."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ragged_outside_cases as ROC
import ragged_train_cases as TC
import ragged_vl_train_cases as VC
from conftest import grad_check

pytestmark = pytest.mark.gpu


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32).cuda()


# ---- 1. the loss kernels alone --------------------------------------------------------------------------------------------------------
class _Chart:
    pass


def _vg(vg, lens, alpha=0.7):
    """harness.VGLoss on the device -> (value, d vg, status word or None) under an upstream cotangent of 1.7."""
    from cliora_amd import harness as H
    t = vg.float().cuda().requires_grad_(True)
    m = H.VGLoss(alpha)
    v = m(t) if lens is None else m(t, lens)
    (1.7 * v).backward()
    torch.cuda.synchronize()
    return v.detach().clone(), t.grad.clone(), (None if lens is None else int(m.status.item()))


def _contrastive(smax, ins, outs, lens, margin=0.2, alpha=0.7):
    from cliora_amd import harness as H
    t = [x.float().cuda().requires_grad_(True) for x in (smax, ins, outs)]
    d = _Chart()
    d.all_atten_score, d.inside_s, d.outside_s = torch.stack([t[0], t[0] - 1.0], -1), t[1], t[2]
    m = H.ContrastiveLoss(margin=margin, alpha_contr=alpha)
    assert m.fused
    v = m(d) if lens is None else m(d, lens)
    (1.7 * v).backward()
    torch.cuda.synchronize()
    return v.detach().clone(), [x.grad.clone() for x in t], (None if lens is None else int(m.status.item()))


@functools.lru_cache(maxsize=None)
def _loss_reference(name):
    """The fp64 restatements on a case's inputs, value and gradients under the cotangent 1.7, computed once."""
    B, L, Rn, lengths = VC.LOSS_CASES[name]
    vg, smax, ins, outs = [t.requires_grad_(True) for t in VC.loss_inputs(name)]
    l_vg = VC.vg_loss_ragged(vg, lengths, 0.7)
    (1.7 * l_vg).backward()
    gap = [None]
    l_con = VC.contrastive_loss_ragged(ins, outs, smax, lengths, 0.2, 0.7, clearance=gap)
    (1.7 * l_con).backward()
    return dict(vg=(float(l_vg.detach()), vg.grad), con=(float(l_con.detach()), [smax.grad, ins.grad, outs.grad]), clearance=gap[0])


@pytest.mark.parametrize('name', sorted(VC.LOSS_CASES))
def test_vg_loss_ragged_against_the_fp64_definition(name):
    B, L, Rn, lengths = VC.LOSS_CASES[name]
    vg = VC.loss_inputs(name)[0]
    want, want_g = _loss_reference(name)['vg']
    v, g, status = _vg(vg, _lens(lengths))
    err_v = abs(float(v) - want) / max(1.0, abs(want))
    err_g = float((g.cpu().double() / 1.7 - want_g / 1.7).abs().max()) / max(1.0, float((want_g / 1.7).abs().max()))
    print('vg %s: value %.6f (fp64 %.6f, err %.2e), gradient err %.2e of scale' % (name, float(v), want, err_v, err_g))
    assert status == 0
    assert err_v <= VC.VG_BOUND
    assert float((g.cpu().double() - want_g).abs().max()) <= VC.VG_BOUND * max(1.0, float(want_g.abs().max()))
    words = VC.word_mask(L, lengths)
    assert not g.cpu().permute(0, 2, 1, 3)[~words].any()                 # d vg[a, :, l, :] for l >= n_a: exactly 0
    assert float(want_g.abs().max()) > 1e-4
    # NaN in every word beyond a sentence's length changes no bit
    vn, gn, _ = _vg(VC.poison(vg.permute(0, 2, 1, 3), words).permute(0, 2, 1, 3).contiguous(), _lens(lengths))
    assert torch.equal(v, vn) and torch.equal(g, gn)
    # every length = L: the bits of cliora_vg_loss
    full = _vg(vg, _lens([L] * B))
    old = _vg(vg, None)
    assert torch.equal(full[0], old[0]) and torch.equal(full[1], old[1]) and full[2] == 0


@pytest.mark.parametrize('name', sorted(VC.LOSS_CASES))
def test_contrastive_loss_ragged_against_the_fp64_definition(name):
    B, L, Rn, lengths = VC.LOSS_CASES[name]
    _, smax, ins, outs = VC.loss_inputs(name)
    ref = _loss_reference(name)
    want, want_g = ref['con']
    # the inputs keep every hinge argument clear of its kink, where fp32 and fp64 may take different sides (a property of the seeded
    # inputs, as in test_fused_contrastive_loss_matches_the_torch_formula, whose inputs these are)
    assert ref['clearance'] >= VC.HINGE_CLEARANCE, ref['clearance']
    v, g, status = _contrastive(smax, ins, outs, _lens(lengths))
    err_v = abs(float(v) - want) / max(1.0, abs(want))
    errs = [float((a.cpu().double() - b).abs().max()) / max(1.0, float(b.abs().max())) for a, b in zip(g, want_g)]
    print('contrastive %s: value %.6f (fp64 %.6f, err %.2e), gradient errs of scale %s' % (name, float(v), want, err_v, ' '.join('%.2e' % e for e in errs)))
    assert status == 0
    assert err_v <= VC.CONTRASTIVE_VALUE_BOUND
    rel, floor = VC.CONTRASTIVE_GRAD_BOUND
    for a, b in zip(g, want_g):
        assert float((a.cpu().double() - b).abs().max()) <= rel * max(1.0, float(b.abs().max())) + floor
    assert want > 0 and float(want_g[0].abs().max()) > 1e-4
    own = torch.from_numpy(TC.own_mask(L, lengths))
    d_smax, d_ins, d_outs = [x.cpu() for x in g]
    assert not d_smax.permute(0, 2, 1)[~own].any() and not d_ins[~own].any() and not d_outs[~own].any()
    # NaN in every input beyond the triangles changes no bit
    vn, gn, _ = _contrastive(VC.poison(smax.permute(0, 2, 1), own).permute(0, 2, 1).contiguous(), VC.poison(ins, own), VC.poison(outs, own),
                             _lens(lengths))
    assert torch.equal(v, vn) and all(torch.equal(a, b) for a, b in zip(g, gn))
    # every length = L: the bits of cliora_contrastive_loss
    full = _contrastive(smax, ins, outs, _lens([L] * B))
    old = _contrastive(smax, ins, outs, None)
    assert torch.equal(full[0], old[0]) and all(torch.equal(a, b) for a, b in zip(full[1], old[1])) and full[2] == 0


def test_loss_entries_count_bad_lengths_and_write_nothing_for_them():
    B, L, Rn, lengths = VC.LOSS_CASES['B6']
    vg, smax, ins, outs = VC.loss_inputs('B6')
    bad = list(lengths)
    bad[1], bad[4] = 0, L + 1
    v, g, status = _vg(vg, _lens(bad))
    assert status == 2 and bool(torch.isfinite(v)) and bool(torch.isfinite(g).all())
    assert not g[1].any() and not g[4].any() and g[0].any()
    v, g, status = _contrastive(smax, ins, outs, _lens(bad))
    assert status == 2 and bool(torch.isfinite(v)) and all(bool(torch.isfinite(x).all()) for x in g)
    for x in (1, 4):
        assert not g[0][x].any() and not g[1][x].any() and not g[2][x].any()
    assert g[0][0].any() and g[1][0].any()


# ---- 2. the chart -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the oracle's results of a case, computed once and shared."""
    D, Rn, lengths, share = VC.GPU_CASES[name]
    L = max(lengths)
    P, xs, objs, mask = VC.vl_case(D, Rn, lengths, seed=900 + D, share=share)
    W = TC.weights(L, lengths, D, seed=17)
    loss, grads, dxs, dobjs, charts = VC.oracle_sum(P, xs, objs, lengths, W, mask, 'unit', share)
    return dict(D=D, R=Rn, L=L, lengths=lengths, share=share, P=P, xs=xs, xp=ROC.padded(xs, L), obj=torch.stack(objs), mask=mask, W=W, loss=loss,
                grads=grads, dxs=dxs, dobjs=dobjs, charts=charts)


def _module(c):
    from cliora_amd.cliora import DioraMLP
    m = DioraMLP(c['D'], outside=True, normalize='unit', compress=False, share=c['share'])
    sd = m.state_dict()
    for k in sd:
        src = 'inside_' + k[len('outside_'):] if c['share'] and k.startswith('outside_') else k
        sd[k] = c['P'][src].detach().clone()
    m.load_state_dict(sd)
    return m.cuda().train()


def _run(m, c, lengths, W, ragged=True, mask=None):
    """Forward + backward with the cotangents W -> dict(charts, grads {parameter name: tensor}, dx, dobj)."""
    from cliora_amd import ragged as RG
    for p in m.parameters():
        p.grad = None
    x = c['xp'].clone().cuda().requires_grad_(True)
    obj = c['obj'].clone().cuda().requires_grad_(True)
    m.dropout_mask = (c['mask'] if mask is None else mask).cuda()
    if ragged:
        m._ragged_train = (_lens(lengths), RG.root_level_mask(lengths))
    try:
        m(x, x.detach(), obj, obj.detach())
    finally:
        m._ragged_train = None
    if ragged:
        assert int(m._ragged_status.item()) == 0
    ch = m.chart
    charts = [ch.inside_h, ch.inside_s, ch.outside_h, ch.outside_s]
    torch.autograd.backward(charts, [w.float().cuda() for w in W])
    torch.cuda.synchronize()
    return dict(charts=[t.detach().clone() for t in charts], grads={n: p.grad.clone() for n, p in m.named_parameters()}, dx=x.grad.clone(),
                dobj=obj.grad.clone())


def _same_bits(a, b, what):
    for k, (u, v) in enumerate(zip(a['charts'], b['charts'])):
        assert torch.equal(u, v), (what, TC.CHARTS[k])
    assert sorted(a['grads']) == sorted(b['grads'])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), (what, k)
    assert torch.equal(a['dx'], b['dx']), (what, 'dx')
    assert torch.equal(a['dobj'], b['dobj']), (what, 'dobj')


@pytest.mark.parametrize('name', sorted(VC.GPU_CASES))
def test_charts_and_gradients_against_the_oracle(name, mfma_mode):
    c = _case(name)
    lengths, L = c['lengths'], c['L']
    m = _module(c)
    got = _run(m, c, lengths, c['W'])
    worst = dict.fromkeys(TC.CHARTS, 0.0)
    fails = []
    for b, n in enumerate(lengths):                      # the charts on each own triangle
        own = torch.from_numpy(ROC.own_cells(L, n))
        for k, cname in enumerate(TC.CHARTS):
            have, want = got['charts'][k][b].cpu().double()[own], c['charts'][b][cname]
            assert bool(torch.isfinite(have).all()), (cname, b, n)
            err = float(((have - want).abs() / want.abs().clamp(min=1.0)).max())
            worst[cname] = max(worst[cname], err)
            if err > VC.FORWARD_BOUND:
                fails.append((cname, b, n, err))
    print('%s %s charts, worst relative errors: %s' % (name, mfma_mode, ', '.join('%s %.3e' % kv for kv in worst.items())))
    assert not fails, fails[:8]
    assert sorted(got['grads']) == sorted(c['grads'])
    have_dx = torch.cat([got['dx'][b, :n].cpu().double().reshape(-1) for b, n in enumerate(lengths)])
    want_dx = torch.cat([d.reshape(-1) for d in c['dxs']])
    pairs = [(k, got['grads'][k].cpu().double(), c['grads'][k]) for k in sorted(c['grads'])]
    pairs += [('d x_span', have_dx, want_dx), ('d obj_span', got['dobj'].cpu().double(), torch.stack(c['dobjs']))]
    for k, have, want in pairs:                          # the figures first, then the gradients
        d = (have - want).abs().flatten()
        sc = max(1.0, float(want.abs().max()))
        print('%s %s grad %-40s max err %.3e median %.3e of scale %.3e' % (name, mfma_mode, k, float(d.max()) / sc, float(d.median()) / sc, sc))
    moved = 0
    for k, have, want in pairs:
        assert bool(torch.isfinite(have).all()), k
        grad_check(have, want, mfma_mode, VC.GRAD_STRICT, '%s %s' % (name, k))
        moved += int(float(want.abs().max()) > 1e-2)
    assert moved >= 4 and float(torch.stack(c['dobjs']).abs().max()) > 1e-2          # a reference that moves the tensors, the regions too
    for b, n in enumerate(lengths):                      # d x of the padded positions: exactly 0
        assert not got['dx'][b, n:].any(), (b, n)


@pytest.mark.parametrize('name', ['D32-R4', 'D24-R5', 'D32-R4-unshared'])
def test_nan_cotangents_two_runs_and_both_chain_schedules_give_equal_bits(name, mfma_mode):
    from cliora_amd import _lib
    c = _case(name)
    m = _module(c)
    first = _run(m, c, c['lengths'], c['W'])
    _same_bits(first, _run(m, c, c['lengths'], c['W']), 'second run')
    Wn = TC.weights(c['L'], c['lengths'], c['D'], seed=17, beyond=float('nan'))
    assert any(bool(torch.isnan(w).any()) for w in Wn)
    _same_bits(first, _run(m, c, c['lengths'], Wn), 'NaN beyond the triangles')
    prev = _lib.set_wavefront('off')
    try:
        for mode in ('off', 'on'):                       # CLIORA_WAVEFRONT 0 / 1
            _lib.set_wavefront(mode)
            _same_bits(first, _run(m, c, c['lengths'], c['W']), 'wavefront ' + mode)
    finally:
        _lib.set_wavefront(prev)


def _c_run(m, c, fill):
    """Both entries through the C ABI, every buffer the library is handed -- outputs, workspaces, masked-cotangent buffers, gradients --
    filled with `fill` first.  -> (charts, grads by _lib.PARAM_FIELDS name, dx, dobj, status)."""
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import _param_struct, _ptr, _stream
    xp, lengths = c['xp'], c['lengths']
    B, L, D = xp.shape
    plan = _lib.get_plan(B, L, D, m.share, m.normalize, c['R'], 0)
    Cc = plan.C

    def buf(*shape):
        return torch.empty(shape, device='cuda', dtype=torch.float32).fill_(fill)
    ptens = {k: (v.detach().contiguous() if v is not None else None) for k, v in zip(_lib.PARAM_FIELDS, m._param_tensors())}
    pst = _param_struct(ptens)
    x, obj, drop, lens = xp.clone().cuda().contiguous(), c['obj'].clone().cuda().contiguous(), c['mask'].cuda().contiguous(), _lens(lengths)
    mask = ragged.root_level_mask(lengths)
    outs = [buf(B, Cc, D), buf(B, Cc, 1), buf(B, Cc, D), buf(B, Cc, 1)]
    inside_c = buf(B, Cc, D)
    ws, wsb = buf((plan.fwd_bytes + 3) // 4), buf((plan.bwd_bytes + 3) // 4)
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    _lib.call('cliora_chart_forward_ragged_train_vl', plan.handle, C.byref(pst), _ptr(x), _ptr(obj), _ptr(drop), *map(_ptr, outs), _ptr(inside_c),
              _ptr(ws), plan.fwd_bytes, 1, _ptr(lens), mask, _ptr(status), _stream())
    cots = [w.float().cuda().contiguous() for w in c['W']]
    masked = [buf(*t.shape) for t in cots]
    g = {k: (buf(*t.shape) if t is not None else None) for k, t in ptens.items()}
    gst = _param_struct(g)
    dx, dobj = buf(B, L, D), buf(*obj.shape)
    _lib.call('cliora_chart_backward_ragged_vl', plan.handle, C.byref(pst), _ptr(x), _ptr(obj), _ptr(drop), *map(_ptr, outs), *map(_ptr, cots), None,
              _ptr(ws), plan.fwd_bytes, _ptr(wsb), plan.bwd_bytes, _ptr(dx), _ptr(dobj), C.byref(gst), 1, _ptr(lens), mask,
              *map(_ptr, masked), _stream())
    torch.cuda.synchronize()
    return outs, {k: v for k, v in g.items() if v is not None}, dx, dobj, int(status.item())


@pytest.mark.parametrize('name', ['D32-R4', 'D24-R5', 'D128-R36'])
def test_nan_filled_workspaces_change_nothing(name, mfma_mode):
    """The attention backward runs over every cell of a level; a cell beyond a triangle must add an exact zero whatever the buffers
    held before the call."""
    from cliora_amd import _lib
    c = _case(name)
    m = _module(c)
    zero, nan = (_c_run(m, c, f) for f in (0.0, float('nan')))
    assert zero[4] == 0 and nan[4] == 0
    for b, n in enumerate(c['lengths']):                 # the charts beyond a triangle are unspecified: the own cells are compared
        own = torch.from_numpy(ROC.own_cells(c['L'], n)).cuda()
        for u, v in zip(zero[0], nan[0]):
            assert torch.equal(u[b, own], v[b, own]), (b, n)
    for k in zero[1]:
        assert torch.equal(zero[1][k], nan[1][k]) and bool(torch.isfinite(nan[1][k]).all()), k
    for i in (2, 3):
        assert torch.equal(zero[i], nan[i]) and bool(torch.isfinite(nan[i]).all())
    got = _run(m, c, c['lengths'], c['W'])               # ... and the module's node computes what the entries compute
    assert torch.equal(got['dx'], nan[2]) and torch.equal(got['dobj'], nan[3])
    for field, t in zip(_lib.PARAM_FIELDS, m._param_tensors()):
        if t is not None:
            pname = [n for n, p in m.named_parameters() if p is t][0]
            assert torch.equal(got['grads'][pname], nan[1][field]), field


@pytest.mark.parametrize('name', sorted(VC.GPU_CASES))
def test_every_length_equal_to_L_is_chart_function_bit_for_bit(name, mfma_mode):
    c = _case(name)
    B, L = len(c['lengths']), c['L']
    m = _module(c)
    full = [L] * B
    W = TC.weights(L, full, c['D'], seed=23)
    want = _run(m, c, full, W, ragged=False)
    got = _run(m, c, full, W)
    _same_bits(want, got, 'lengths = L')


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_vl_entries():
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import _param_struct, _ptr, _stream
    D, B, L, Rn = 32, 2, 5, 4
    lib = _lib.lib()
    x = torch.randn(B, L, D).cuda()
    lens = _lens([5, 3])
    mask = ragged.root_level_mask([5, 3])
    status = torch.zeros(1, dtype=torch.int32).cuda()
    c = dict(D=D, share=True, P=ROC.small_case(D, [5, 3], seed=1)[0])
    m = _module(c)

    def call(entry, plan, flags=1, compress=False, obj=True):
        names = dict(zip(_lib.PARAM_FIELDS, m._param_tensors()))
        if compress:
            names['root_mat'] = torch.randn(D, D).cuda()
        pst = _param_struct({k: (v.detach().contiguous() if v is not None else None) for k, v in names.items()})
        Cc = plan.C
        bufs = [torch.zeros(B, Cc, D).cuda(), torch.zeros(B, Cc, 1).cuda(), torch.zeros(B, Cc, D).cuda(), torch.zeros(B, Cc, 1).cuda()]
        ic = torch.zeros(B, Cc, D).cuda()
        ws = torch.empty(plan.fwd_bytes + plan.pair_bytes, dtype=torch.uint8).cuda()
        dm = torch.ones(B, Cc, Rn).cuda()
        ob = torch.randn(B, Rn, D).cuda() if obj else None
        if entry == 'forward':
            rc = lib.cliora_chart_forward_ragged_train_vl(plan.handle, C.byref(pst), _ptr(x), _ptr(ob), _ptr(dm), *map(_ptr, bufs), _ptr(ic), _ptr(ws),
                                                          ws.numel(), flags, _ptr(lens), mask, _ptr(status), _stream())
        else:
            wsb = torch.empty(max(plan.bwd_bytes, 4), dtype=torch.uint8).cuda()
            g = _param_struct({k: (torch.empty_like(v) if v is not None else None) for k, v in names.items()})
            rc = lib.cliora_chart_backward_ragged_vl(plan.handle, C.byref(pst), _ptr(x), _ptr(ob), _ptr(dm), *map(_ptr, bufs), *map(_ptr, bufs), None,
                                                     _ptr(ws), ws.numel(), _ptr(wsb), wsb.numel(), _ptr(torch.empty_like(x)),
                                                     _ptr(torch.empty(B, Rn, D).cuda()), C.byref(g), flags, _ptr(lens), mask,
                                                     *map(_ptr, [torch.empty_like(t) for t in bufs]), _stream())
        torch.cuda.synchronize()
        return rc, lib.cliora_last_error().decode()

    plan = _lib.get_plan(B, L, D, True, 'unit', Rn, 0)
    assert call('forward', plan)[0] == 0 and int(status.item()) == 0
    text_plan = _lib.get_plan(B, L, D, True, 'unit', 0, 0)
    lstm_plan = _lib.get_plan(B, L, D, True, 'unit', 0, 0, arch=1)
    long_plan = _lib.get_plan(B, 65, D, True, 'unit', Rn, 0)
    for entry in ('forward', 'backward'):
        name = 'cliora_chart_%s_ragged' % entry + ('_train_vl' if entry == 'forward' else '_vl')
        cases = [(dict(plan=text_plan, obj=False), 'text-only plans'), (dict(plan=plan, obj=False), 'needs obj_span'),
                 (dict(plan=plan, compress=True), 'compress'), (dict(plan=lstm_plan), 'TreeLSTM'),
                 (dict(plan=plan, flags=1 | _lib.FWD_PAIR_STATES), 'PAIR_STATES'), (dict(plan=long_plan), 'L > 64')]
        if entry == 'forward':
            cases.append((dict(plan=plan, flags=1 | _lib.FWD_NO_BACKWARD), 'NO_BACKWARD'))
        seen = set()
        for kw, word in cases:
            rc, msg = call(entry, **kw)
            assert rc != 0 and word in msg and msg.startswith(name + ':'), (entry, word, rc, msg)
            seen.add(msg)
        assert len(seen) == len(cases)                   # each with a message of its own
    # the module under no_grad has no use for the training state
    m._ragged_train = (lens, mask)
    try:
        with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='gradients enabled'):
            m(x, x, torch.randn(B, Rn, D).cuda(), torch.randn(B, Rn, D).cuda())
    finally:
        m._ragged_train = None


# ---- 4. one optimizer step ------------------------------------------------------------------------------------------------------------
STEP_LENGTHS = [7, 1, 3, 2, 6, 3, 5, 4, 7]
STEP = dict(D=32, V=97, R=4, img=16, K=5, lr=2e-3, margin=0.2, alpha_contr=1.0, alpha_vg=1.0)


def _step_net(seed=41, **weights):
    from cliora_amd import harness as H
    s = STEP
    torch.manual_seed(seed)
    net = H.build_net(s['D'], torch.nn.Embedding(s['V'], 32), obj_feats=True, img_dim=s['img'], k_neg=s['K'], vg_loss=True, use_contr=True,
                      vl_margin=s['margin'], alpha_contr=s['alpha_contr'], alpha_vg=s['alpha_vg'], **weights)
    for p in net.img_encoder.parameters():               # built as zeros: every region score would tie
        p.data.normal_(0.0, 0.2)
    # the bilinear scores as drawn run to +-6 a level and the contrastive marginals exp(in_s + out_s - in_s[root]) to 1e6: scaled so
    # that the three terms are of one order and the bound on the total holds each of them
    for m in {net.diora.inside_score_func, net.diora.outside_score_func}:
        m.mat.data.mul_(0.1)
    return net


def _step_data(lengths, seed=4):
    s = STEP
    rs = np.random.RandomState(seed)
    sentences = [rs.randint(1, s['V'], size=n).tolist() for n in lengths]
    neg = torch.from_numpy(rs.randint(1, s['V'], size=s['K']))
    feats = torch.relu(torch.randn(len(lengths), s['R'], s['img'], generator=torch.Generator().manual_seed(seed)))
    L = max(lengths)
    torch.manual_seed(seed + 1)
    mask = torch.nn.functional.dropout(torch.ones(len(lengths), L * (L + 1) // 2, s['R']), 0.1, True)      # rows in PACK order
    return sentences, neg, feats, mask


def test_step_ragged_with_regions_is_one_adam_step_on_the_oracles_gradients(mfma_mode):
    from cliora_amd import harness as H, ragged
    s = STEP
    net = _step_net()
    assert net.loss_func_names == ['reconstruct_softmax_loss', 'vg_loss', 'contrastive_loss']
    sentences, neg, feats, mask = _step_data(STEP_LENGTHS)
    (order,) = ragged.pack([len(x) for x in sentences], 64, float('inf'))      # one pack; its chart holds the sentences in this order
    # the oracle in fp64: token-weighted reconstruction + the two restatements, its gradients, clip_grad_norm_(5.0) and one Adam step
    sd = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, p in net.named_parameters() if p.requires_grad}
    want_loss, terms = VC.oracle_step_loss(sd, [sentences[i] for i in order], feats[order].double(), neg, mask, s['margin'], s['alpha_contr'],
                                           s['alpha_vg'])
    want_loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    start = {k: v.detach().clone() for k, v in leaves.items()}
    for k, v in leaves.items():
        v.grad = grads[k].clone()
    torch.nn.utils.clip_grad_norm_(list(leaves.values()), 5.0)
    clipped = {k: v.grad.clone() for k, v in leaves.items()}
    torch.optim.Adam(list(leaves.values()), lr=s['lr'], betas=(0.9, 0.999), eps=1e-8).step()
    net = net.cuda()
    net.diora.dropout_mask = mask.cuda()
    tr = H.Trainer(net, lr=s['lr'])
    out = tr.step_ragged(sentences, neg_samples=neg.cuda(), obj_feats=feats.cuda(), max_waste=float('inf'))
    torch.cuda.synchronize()
    print('step_ragged %s: loss %.6f, oracle %.6f (%s)' % (mfma_mode, out['total_loss'], float(want_loss.detach()),
                                                           ', '.join('%s %.6f' % (k, float(v.detach())) for k, v in terms.items())))
    vals = [float(v.detach()) for v in terms.values()]
    assert min(vals) > 1e-2 and max(vals) <= 100 * min(vals)             # three terms that count in the total
    assert abs(out['total_loss'] - float(want_loss.detach())) <= 1e-4 * max(1.0, abs(float(want_loss.detach())))
    assert net.training
    for k, p in net.named_parameters():
        if k not in leaves:
            continue
        have, want = p.detach().cpu().double(), leaves[k].detach()
        # as test_gpu_ragged_train.py: where the oracle's gradient is within the accepted gradient error its sign is not determined
        # and Adam's first step is held to its reach, lr; every other element to grad_check.  A gradient of exactly 0 is such an
        # element here: img_encoder.fc_vis.bias adds the same amount to every region's and every image's VG logit, which cancels in
        # the cross entropy, so its true gradient is zero and the device's is rounding residue (test_gpu_harness.py meets the same).
        noise = clipped[k].abs() <= VC.GRAD_STRICT * max(1.0, float(clipped[k].abs().max()))
        if noise.any():
            assert float((have - start[k])[noise].abs().max()) <= s['lr'] * (1 + 1e-3), k
        if (~noise).any():
            grad_check(have[~noise], want[~noise], mfma_mode, VC.GRAD_STRICT, k)
        assert float((have - start[k]).abs().max()) > 0 or not grads[k].any(), k
    assert any(grads[k].any() for k in leaves if k.startswith('img_encoder.'))


def test_step_ragged_with_regions_at_one_length_is_step_and_takes_the_structured_terms():
    from cliora_amd import harness as H
    s = STEP
    same_lengths = [6] * 5
    sentences, neg, feats, mask = _step_data(same_lengths, seed=9)
    labels = [[('np', b % 3, 3), ('np', 0, 5)] for b in range(5)]

    def trainer(**weights):
        net = _step_net(seed=43, **weights).cuda()
        return H.Trainer(net, lr=s['lr'])
    tr = trainer()
    tr.net.diora.dropout_mask = mask.cuda()
    want = tr.step(dict(sentences=torch.tensor(sentences).cuda(), neg_samples=neg.cuda(), obj_feats=feats.cuda()))['total_loss']
    tr = trainer()
    tr.net.diora.dropout_mask = mask.cuda()
    got = tr.step_ragged(sentences, neg_samples=neg.cuda(), obj_feats=feats.cuda())['total_loss']
    print('one length: step %.6f, step_ragged %.6f' % (want, got))
    assert abs(got - want) <= 1e-4 * max(1.0, abs(want))
    mixed, neg, feats, mask = _step_data(STEP_LENGTHS)
    mixed_labels = [[('np', 0, 2), ('np', 1, n - 1)] if n >= 4 else [] for n in STEP_LENGTHS]
    res = {}
    for w in (0.0, 1.0):
        tr = trainer(bracket_loss_weight=w)
        tr.net.diora.dropout_mask = mask.cuda()
        res[w] = tr.step_ragged(mixed, neg_samples=neg.cuda(), obj_feats=feats.cuda(), entity_labels=mixed_labels, max_waste=float('inf'))['total_loss']
        assert all(bool(torch.isfinite(p).all()) for p in tr.net.parameters())
    print('mixed lengths: without the bracket term %.6f, with it %.6f' % (res[0.0], res[1.0]))
    assert np.isfinite(res[1.0]) and abs(res[1.0] - res[0.0]) > 1e-2
