"""Training text-only DIORA through a padded chart of mixed lengths on the device (cliora_chart_forward_ragged_train,
cliora_chart_backward_ragged, diora.RaggedChartFunction, ragged.forward_ragged_train, Trainer.step_ragged).
The yardstick is the fp64 oracle on one sentence at its exact length, summed over the sentences (ragged_train_cases.oracle_sum);
bitwise claims are against the library's existing entries and against a second run."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ragged_outside_cases as ROC
import ragged_train_cases as TC
from conftest import grad_check

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs and the oracle's results of a case, computed once and shared."""
    D, lengths, share, normalize, scale = TC.GPU_CASES[name]
    L = max(lengths)
    P, xs, _ = ROC.small_case(D, lengths, seed=900 + D, share=share, scale=scale)
    W = TC.weights(L, lengths, D, seed=17)
    loss, grads, dxs, charts = TC.oracle_sum(P, xs, lengths, W, normalize, share)
    return dict(D=D, L=L, lengths=lengths, share=share, normalize=normalize, P=P, xs=xs, xp=ROC.padded(xs, L), W=W, loss=loss, grads=grads,
                dxs=dxs, charts=charts)


def _module(c):
    from test_gpu_parity import _module_from_params
    return _module_from_params(c['P'], c['D'], c['share'], c['normalize']).train()


def _lens(lengths):
    return torch.tensor(lengths, dtype=torch.int32).cuda()


def _forward(m, x, lengths):
    """The module's training forward through RaggedChartFunction -> the four charts (in the graph); the status word must be 0."""
    from cliora_amd import ragged
    m._ragged_train = (_lens(lengths), ragged.root_level_mask(lengths))
    try:
        m(x, x)
    finally:
        m._ragged_train = None
    assert int(m._ragged_status.item()) == 0
    ch = m.chart
    return [ch.inside_h, ch.inside_s, ch.outside_h, ch.outside_s]


def _run(m, xp, lengths, W, ragged=True):
    """Forward + backward with the cotangents W -> dict(charts, grads {parameter name: tensor}, dx)."""
    for p in m.parameters():
        p.grad = None
    x = xp.clone().cuda().requires_grad_(True)
    if ragged:
        charts = _forward(m, x, lengths)
    else:
        m(x, x)
        charts = [m.chart.inside_h, m.chart.inside_s, m.chart.outside_h, m.chart.outside_s]
    torch.autograd.backward(charts, [w.float().cuda() for w in W])
    torch.cuda.synchronize()
    return dict(charts=[t.detach().clone() for t in charts], grads={n: p.grad.clone() for n, p in m.named_parameters()}, dx=x.grad.clone())


def _same_bits(a, b, what):
    for k, (u, v) in enumerate(zip(a['charts'], b['charts'])):
        assert torch.equal(u, v), (what, TC.CHARTS[k])
    assert sorted(a['grads']) == sorted(b['grads'])
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), (what, k)
    assert torch.equal(a['dx'], b['dx']), (what, 'dx')


# ---- items 1-3: against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(TC.GPU_CASES))
def test_charts_and_gradients_against_the_oracle(name, mfma_mode):
    c = _case(name)
    lengths, L = c['lengths'], c['L']
    m = _module(c)
    got = _run(m, c['xp'], lengths, c['W'])
    worst = dict.fromkeys(TC.CHARTS, 0.0)
    fails = []
    for b, n in enumerate(lengths):                      # 1. the charts on each own triangle
        own = torch.from_numpy(ROC.own_cells(L, n))
        for k, cname in enumerate(TC.CHARTS):
            have, want = got['charts'][k][b].cpu().double()[own], c['charts'][b][cname]
            assert bool(torch.isfinite(have).all()), (cname, b, n)
            err = float(((have - want).abs() / want.abs().clamp(min=1.0)).max())
            worst[cname] = max(worst[cname], err)
            if err > TC.FORWARD_BOUND:
                fails.append((cname, b, n, err))
    print('%s %s charts, worst relative errors: %s' % (name, mfma_mode, ', '.join('%s %.3e' % kv for kv in worst.items())))
    assert not fails, fails[:8]
    assert sorted(got['grads']) == sorted(c['grads'])
    have_dx = torch.cat([got['dx'][b, :n].cpu().double().reshape(-1) for b, n in enumerate(lengths)])
    want_dx = torch.cat([d.reshape(-1) for d in c['dxs']])
    pairs = [(k, got['grads'][k].cpu().double(), c['grads'][k]) for k in sorted(c['grads'])] + [('d x_span', have_dx, want_dx)]
    for k, have, want in pairs:                          # the figures first, then 2. the gradients
        d = (have - want).abs().flatten()
        sc = max(1.0, float(want.abs().max()))
        print('%s %s grad %-40s max err %.3e median %.3e of scale %.3e' % (name, mfma_mode, k, float(d.max()) / sc, float(d.median()) / sc, sc))
    moved = 0
    for k, have, want in pairs:
        assert bool(torch.isfinite(have).all()), k
        grad_check(have, want, mfma_mode, TC.GRAD_STRICT, '%s %s' % (name, k))
        moved += int(float(want.abs().max()) > 1e-2)
    assert moved >= 3                                    # a reference that moves the tensors
    for b, n in enumerate(lengths):                      # 3. d x of the padded positions: exactly 0
        assert not got['dx'][b, n:].any(), (b, n)


# ---- items 4, 5, 7: what must not get through, and two runs ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['D32', 'D24', 'D32-unshared'])
def test_nan_cotangents_beyond_the_triangles_change_nothing_and_two_runs_agree(name, mfma_mode):
    c = _case(name)
    m = _module(c)
    first = _run(m, c['xp'], c['lengths'], c['W'])
    _same_bits(first, _run(m, c['xp'], c['lengths'], c['W']), 'second run')
    Wn = TC.weights(c['L'], c['lengths'], c['D'], seed=17, beyond=float('nan'))
    assert any(bool(torch.isnan(w).any()) for w in Wn)
    _same_bits(first, _run(m, c['xp'], c['lengths'], Wn), 'NaN beyond the triangles')


def _c_run(m, xp, lengths, W, fill=None, flags=1, root_levels=None, d_split=None):
    """Both entries through the C ABI, every buffer the library is handed -- outputs, workspaces, masked-cotangent buffers, gradients --
    filled with `fill` first.  -> (charts, grads by _lib.PARAM_FIELDS name, dx, status)."""
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import _param_struct, _ptr, _stream
    B, L, D = xp.shape
    plan = _lib.get_plan(B, L, D, m.share, m.normalize, 0, 0)
    Cc = plan.C

    def buf(*shape):
        t = torch.empty(shape, device='cuda', dtype=torch.float32)
        return t if fill is None else t.fill_(fill)
    ptens = {k: (v.detach().contiguous() if v is not None else None) for k, v in zip(_lib.PARAM_FIELDS, m._param_tensors())}
    pst = _param_struct(ptens)
    x, lens = xp.clone().cuda().contiguous(), _lens(lengths)
    mask = ragged.root_level_mask(lengths) if root_levels is None else root_levels
    outs = [buf(B, Cc, D), buf(B, Cc, 1), buf(B, Cc, D), buf(B, Cc, 1)]
    ws, wsb = buf((plan.fwd_bytes + 3) // 4), buf((plan.bwd_bytes + 3) // 4)
    status = torch.full((1,), 77, dtype=torch.int32, device='cuda')
    _lib.call('cliora_chart_forward_ragged_train', plan.handle, C.byref(pst), _ptr(x), None, None, *map(_ptr, outs), None, _ptr(ws),
              plan.fwd_bytes, flags, _ptr(lens), mask, _ptr(status), _stream())
    cots = [w.float().cuda().contiguous() for w in W]
    masked = [buf(*t.shape) for t in cots]
    g = {k: (buf(*t.shape) if t is not None else None) for k, t in ptens.items()}
    gst = _param_struct(g)
    dx = buf(B, L, D)
    _lib.call('cliora_chart_backward_ragged', plan.handle, C.byref(pst), _ptr(x), None, None, *map(_ptr, outs), *map(_ptr, cots), _ptr(d_split),
              _ptr(ws), plan.fwd_bytes, _ptr(wsb), plan.bwd_bytes, _ptr(dx), None, C.byref(gst), flags & 1, _ptr(lens), mask,
              *map(_ptr, masked), _stream())
    torch.cuda.synchronize()
    return outs, {k: v for k, v in g.items() if v is not None}, dx, int(status.item())


@pytest.mark.parametrize('name', ['D32', 'D24', 'D128'])
def test_nan_filled_workspaces_change_nothing(name, mfma_mode):
    c = _case(name)
    m = _module(c)
    zero, nan = (_c_run(m, c['xp'], c['lengths'], c['W'], fill=f) for f in (0.0, float('nan')))
    assert zero[3] == 0 and nan[3] == 0
    for b, n in enumerate(c['lengths']):                 # the charts beyond a triangle are unspecified: the own cells are compared
        own = torch.from_numpy(ROC.own_cells(c['L'], n)).cuda()
        for u, v in zip(zero[0], nan[0]):
            assert torch.equal(u[b, own], v[b, own]), (b, n)
    for k in zero[1]:
        assert torch.equal(zero[1][k], nan[1][k]) and bool(torch.isfinite(nan[1][k]).all()), k
    assert torch.equal(zero[2], nan[2]) and bool(torch.isfinite(nan[2]).all())
    # ... and the module's node computes what the entries compute
    from cliora_amd import _lib
    got = _run(m, c['xp'], c['lengths'], c['W'])
    assert torch.equal(got['dx'], nan[2])
    for field, t in zip(_lib.PARAM_FIELDS, m._param_tensors()):
        if t is not None:
            pname = [n for n, p in m.named_parameters() if p is t][0]
            assert torch.equal(got['grads'][pname], nan[1][field]), field


# ---- item 6: every length = L is the uniform chart node, to the bit ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['D32', 'D24', 'D128', 'D32-unshared', 'D32-none'])
def test_every_length_equal_to_L_is_chart_function_bit_for_bit(name, mfma_mode):
    from cliora_amd import _lib
    c = _case(name)
    B, L = len(c['lengths']), c['L']
    m = _module(c)
    full = [L] * B
    W = TC.weights(L, full, c['D'], seed=23)
    prev = _lib.set_resident('off')
    try:
        want = _run(m, c['xp'], full, W, ragged=False)
        got = _run(m, c['xp'], full, W)
    finally:
        _lib.set_resident(prev)
    _same_bits(want, got, 'lengths = L')


# ---- item 8: the two schedules of the backward chains ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['D32', 'D128', 'D32-unshared'])
def test_wavefront_off_and_on_give_equal_bits(name, mfma_mode):
    from cliora_amd import _lib
    c = _case(name)
    m = _module(c)
    res = {}
    prev = _lib.set_wavefront('off')
    try:
        for mode in ('off', 'on'):
            _lib.set_wavefront(mode)
            res[mode] = _run(m, c['xp'], c['lengths'], c['W'])
    finally:
        _lib.set_wavefront(prev)
    _same_bits(res['off'], res['on'], 'wavefront off / on')


# ---- item 9: the split-cotangent path ------------------------------------------------------------------------------------------------
def _bracket_sets(lengths):
    """Per sentence (required, forbidden) inside its own length: one required bracket, a forbidden one from five words on."""
    req, forb = [], []
    for n in lengths:
        req.append([(1, n - 2)] if n >= 4 else ([(0, 1)] if n == 3 else []))
        forb.append([(1, 2)] if n >= 5 else [])
    return req, forb


def test_bracket_nll_on_a_ragged_chart(mfma_mode):
    from cliora_amd import _lib, structured
    from cliora_amd.constrained import pack_brackets
    from oracle import diora_ref as R
    from structured_cases import GRAD_BOUND, BOUND, torch_log_prob
    from test_gpu_posterior import _scores
    c = _case('D32')
    lengths, L, B = c['lengths'], c['L'], len(c['lengths'])
    req, forb = _bracket_sets(lengths)
    # the oracle: every sentence at its exact length, -log_prob by autograd, the mean over the sentences (all are feasible)
    P64 = {k: v.detach().double().requires_grad_(True) for k, v in c['P'].items()}
    total, dxs = 0.0, []
    for b, (x, n) in enumerate(zip(c['xs'], lengths)):
        x64 = x.detach().double().requires_grad_(True)
        dxs.append(x64)
        if n < 3:
            continue                                     # no inner bracket: log_prob = 0
        o = R.diora_forward(P64, x64[None], outside=True, normalize='unit', share=True, keep_pairs=True)
        rows = [(s, e, 1) for s, e in req[b]] + [(s, e, 0) for s, e in forb[b]]
        total = total - torch_log_prob({lv: s[0, :, :, 0] for lv, s in o['pair_s_in'].items()}, n, rows) / B
    total.backward()
    m = _module(c)
    x = c['xp'].clone().cuda().requires_grad_(True)
    _forward(m, x, lengths)
    # d_split of the kernel, given the lengths by the module's holder, against the fp64 restatement on the device's own scores
    brackets = pack_brackets(req, forb)
    res = structured.bracket_grad(m, brackets)
    assert res.status.tolist() == [0] and bool(res.feasible.all())
    want = structured.bracket_grad_numpy(_scores(m), lengths, brackets.numpy())
    some = 0.0
    for level, g in structured.split_rows_by_level(m._plan, res.d_split).items():
        err = float(np.abs(g.cpu().numpy().astype(np.float64) - want[level]).max())
        some = max(some, float(np.abs(want[level]).max()))
        assert err <= BOUND, (level, err)
    assert some > 1e-3                                   # gradients, not zeros
    nll = m.bracket_nll(req, forb)
    nll.backward()
    torch.cuda.synchronize()
    assert abs(float(nll.detach()) - float(total.detach())) <= BOUND * max(1.0, abs(float(total.detach())))
    moved = 0
    for k, p in m.named_parameters():
        ref = P64[k].grad
        if ref is None:                                  # the loss reads the inside pass only
            assert p.grad is None or not p.grad.any(), k
            continue
        grad_check(p.grad, ref, mfma_mode, GRAD_BOUND, k)
        moved += int(float(ref.abs().max()) > 1e-2)
    assert moved >= 3
    have_dx, want_dx = [], []
    for b, n in enumerate(lengths):
        assert not x.grad[b, n:].any()
        if dxs[b].grad is not None:
            have_dx.append(x.grad[b, :n].cpu().double().reshape(-1))
            want_dx.append(dxs[b].grad.reshape(-1))
        else:
            assert not x.grad[b, :n].any()
    grad_check(torch.cat(have_dx), torch.cat(want_dx), mfma_mode, GRAD_BOUND, 'd x_span')


# ---- item 10: one optimizer step ----------------------------------------------------------------------------------------------------
STEP_SENTENCES_LENGTHS = [7, 1, 3, 2, 6, 3, 5, 4, 7]


def test_step_ragged_is_one_adam_step_on_the_oracles_gradients(mfma_mode):
    from cliora_amd import harness as H
    D, V, K, lr = 32, 97, 5, 2e-3
    torch.manual_seed(41)
    net = H.build_net(D, torch.nn.Embedding(V, 32), k_neg=K)
    rs = np.random.RandomState(4)
    sentences = [rs.randint(1, V, size=n).tolist() for n in STEP_SENTENCES_LENGTHS]
    neg = torch.from_numpy(rs.randint(1, V, size=K))
    # the oracle in fp64: the token-weighted loss, its gradients, clip_grad_norm_(5.0) and one Adam step
    sd = {k: v.detach().double().clone() for k, v in net.state_dict().items()}
    leaves = {k: sd[k].requires_grad_(True) for k, _ in net.named_parameters()}
    want_loss = TC.oracle_step_loss(sd, sentences, neg)
    want_loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    start = {k: v.detach().clone() for k, v in leaves.items()}
    for k, v in leaves.items():
        v.grad = grads[k].clone()
    torch.nn.utils.clip_grad_norm_(list(leaves.values()), 5.0)
    clipped = {k: v.grad.clone() for k, v in leaves.items()}
    torch.optim.Adam(list(leaves.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8).step()
    net = net.cuda()
    tr = H.Trainer(net, lr=lr)
    out = tr.step_ragged(sentences, neg_samples=neg.cuda())
    torch.cuda.synchronize()
    print('step_ragged %s: loss %.6f, oracle %.6f' % (mfma_mode, out['total_loss'], float(want_loss.detach())))
    assert abs(out['total_loss'] - float(want_loss.detach())) <= 1e-4 * max(1.0, abs(float(want_loss.detach())))
    assert net.training
    for k, p in net.named_parameters():
        have, want = p.detach().cpu().double(), leaves[k].detach()
        # Adam's first step moves an element by lr g / (|g| + eps): where the oracle's gradient is no larger than the error the project
        # accepts on a gradient (GRAD_STRICT of the tensor's scale), its sign is not determined, and the element is held to the
        # step's reach from its start, lr; every other element to grad_check (test_gpu_harness.py argues the same way)
        noise = clipped[k].abs() <= TC.GRAD_STRICT * max(1.0, float(clipped[k].abs().max()))
        noise &= clipped[k] != 0                         # a gradient of exactly 0 (an embedding row no sentence uses) moves nothing
        if noise.any():
            assert float((have - start[k])[noise].abs().max()) <= lr * (1 + 1e-3), k
        if (~noise).any():
            grad_check(have[~noise], want[~noise], mfma_mode, TC.GRAD_STRICT, k)
        assert float((have - start[k]).abs().max()) > 0 or not grads[k].any(), k


def test_step_ragged_adds_the_structured_terms_the_net_weighs():
    """build_net(bracket_loss_weight=..., risk_loss_weight=..., entropy_loss_weight=...) in step_ragged: on sentences of ONE length --
    one pack, nothing padded -- the step's loss is Trainer.step's on the same batch with the same entity_labels (1e-4 relative: the
    reconstruction head sees the leaves as N sentences of one word); on mixed lengths the terms are there and finite."""
    from cliora_amd import harness as H
    D, V, K = 32, 97, 5
    rs = np.random.RandomState(9)
    neg = torch.from_numpy(rs.randint(1, V, size=K)).cuda()

    def trainer(**weights):
        torch.manual_seed(43)
        return H.Trainer(H.build_net(D, torch.nn.Embedding(V, 32), k_neg=K, **weights).cuda(), lr=2e-3)
    weights = dict(bracket_loss_weight=1.0, risk_loss_weight=0.5, entropy_loss_weight=0.05)
    same = [rs.randint(1, V, size=6).tolist() for _ in range(5)]
    labels = [[('np', b % 3, 3), ('np', 0, 5)] for b in range(5)]          # (label, pos, size): nested phrases inside six words
    want = trainer(**weights).step(dict(sentences=torch.tensor(same).cuda(), neg_samples=neg, entity_labels=labels))['total_loss']
    got = trainer(**weights).step_ragged(same, neg_samples=neg, entity_labels=labels)['total_loss']
    plain = trainer().step_ragged(same, neg_samples=neg, entity_labels=labels)['total_loss']
    print('one length: step %.6f, step_ragged %.6f, without the terms %.6f' % (want, got, plain))
    assert abs(got - want) <= 1e-4 * max(1.0, abs(want)) and abs(got - plain) > 1e-2
    mixed = [rs.randint(1, V, size=n).tolist() for n in STEP_SENTENCES_LENGTHS]
    mixed_labels = [[('np', 0, 2), ('np', 1, n - 1)] if n >= 4 else [] for n in STEP_SENTENCES_LENGTHS]
    tr = trainer(**weights)
    first = tr.step_ragged(mixed, neg_samples=neg, entity_labels=mixed_labels)['total_loss']
    base = trainer().step_ragged(mixed, neg_samples=neg)['total_loss']
    assert np.isfinite(first) and abs(first - base) > 1e-2
    assert all(bool(torch.isfinite(p).all()) for p in tr.net.parameters())


# ---- item 11: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_new_entries():
    from cliora_amd import _lib, ragged
    from cliora_amd.diora import _param_struct, _ptr, _stream
    D, B, L = 32, 2, 5
    lib = _lib.lib()
    x = torch.randn(B, L, D).cuda()
    lens = _lens([5, 3])
    mask = ragged.root_level_mask([5, 3])
    status = torch.zeros(1, dtype=torch.int32).cuda()
    P = ROC.small_case(D, [5, 3], seed=1)[0]
    from test_gpu_parity import _module_from_params
    m = _module_from_params(P, D, True, 'unit').train()

    def call(entry, plan, flags=1, compress=False, drop=False, obj=False):
        names = dict(zip(_lib.PARAM_FIELDS, m._param_tensors()))
        if compress:
            names['root_mat'] = torch.randn(D, D).cuda()
        pst = _param_struct({k: (v.detach().contiguous() if v is not None else None) for k, v in names.items()})
        Cc = plan.C
        bufs = [torch.zeros(B, Cc, D).cuda(), torch.zeros(B, Cc, 1).cuda(), torch.zeros(B, Cc, D).cuda(), torch.zeros(B, Cc, 1).cuda()]
        ws = torch.empty(plan.fwd_bytes + plan.pair_bytes, dtype=torch.uint8).cuda()
        dm = torch.ones(B, Cc, 4).cuda() if drop else None
        ob = torch.zeros(B, 4, D).cuda() if obj else None
        if entry == 'forward':
            rc = lib.cliora_chart_forward_ragged_train(plan.handle, C.byref(pst), _ptr(x), _ptr(ob), _ptr(dm), *map(_ptr, bufs), None, _ptr(ws),
                                                       ws.numel(), flags, _ptr(lens), mask, _ptr(status), _stream())
        else:
            wsb = torch.empty(max(plan.bwd_bytes, 4), dtype=torch.uint8).cuda()
            g = _param_struct({k: (torch.empty_like(v) if v is not None else None) for k, v in names.items()})
            rc = lib.cliora_chart_backward_ragged(plan.handle, C.byref(pst), _ptr(x), _ptr(ob), _ptr(dm), *map(_ptr, bufs), *map(_ptr, bufs), None,
                                                  _ptr(ws), ws.numel(), _ptr(wsb), wsb.numel(), _ptr(torch.empty_like(x)), None, C.byref(g), flags,
                                                  _ptr(lens), mask, *map(_ptr, [torch.empty_like(t) for t in bufs]), _stream())
        torch.cuda.synchronize()
        return rc, lib.cliora_last_error().decode()

    plan = _lib.get_plan(B, L, D, True, 'unit', 0, 0)
    assert call('forward', plan)[0] == 0 and int(status.item()) == 0
    vl_plan = _lib.get_plan(B, L, D, True, 'unit', 4, 0)
    lstm_plan = _lib.get_plan(B, L, D, True, 'unit', 0, 0, arch=1)
    long_plan = _lib.get_plan(B, 65, D, True, 'unit', 0, 0)
    for entry in ('forward', 'backward'):
        name = 'cliora_chart_%s_ragged' % entry
        cases = [(dict(plan=vl_plan, obj=True), 'CLIORA plans'), (dict(plan=plan, compress=True), 'compress'),
                 (dict(plan=lstm_plan), 'TreeLSTM'), (dict(plan=plan, flags=1 | _lib.FWD_PAIR_STATES), 'PAIR_STATES'),
                 (dict(plan=long_plan), 'L > 64'), (dict(plan=plan, drop=True), 'drop_mask')]
        if entry == 'forward':
            cases.append((dict(plan=plan, flags=1 | _lib.FWD_NO_BACKWARD), 'NO_BACKWARD'))
        seen = set()
        for kw, word in cases:
            rc, msg = call(entry, **kw)
            assert rc != 0 and word in msg and msg.startswith(name), (entry, word, rc, msg)
            seen.add(msg)
        assert len(seen) == len(cases)                   # each with a message of its own
    # a length of 0 or L + 1 is reported through the status word
    c = _case('D32')
    mm = _module(c)
    for bad, count in (([7, 0, 3, 2, 6, 3], 1), ([7, 1, 8, 2, 0, 3], 2)):
        lens_bad = _lens(bad)
        xs = c['xp'].clone().cuda().requires_grad_(True)
        mm._ragged_train = (lens_bad, ragged.root_level_mask(bad))
        try:
            mm(xs, xs)
        finally:
            mm._ragged_train = None
        assert int(mm._ragged_status.item()) == count
    net_sentences = [[1, 2, 3], [4]]
    from cliora_amd import harness as H
    net = H.build_net(D, torch.nn.Embedding(11, 32), k_neg=3).cuda()
    seen = list(ragged.forward_ragged_train(net, net_sentences))
    assert len(seen) >= 1 and all(int(d._ragged_status.item()) == 0 for _, _, d in seen[-1:])
    # the module: eval mode under no_grad has no use for the training state; the inference state keeps its refusal
    mm._ragged_train = (_lens(c['lengths']), ragged.root_level_mask(c['lengths']))
    try:
        with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='gradients enabled'):
            mm(c['xp'].cuda(), c['xp'].cuda())
    finally:
        mm._ragged_train = None
    mm._ragged = (_lens(c['lengths']), ragged.root_level_mask(c['lengths']))
    try:
        with pytest.raises(_lib.ChartLibError, match='inference only'):
            mm(c['xp'].cuda(), c['xp'].cuda())
    finally:
        mm._ragged = None
