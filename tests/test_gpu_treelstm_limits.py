"""DioraTreeLSTM at the limits of its plan and in both arithmetic modes, against the fp64 oracle (lstm_cases.py): padded widths
(D != Dp: the copy tables, vload_ext, pad columns that must stay exact zeros), the exact-fp32 gate projections (set_mfma_mode('f32') and
CLIORA_LSTM_PROJ=f32), run_outside = 0, L = 1 / 2 / 3 / 63 / 64, Dp = 16 / 272 / 512, the CLIORA_GEMM3_SHAPE tiles, workspaces and outputs
that arrive full of NaN, one sentence alone against the same sentence in a batch, both schedules, and the module's refusals.
Bounds: lstm_cases.OUT_TOL / GRAD_TOL, element-wise maxima in both modes (no ReLU on this path); PARITY UNPINNED as in test_gpu_treelstm.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lstm_cases as LC
from test_gpu_treelstm import _module

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = LC.KEYS


def _forward_backward(m, x, cot):
    """One training-mode forward and backward with the cotangents of `cot` -> (the six charts, x with its gradient)."""
    m.train()
    for p in m.parameters():
        p.grad = None
    xg = x.clone().cuda().requires_grad_(True)
    m(xg, xg)
    outs = {k: getattr(m, k) for k in KEYS}
    torch.autograd.backward([outs[k] for k in cot], [cot[k].cuda() for k in cot])
    torch.cuda.synchronize()
    return outs, xg


def _snapshot(m, outs, xg):
    """Every chart and gradient of a run as host arrays, by name."""
    d = {'out_' + k: v.detach().cpu().numpy() for k, v in outs.items()}
    d['x'] = xg.grad.cpu().numpy()
    d.update({k: p.grad.cpu().numpy() for k, p in m.named_parameters() if p.grad is not None})
    return d


def _check_against_oracle(get_out, get_grad, x_grad, ref, what):
    """Charts within OUT_TOL and gradients within GRAD_TOL of the fp64 oracle `ref`; a gradient the oracle does not have is None or
    all zeros.  -> (worst chart, worst gradient) relative errors."""
    errs_o = {k: LC.rel_err(get_out(k), ref['out'][k]) for k in KEYS}
    errs_g = {'x_span': LC.rel_err(x_grad, ref['x_grad'])}
    for k, g in ref['grad'].items():
        got = get_grad(k)
        if g is None:
            assert got is None or not np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got).any(), '%s: %s has a gradient the oracle has not' % (what, k)
        else:
            assert got is not None, '%s: %s has no gradient' % (what, k)
            errs_g[k] = LC.rel_err(got, g)
    for k, e in errs_o.items():
        assert e <= LC.OUT_TOL, '%s: %s %.3e' % (what, k, e)
    for k, e in errs_g.items():
        assert e <= LC.GRAD_TOL, '%s: grad %s %.3e' % (what, k, e)
    return max(errs_o.values()), max(errs_g.values())


@pytest.mark.parametrize('D,B,L,share,outside', LC.CASES)
def test_parity_at_the_limits(D, B, L, share, outside, mfma_mode):
    """One training-mode forward and backward with all cotangents at every case of lstm_cases.CASES, in both arithmetic modes: every
    chart within OUT_TOL and every gradient within GRAD_TOL of the fp64 oracle; the exact-fp32 mode within F32_OUT_TOL / F32_GRAD_TOL."""
    P, x, cot = LC.case(D, B, L, share, outside)
    ref = LC.oracle64(D, B, L, share, outside)
    m = _module(P, D, share, outside=outside)
    outs, xg = _forward_backward(m, x, cot)
    C = L * (L + 1) // 2
    for k in KEYS:       # the caller's width, not the padded one
        assert tuple(outs[k].shape) == (B, C, 1 if k.endswith('_s') else D) and outs[k].is_contiguous(), k
    assert tuple(xg.grad.shape) == (B, L, D)
    if not outside:
        for k in KEYS[3:]:
            assert float(outs[k].detach().abs().max()) == 0.0, k
    named = dict(m.named_parameters())
    for k, p in named.items():
        assert p.grad is None or (p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all())), k
    what = 'D %d B %d L %d share %d outside %d %s' % (D, B, L, share, outside, mfma_mode)
    eo, eg = _check_against_oracle(lambda k: outs[k], lambda k: named[k].grad, xg.grad, ref, what)
    print('\n%s: charts %.3e gradients %.3e  (MEASURED: %s)' % (what, eo, eg, LC.MEASURED.get((D, B, L, share, outside), {}).get(mfma_mode)))
    if mfma_mode == 'f32':
        assert eo <= LC.F32_OUT_TOL and eg <= LC.F32_GRAD_TOL, what


@pytest.mark.parametrize('D,B,L,share,outside', LC.CASES)
def test_trees_at_the_limits(D, B, L, share, outside, mfma_mode):
    """After an eval forward, cky() gives the trees of the oracle's fp64 split scores.  In the split-bf16 mode a tree may differ where
    it ties with the reference's under the REFERENCE's scores (CKY objective within 1e-4: the allowance of
    test_gpu_parity.py::test_limits_of_the_plan); the exact-fp32 mode must reproduce the trees."""
    from oracle import diora_ref as R
    P, x, _ = LC.case(D, B, L, share, outside)
    pair_s = LC.oracle64(D, B, L, share, outside)['pair_s_in']
    want = R.cky_trees(pair_s, B, L)
    m = _module(P, D, share, outside=outside).eval()
    with torch.no_grad():
        m(x.cuda(), x.cuda())
    got = m.cky()
    assert len(got) == B
    for b in range(B):
        if str(got[b]) == str(want[b]):
            continue
        assert mfma_mode == 'bf16x3', 'exact-fp32 mode must reproduce the trees (sentence %d)' % b
        gap = R.tree_score(pair_s, b, want[b]) - R.tree_score(pair_s, b, got[b])
        assert 0.0 <= gap <= 1e-4, (b, gap)


def _nan_buffers(real):
    def chart_buffers(plan, dev, flags, *widths):
        outs, ws, nbytes = real(plan, dev, flags, *widths)
        for o in outs:
            o.fill_(float('nan'))
        ws.view(torch.float32).fill_(float('nan'))
        return outs, ws, nbytes
    return chart_buffers


def _nan_block(nbytes):
    """A NaN-filled block of the backward workspace's size, freed at once: the caching allocator is likely to hand the same block to
    the backward's torch.empty (not guaranteed)."""
    t = torch.empty(nbytes, device='cuda', dtype=torch.uint8)
    t.view(torch.float32).fill_(float('nan'))
    del t


def _assert_same_bits(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.isfinite(b[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('D,B,L,share', [(33, 3, 9, False), (100, 2, 17, True)])
def test_uninitialised_buffers_are_not_read(monkeypatch, D, B, L, share):
    """The forward workspace and the six outputs come from torch.empty.  Filled with NaN before the library sees them, every chart
    and gradient must be finite and the bits of a normal run: nothing may be read before the call writes it, and a pad column may not
    pick up what the buffer held.  The forward workspace holds floats only (plan.cpp: FwdLayout; the index tables live in the plan's own
    device memory), so the whole of it is filled.  The backward half is best effort: a NaN-filled block of plan.bwd_bytes is allocated
    and freed immediately before backward, which the caching allocator is likely, not certain, to reuse for the backward workspace."""
    import cliora_amd.treelstm as T
    P, x, cot = LC.case(D, B, L, share, True)
    m = _module(P, D, share)
    first = _snapshot(m, *_forward_backward(m, x, cot))
    monkeypatch.setattr(T, 'chart_buffers', _nan_buffers(T.chart_buffers))
    m.train()
    for p in m.parameters():
        p.grad = None
    xg = x.clone().cuda().requires_grad_(True)
    m(xg, xg)
    outs = {k: getattr(m, k) for k in KEYS}
    cots = [cot[k].cuda() for k in KEYS]
    torch.cuda.synchronize()
    _nan_block(m._plan.bwd_bytes)
    torch.autograd.backward([outs[k] for k in KEYS], cots)
    torch.cuda.synchronize()
    _assert_same_bits(first, _snapshot(m, outs, xg))


def test_uninitialised_buffers_are_not_read_mlp(monkeypatch, mfma_mode):
    """The same for DioraMLP at a padded width (D 33 -> Dp 48, B 3, L 9), which has the same pad columns.  Its forward workspace keeps the
    ReLU bits of the compose outputs as integers, but writes every word before the backward reads it, so nothing is excluded."""
    import cliora_amd.diora as Dm
    from oracle import synth
    from test_gpu_parity import CHARTS, _module_from_params
    D, B, L = 33, 3, 9
    P, x, cot = synth.diora_case(D, B, L, 23)
    m = _module_from_params(P, D, True, 'unit')

    def run(nan):
        m.train()
        for p in m.parameters():
            p.grad = None
        xg = x.clone().cuda().requires_grad_(True)
        m(xg, xg)
        outs = {k: getattr(m, k) for k in CHARTS}
        cots = [cot[k].cuda() for k in CHARTS]
        torch.cuda.synchronize()
        if nan:
            _nan_block(m._plan.bwd_bytes)
        torch.autograd.backward([outs[k] for k in CHARTS], cots)
        torch.cuda.synchronize()
        return _snapshot(m, outs, xg)
    first = run(False)
    monkeypatch.setattr(Dm, 'chart_buffers', _nan_buffers(Dm.chart_buffers))
    _assert_same_bits(first, run(True))


def test_a_sentence_alone_is_the_sentence_in_its_batch():
    """Batch independence at a padded width: sentence 1 of (33, 3, 9, shared) run alone as B = 1 gives the batch's charts for that
    sentence, and -- with only that sentence's cotangents non-zero in the batch -- its x.grad, within 1e-6 of scale (the two runs use
    different row tilings: equal bits are not promised)."""
    D, B, L, share = 33, 3, 9, True
    P, x, cot = LC.case(D, B, L, share, True)
    m = _module(P, D, share)
    only1 = {k: torch.zeros_like(v) for k, v in cot.items()}
    for k in cot:
        only1[k][1] = cot[k][1]
    outs, xg = _forward_backward(m, x, only1)
    batch = {k: outs[k][1].detach().cpu().numpy().astype(np.float64) for k in KEYS}
    batch_dx = xg.grad[1].cpu().numpy().astype(np.float64)
    outs1, xg1 = _forward_backward(m, x[1:2], {k: v[1:2] for k, v in cot.items()})
    for k in KEYS:
        assert tuple(outs1[k].shape)[0] == 1
        assert LC.rel_err(outs1[k][0], batch[k]) <= 1e-6, k
    assert LC.rel_err(xg1.grad[0], batch_dx) <= 1e-6


@pytest.mark.parametrize('D,B,L,share', [(16, 1, 3, True), (33, 2, 4, False), (64, 2, 2, False)])
def test_schedules_give_the_same_bits(D, B, L, share):
    """set_wavefront('off') against 'on' at the smallest two-stream chart (L = 3, one sentence, Dp = 16), a padded unshared one, and
    L = 2, where 'on' runs on one stream (wavefront_pays_lstm) and must not fail: every output and gradient bit."""
    from cliora_amd import _lib
    P, x, cot = LC.case(D, B, L, share, True)
    m = _module(P, D, share)
    prev = _lib.set_wavefront('off')
    try:
        runs = []
        for mode in ('off', 'on'):
            _lib.set_wavefront(mode)
            runs.append(_snapshot(m, *_forward_backward(m, x, cot)))
    finally:
        _lib.set_wavefront(prev)
    _assert_same_bits(runs[0], runs[1])


SETTINGS = (('proj_f32', {'CLIORA_LSTM_PROJ': 'f32'}), ('default', {}), ('shape_0', {'CLIORA_GEMM3_SHAPE': '0'}),
            ('shape_22', {'CLIORA_GEMM3_SHAPE': '22'}), ('shape_11', {'CLIORA_GEMM3_SHAPE': '11'}))


def _probe(tmp_path, tag, env, D, B, L, share):
    out = str(tmp_path / ('lstm_%s.npz' % tag))
    e = {k: v for k, v in os.environ.items() if k not in ('CLIORA_LSTM_PROJ', 'CLIORA_GEMM3_SHAPE', 'CLIORA_MFMA')}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'lstm_probe.py'), str(D), str(B), str(L), str(int(share)), out], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize('D,B,L,share', LC.PROBE_SHAPES)
def test_process_wide_switches(tmp_path, D, B, L, share):
    """CLIORA_LSTM_PROJ and CLIORA_GEMM3_SHAPE are read once per process: tools/lstm_probe.py runs each setting as a fresh child, one at a
    time.  The projections feed the forward, so no two settings need agree to the bit; every setting's charts and gradients are held
    to the fp64 oracle (computed here), and the worst difference from the CLIORA_LSTM_PROJ=f32 run is printed."""
    ref = LC.oracle64(D, B, L, share, True)
    base, worst = None, {}
    for tag, env in SETTINGS:
        got = _probe(tmp_path, tag, env, D, B, L, share)
        what = 'D %d B %d L %d share %d %s' % (D, B, L, share, tag)
        eo, eg = _check_against_oracle(lambda k: got['out_' + k], got.get, got['x'], ref, what)
        if base is None:
            base = got
        else:
            assert set(got) == set(base)
            worst[tag] = max(LC.rel_err(got[k], base[k].astype(np.float64)) for k in base)
        print('\n%s: charts %.3e gradients %.3e of the fp64 oracle' % (what, eo, eg))
    print('worst difference from CLIORA_LSTM_PROJ=f32, of scale:', {k: '%.2e' % v for k, v in worst.items()})


def test_refusals_come_before_any_launch():
    """What the TreeLSTM module does not run it refuses, each before anything is launched, and a valid call after them still gives the
    oracle's charts."""
    from cliora_amd import _lib
    from cliora_amd.treelstm import DioraTreeLSTM
    D, B, L, share = 33, 3, 9, True
    P, x, _ = LC.case(D, B, L, share, True)
    m = _module(P, D, share).eval()
    with torch.no_grad():
        long = torch.randn(2, 65, D).cuda()
        with pytest.raises(_lib.ChartLibError, match=r'64.*TreeLSTM plans'):
            m(long, long)
        assert m.chart is None
        obj = torch.randn(B, 4, D).cuda()
        with pytest.raises(NotImplementedError, match='text-only'):
            m(x.cuda(), x.cuda(), obj, obj)
        assert m.chart is None
        m.__dict__['_ragged'] = (torch.full((B,), L, dtype=torch.int32).cuda(), 1 << (L - 1))
        try:
            with pytest.raises(NotImplementedError, match='mixed lengths'):
                m(x.cuda(), x.cuda())
        finally:
            m.__dict__['_ragged'] = None
        assert m.chart is None
    with pytest.raises(NotImplementedError, match='compress'):
        DioraTreeLSTM(D, compress=True)
    with pytest.raises(_lib.ChartLibError, match='text-only'):
        _lib.Plan(2, 5, 16, R=4, arch=1)
    with torch.no_grad():
        m(x.cuda(), x.cuda())
    ref = LC.oracle64(D, B, L, share, True)
    for k in KEYS:
        assert LC.rel_err(getattr(m, k), ref['out'][k]) <= LC.OUT_TOL, k
