"""Every chart GEMM and compose kernel instance of tests/dispatch_cases.py, run on the shape that takes it, with the launch record on,
against the fp64 oracle -- both arithmetic modes.

Per case: forward and backward under _lib.launch_record() with the cotangents of oracle.synth.diora_case; the case's expected entries
must be in the record; then the project's rules (no new constant):
  charts      within 1e-4 of the tensor's scale of oracle.diora_ref.diora_forward run in fp64;
  gradients   f32 mode: error quantiles q50 / q99 / max relative to max |fp64| within 3x the fp32 oracle's on the same case plus the
              floors 2e-7 / 2e-6 / 2e-5 (test_c2_full_size_gradients_vs_fp64's rule; the fp32 oracle is computed here);
              split-bf16 mode: conftest.grad_check(full_size=False) against the fp64 gradients.
The measured errors of every case go to dispatch_accuracy_<mode>.json in the directory CLIORA_ACCURACY_DIR names, by default
accuracy_out/ in the repository (ignored by git).  A run starts the files afresh; only the placement children, processes of their own,
add their cases to what the parent run wrote.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import dispatch_cases as DC
from conftest import ROOT, grad_check

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-4
_REPORT = {}


def _module(P, D, share):
    from cliora_amd.diora import DioraMLP
    m = DioraMLP(D, share=share)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    return m.cuda()


_CHILD = 'CLIORA_DISPATCH_PLACEMENT_CHILD'      # set for the placement children: they append to the parent run's report
_STARTED = set()


def _write_report(mode):
    out_dir = os.environ.get('CLIORA_ACCURACY_DIR') or os.path.join(ROOT, 'accuracy_out')
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'dispatch_accuracy_%s.json' % mode)
    if mode not in _STARTED and not os.environ.get(_CHILD) and os.path.exists(path):
        os.remove(path)                 # a fresh file per run: nothing of an earlier run or another checkout stays in it
    _STARTED.add(mode)
    old = {}
    if os.path.exists(path):            # this run's earlier cases, and in a placement child the parent run's
        try:
            old = json.load(open(path)).get('cases', {})
        except ValueError:
            old = {}
    old.update(_REPORT.get(mode, {}))
    with open(path, 'w') as f:
        json.dump(dict(mode=mode, unit='error / max|fp64 value| of the tensor', cases=old), f, indent=1, sort_keys=True)


def _check_record(c, mode, rec):
    missing = [e for e in c['expect'][mode] if not DC.covers(e, rec)]
    assert not missing, (missing, sorted(rec))
    sets = c['dma3x'].get(mode)
    if sets is not None:
        early, tail = sets
        got = {e for e in rec if e.startswith('tn_gemm_dma3x')}
        # forced placements (tests/test_gpu_wgrad_placement.py's switches, read once per process) name the one admissible set
        step = os.environ.get('CLIORA_WGRAD_EARLY_STEP')
        admissible = [early, tail] if step is None else [tail] if int(step) < 0 else [early]
        assert got in admissible, (sorted(got), [sorted(s) for s in admissible])


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_dispatch_case_against_fp64(name, mfma_mode):
    from cliora_amd import _lib
    c = DC.CASES[name]
    P, x, cot = DC.case_inputs(c)
    m = _module(P, c['D'], c['share']).train()
    prev = _lib.set_wavefront(c['wavefront'])
    try:
        with _lib.launch_record() as rec:
            xg = x.clone().cuda().requires_grad_(True)
            m(xg, xg)
            torch.autograd.backward([getattr(m, k) for k in DC.CHARTS], [cot[k].cuda() for k in DC.CHARTS])
            torch.cuda.synchronize()
    finally:
        _lib.set_wavefront(prev)
    print('%s %s record: %s' % (name, mfma_mode, sorted(rec)))
    _check_record(c, mfma_mode, rec)

    ref = DC.oracle(name)
    named = dict(m.named_parameters())
    report = dict(shape=[c['D'], c['B'], c['L'], c['share']], seed=c['seed'], record=sorted(rec), tensors={})
    worst = 0.0
    for k in DC.CHARTS:
        o64 = ref['out64'][k]
        err = float((getattr(m, k).detach().cpu().double() - o64).abs().max())
        scale = max(1.0, float(o64.abs().max()))
        report['tensors']['out.' + k] = dict(err=err / scale, over_bound=err / (OUT_TOL * scale))
    grads = {k: (xg.grad if k == 'x_span' else named[k].grad) for k in ref['grad64']}
    for k, g64 in ref['grad64'].items():
        hip, o32 = DC.dist(grads[k], g64), ref['fp32_dist'][k]
        r = dict(hip=hip, fp32_oracle=o32)
        if mfma_mode == 'f32':
            r['over_bound'] = max(hip[q] / (3.0 * o32[q] + fl) for q, fl in (('q50', 2e-7), ('q99', 2e-6), ('max', 2e-5)))
        else:       # grad_check(full_size=False): median 5e-4, q99 1e-2 (from 1000 elements), max 5e-2 of max(1, scale)
            sc = max(1e-30, float(g64.abs().max()))
            rel = sc / max(1.0, sc)
            r['over_bound'] = max(hip['q50'] * rel / 5e-4, hip['q99'] * rel / 1e-2 if g64.numel() >= 1000 else 0.0, hip['max'] * rel / 5e-2)
        report['tensors'][k] = r
    worst = max(t['over_bound'] for t in report['tensors'].values())
    report['largest_over_bound'] = worst
    _REPORT.setdefault(mfma_mode, {})[name + ''.join('+%s=%s' % (v, os.environ[v]) for v in sorted(DC.PLACEMENTS[0]) if v in os.environ)] = report
    _write_report(mfma_mode)
    print('%s %s largest error / bound: %.3f' % (name, mfma_mode, worst))
    for k, t in sorted(report['tensors'].items()):
        print('   %-28s %s' % (k, {a: ('%.3g' % b if isinstance(b, float) else {q: '%.3g' % v for q, v in b.items()}) for a, b in t.items()}))

    for k in DC.CHARTS:
        o64 = ref['out64'][k]
        err = float((getattr(m, k).detach().cpu().double() - o64).abs().max())
        assert err <= OUT_TOL * max(1.0, float(o64.abs().max())), (k, err)
    for k, g64 in ref['grad64'].items():
        if mfma_mode == 'f32':
            hip, o32 = report['tensors'][k]['hip'], ref['fp32_dist'][k]
            for q, floor in (('q50', 2e-7), ('q99', 2e-6), ('max', 2e-5)):
                assert hip[q] <= 3.0 * o32[q] + floor, (k, q, hip[q], o32[q])
        else:
            grad_check(grads[k], g64, mfma_mode, 2e-4, k, full_size=False)


_FWD = {}


@pytest.mark.parametrize('wavefront', DC.FORWARD_CASE['wavefront'])
def test_wide_level_project_forward(wavefront, mfma_mode):
    """level_project<5,..>: 3 248 cells at level 1 of both passes (D 400, B 232, L 15), forward only.  The charts of eight sentences --
    the first, the last, six whose level-1 cells straddle a 16-row group -- against the fp64 oracle run on those sentences alone; every
    chart finite; and the two schedules bitwise equal (all schedules are).  NOT asserted: bitwise equality with
    the same eight sentences run as a batch of eight.  The code does not claim it -- DESIGN.md section 13 ("Not bitwise"): the level
    kernels choose tile shapes and the parts of a cell's aggregate by a level's row count, so the sums run in another order."""
    from cliora_amd import _lib
    from oracle import diora_ref as R
    c = DC.FORWARD_CASE
    P, x, _ = DC.case_inputs(c)
    m = _module(P, c['D'], c['share']).eval()
    prev = _lib.set_wavefront(wavefront)
    try:
        with _lib.launch_record() as rec, torch.no_grad():
            xg = x.cuda()
            m(xg, xg)
            torch.cuda.synchronize()
    finally:
        _lib.set_wavefront(prev)
    print('forward %s %s record: %s' % (wavefront, mfma_mode, sorted(rec)))
    missing = [e for e in c['expect'][mfma_mode] if not DC.covers(e, rec)]
    assert not missing, (missing, sorted(rec))
    got = {k: getattr(m, k).detach().cpu() for k in DC.CHARTS}
    for k in DC.CHARTS:
        assert bool(torch.isfinite(got[k]).all()), k
    pick = DC.forward_sentences(c['B'], c['L'])
    if 'ref' not in _FWD:
        with torch.no_grad():
            P64 = {k: v.double() for k, v in P.items()}
            x64 = x[pick].double()
            _FWD['ref'] = {k: v.detach() for k, v in R.diora_forward(P64, x64, x64).items() if k in DC.CHARTS}
    for k in DC.CHARTS:
        o64 = _FWD['ref'][k]
        err = float((got[k][pick].double() - o64).abs().max())
        print('forward %s %s %s: %.3g of scale' % (wavefront, mfma_mode, k, err / max(1.0, float(o64.abs().max()))))
        assert err <= OUT_TOL * max(1.0, float(o64.abs().max())), (k, err)
    other = _FWD.setdefault(('charts', mfma_mode), (wavefront, got))
    if other[0] != wavefront:
        for k in DC.CHARTS:
            assert torch.equal(other[1][k], got[k]), (k, other[0], wavefront)


@pytest.mark.parametrize('placement', range(len(DC.PLACEMENTS)))
def test_strided_range_cases_under_both_placements(placement):
    """The three cases around the strided range (widths 336, 416, 432) once more in a fresh process under each forced placement of the
    weight-gradient pieces (tests/test_gpu_wgrad_placement.py): early part + two-range tail, and everything in the tail, whatever this
    device's queue count lets the automatic choice be.  The record check in the child names the one admissible set."""
    env = dict(os.environ, **DC.PLACEMENTS[placement])
    env[_CHILD] = '1'
    sel = ['tests/test_gpu_dispatch.py::test_dispatch_case_against_fp64[%s-%s]' % (mode, n) for n in DC.PLACEMENT_CASES for mode in DC.MODES]
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-s', '-p', 'no:cacheprovider', '-m', 'gpu'] + sel,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
