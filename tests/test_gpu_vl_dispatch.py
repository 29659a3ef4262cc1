"""Every attention, region-gradient, scorer, region-max and contrastive kernel instance of tests/vl_cases.py, run on the shape that takes
it, with the launch record on, against fp64 -- both arithmetic modes.  The vision-language counterpart of test_gpu_dispatch.py.

The scorer, region-max and contrastive entries are called directly (VLScoreFunction, VLMaxFunction, FusedContrastive on a
_lib.Plan(B, L, D, R=R)) on drawn tensors, the backward once per gradient, so that a call's record names the instance of that one
GEMM; the attention kernels run in a chart step (L <= 4 but for one case) with a fixed dropout mask replayed into the oracle.
Per call the case's expected entries must be in the record, and the record's GEMM entries must be exactly the expected ones.  Then
the project's rules (no new constant):
  chart outputs       within 1e-4 of the tensor's scale of oracle.diora_ref.diora_forward run in fp64;
  gradients, and the outputs of the directly called entries
                      f32 mode: error quantiles q50 / q99 / max relative to max |fp64| within 3x the fp32 oracle's on the same case
                      plus the floors 2e-7 / 2e-6 / 2e-5 (the fp32 oracle is computed here, on vl_cases.ORACLE_THREADS threads);
                      split-bf16 mode: conftest.grad_check(full_size=False) against fp64.
                      The contrastive kernels do the same fp32 arithmetic in both modes and are held to the first rule in both;
                      the loss VALUE, one number, to test_gpu_harness's 1e-5 of max(1, |loss|).
  arg-max indices     equal to fp64's wherever the fp64 gap between the two best regions exceeds the clearance (vl_cases.max_oracle;
                      split-bf16 mode: vl_cases.split_bf16_clearance).
The measured errors of every case go to vl_accuracy_<mode>.json in the directory CLIORA_ACCURACY_DIR names, by default accuracy_out/
in the repository (ignored by git), beside dispatch_accuracy_<mode>.json.  A run starts the files afresh.
"""
import json
import os

import pytest
import torch

import vl_cases as V
from conftest import ROOT, grad_check

pytestmark = pytest.mark.gpu

OUT_TOL = 1e-4
VALUE_TOL = 1e-5            # test_gpu_harness.test_fused_contrastive_loss_matches_the_torch_formula's bound on the loss value
KINDS = {k: sorted(n for n, c in V.CASES.items() if c['kind'] == k) for k in ('score', 'max', 'contrastive', 'chart')}
_REPORT = {}
_STARTED = set()


def _write_report(mode):
    out_dir = os.environ.get('CLIORA_ACCURACY_DIR') or os.path.join(ROOT, 'accuracy_out')
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'vl_accuracy_%s.json' % mode)
    if mode not in _STARTED and os.path.exists(path):
        os.remove(path)                 # a fresh file per run: nothing of an earlier run or another checkout stays in it
    _STARTED.add(mode)
    old = {}
    if os.path.exists(path):            # this run's earlier cases
        try:
            old = json.load(open(path)).get('cases', {})
        except ValueError:
            old = {}
    old.update(_REPORT.get(mode, {}))
    with open(path, 'w') as f:
        json.dump(dict(mode=mode, unit='error / max|fp64 value| of the tensor', cases=old), f, indent=1, sort_keys=True)


class _Judge:
    """Collects a case's measurements, writes them to the report, and only then asserts them (a miss leaves its figures behind)."""

    def __init__(self, name, mode, c):
        self.name, self.mode = name, mode
        self.report = dict(case={k: v for k, v in c.items() if k != 'what'}, what=c['what'], record={}, tensors={})
        self.checks = []

    def record(self, call, rec, expected, exact_gemms=True):
        self.report['record'][call] = sorted(rec)
        print('%s %s %s record: %s' % (self.name, self.mode, call, sorted(rec)))
        missing = [e for e in expected if not V.covers(e, rec)]
        assert not missing, (call, missing, sorted(rec))
        if exact_gemms:         # one gradient per call: the GEMMs of the record are that gradient's and no other
            gemm = lambda s: {e for e in s if 'gemm' in e}
            assert gemm(rec) == gemm(expected), (call, sorted(gemm(rec)), sorted(gemm(expected)))

    def quantiles(self, key, got, ref64, o32, rule=None):
        """the rule for gradients and directly computed outputs (module docstring); rule: 'f32' to hold a mode-independent kernel to the
        exact mode's rule in both modes"""
        rule = rule or self.mode
        assert got is not None, key
        got = got.detach().cpu()
        assert tuple(got.shape) == tuple(ref64.shape) and bool(torch.isfinite(got).all()), key
        hip = V.dist(got, ref64)
        self.report['tensors'][key] = dict(hip=hip, fp32_oracle=o32, over_bound=V.over_bound(hip, o32, ref64, rule))

        def check():
            if rule == 'f32':
                for q, floor in V.F32_FLOORS:
                    assert hip[q] <= 3.0 * o32[q] + floor, (key, q, hip[q], o32[q])
            else:
                grad_check(got, ref64, rule, 2e-4, key, full_size=False)
        self.checks.append(check)

    def within(self, key, got, ref64, tol):
        """every element within tol of max(1, scale): the rule for chart outputs"""
        got = got.detach().cpu().double().reshape(ref64.shape)
        err, scale = float((got - ref64).abs().max()), max(1.0, float(ref64.abs().max()))
        self.report['tensors'][key] = dict(err=err / scale, over_bound=err / (tol * scale))

        def check():
            assert err <= tol * scale, (key, err, scale)
        self.checks.append(check)

    def note(self, key, value):
        self.report[key] = value

    def finish(self):
        t = self.report['tensors']
        worst = max((v['over_bound'], k) for k, v in t.items())
        self.report['largest_over_bound'] = worst[0]
        _REPORT.setdefault(self.mode, {})[self.name] = self.report
        _write_report(self.mode)
        print('%s %s largest error / bound: %.3f (%s)' % (self.name, self.mode, worst[0], worst[1]))
        for k, v in sorted(t.items()):
            print('   %-28s %s' % (k, {a: ('%.3g' % b if isinstance(b, float) else {q: '%.3g' % x for q, x in b.items()}) for a, b in v.items()}))
        for check in self.checks:
            check()


def _plan(c):
    from cliora_amd import _lib
    return _lib.Plan(c['B'], c['L'], c['D'], R=c['R'])


@pytest.mark.parametrize('training', (True, False), ids=('train', 'eval'))
@pytest.mark.parametrize('name', KINDS['score'])
def test_dense_scorers_against_fp64(name, training, mfma_mode):
    """cliora_vl_scores_forward / _backward on drawn tensors: both score tensors, then each of the four gradients in a call of its own
    under a dense cotangent on all_atten_score AND vg_atten_score (eval mode: both reach the chart rows and obj_span, the words go
    through unit(x_word))."""
    from cliora_amd import _lib
    from cliora_amd.cliora import VLScoreFunction
    c = V.CASES[name]
    exp = V.expect(name, mfma_mode)
    t = {k: v.cuda() for k, v in V.score_inputs(c).items()}
    ref = V.score_oracle(name, training)
    plan = _plan(c)
    j = _Judge('%s[%s]' % (name, 'train' if training else 'eval'), mfma_mode, c)
    order = ('inside_h', 'outside_h', 'obj_span', 'x_word', 'obj_word')

    def forward(leaf=None):
        a = {k: t[k].clone() for k in order}
        if leaf:
            a[leaf].requires_grad_(True)
        out = VLScoreFunction.apply(plan, training, *[a[k] for k in order], True)
        torch.cuda.synchronize()
        return a, out
    with _lib.launch_record() as rec:
        _, (all_att, vg) = forward()
    j.record('forward', rec, exp['forward'])
    j.quantiles('all_atten_score', all_att, ref['ref64']['all_atten_score'], ref['fp32_dist']['all_atten_score'])
    j.quantiles('vg_atten_score', vg, ref['ref64']['vg_atten_score'], ref['fp32_dist']['vg_atten_score'])
    for want in V.SCORE_GRADS:
        leaf = 'inside_h' if want == 'sum_h' else want
        a, out = forward(leaf)
        with _lib.launch_record() as rec:
            torch.autograd.backward(list(out), [t['cot_all'], t['cot_vg']])
            torch.cuda.synchronize()
        j.record(want, rec, exp[want])
        j.quantiles('grad.' + want, a[leaf].grad, ref['ref64'][want], ref['fp32_dist'][want])
    j.finish()


@pytest.mark.parametrize('name', KINDS['max'])
def test_region_max_against_fp64(name, mfma_mode):
    """cliora_vl_scores_max_forward / _backward: the values against the fp64 maximum, the regions equal to fp64's outside the clearance,
    and the two gradients, each in a call of its own, against the fp64 sums over the arg max."""
    from cliora_amd import _lib
    from cliora_amd.cliora import VLMaxFunction
    c = V.CASES[name]
    exp = V.expect(name, mfma_mode)
    t = {k: v.cuda() for k, v in V.max_inputs(c).items()}
    o = V.max_oracle(name)
    plan = _plan(c)
    j = _Judge(name, mfma_mode, c)
    order = ('inside_h', 'outside_h', 'obj_span')

    def forward(leaf=None):
        a = {k: t[k].clone() for k in order}
        if leaf:
            a[leaf].requires_grad_(True)
        out = VLMaxFunction.apply(plan, *[a[k] for k in order])
        torch.cuda.synchronize()
        return a, out
    with _lib.launch_record() as rec:
        _, (vmax, arg) = forward()
    j.record('forward', rec, exp['forward'])
    arg = arg.cpu()
    assert arg.dtype == torch.int32 and int(arg.min()) >= 0 and int(arg.max()) < c['R']
    j.quantiles('values', vmax, o['val64'], o['fp32_dist'])
    clearance = o['clearance'] if mfma_mode == 'f32' else V.split_bf16_clearance(o)
    clear = o['gap'] > clearance
    differ = arg.long() != o['arg64']
    j.note('indices', dict(clearance=clearance, left_out=float((~clear).double().mean()), differ_inside=int((differ & ~clear).sum()),
                           differ_outside=int((differ & clear).sum()), differ_outside_exact_clearance=int((differ & o['clear']).sum())))
    print('%s %s indices: %s' % (name, mfma_mode, j.report['indices']))
    g64, g32 = V.max_backward_ref(name, arg)
    for want in ('sum_h', 'obj_span'):
        leaf = 'inside_h' if want == 'sum_h' else want
        a, (v2, _) = forward(leaf)
        with _lib.launch_record() as rec:
            v2.backward(t['cot'])
            torch.cuda.synchronize()
        j.record(want, rec, exp[want])
        j.quantiles('grad.' + want, a[leaf].grad, g64[want], g32[want])

    def same_regions():
        assert not bool((differ & clear).any()), j.report['indices']
    j.checks.append(same_regions)
    j.finish()


@pytest.mark.parametrize('name', KINDS['contrastive'])
def test_contrastive_loss_against_fp64(name, mfma_mode):
    """cliora_contrastive_loss / _ragged: the loss and the gradient of every input under a non-unit upstream cotangent."""
    from cliora_amd import harness as H
    c = V.CASES[name]
    o = V.contrastive_oracle(name)
    t = {k: v.clone().cuda().requires_grad_(True) for k, v in V.contrastive_inputs(c).items()}
    j = _Judge(name, mfma_mode, c)
    extra, status = (), [None]
    if c['lengths'] is not None:
        extra = (torch.tensor(c['lengths'], dtype=torch.int32, device='cuda'), status)
    loss = H.FusedContrastive.apply(t['smax'], t['inside_s'], t['outside_s'], c['margin'], c['alpha'], *extra)
    (loss * V.CONTRASTIVE_COT).backward()
    torch.cuda.synchronize()
    if c['lengths'] is not None:
        assert int(status[0].item()) == 0
    j.within('loss', loss, o['ref64']['loss'], VALUE_TOL)
    for k in ('smax', 'inside_s', 'outside_s'):
        j.quantiles('grad.' + k, t[k].grad, o['ref64'][k], o['fp32_dist'][k], rule='f32')
    j.finish()


@pytest.mark.parametrize('name', KINDS['chart'])
def test_attention_chart_against_fp64(name, mfma_mode):
    """cell_attend_fwd / cell_attend_bwd / obj_grad_reduce in a chart step: forward and backward under the cotangents of
    vl_cases.chart_inputs with the case's dropout mask, against oracle.diora_ref.diora_forward in fp64 with the mask replayed."""
    from cliora_amd import _lib
    from cliora_amd.cliora import DioraMLP
    c = V.CASES[name]
    P, t, mask, cot = V.chart_inputs(c)
    m = DioraMLP(c['D'], share=c['share'])
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    m = m.cuda().train(c['training'])
    m.lazy_region_scores = False          # the dense all_atten_score takes a cotangent
    if c['training']:
        m.dropout_mask = mask.cuda()
    tg = {k: v.clone().cuda().requires_grad_(True) for k, v in t.items()}
    j = _Judge(name, mfma_mode, c)
    with _lib.launch_record() as rec:
        m(tg['x_span'], tg['x_word'], tg['obj_span'], tg['obj_word'])
        torch.autograd.backward([getattr(m, k) for k in V.CHART_COTS], [cot[k].cuda() for k in V.CHART_COTS])
        torch.cuda.synchronize()
    j.record('step', rec, V.expect(name, mfma_mode)['step'], exact_gemms=False)
    other = {'%s<%d>' % (k, 25 - V.nrw(c['R'])) for k in ('cell_attend_fwd', 'cell_attend_bwd', 'obj_grad_reduce')}
    assert not other & rec, sorted(other & rec)
    ref = V.chart_oracle(name)
    for k in V.CHART_OUTS:
        j.within('out.' + k, getattr(m, k), ref['ref64']['out.' + k], OUT_TOL)
    named = dict(m.named_parameters())
    for k, g64 in ref['ref64'].items():
        if k.startswith('out.'):
            continue
        j.quantiles(k, tg[k].grad if k in tg else named[k].grad, g64, ref['fp32_dist'][k])
    j.finish()
