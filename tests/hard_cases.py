"""The cases of the hard-chart tests (tests/test_hard_cpu.py, tests/test_gpu_hard.py): shapes, inputs and the fp64 yardstick.

Each shape is the smallest at which a part of cliora_chart_forward_hard can go wrong.  Inputs are
oracle.synth.diora_case(D, B, L, seed): N(0, 1) parameters and words, random cotangents on the four charts.

clear: every cell of both passes keeps its best split MARGIN_REL * max|inside_s| ahead of the second best in the fp64 restatement
(cliora_amd.hard.hard_forward_torch), so the device has to select the very same splits; test_hard_cpu.py asserts the margin.  The other
cases are compared teacher-forced only (the restatement run under the device's own selection): wide or long charts come within 5e-6 of
a tie somewhere, `normalize='none'` within 1e-9 of scale, and with a zero score matrix every split of a cell ties exactly.
"""
import torch

MARGIN_REL = 1e-4          # the project's output tolerance (OUT_TOL of tests/test_gpu_dispatch.py): a clear cell's margin, of max |inside_s|
RELU_MARGIN = 5e-7         # tests/dispatch_cases.py: RELU_MARGIN
# The one case whose clearance is taken over the pairs the hard chart composes, not over every pair: B 1 / L 128 / D 16 has 44 M ReLU
# pre-activations over all pairs of both passes, whose smallest |z| / std is 2e-8 .. 2e-7 at every seed tried (11 .. 18: the expected
# minimum of that many is 3e-8), so no seed reaches 5e-7.  The case is an eval forward (no gradient is taken), the pairs a hard cell does
# not select are multiplied by 0, and the selected pairs' clearance at seed 11 is 5.6e-7.  (L 65 is seeded for every pair: seed 17.)
SELECTED_PAIRS_ONLY = ('l128',)

CHARTS = ('inside_h', 'inside_s', 'outside_h', 'outside_s')


def _c(D, B, L, seed, share=True, outside=True, normalize='unit', clear=False, train=True, ties=False, what=''):
    return dict(D=D, B=B, L=L, seed=seed, share=share, outside=outside, normalize=normalize, clear=clear, train=train, ties=ties, what=what)


CASES = {
    'l1': _c(16, 2, 1, 11, what='no level'),
    'l2': _c(16, 3, 2, 11, what='N = 1 everywhere'),
    'l3': _c(16, 3, 3, 11, clear=True, what='the first real choice'),
    'b3l5': _c(16, 3, 5, 11, what='row tiles with a tail, one column block; a plan the resident kernels would take'),
    'd24': _c(24, 3, 4, 11, what='padded charts (Dp 32)'),
    'd100': _c(100, 17, 6, 11, clear=True, what='Dp 112'),
    'b17l10': _c(48, 17, 10, 11, what='more than 8 row tiles at level 1'),
    'd400': _c(400, 4, 8, 11, clear=True, what='five column blocks, the 133 KB image'),
    'd48': _c(48, 4, 8, 11, clear=True, what='three column tiles in one block'),
    'unshared': _c(48, 5, 5, 11, share=False, clear=True, what='outside-side weights'),
    'inside_only': _c(16, 3, 5, 11, outside=False, what='inside pass only'),
    'none': _c(16, 3, 4, 11, normalize='none', what="normalize='none': teacher-forced only"),
    'l64': _c(16, 2, 64, 11, what='lane 63 of the tail, training'),
    'l65': _c(16, 1, 65, 17, train=False, what='the LONG tail, N crossing 64'),
    'l128': _c(16, 1, 128, 11, train=False, what='the LONG tail, 127 splits'),
    'ties': _c(16, 3, 5, 11, ties=True, what='inside_score_func.mat = 0: every split of a cell scores the same'),
}
CLEAR = tuple(sorted(n for n, c in CASES.items() if c['clear']))


def case_inputs(c):
    """-> (params by state_dict name, x_span, cotangents): oracle.synth.diora_case, with the score matrix zeroed for the ties case."""
    from oracle import synth
    P, x, cot = synth.diora_case(c['D'], c['B'], c['L'], c['seed'], share=c['share'])
    if c['ties']:
        P = dict(P)
        P['inside_score_func.mat'] = torch.zeros_like(P['inside_score_func.mat'])
    return P, x, cot


_REF = {}


def reference(name):
    """The fp64 restatement of the case under its OWN selection (first argmax), computed once per process and left unchanged."""
    if name not in _REF:
        from cliora_amd.hard import hard_forward_torch
        c = CASES[name]
        P, x, _ = case_inputs(c)
        with torch.no_grad():
            _REF[name] = hard_forward_torch(P, x, c['share'], c['normalize'], outside=c['outside'])
    return _REF[name]


def min_margin_rel(r):
    """Smallest best-minus-second-best margin over the cells of both passes, relative to max |inside_s|."""
    scale = max(1e-30, float(r['inside_s'].abs().max()))
    return min(float(r['margin_in'].min()), float(r['margin_out'].min())) / scale


def teacher_forced(c, selection, dtype, with_grads):
    """The restatement under the given (device) selection in `dtype` -> (charts, gradients by parameter name + 'x_span' or None)."""
    from cliora_amd.hard import hard_forward_torch
    P, x, cot = case_inputs(c)
    Pd = {k: v.detach().to(dtype).requires_grad_(with_grads) for k, v in P.items()}
    xd = x.detach().to(dtype).requires_grad_(with_grads)
    with torch.set_grad_enabled(with_grads):
        o = hard_forward_torch(Pd, xd, c['share'], c['normalize'], outside=c['outside'], selection=selection, dtype=dtype)
    charts = {k: (o[k].detach().unsqueeze(-1) if o[k].dim() == 2 else o[k].detach()) for k in CHARTS}
    if not with_grads:
        return charts, None
    sum((o[k] * (cot[k].to(dtype).squeeze(-1) if o[k].dim() == 2 else cot[k].to(dtype))).sum() for k in CHARTS).backward()
    g = {k: v.grad.detach() for k, v in Pd.items() if v.grad is not None}
    g['x_span'] = xd.grad.detach()
    return charts, g
