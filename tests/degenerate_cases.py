"""Seeded degenerate inputs shared by test_degenerate_cpu.py and test_gpu_degenerate.py (not a test module): rows whose norm is zero or
below the unit-norm clamp (utils.py:10-14, eps = 1e-8), exact ties in CKY and in the region max, ReLU pre-activations of exactly +0, and
the zero-initialised image encoder (utils.py:45-50) a CLIORA run starts from.

The cases (D, B, L[, R] in CASES_*):
  a  text DioraMLP, zero biases.  Sentence 0: word 1 = 0, word 4 scaled to a sub-eps norm; sentence 1: all zero; sentence 2: words 0 and
     1 = 0 (cell (0, 2) composes [0; 0]: pre-activation exactly +0); sentence 3 untouched.
  b  every composed cell sub-eps: h_fcs.2.weight x 1e-11, h_fcs.2.bias x 0, root_vector_out_h x 1e-10 (both modules when unshared).
  c  TreeLSTM, B x 0.  Sentence 0: word 1 = 0; sentence 1: word 2 sub-eps; sentence 2: words 0 and 1 = 0.
  d  EXCLUDED: an all-zero TreeLSTM sentence.  Every cell of it is a clamp row whose backward multiplies by 1 / eps, and tanh'(0) = 1
     passes that factor on unreduced from level to level (in DioraMLP the ReLU at +0 stops it): the gradient grows by 1e8 per level
     and the fp32 oracle itself overflows at L 5 (measured: non-finite x.grad).  There is nothing finite to compare with.
  e  CLIORA DioraMLP with obj_span = obj_word = 0 (what the zero image encoder produces), train mode with a recorded dropout mask;
     `edits`: case a's leaf edits (and zero biases) on top.
  f  CLIORA with duplicated region rows: exact ties in the region max.
  g  harness.build_net as built (zero img_encoder), all three losses -- built in the tests themselves.

The sub-eps scale.  The plain construction scales a word by 1e-10.  The leaf is tanh(W x) with W, x ~ N(0, 1): its norm is about D times the scale,
4.8e-9 at D 48 but 4e-8 -- above eps -- at D 400.  So the scale is 1e-10 * 48 / max(D, 48): 1e-10 up to D 48, and a pre-norm of about
eps / 2 at every width (what the CPU test pins through the class counts).

How to compare (compare_rows / measure_rows).  A clamp row's gradient is 1 / eps times an ordinary one (1 / eps^2 at the twice-normalised
CLIORA leaf), so a whole-tensor scale would hide every ordinary row: chart outputs and x gradients are split by the fp64 oracle's class
of the row (norm 0, (0, 0.5], 1), each group is checked against its own max(1, largest |reference|), and a group whose rows span more
than a factor of 100 in magnitude is checked row by row.  Parameter gradients keep the whole-tensor scale.

The device tests `norm > eps` where torch's clamp passes the gradient at `norm >= eps`: they differ only AT eps, so no row of a case
may sit near it -- classify() refuses a norm in (0.5, 1 - 1e-6).
"""
import functools

import numpy as np
import torch

from oracle import chart_layout as CL
from oracle import diora_ref as R

OUT_TOL = 1e-4         # outputs, the project's forward bound
GRAD_TOL = 2e-4        # gradients, conftest.grad_check(t, ref, mode, GRAD_TOL)
CHARTS = ('inside_h', 'inside_s', 'outside_h', 'outside_s')
CHARTS6 = ('inside_h', 'inside_c', 'inside_s', 'outside_h', 'outside_c', 'outside_s')
ROW_CHARTS = ('inside_h', 'inside_c', 'outside_h', 'outside_c')      # the unit-normalised charts: rows with a class
VL_OUTS = CHARTS + ('inside_c', 'all_atten_score', 'vg_atten_score', 'atten_score')

CASES_A = [(48, 4, 6, True), (48, 4, 6, False), (33, 4, 6, True), (400, 4, 5, True)]
CASES_B = [(48, 3, 6, True), (48, 3, 6, False), (400, 2, 5, True)]
CASES_C = [(32, 3, 5), (400, 2, 5)]
CASES_E = [(48, 3, 6, 5, False), (64, 2, 5, 36, False), (400, 2, 5, 36, False), (48, 3, 6, 5, True), (64, 2, 5, 36, True)]      # ..., edits
CASES_F = [(48, 3, 6, 36), (32, 2, 5, 5)]
SEED = dict(a=7101, b=7202, c=7303, e=7404, f=7505, g=7606)
# A ReLU pre-activation within rounding of zero is a kink: the split-bf16 compose GEMMs perturb it by ~1e-5 of its scale
# (conftest.grad_check), the unit switches on or off, and in a 48-wide chart that one unit moves EVERY element of a vector such as
# root_vector_out_h.grad (case a, D 48, shared, seed 7101: 1.57e-5 at a scale of 30 in sentence 2's outside pass moved the median of
# that gradient to 1.7e-3 of scale on the MI355X).  The cases that run in both arithmetic modes at D <= 64 are therefore seeded so
# that no pre-activation other than an exact zero lies within KINK_MARGIN of its layer's largest (relu_margin, checked by the CPU
# test); seed_search() found these, the first of SEED[name], SEED[name] + 1, ... that keeps the margin.  At D 400 a kink moves 1 / 400
# of a row and stays inside the statistical bounds, as in the project's other tests.
KINK_MARGIN = 2e-5          # the perturbation with a margin of two
CASE_SEED = {('a', 48, 4, 6, True): 7116, ('a', 48, 4, 6, False): 7116, ('a', 33, 4, 6, True): 7102, ('b', 48, 3, 6, False): 7204,
             ('e', 48, 3, 6, 5, True): 7405, ('f', 48, 3, 6, 36): 7509}


def seed_of(name, *args):
    return CASE_SEED.get((name,) + args, SEED[name])


def sub_eps_scale(D):
    return 1e-10 * 48.0 / max(D, 48)


def zero_biases(P):
    for k in P:
        if k.endswith('.bias') or k.endswith('.B'):
            P[k] = P[k] * 0.0
    return P


def leaf_edits(x):
    """Case a's edits on a (B, L, D) batch, in place, for the sentences and words it has."""
    B, L, D = x.shape
    x[0, 1] = 0.0
    if L > 4:
        x[0, 4] *= sub_eps_scale(D)
    if B > 1:
        x[1] = 0.0
    if B > 2:
        x[2, 0] = 0.0
        x[2, 1] = 0.0
    return x


def _cot(g, B, L, D, keys):
    C = CL.n_cells(L)
    return {k: torch.randn((B, C, 1 if k.endswith('_s') else D), generator=g) for k in keys}


@functools.lru_cache(maxsize=None)
def case_a(D, B, L, share):
    seed = seed_of('a', D, B, L, share)
    P = zero_biases(R.init_params(D, share=share, seed=seed))
    g = torch.Generator().manual_seed(seed + 1)
    x = leaf_edits(torch.randn(B, L, D, generator=g))
    return dict(kind='mlp', name='a', D=D, B=B, L=L, share=share, P=P, x_span=x, cot=_cot(g, B, L, D, CHARTS))


@functools.lru_cache(maxsize=None)
def case_b(D, B, L, share):
    seed = seed_of('b', D, B, L, share)
    P = R.init_params(D, share=share, seed=seed)
    for pre in ('inside',) if share else ('inside', 'outside'):
        P[pre + '_compose_func.h_fcs.2.weight'] = P[pre + '_compose_func.h_fcs.2.weight'] * 1e-11
        P[pre + '_compose_func.h_fcs.2.bias'] = P[pre + '_compose_func.h_fcs.2.bias'] * 0.0
    P['root_vector_out_h'] = P['root_vector_out_h'] * 1e-10
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, L, D, generator=g)
    return dict(kind='mlp', name='b', D=D, B=B, L=L, share=share, P=P, x_span=x, cot=_cot(g, B, L, D, CHARTS))


@functools.lru_cache(maxsize=None)
def case_c(D, B, L):
    P = zero_biases(R.init_params_treelstm(D, seed=SEED['c']))
    g = torch.Generator().manual_seed(SEED['c'] + 1)
    x = torch.randn(B, L, D, generator=g)
    x[0, 1] = 0.0
    x[1, 2] *= sub_eps_scale(D)
    if B > 2:
        x[2, 0] = 0.0
        x[2, 1] = 0.0
    return dict(kind='lstm', name='c', D=D, B=B, L=L, share=True, P=P, x_span=x, cot=_cot(g, B, L, D, CHARTS6))


def _vl_case(name, D, B, L, Rg, P, g, obj_span, obj_word, edits):
    C = CL.n_cells(L)
    x_span, x_word = torch.randn(B, L, D, generator=g), torch.randn(B, L, D, generator=g)
    if edits:
        leaf_edits(x_span)
    mask = (torch.rand(B, C, Rg, generator=g) > 0.1).float() / 0.9          # pre-scaled keep mask of nn.Dropout(0.1), chart order
    cot = _cot(g, B, L, D, CHARTS)
    cot['all_atten_score'] = torch.randn(B, B, C, Rg, generator=g)          # used by the dense run only (lazy_region_scores False)
    cot['vg_atten_score'] = torch.randn(B, B, L, Rg, generator=g)
    return dict(kind='vl', name=name, D=D, B=B, L=L, R=Rg, share=True, P=P, x_span=x_span, x_word=x_word, obj_span=obj_span,
                obj_word=obj_word, mask=mask, cot=cot)


@functools.lru_cache(maxsize=None)
def case_e(D, B, L, Rg, edits):
    seed = seed_of('e', D, B, L, Rg, edits)
    P = R.init_params(D, share=True, seed=seed)
    if edits:
        zero_biases(P)
    g = torch.Generator().manual_seed(seed + 1)
    return _vl_case('e', D, B, L, Rg, P, g, torch.zeros(B, Rg, D), torch.zeros(B, Rg, D), edits)


def duplicate_pairs(Rg):
    """(row, its copy) of case f."""
    return [(r, r + 20) for r in range(10)] if Rg == 36 else [(0, 3)]


@functools.lru_cache(maxsize=None)
def case_f(D, B, L, Rg):
    seed = seed_of('f', D, B, L, Rg)
    P = R.init_params(D, share=True, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    obj_span, obj_word = 0.3 * torch.randn(B, Rg, D, generator=g), 0.3 * torch.randn(B, Rg, D, generator=g)
    for r, d in duplicate_pairs(Rg):
        obj_span[:, d] = obj_span[:, r]
        obj_word[:, d] = obj_word[:, r]
    return _vl_case('f', D, B, L, Rg, P, g, obj_span, obj_word, False)


# ---- the oracle on a case -----------------------------------------------------------------------------------------------------------
class _ClampFreeBackward(torch.autograd.Function):
    """The self-check's mutant of unit_norm: the forward of x / max(||x||, eps), and the backward of unit_norm WITHOUT its clamp --
    (v - n (n . v)) / ||x|| with n = x / ||x|| -- which is what a kernel that forgot the branch would compute on a sub-eps row.  An
    exactly-zero row keeps v / eps, so that the mutant is told apart by the sub-eps rows and not by a division by zero.  (The
    milder mutant (v - h (h . v)) / eps, h = x / eps, is invisible at the twice-normalised CLIORA leaf: the gradient that reaches the
    first norm has passed the second one's projection and is orthogonal to h already.)"""

    @staticmethod
    def forward(ctx, x):
        nr = x.norm(p=2, dim=-1, keepdim=True)
        ctx.save_for_backward(x, nr)
        return x / nr.clamp(min=R.EPS)

    @staticmethod
    def backward(ctx, v):
        x, nr = ctx.saved_tensors
        safe = torch.where(nr > 0, nr, torch.ones_like(nr))
        n = x / safe
        return torch.where(nr > 0, (v - n * (n * v).sum(-1, keepdim=True)) / safe, v / R.EPS)


def _einsum_by_rows(eq, q, k):
    """einsum('abx,cdx->acbd') as a product and a sum over the last axis: every score is reduced on its own, in an order that depends on
    the row's length alone, so copies of a region row score bitwise the same whatever their position.  A BLAS GEMM does not promise
    that (an edge column may be summed in another order: seen at R 5 on a 16-thread host), and a last-bit difference between two copies
    would hand the reference's tie to rounding."""
    if eq != 'abx,cdx->acbd':
        return _EINSUM(eq, q, k)
    return (q[:, None, :, None, :] * k[None, :, None, :, :]).sum(-1)


_EINSUM = torch.einsum


def _last_max(t):
    """The self-check's mutant of the region max: the LAST of equal scores takes the gradient (the values are the same)."""
    return t.flip(-1)


def vl_keys(lazy):
    return CHARTS + ('vg_atten_score',) + (() if lazy else ('all_atten_score',))


def run_oracle(case, dtype, lazy=True, mutant=None):
    """The oracle on a case at `dtype`, with the case's cotangents (and, CLIORA, the two VL losses on its own outputs) ->
    dict(out={name: tensor}, grad={name: tensor}, pair_s_in).  mutant: None, 'no_clamp_backward' or 'last_region'."""
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in case['P'].items()}
    inp = {k: case[k].detach().to(dtype).requires_grad_(True) for k in ('x_span', 'x_word', 'obj_span', 'obj_word') if k in case}
    B, L = case['B'], case['L']
    C = CL.n_cells(L)
    orig_unit, orig_drop = R.unit_norm, R.F.dropout
    if case['kind'] == 'vl':
        R.torch.einsum = _einsum_by_rows
    if mutant == 'no_clamp_backward':
        R.unit_norm = _ClampFreeBackward.apply
    try:
        if case['kind'] == 'vl':
            mask = case['mask'].to(dtype)
            off = [C - (L - lv) * (L - lv + 1) // 2 for lv in range(L)] + [C]
            calls = {'i': 0}

            def replay(x, p, training):            # one call per level, leaves first: the level's slice of the recorded mask
                i = calls['i']
                calls['i'] += 1
                return x * mask[:, off[i]:off[i + 1]]
            R.F.dropout = replay
            ref = R.diora_forward(P, inp['x_span'], inp['x_word'], inp['obj_span'], inp['obj_word'], training=True, keep_pairs=True)
            assert calls['i'] == L
        else:
            ref = R.diora_forward(P, inp['x_span'], inp['x_span'], share=case['share'], training=True, keep_pairs=True,
                                  arch='treelstm' if case['kind'] == 'lstm' else 'mlp')
    finally:
        R.unit_norm, R.F.dropout, R.torch.einsum = orig_unit, orig_drop, _EINSUM
    keys = vl_keys(lazy) if case['kind'] == 'vl' else tuple(case['cot'])
    loss = sum((ref[k] * case['cot'][k].to(dtype)).sum() for k in keys)
    losses = {}
    if case['kind'] == 'vl':
        pick = _last_max if mutant == 'last_region' else (lambda t: t)
        losses['contrastive'] = R.contrastive_loss(ref['inside_s'], ref['outside_s'], pick(ref['all_atten_score']), 0.2, 1.0)
        losses['vg'] = R.vg_loss(pick(ref['vg_atten_score']), 1.0)
        loss = loss + losses['contrastive'] + losses['vg']
    loss.backward()
    names = VL_OUTS if case['kind'] == 'vl' else CHARTS6
    grad = {k: p.grad.detach() for k, p in P.items() if p.grad is not None}
    grad.update({k: t.grad.detach() for k, t in inp.items() if t.grad is not None})
    return dict(out={k: ref[k].detach() for k in names}, grad=grad, losses={k: float(v.detach()) for k, v in losses.items()},
                pair_s_in={lv: s.detach() for lv, s in ref['pair_s_in'].items()})


@functools.lru_cache(maxsize=None)
def oracle64(builder, args, lazy=True):
    """The fp64 reference of a case, computed once and shared (never modified by a test)."""
    return run_oracle(builder(*args), torch.float64, lazy)


def relu_margin(case):
    """The smallest |pre-activation| / (largest |pre-activation| of the same layer call) over both ReLU layers of every compose call
    of the fp64 oracle on a DioraMLP / CLIORA case, exact zeros left out (they are zero in any arithmetic)."""
    worst = [float('inf')]
    orig = R.compose_mlp

    def spy(W, a, b):
        z1 = R.F.linear(torch.cat([a, b], 1), W['W1'], W['b1'])
        z2 = R.F.linear(R.F.relu(z1), W['W2'], W['b2'])
        for z in (z1.detach().abs(), z2.detach().abs()):
            nz = z[z > 0]
            if nz.numel():
                worst[0] = min(worst[0], float(nz.min()) / float(z.max()))
        return orig(W, a, b)
    R.compose_mlp = spy
    try:
        run_oracle(case, torch.float64)
    finally:
        R.compose_mlp = orig
    return worst[0]


def needs_kink_margin(cid):
    return cid[0] in 'abef' and cid[1] <= 64


def seed_search(tries=200):
    """{case id: seed} for the cases whose family seed does not keep KINK_MARGIN (what CASE_SEED holds)."""
    found = {}
    for cid, fn, args in all_cases():
        if not needs_kink_margin(cid):
            continue
        for seed in range(SEED[cid[0]], SEED[cid[0]] + tries):
            CASE_SEED[cid] = seed
            fn.cache_clear()
            if relu_margin(fn(*args)) >= KINK_MARGIN:
                break
        else:
            raise RuntimeError('no seed for %r' % (cid,))
        if seed != SEED[cid[0]]:
            found[cid] = seed
        else:
            del CASE_SEED[cid]
    return found


# ---- classes ------------------------------------------------------------------------------------------------------------------------
ZERO, SUB_EPS, UNIT = 0, 1, 2


def classify(rows):
    """(..., W) rows -> (...) int64 classes: ZERO (norm exactly 0), SUB_EPS (0 < norm <= 0.5: a pre-norm of at most eps / 2),
    UNIT (within 1e-6 of 1); -1 for anything else, which no case may contain."""
    n = rows.detach().double().cpu().norm(dim=-1)
    cls = torch.full(n.shape, -1, dtype=torch.int64)
    cls[n == 0.0] = ZERO
    cls[(n > 0.0) & (n <= 0.5)] = SUB_EPS
    cls[(n - 1.0).abs() <= 1e-6] = UNIT
    return cls


def class_counts(out, keys):
    """{chart: [rows of class ZERO, SUB_EPS, UNIT]}; a row outside the three classes raises."""
    res = {}
    for k in keys:
        cls = classify(out[k])
        assert int((cls < 0).sum()) == 0, '%s: a row norm near the clamp boundary: %r' % (k, out[k].double().norm(dim=-1)[cls < 0])
        res[k] = [int((cls == c).sum()) for c in (ZERO, SUB_EPS, UNIT)]
    return res


def leaf_class(ref, L):
    """The class of each word's leaf (B, L): the rows x_span.grad is split by.  A CLIORA leaf that is normalised twice (a sub-eps u,
    then u + 0 again below eps) is told apart from the rest by the per-row rule of row_groups."""
    return classify(ref['out']['inside_h'][:, :L])


def row_groups(ref_rows, cls):
    """Index tensors over the rows (N, W) of a reference: one group per class, a group whose rows' magnitudes span more than a factor
    of 100 one group per row."""
    mag = ref_rows.abs().amax(dim=-1)
    groups = []
    for c in torch.unique(cls).tolist():
        idx = torch.nonzero(cls == c).flatten()
        m = mag[idx]
        if idx.numel() > 1 and float(m.max()) > 100.0 * float(m.min()):
            groups += [idx[i:i + 1] for i in range(idx.numel())]
        else:
            groups.append(idx)
    return groups


def _rows(t, W):
    return t.detach().double().cpu().reshape(-1, W)


def compare_rows(t, ref, cls, check, what):
    """check(t rows, reference rows, what) on every group of row_groups (the reference's rows of width ref.shape[-1], classes cls)."""
    W = ref.shape[-1]
    a, b = _rows(t, W), _rows(ref, W)
    for gi, idx in enumerate(row_groups(b, cls.flatten())):
        check(a[idx], b[idx], '%s[group %d, %d rows, first %d]' % (what, gi, idx.numel(), int(idx[0])))


def out_check(a, b, what):
    err, sc = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
    assert err <= OUT_TOL * sc, '%s: err %.3e scale %.3e' % (what, err, sc)      # a NaN fails too


def rel_err(a, b):
    """max |a - b| / max(1, max |b|) of one group / tensor."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max())) if b.numel() else 0.0


def measure_rows(t, ref, cls):
    """The largest rel_err over the groups of compare_rows."""
    W = ref.shape[-1]
    a, b = _rows(t, W), _rows(ref, W)
    return max(rel_err(a[idx], b[idx]) for idx in row_groups(b, cls.flatten()))


def row_keyed(name):
    """Tensors compared by row groups (and the chart whose classes split them); everything else is a parameter gradient."""
    return name in ('x_span', 'x_word')


def measure(got_out, got_grad, ref, L, out_keys):
    """-> (worst output rel_err, worst gradient rel_err) of a run against a reference of run_oracle, by the rule above."""
    w_out = 0.0
    for k in out_keys:
        if k in ROW_CHARTS:
            w_out = max(w_out, measure_rows(got_out[k], ref['out'][k], classify(ref['out'][k])))
        else:
            w_out = max(w_out, rel_err(got_out[k], ref['out'][k]))
    lc = leaf_class(ref, L)
    w_grad = 0.0
    for k, g in ref['grad'].items():
        w_grad = max(w_grad, measure_rows(got_grad[k], g, lc) if row_keyed(k) else rel_err(got_grad[k], g))
    return w_out, w_grad


def all_cases():
    """(case id, builder, its arguments) of every seeded case."""
    for name, fn, rows in (('a', case_a, CASES_A), ('b', case_b, CASES_B), ('c', case_c, CASES_C), ('e', case_e, CASES_E), ('f', case_f, CASES_F)):
        for args in rows:
            yield (name,) + args, fn, args


def out_keys_of(case):
    return VL_OUTS if case['kind'] == 'vl' else (CHARTS6 if case['kind'] == 'lstm' else CHARTS)


def assert_matches(got_out, got_grad, ref, L, out_keys, mode):
    """Every output and gradient of a run against a reference of run_oracle, by the rule in this file's docstring: OUT_TOL on the
    outputs, conftest.grad_check(..., mode, GRAD_TOL) on the gradients, the rows of the charts and of the x gradients by class."""
    from conftest import grad_check

    def gcheck(a, b, what):
        assert bool(torch.isfinite(a).all()), what + ': not finite'
        grad_check(a, b, mode, GRAD_TOL, what)
    dbl = lambda t: t.detach().double().cpu()
    for k in out_keys:
        assert bool(torch.isfinite(got_out[k]).all()), k + ': not finite'
        if k in ROW_CHARTS:
            compare_rows(got_out[k], ref['out'][k], classify(ref['out'][k]), out_check, k)
        else:
            out_check(dbl(got_out[k]), dbl(ref['out'][k]), k)
    lc = leaf_class(ref, L)
    for k, g in ref['grad'].items():
        assert got_grad.get(k) is not None, k
        if row_keyed(k):
            compare_rows(got_grad[k], g, lc, gcheck, k)
        else:
            gcheck(dbl(got_grad[k]), dbl(g), k)


def cky_gaps(pair_s, b, n):
    """The gap between the best and the second-best CKY candidate of every cell with a choice of sentence b (length n), in fp64."""
    val = {(0, p): 1.0 for p in range(n)}
    gaps = []
    for level in range(1, n):
        s = pair_s[level][b, :, :, 0].detach().double().numpy()
        for pos in range(n - level):
            rel = s[pos, :level] - s[pos, :level].max()
            cand = np.array([val[(k, pos)] + val[(level - k - 1, pos + k + 1)] + rel[k] for k in range(level)])
            top = np.sort(cand)[::-1]
            val[(level, pos)] = top[0]
            if level > 1:
                gaps.append(float(top[0] - top[1]))
    return gaps


# ---- constants pinned by test_degenerate_cpu.py --------------------------------------------------------------------------------------
# {case id: {chart: [ZERO, SUB_EPS, UNIT rows]}} of the fp64 oracle (the fp32 oracle gives the same): a later edit that stops reaching
# the clamp branch changes them.
CLASS_COUNTS = {
    ('a', 48, 4, 6, True): {'inside_h': [25, 1, 58], 'inside_c': [84, 0, 0], 'outside_h': [0, 0, 84], 'outside_c': [84, 0, 0]},
    ('a', 48, 4, 6, False): {'inside_h': [25, 1, 58], 'inside_c': [84, 0, 0], 'outside_h': [0, 0, 84], 'outside_c': [84, 0, 0]},
    ('a', 33, 4, 6, True): {'inside_h': [25, 1, 58], 'inside_c': [84, 0, 0], 'outside_h': [0, 0, 84], 'outside_c': [84, 0, 0]},
    ('a', 400, 4, 5, True): {'inside_h': [19, 1, 40], 'inside_c': [60, 0, 0], 'outside_h': [0, 0, 60], 'outside_c': [60, 0, 0]},
    ('b', 48, 3, 6, True): {'inside_h': [0, 45, 18], 'inside_c': [63, 0, 0], 'outside_h': [0, 63, 0], 'outside_c': [63, 0, 0]},
    ('b', 48, 3, 6, False): {'inside_h': [0, 45, 18], 'inside_c': [63, 0, 0], 'outside_h': [0, 63, 0], 'outside_c': [63, 0, 0]},
    ('b', 400, 2, 5, True): {'inside_h': [0, 20, 10], 'inside_c': [30, 0, 0], 'outside_h': [0, 30, 0], 'outside_c': [30, 0, 0]},
    ('c', 32, 3, 5): {'inside_h': [4, 1, 40], 'inside_c': [4, 1, 40], 'outside_h': [0, 0, 45], 'outside_c': [0, 0, 45]},
    ('c', 400, 2, 5): {'inside_h': [1, 1, 28], 'inside_c': [1, 1, 28], 'outside_h': [0, 0, 30], 'outside_c': [0, 0, 30]},
    ('e', 48, 3, 6, 5, False): {'inside_h': [0, 0, 63], 'inside_c': [63, 0, 0], 'outside_h': [0, 0, 63]},
    ('e', 64, 2, 5, 36, False): {'inside_h': [0, 0, 30], 'inside_c': [30, 0, 0], 'outside_h': [0, 0, 30]},
    ('e', 400, 2, 5, 36, False): {'inside_h': [0, 0, 30], 'inside_c': [30, 0, 0], 'outside_h': [0, 0, 30]},
    ('e', 48, 3, 6, 5, True): {'inside_h': [25, 0, 38], 'inside_c': [63, 0, 0], 'outside_h': [0, 0, 63]},
    ('e', 64, 2, 5, 36, True): {'inside_h': [16, 0, 14], 'inside_c': [30, 0, 0], 'outside_h': [0, 0, 30]},
    ('f', 48, 3, 6, 36): {'inside_h': [0, 0, 63], 'inside_c': [45, 0, 18], 'outside_h': [0, 0, 63]},
    ('f', 32, 2, 5, 5): {'inside_h': [0, 0, 30], 'inside_c': [20, 0, 10], 'outside_h': [0, 0, 30]},
}

# The oracle's own fp32 run against its fp64 run, by the rule above: the worst (output, gradient) rel_err over all cases.  The CPU test
# asserts each case stays within 1 / 20 of OUT_TOL / GRAD_TOL.
MEASURED_ORACLE_FP32 = (1.80e-6, 7.76e-6)      # outputs: case b D 400; gradients: case c D 400

# The device against the fp64 oracle on the MI355X, worst (output, gradient) rel_err per case family and arithmetic mode over every
# shape and schedule of test_gpu_degenerate.py, as that test prints them.  In 'bf16x3' the gradient figure is
# the maximum element error, which conftest.grad_check bounds by 5e-2 (its median bound is the tight one).
MEASURED_DEVICE = {
    # (case, mode, path): (outputs, gradients)
    ('a', 'f32', 'launches'): (9.33e-7, 2.79e-6), ('a', 'f32', 'resident'): (4.16e-7, 8.51e-7),
    ('a', 'bf16x3', 'launches'): (9.03e-6, 1.30e-4), ('a', 'bf16x3', 'resident'): (4.16e-7, 8.51e-7),
    ('b', 'f32', 'launches'): (1.24e-6, 5.29e-6), ('b', 'f32', 'resident'): (7.65e-7, 1.37e-6),
    ('b', 'bf16x3', 'launches'): (1.89e-6, 6.71e-6), ('b', 'bf16x3', 'resident'): (7.65e-7, 1.37e-6),
    ('c', 'f32', 'launches'): (1.06e-5, 3.30e-5),       # the hardware exp / rcp forms of the gates (lstm_kernels.hpp): 1e-7 absolute per gate
    ('e', 'f32', 'launches'): (1.21e-6, 4.93e-6), ('e', 'bf16x3', 'launches'): (9.05e-6, 3.69e-5),
    ('f', 'f32', 'launches'): (3.50e-7, 1.45e-6), ('f', 'bf16x3', 'launches'): (6.93e-6, 3.16e-5),
    ('g', 'f32', 'launches'): (None, 7.64e-6), ('g', 'bf16x3', 'launches'): (None, 1.31e-5),        # parameter gradients, eval and train alike
}
# Before the fix of lstm_tanh (lstm_kernels.hpp) case c measured outputs 2.1e-1 / gradients 4.0e-1: the sub-eps leaf came out as zeros.
