"""The HIP kernels on the inputs training really starts from (tests/degenerate_cases.py; premises in tests/test_degenerate_cpu.py):
rows whose norm is zero or below the unit-norm clamp, exact ties in CKY and in the region max, ReLU pre-activations of exactly +0 and
the zero-initialised image encoder -- against the fp64 CPU oracle, rows compared class by class (degenerate_cases.assert_matches).

Every `h = g / max(||g||, 1e-8)` site of the kernels and the case that takes its clamp branch (a zero or sub-eps row).  D <= 64 plans
run the sentence-resident kernels unless cliora_set_resident is 'off'; the merged grids need cliora_set_wavefront 'merged'.

  site                           kernel, row                                      reached by
  chart_kernels.hpp:96           unit_norm_rows: leaves, outside root (forward)   a (leaves), b (root); launches: resident off, or D 400
  chart_kernels.hpp:420          unit_norm_bwd: leaf_bwd_pre, cell_dnorm,         a (leaves, sentence 1's inside root), b (outside
                                 cell_attend_bwd, the TreeLSTM backward           leaves); c; e with the leaf edits
  chart_kernels.hpp:487          root_bwd                                         b (root_vector_out_h x 1e-10), launches and resident
  chart_kernels.hpp:578          NormBwdLevelE: levels 1 .. L-2 (backward GEMM)   a (sentence 2's cell (0, 2), sentence 1), b; launches
  level_kernels.hpp:693          score_cell: the newest level's partial rows      a, b; launches, wavefront off / on / merged
  level_kernels.hpp:807          project_block (level_project)                    a, b; launches, wavefront off / on
  level_kernels.hpp:889          finish_cells: inside root, outside leaves        a (sentence 1's root), b; launches, every wavefront mode
  level_kernels.hpp:987          project_tile (level_project2)                    a, b; launches, wavefront merged
  resident_kernels.hpp:366       res_cell_fwd: composed cells                     a, b at D 48 / 33, resident on
  resident_kernels.hpp:471       resident_fwd: leaves                             a at D 48 / 33, resident on
  resident_kernels.hpp:493       resident_fwd: outside root                       b at D 48, resident on
  resident_kernels.hpp:557       res_dnorm (resident_bwd)                         a, b at D 48 / 33, resident on
  lstm_kernels.hpp:57            TreeLSTM composed cells (h and c)                c (sentence 2's cell (0, 2))
  lstm_kernels.hpp:349           TreeLSTM leaves (h and c)                        c
  vl_kernels.hpp:82              cell_attend_fwd: u = unit(aggregate)             e with the leaf edits (zero and sub-eps leaves, zero cells)
  vl_kernels.hpp:117             cell_attend_fwd: h = unit(u + context)           e with the leaf edits (zero rows)
  vl_kernels.hpp:123             cell_attend_fwd: c = unit(context), leaves       e (the context of zero regions is 0), f (ordinary)

Tolerances: OUT_TOL = 1e-4 on outputs, conftest.grad_check(t, ref, mfma_mode, 2e-4) on gradients, each against the scale of its own
class of rows.  Every test prints what it measured (`MEASURED ...`, pytest -s); the figures taken on the MI355X are kept in
degenerate_cases.MEASURED_DEVICE and DESIGN.md section 16.
"""
import numpy as np
import pytest
import torch

import degenerate_cases as DC
import posterior_cases as PC
from conftest import grad_check
from oracle import diora_ref as R
from test_gpu_parity import _module_from_params

pytestmark = pytest.mark.gpu


def _schedules(D):
    """(cliora_set_resident, cliora_set_wavefront) of the runs of a text case: the launch path in its three orders, and the resident
    kernels where a row fits a wavefront."""
    launches = [('off', 'off'), ('off', 'on'), ('off', 'merged')]
    return launches + ([('on', 'off')] if D <= 64 else [])


def _treelstm_module(P, D):
    from cliora_amd.treelstm import DioraTreeLSTM
    m = DioraTreeLSTM(D, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    return m.cuda()


def _run_text(m, case, keys):
    for p in m.parameters():
        p.grad = None
    xg = case['x_span'].clone().cuda().requires_grad_(True)
    m.train()
    m(xg, xg)
    outs = {k: getattr(m, k) for k in keys}
    torch.autograd.backward([outs[k] for k in keys], [case['cot'][k].cuda() for k in keys])
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    grads['x_span'] = xg.grad.detach().clone()
    return {k: v.detach().clone() for k, v in outs.items()}, grads


def _classes_match(outs, ref, keys):
    """The device's class of every chart row is the oracle's, and an exactly-zero row is exactly zero on the device."""
    for k in keys:
        want = DC.classify(ref['out'][k])
        assert torch.equal(DC.classify(outs[k]), want), k
        zero_rows = outs[k].cpu()[want == DC.ZERO]
        assert bool((zero_rows == 0.0).all()), k


def _equal_bits(a, b, what):
    for part_a, part_b in zip(a, b):
        assert set(part_a) == set(part_b), what
        for k in part_a:
            assert torch.equal(part_a[k], part_b[k]), (what, k)


def _text_case(builder, args, mode, module, keys):
    """A text case under every schedule against the fp64 oracle; -> {schedule: (outs, grads)}."""
    from cliora_amd import _lib
    case, ref = builder(*args), DC.oracle64(builder, args)
    D, L = case['D'], case['L']
    m = module(case)
    rows = [k for k in DC.ROW_CHARTS if k in keys]
    res = {}
    prev_r, prev_w = _lib.set_resident('auto'), _lib.set_wavefront('auto')
    try:
        scheds = _schedules(D) if case['kind'] == 'mlp' else [('auto', 'off'), ('auto', 'on')]
        for resident, wavefront in scheds:
            _lib.set_resident(resident)
            _lib.set_wavefront(wavefront)
            outs, grads = _run_text(m, case, keys)
            w_out, w_grad = DC.measure(outs, grads, ref, L, keys)
            print('MEASURED %s %s %s resident=%s wavefront=%s: outputs %.3e gradients %.3e' % (case['name'], args, mode, resident, wavefront, w_out, w_grad))
            DC.assert_matches(outs, grads, ref, L, keys, mode)
            _classes_match(outs, ref, rows)
            if case['kind'] == 'mlp':
                assert float(m.inside_c.abs().max()) == 0.0 and float(m.outside_c.abs().max()) == 0.0
            _equal_bits((outs, grads), _run_text(m, case, keys), 'second run, resident=%s wavefront=%s' % (resident, wavefront))
            res[(resident, wavefront)] = (outs, grads)
        first = scheds[0]
        for s in scheds[1:]:
            if s[0] == first[0]:         # the same kernels scheduled differently: the same bits
                _equal_bits(res[first], res[s], '%s against %s' % (s, first))
    finally:
        _lib.set_resident(prev_r)
        _lib.set_wavefront(prev_w)
    if mode == 'f32' and ('on', 'off') in res:
        # the resident kernels against the launches, by the bounds of test_gpu_resident.py (5e-6 / 3e-5 of scale), rows by class
        (o1, g1), (o0, g0) = res[('on', 'off')], res[('off', 'off')]
        lc = DC.leaf_class(ref, L)
        for k in keys:
            worst = DC.measure_rows(o1[k], o0[k], DC.classify(ref['out'][k])) if k in rows else DC.rel_err(o1[k], o0[k])
            assert worst <= 5e-6, (k, worst)
        for k in g0:
            worst = DC.measure_rows(g1[k], g0[k], lc) if DC.row_keyed(k) else DC.rel_err(g1[k], g0[k])
            assert worst <= 3e-5, (k, worst)
    return case, ref, m, res


def _mlp_module(case):
    return _module_from_params(case['P'], case['D'], case['share'], 'unit')


@pytest.mark.parametrize('D,B,L,share', DC.CASES_A)
def test_case_a_zero_and_sub_eps_leaf_rows(D, B, L, share, mfma_mode):
    """Zero words, a sub-eps word, an all-zero sentence and a cell composed of [0; 0] with zero biases (ReLU at exactly +0): outputs,
    classes, gradients under every schedule; the trees and spans of all four sentences -- sentence 1 is all exact ties (the first
    maximum at every cell), sentence 2 ties exactly at cell (0, 2), the rest is beyond ragged_cases.NEAR_TIE (test_degenerate_cpu.py)
    -- and the posterior of the tied sentence."""
    from cliora_amd import _lib
    case, ref, m, _ = _text_case(DC.case_a, (D, B, L, share), mfma_mode, _mlp_module, DC.CHARTS)
    want = R.cky_trees(ref['pair_s_in'], B, L)
    m.eval()
    for resident in (['off', 'on'] if D <= 64 else ['off']):
        prev = _lib.set_resident(resident)
        try:
            with torch.no_grad():
                x = case['x_span'].clone().cuda()
                m(x, x)
            assert [str(t) for t in m.cky()] == [str(t) for t in want], resident
            assert m.cky_spans().tolist() == [[list(s) for s in R.tree_spans(t)] for t in want], resident
            post = m.span_posteriors()
            marg = post.marginals.cpu().numpy()
        finally:
            _lib.set_resident(prev)
        from cliora_amd.posterior import cell_id
        mu, log_z, _, _ = PC.enumerate_posteriors({lv: s.numpy()[..., 0] for lv, s in ref['pair_s_in'].items()}, 1, L)
        for level in range(1, L):
            row = [float(marg[1, cell_id(L, level, p)]) for p in range(L - level)]
            assert max(row) - min(row) <= PC.BOUND, (level, row)                         # one marginal per level
            for p in range(L - level):
                assert abs(row[p] - mu[(level, p)]) <= PC.BOUND, (level, p)
        assert abs(float(post.log_z[1]) - log_z) <= PC.BOUND * max(1.0, abs(log_z))


@pytest.mark.parametrize('D,B,L,share', DC.CASES_B)
def test_case_b_every_composed_cell_below_eps(D, B, L, share, mfma_mode):
    """Every composed cell of both charts and the outside root take the clamp branch, forward and backward, under every schedule."""
    _text_case(DC.case_b, (D, B, L, share), mfma_mode, _mlp_module, DC.CHARTS)


@pytest.mark.parametrize('D,B,L', DC.CASES_C)
def test_case_c_treelstm_zero_and_sub_eps_leaves(D, B, L):
    """TreeLSTM leaves and the cell composed of two zero leaves: h and c both normalised, all six charts carry a cotangent."""
    _text_case(DC.case_c, (D, B, L), 'f32', lambda case: _treelstm_module(case['P'], case['D']), DC.CHARTS6)


# ---- CLIORA ---------------------------------------------------------------------------------------------------------------------------
def _vl_module(case, lazy):
    from cliora_amd.cliora import DioraMLP
    m = DioraMLP(case['D'], outside=True, normalize='unit', compress=False, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = case['P'][k if k in case['P'] else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    m = m.cuda().train()
    m.lazy_region_scores = lazy
    m.dropout_mask = case['mask'].cuda()
    return m


def _run_vl(m, case, lazy):
    """Forward in train mode with the recorded mask, the two VL losses on the device's outputs added to the cotangent sum, backward.
    -> (outs, grads, region max (values, indices) of all_atten_score)."""
    from cliora_amd.cliora import LazyRegionScores
    for p in m.parameters():
        p.grad = None
    t = {k: case[k].clone().cuda().requires_grad_(True) for k in ('x_span', 'x_word', 'obj_span', 'obj_word')}
    m(t['x_span'], t['x_word'], t['obj_span'], t['obj_word'])
    assert isinstance(m.all_atten_score, LazyRegionScores) == lazy
    rmax = m.all_atten_score.max(-1)
    lc = R.contrastive_loss(m.inside_s, m.outside_s, m.all_atten_score, 0.2, 1.0)
    lv = R.vg_loss(m.vg_atten_score, 1.0)
    keys = DC.vl_keys(lazy)
    (lc + lv + sum((getattr(m, k) * case['cot'][k].cuda()).sum() for k in keys)).backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        outs = {k: getattr(m, k) for k in DC.VL_OUTS if k != 'all_atten_score'}
        outs['all_atten_score'] = m.all_atten_score.materialize() if lazy else m.all_atten_score
        outs = {k: v.detach().clone() for k, v in outs.items()}
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    grads.update({k: v.grad.detach().clone() for k, v in t.items() if v.grad is not None})
    losses = dict(contrastive=float(lc.detach()), vg=float(lv.detach()))
    return outs, grads, (rmax.values.detach().clone(), rmax.indices.clone()), losses


def _vl_against_oracle(case, ref, outs, grads, losses, mode, what):
    w_out, w_grad = DC.measure(outs, grads, ref, case['L'], DC.VL_OUTS)
    print('MEASURED %s %s: outputs %.3e gradients %.3e' % (what, mode, w_out, w_grad))
    DC.assert_matches(outs, grads, ref, case['L'], DC.VL_OUTS, mode)
    _classes_match(outs, ref, ('inside_h', 'inside_c', 'outside_h'))
    for k, want in ref['losses'].items():
        assert abs(losses[k] - want) <= 1e-4 * max(1.0, abs(want)), (k, losses[k], want)


@pytest.mark.parametrize('lazy', [True, False])
@pytest.mark.parametrize('D,B,L,Rg,edits', DC.CASES_E)
def test_case_e_zero_image_encoder(D, B, L, Rg, edits, lazy, mfma_mode):
    """obj_span = obj_word = 0, what the zero-initialised ImageEncoder hands the chart in the first steps of a run: every VL score is
    exactly 0, every region ties (region 0 takes the gradient), the attention context is 0 and inside_c = unit(0) goes through the clamp;
    with case a's leaf edits on top, zero and sub-eps rows go through both norms of the leaf."""
    args = (D, B, L, Rg, edits)
    case, ref = DC.case_e(*args), DC.oracle64(DC.case_e, args, lazy)
    m = _vl_module(case, lazy)
    outs, grads, (vmax, arg), losses = _run_vl(m, case, lazy)
    _vl_against_oracle(case, ref, outs, grads, losses, mfma_mode, 'e %s lazy=%s' % (args, lazy))
    for k in ('all_atten_score', 'vg_atten_score', 'atten_score'):
        assert bool((outs[k] == 0.0).all()), k
    assert bool((outs['inside_c'] == 0.0).all())
    assert bool((vmax == 0.0).all()) and bool((arg == 0).all())                 # the first of equal scores, dense and lazy alike
    outs2, grads2, _, _ = _run_vl(m, case, lazy)
    _equal_bits((outs, grads), (outs2, grads2), 'second run')


@pytest.mark.parametrize('D,B,L,Rg', DC.CASES_F)
def test_case_f_duplicated_regions_tie_in_the_region_max(D, B, L, Rg, mfma_mode):
    """Copies of region rows score bitwise the same on the device; the lazy region max (region_key: the smallest region index among
    equal scores) picks the lower one, as torch.max does on the dense tensor, and that choice decides which row of obj_span gets the
    gradient.  The sum over a pair of rows holds whatever the tie rule: a failure there is a wrong gradient, not a wrong tie."""
    args = (D, B, L, Rg)
    case = DC.case_f(*args)
    pairs = DC.duplicate_pairs(Rg)
    res = {}
    for lazy in (False, True):
        ref = DC.oracle64(DC.case_f, args, lazy)
        m = _vl_module(case, lazy)
        outs, grads, (vmax, arg), losses = res[lazy] = _run_vl(m, case, lazy)
        for k in ('all_atten_score', 'vg_atten_score'):
            for lo, hi in pairs:
                assert torch.equal(outs[k][..., lo], outs[k][..., hi]), (k, lo, hi, lazy)
        for lo, hi in pairs:
            assert int((arg == hi).sum()) == 0, (hi, lazy)
        assert int(sum((arg == lo).sum() for lo, _ in pairs)) > 0                 # ties do decide some of the maxima
        for k in ('obj_span', 'obj_word'):
            for lo, hi in pairs:
                grad_check(grads[k][:, lo] + grads[k][:, hi], ref['grad'][k][:, lo] + ref['grad'][k][:, hi], mfma_mode, DC.GRAD_TOL,
                           '%s rows %d + %d, lazy=%s' % (k, lo, hi, lazy))
        _vl_against_oracle(case, ref, outs, grads, losses, mfma_mode, 'f %s lazy=%s' % (args, lazy))
    dense_max = res[False][0]['all_atten_score'].max(-1)
    assert torch.equal(res[True][2][0], dense_max.values) and torch.equal(res[True][2][1], dense_max.indices)
    assert torch.equal(res[True][2][1], res[False][2][1])


# ---- the first training step as built ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
def test_case_g_first_training_step_with_the_zero_image_encoder(train, mfma_mode):
    """harness.build_net with its own zero img_encoder, left untouched, all three losses: eval mode with gradients on (as
    test_gpu_configs.test_c3_cliora_full_size) and train mode with a recorded dropout mask and the lazy region max (as
    test_c3_cliora_full_size_training_mode), against the same oracle chain.  The image encoder must get a gradient that lets the run
    leave its initial state, and one Trainer.step must leave every parameter finite."""
    from cliora_amd import harness as H
    B, L, D, Rg, V, E, K, IMG = 4, 6, 48, 36, 300, 64, 20, 32
    C = L * (L + 1) // 2
    torch.manual_seed(DC.SEED['g'])
    net = H.build_net(D, torch.nn.Embedding(V, E), obj_feats=True, img_dim=IMG, k_neg=K, vg_loss=True, use_contr=True,
                      vl_margin=0.2, alpha_contr=1.0, alpha_vg=1.0)
    assert all(float(p.abs().max()) == 0.0 for p in net.img_encoder.parameters())          # as built
    g = torch.Generator().manual_seed(DC.SEED['g'] + 1)
    sentences = torch.randint(0, V, (B, L), generator=g)
    neg = torch.randperm(V, generator=g)[:K]
    obj = torch.relu(torch.randn(B, Rg, IMG, generator=g))
    mask = (torch.rand(B, C, Rg, generator=g) > 0.1).float() / 0.9
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.cuda().train(train)
    if train:
        net.diora.dropout_mask = mask.cuda()
        assert net.diora.lazy_region_scores
    out = net(sentences.cuda(), obj.cuda(), neg.cuda())
    out['total_loss'].mean(0).sum().backward()
    torch.cuda.synchronize()
    diora = net.diora

    P = {k[len('diora.'):]: v.clone().double().requires_grad_(True) for k, v in sd.items() if k.startswith('diora.')}
    emb_w = sd['embed.embeddings.weight'].clone().double()
    mat, mat1 = sd['embed.mat'].clone().double().requires_grad_(True), sd['embed.mat1'].clone().double().requires_grad_(True)
    iw = {k: sd['img_encoder.' + k].clone().double().requires_grad_(True) for k in ('fc.weight', 'fc.bias', 'fc_vis.weight', 'fc_vis.bias')}
    rmat = sd['reconstruct_softmax_loss.mat'].clone().double().requires_grad_(True)
    xs, xw = R.embed_forward(emb_w, mat, mat1, sentences)
    os_, ow = R.image_encoder_forward(iw['fc.weight'], iw['fc.bias'], iw['fc_vis.weight'], iw['fc_vis.bias'], obj)
    off = [C - (L - lv) * (L - lv + 1) // 2 for lv in range(L)] + [C]
    calls = {'i': 0}
    orig = R.F.dropout

    def replay(x, p, training):
        i = calls['i']
        calls['i'] += 1
        return x * mask[:, off[i]:off[i + 1]].double()
    if train:
        R.F.dropout = replay
    try:
        ref = R.diora_forward(P, xs, xw, os_, ow, training=train)
    finally:
        R.F.dropout = orig
    assert calls['i'] == (L if train else 0)
    l_rec = R.reconstruction_loss(emb_w, rmat, sentences, neg, ref['outside_h'])
    l_vg = R.vg_loss(ref['vg_atten_score'], 1.0)
    l_con = R.contrastive_loss(ref['inside_s'], ref['outside_s'], ref['all_atten_score'], 0.2, 1.0)
    (l_rec + l_vg + l_con).backward()

    for k in ('inside_h', 'inside_s', 'outside_h', 'outside_s', 'inside_c', 'vg_atten_score', 'atten_score'):
        DC.out_check(getattr(diora, k).detach().double().cpu(), ref[k].detach(), k)
    assert float(diora.inside_c.abs().max()) == 0.0 and float(diora.vg_atten_score.abs().max()) == 0.0
    rmax = diora.all_atten_score.max(-1)
    assert float(rmax.values.abs().max()) == 0.0 and int(rmax.indices.abs().max()) == 0
    for name, want in (('reconstruct_softmax_loss', l_rec), ('vg_loss', l_vg), ('contrastive_loss', l_con)):
        got = float(out[name].sum())
        assert abs(got - float(want)) <= 1e-4 * max(1.0, abs(float(want))), (name, got, float(want))
    named = dict(net.named_parameters())
    worst = 0.0
    checks = [('diora.' + k, p) for k, p in P.items() if p.grad is not None]          # shared weights: the outside_* aliases take no part
    checks += [('img_encoder.' + k, p) for k, p in iw.items()] + [('embed.mat', mat), ('embed.mat1', mat1)]
    for name, p in checks:
        assert p.grad is not None and named[name].grad is not None, name
        assert bool(torch.isfinite(named[name].grad).all()), name
        worst = max(worst, DC.rel_err(named[name].grad, p.grad))
        grad_check(named[name].grad, p.grad, mfma_mode, DC.GRAD_TOL, name)
    print('MEASURED g %s %s: gradients %.3e' % ('train' if train else 'eval', mfma_mode, worst))
    assert float(named['img_encoder.fc.weight'].grad.abs().max()) > 0.0               # the run can leave its initial state
    assert float(iw['fc.weight'].grad.abs().max()) > 0.0
    # one optimiser step from the state as built
    trainer = H.Trainer(net, lr=2e-3, k_neg=K)
    res = trainer.step(dict(sentences=sentences.cuda(), obj_feats=obj.cuda(), neg_samples=neg.cuda()))
    torch.cuda.synchronize()
    assert np.isfinite(res['total_loss'])
    for n, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), n
    assert float(net.img_encoder.fc.weight.abs().max()) > 0.0
