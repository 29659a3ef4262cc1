"""The premises of tests/test_gpu_degenerate.py, on the CPU oracle alone (tests/degenerate_cases.py): every case reaches the rows it is
about (class counts pinned as constants), is finite in fp32, is well-posed (the fp32 oracle sits within 1 / 20 of the GPU test's
bounds of the fp64 one, by the same row-wise rule), ties where it is meant to tie and nowhere near a tie elsewhere -- and the
comparison rule fails when the clamp branch's backward or the tie rule is wrong (the self-checks at the end).
"""
import numpy as np
import pytest
import torch

import degenerate_cases as DC
import posterior_cases as PC
import ragged_cases as RC
from oracle import chart_layout as CL
from oracle import diora_ref as R

ALL = list(DC.all_cases())
IDS = ['-'.join(str(v) for v in cid) for cid, _, _ in ALL]


@pytest.mark.parametrize('cid,builder,args', ALL, ids=IDS)
def test_classes_finiteness_and_the_oracles_own_error(cid, builder, args):
    case = builder(*args)
    for lazy in ((True, False) if case['kind'] == 'vl' else (True,)):
        r64 = DC.oracle64(builder, args, lazy)
        r32 = DC.run_oracle(case, torch.float32, lazy)
        keys = [k for k in DC.ROW_CHARTS if k in r64['out']]
        assert DC.class_counts(r64['out'], keys) == DC.CLASS_COUNTS[cid]
        assert DC.class_counts(r32['out'], keys) == DC.CLASS_COUNTS[cid]
        for k in keys:
            assert torch.equal(DC.classify(r32['out'][k]), DC.classify(r64['out'][k])), k
        for k, v in list(r32['out'].items()) + list(r32['grad'].items()):
            assert bool(torch.isfinite(v).all()), k
        w_out, w_grad = DC.measure(r32['out'], r32['grad'], r64, case['L'], DC.out_keys_of(case))
        print('%s lazy=%s: fp32 oracle against fp64, outputs %.3e gradients %.3e' % (cid, lazy, w_out, w_grad))
        assert w_out <= DC.MEASURED_ORACLE_FP32[0] * 1.001 <= DC.OUT_TOL / 20
        assert w_grad <= DC.MEASURED_ORACLE_FP32[1] * 1.001 <= DC.GRAD_TOL / 20
        DC.assert_matches(r32['out'], r32['grad'], r64, case['L'], DC.out_keys_of(case), 'f32')


@pytest.mark.parametrize('cid,builder,args', [c for c in ALL if DC.needs_kink_margin(c[0])], ids=[i for i, c in zip(IDS, ALL) if DC.needs_kink_margin(c[0])])
def test_no_relu_pre_activation_within_rounding_of_zero(cid, builder, args):
    """The cases that run in the split-bf16 mode at D <= 64 keep every pre-activation that is not an exact zero KINK_MARGIN of its
    layer's scale away from zero (degenerate_cases.CASE_SEED): no gradient of theirs hinges on which side a rounding lands."""
    assert DC.relu_margin(builder(*args)) >= DC.KINK_MARGIN


def test_the_seed_table_is_what_the_search_finds():
    saved = dict(DC.CASE_SEED)
    try:
        DC.CASE_SEED.clear()
        assert DC.seed_search() == saved
    finally:
        DC.CASE_SEED.clear()
        DC.CASE_SEED.update(saved)
        for fn in (DC.case_a, DC.case_b, DC.case_e, DC.case_f):
            fn.cache_clear()
        DC.oracle64.cache_clear()


@pytest.mark.parametrize('D,B,L,share', DC.CASES_A)
def test_case_a_reaches_the_rows_it_names(D, B, L, share):
    r = DC.oracle64(DC.case_a, (D, B, L, share))
    ih, oh = DC.classify(r['out']['inside_h']), DC.classify(r['out']['outside_h'])
    assert bool((ih[1] == DC.ZERO).all()) and bool((oh[1] == DC.UNIT).all())          # the all-zero sentence: inside 0, outside unit
    zeros0 = torch.nonzero(ih[0] == DC.ZERO).flatten().tolist()
    assert zeros0 == [1] and int(ih[0, 4]) == DC.SUB_EPS
    n4 = float(r['out']['inside_h'][0, 4].norm())
    assert 0.2 <= n4 <= 0.5, n4                                                        # a pre-norm of about eps / 2 at every width
    assert torch.nonzero(ih[2] == DC.ZERO).flatten().tolist() == [0, 1, CL.cell_id(L, 1, 0)]
    assert bool((ih[3] == DC.UNIT).all())
    # the clamp rows' gradients are 1 / eps times the rest: the reason for the row-wise rule
    gx = r['grad']['x_span'].abs().amax(-1)
    assert float(gx[0, 4]) > 1e7 * float(gx[3].max())


@pytest.mark.parametrize('D,B,L,share', DC.CASES_B)
def test_case_b_every_composed_cell_is_below_eps(D, B, L, share):
    r = DC.oracle64(DC.case_b, (D, B, L, share))
    ih, oh = DC.classify(r['out']['inside_h']), DC.classify(r['out']['outside_h'])
    assert bool((ih[:, :L] == DC.UNIT).all()) and bool((ih[:, L:] == DC.SUB_EPS).all())
    assert bool((oh == DC.SUB_EPS).all())                                              # the root included


def test_the_excluded_all_zero_treelstm_sentence_overflows_the_fp32_oracle():
    """Case d: why no TreeLSTM case holds an all-zero sentence (degenerate_cases.py)."""
    D, B, L = 32, 3, 5
    case = dict(DC.case_c(D, B, L))
    x = case['x_span'].clone()
    x[1] = 0.0
    case['x_span'] = x
    r32 = DC.run_oracle(case, torch.float32)
    assert not all(bool(torch.isfinite(v).all()) for v in r32['grad'].values())


@pytest.mark.parametrize('D,B,L,share', DC.CASES_A)
def test_case_a_trees_and_ties(D, B, L, share):
    case = DC.case_a(D, B, L, share)
    r64 = DC.oracle64(DC.case_a, (D, B, L, share))
    r32 = DC.run_oracle(case, torch.float32)
    t64, t32 = R.cky_trees(r64['pair_s_in'], B, L), R.cky_trees(r32['pair_s_in'], B, L)
    assert [str(t) for t in t64] == [str(t) for t in t32]
    first_max = _right_branching(L)
    assert str(t64[1]) == str(first_max)                       # every candidate of the all-zero sentence ties: the first maximum at every cell
    if L == 6:
        assert str(t64[1]) == '(0, (1, (2, (3, (4, 5)))))'
    # Sentence 1: every gap is exactly 0.  Elsewhere a gap is either EXACTLY 0 in both precisions -- a structural tie between exact
    # zeros, decided by the first-maximum rule like sentence 1: sentence 2's cell (0, 2), whose splits both score 0 + 0 + 0 -- or
    # beyond NEAR_TIE, so that no tree hinges on rounding.
    for b in range(B):
        g64, g32 = DC.cky_gaps(r64['pair_s_in'], b, L), DC.cky_gaps(r32['pair_s_in'], b, L)
        if b == 1:
            assert g64 == [0.0] * len(g64) and g32 == g64
            continue
        for a, c in zip(g64, g32):
            assert (a == 0.0 and c == 0.0) or (a > RC.NEAR_TIE and c > RC.NEAR_TIE), (b, a, c)
        assert (b == 2) == (0.0 in g64), (b, g64)
    # the tied sentence's posterior: every tree weighs the same, so a level's spans share one marginal
    mu, _, trees, prob = PC.enumerate_posteriors({lv: s.numpy()[..., 0] for lv, s in r64['pair_s_in'].items()}, 1, L)
    assert np.allclose(prob, 1.0 / len(trees), atol=1e-15)
    for level in range(1, L):
        row = [mu[(level, p)] for p in range(L - level)]
        assert max(row) - min(row) <= 1e-12, (level, row)


def _right_branching(L):
    t = L - 1
    for w in range(L - 2, -1, -1):
        t = (w, t)
    return t


@pytest.mark.parametrize('D,B,L,Rg', DC.CASES_F)
def test_case_f_duplicated_regions_tie_bitwise_and_the_first_wins(D, B, L, Rg):
    case = DC.case_f(D, B, L, Rg)
    for dt in (torch.float64, torch.float32):
        r = DC.run_oracle(case, dt)
        for k in ('all_atten_score', 'vg_atten_score'):
            s = r['out'][k]
            idx = s.max(-1).indices
            for lo, hi in DC.duplicate_pairs(Rg):
                assert torch.equal(s[..., lo], s[..., hi]), (k, lo, hi)
                assert int((idx == hi).sum()) == 0, (k, hi)                 # torch.max: the lower index of equal scores
            dup_lo = [lo for lo, _ in DC.duplicate_pairs(Rg)]
            assert int(sum((idx == lo).sum() for lo in dup_lo)) > 0, k      # ... and ties do decide some of the maxima


def test_case_g_premise_the_image_encoder_is_built_zero():
    from cliora_amd import harness as H
    net = H.build_net(48, torch.nn.Embedding(300, 64), obj_feats=True, img_dim=32, k_neg=20, vg_loss=True, use_contr=True)
    assert all(float(p.detach().abs().max()) == 0.0 for p in net.img_encoder.parameters())


# ---- the rule can fail for the right reason ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('builder,args', [(DC.case_a, DC.CASES_A[0]), (DC.case_a, DC.CASES_A[3]), (DC.case_b, DC.CASES_B[0]),
                                          (DC.case_b, DC.CASES_B[2]), (DC.case_c, DC.CASES_C[0]), (DC.case_e, DC.CASES_E[3])],
                         ids=['a-48', 'a-400', 'b-48', 'b-400', 'c-32', 'e-48-edits'])
def test_self_check_an_ordinary_unit_norm_backward_in_the_clamp_branch_fails(builder, args):
    """The mutant keeps the forward and uses the ordinary backward (v - n (n . v)) / ||g||, n = g / ||g||, on the sub-eps rows too
    (degenerate_cases._ClampFreeBackward)."""
    case = builder(*args)
    ref = DC.oracle64(builder, args)
    bad = DC.run_oracle(case, torch.float64, mutant='no_clamp_backward')
    keys = DC.out_keys_of(case)
    for k in keys:                                                   # the forward is untouched
        assert torch.equal(bad['out'][k], ref['out'][k]), k
    with pytest.raises(AssertionError):
        DC.assert_matches(bad['out'], bad['grad'], ref, case['L'], keys, 'f32')
    with pytest.raises(AssertionError):                              # ... under the statistical check of the split-bf16 mode too
        DC.assert_matches(bad['out'], bad['grad'], ref, case['L'], keys, 'bf16x3')


@pytest.mark.parametrize('D,B,L,Rg', DC.CASES_F)
def test_self_check_the_last_tied_region_fails_and_the_pair_sum_does_not(D, B, L, Rg):
    case = DC.case_f(D, B, L, Rg)
    ref = DC.oracle64(DC.case_f, (D, B, L, Rg))
    bad = DC.run_oracle(case, torch.float64, mutant='last_region')
    keys = DC.out_keys_of(case)
    assert bad['losses'] == ref['losses']
    # (exact-product mode: one moved region row is 1e-2 of the tensor's scale, which the split-bf16 mode's statistical bound on single
    # elements, 5e-2, lets through -- there the GPU test's own assertion on the arg-max is what catches a wrong tie)
    with pytest.raises(AssertionError):
        DC.assert_matches(bad['out'], bad['grad'], ref, L, keys, 'f32')
    for k in ('obj_span', 'obj_word'):
        for lo, hi in DC.duplicate_pairs(Rg):
            a, b = bad['grad'][k][:, lo] + bad['grad'][k][:, hi], ref['grad'][k][:, lo] + ref['grad'][k][:, hi]
            assert DC.rel_err(a, b) <= 1e-12, (k, lo, hi)
