"""Training CLIORA through a padded chart of mixed lengths, the facts it rests on, on the CPU in fp64: the
padded schedule with the attention over each sentence's own regions, differentiated by torch autograd, gives the sum of the oracle's
per-sentence exact-length gradients, d obj_span and a replayed dropout mask included; the two mixed-length loss definitions reduce to
the reference's at one length and let nothing beyond a triangle through; the torch fallbacks of harness.VGLoss / ContrastiveLoss
compute those definitions."""
import pytest
import torch

import ragged_outside_cases as ROC
import ragged_train_cases as TC
import ragged_vl_train_cases as VC
from oracle import diora_ref as R


@pytest.mark.parametrize('D,lengths,share', VC.CPU_CASES)
def test_padded_schedule_with_regions_differentiates_to_the_per_sentence_gradients(D, lengths, share):
    L = max(lengths)
    assert {1, 2, L} <= set(lengths) and len(set(lengths)) < len(lengths)
    P, xs, objs, mask = VC.vl_case(D, VC.REGIONS, lengths, seed=131 + D, share=share)
    assert bool((mask == 0).any()) and bool((mask > 1).any())            # a mask that drops and rescales
    W = TC.weights(L, lengths, D, seed=7)
    want_loss, want, want_dx, want_dobj, _ = VC.oracle_sum(P, xs, objs, lengths, W, mask, 'unit', share)
    loss, got, dx, dobj = VC.padded_autograd(P, ROC.padded(xs, L), objs, lengths, W, mask, 'unit', share)
    assert abs(loss - want_loss) <= VC.CPU_BOUND * max(1.0, abs(want_loss))          # (1.1e-15 measured: to the last digit)
    worst = 0.0
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        worst = max(worst, TC.rel_err(got[k], want[k]))
    for b, n in enumerate(lengths):
        assert bool(torch.isfinite(dx[b]).all()) and bool(torch.isfinite(dobj[b]).all())
        worst = max(worst, TC.rel_err(dx[b, :n], want_dx[b]), TC.rel_err(dobj[b], want_dobj[b]))
        assert not dx[b, n:].any()                       # d x of every padded position: exactly 0
    assert max(float(d.abs().max()) for d in want_dobj) > 1e-2           # a reference that moves the regions
    print('D %d share=%s: worst relative error %.3e' % (D, share, worst))
    assert worst <= VC.CPU_BOUND


@pytest.mark.parametrize('B,L,Rn', [(5, 4, 6), (3, 1, 2)])
def test_the_definitions_are_the_references_at_one_length(B, L, Rn):
    C = L * (L + 1) // 2
    g = torch.Generator().manual_seed(3)
    all_att = torch.randn(B, B, C, Rn, generator=g, dtype=torch.float64)
    vg = torch.randn(B, B, L, Rn, generator=g, dtype=torch.float64)
    ins, outs = torch.randn(B, C, 1, generator=g, dtype=torch.float64), torch.randn(B, C, 1, generator=g, dtype=torch.float64)
    full = [L] * B
    assert float(VC.vg_loss_ragged(vg, full, 0.7)) == pytest.approx(float(R.vg_loss(vg, 0.7)), rel=0, abs=1e-15)
    want = float(R.contrastive_loss(ins, outs, all_att, 0.2, 0.9))
    got = float(VC.contrastive_loss_ragged(ins, outs, all_att.max(-1).values, full, 0.2, 0.9))
    assert abs(got - want) <= 1e-15 * max(1.0, abs(want))
    if L == 1:
        assert got == 0.0                                # span_length // 2 == 0: no cell enters


def _grads(fn, tensors):
    leaves = [t.clone().requires_grad_(True) for t in tensors]
    v = fn(*leaves)
    (1.7 * v).backward()
    return float(v.detach()), [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves]


@pytest.mark.parametrize('name', ['B6', 'B3', 'B2'])
def test_definitions_and_torch_fallbacks_let_nothing_beyond_the_triangles_through(name):
    """The restatements (which never index beyond a triangle) and the modules' torch paths (which replace what is there by zeros
    before any arithmetic): with NaN in every input beyond the triangles / words, value and gradients are finite and unchanged, the
    gradients there exactly 0, and the two agree."""
    from cliora_amd import harness as H
    B, L, Rn, lengths = VC.LOSS_CASES[name]
    vg, smax, ins, outs = VC.loss_inputs(name)
    own = torch.from_numpy(TC.own_mask(L, lengths))
    words = VC.word_mask(L, lengths)
    lens = torch.tensor(lengths, dtype=torch.int32)
    vg_nan = VC.poison(vg.permute(0, 2, 1, 3), words).permute(0, 2, 1, 3).contiguous()
    smax_nan = VC.poison(smax.permute(0, 2, 1), own).permute(0, 2, 1).contiguous()
    ins_nan, outs_nan = VC.poison(ins, own), VC.poison(outs, own)
    assert all(bool(torch.isnan(t).any()) for t in (vg_nan, smax_nan, ins_nan, outs_nan))

    class Chart:
        pass

    def module_contrastive(s, i, o):
        d = Chart()
        d.inside_s, d.outside_s, d.all_atten_score = i, o, torch.stack([s, s - 1.0], -1)
        return H.ContrastiveLoss(margin=0.2, alpha_contr=0.7)(d, lens)
    ways = {
        'vg restated': (lambda v: VC.vg_loss_ragged(v, lengths, 0.7), (vg,), (vg_nan,)),
        'vg module': (lambda v: H.VGLoss(0.7)(v, lens), (vg,), (vg_nan,)),
        'contrastive restated': (lambda s, i, o: VC.contrastive_loss_ragged(i, o, s, lengths, 0.2, 0.7), (smax, ins, outs), (smax_nan, ins_nan, outs_nan)),
        'contrastive module': (module_contrastive, (smax, ins, outs), (smax_nan, ins_nan, outs_nan)),
    }
    res = {}
    for what, (fn, clean, dirty) in ways.items():
        v0, g0 = _grads(fn, clean)
        v1, g1 = _grads(fn, dirty)
        assert v0 == v1 and abs(v0) > 0 and v0 == v0, what
        for a, b in zip(g0, g1):
            assert bool(torch.isfinite(b).all()) and torch.equal(a, b), what
        res[what] = (v0, g0)
    for kind in ('vg', 'contrastive'):
        (va, ga), (vb, gb) = res[kind + ' restated'], res[kind + ' module']
        assert abs(va - vb) <= 1e-13 * max(1.0, abs(va)), kind
        for a, b in zip(ga, gb):
            assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(a.abs().max())), kind
    d_vg = res['vg module'][1][0]
    assert not d_vg.permute(0, 2, 1, 3)[~words].any()                    # d vg[a, :, l, :] for l >= n_a: exactly 0
    d_smax, d_ins, d_outs = res['contrastive module'][1]
    assert not d_smax.permute(0, 2, 1)[~own].any() and not d_ins[~own].any() and not d_outs[~own].any()
    for x, n in enumerate(lengths):                      # a one-word sentence adds no text term: half(x) is empty, so neither its
        if n == 1:                                       # marginal nor its positive s[x, x] is read
            assert not d_ins[x].any() and not d_outs[x].any() and not d_smax[x, x].any()
            # ... while its image stands as a negative for the other texts; as a text it can only enter their image terms at cell 0
            assert d_smax[:, x].any() and not d_smax[x, :, 1:].any()


def test_uniform_lengths_route_to_the_same_value_as_the_existing_modules():
    from cliora_amd import harness as H
    B, L, Rn, _ = VC.LOSS_CASES['B6']
    vg, smax, ins, outs = VC.loss_inputs('B6')
    lens = torch.full((B,), L, dtype=torch.int32)

    class Chart:
        pass
    d = Chart()
    d.inside_s, d.outside_s, d.all_atten_score = ins, outs, torch.stack([smax, smax - 1.0], -1)
    m = H.ContrastiveLoss(margin=0.2, alpha_contr=0.7)
    assert float(m(d, lens)) == pytest.approx(float(m(d)), rel=1e-14)
    assert float(H.VGLoss(0.7)(vg, lens)) == pytest.approx(float(H.VGLoss(0.7)(vg)), rel=1e-14)
    own, half, root = H.triangle_masks(torch.tensor(VC.LOSS_CASES['B6'][3], dtype=torch.int32), L)
    assert torch.equal(own, torch.from_numpy(TC.own_mask(L, VC.LOSS_CASES['B6'][3])))
    for x, n in enumerate(VC.LOSS_CASES['B6'][3]):
        assert sorted(torch.nonzero(half[x]).view(-1).tolist()) == sorted(VC.half_cells(L, n).tolist())
        assert int(root[x]) == TC.root_cell(L, n)


def test_names_and_refusals_on_the_cpu():
    from cliora_amd import _lib, ragged
    from cliora_amd.harness import build_net
    for name in ('cliora_chart_forward_ragged_train_vl', 'cliora_chart_backward_ragged_vl', 'cliora_vg_loss_ragged',
                 'cliora_contrastive_loss_ragged'):
        assert name in _lib.ABI
    net = build_net(16, torch.nn.Embedding(11, 16), obj_feats=True, img_dim=16)
    feats = torch.randn(1, 3, 16)
    with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='gradients enabled'):
        next(ragged.forward_ragged_train(net, [[1, 2, 3]], obj_feats=feats))
    with pytest.raises(NotImplementedError, match='text-only'):          # a CLIORA net without its regions: as before
        next(ragged.forward_ragged_train(net, [[1, 2, 3]]))
    with pytest.raises(ValueError, match='obj_feats holds'):
        next(ragged.forward_ragged_train(net, [[1, 2, 3], [4]], obj_feats=feats))
    text = build_net(16, torch.nn.Embedding(11, 16))
    with pytest.raises(ValueError, match='text-only net'):
        next(ragged.forward_ragged_train(text, [[1, 2, 3]], obj_feats=feats))
    with pytest.raises(ValueError, match='lengths must be'):
        from cliora_amd import harness as H
        H.VGLoss(0.7)(torch.randn(2, 2, 3, 4), torch.tensor([3, 1]))     # int64 lengths
