"""The outside pass of a right-padded chart made each sentence's own by masking (cliora_chart_forward_ragged),
checked without a GPU: the method on the fp64 oracle, the pair-validity claim it rests on by brute force, and the built library's
exports."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ragged_cases as RC
import ragged_outside_cases as ROC
from oracle import chart_layout as CL
from oracle import diora_ref as R


def _check(P, xs, lengths, Lmax, normalize, share, vl=None):
    """masked_outside on the padded batch == the oracle's outside pass of each sentence at its exact length, fp64, 1e-12 relative on
    every cell of every triangle; every value of the padded charts finite."""
    P64 = ROC.cast(P, torch.float64)
    xp = ROC.padded(xs, Lmax).double()
    kw = {}
    if vl is not None:      # regions per sentence; the words' own projections play no part in the charts
        kw = dict(x_word=xp, obj_span=torch.stack([v[1] for v in vl]).double(), obj_word=torch.stack([v[2] for v in vl]).double())
    with torch.no_grad():
        pad = R.diora_forward(P64, xp, outside=False, normalize=normalize, share=share, **kw)
        oh, os_ = ROC.masked_outside(P64, pad, lengths, normalize, share)
    assert bool(torch.isfinite(oh).all()) and bool(torch.isfinite(os_).all())
    worst = 0.0
    for b, n in enumerate(lengths):
        want = ROC.exact(P, xs[b], normalize, share, vl=vl[b] if vl is not None else None)
        own = torch.from_numpy(ROC.own_cells(Lmax, n))
        for got, w in ((pad['inside_h'][b, own], want['inside_h'][0]), (oh[b, own], want['outside_h'][0]), (os_[b, own], want['outside_s'][0])):
            err = float(((got - w).abs() / w.abs().clamp(min=1.0)).max())
            worst = max(worst, err)
            assert err <= 1e-12, (b, n, err)
    return worst


@pytest.mark.parametrize('normalize', ['unit', 'none'])
def test_masked_outside_pass_is_the_exact_length_outside_pass(normalize):
    P, xs, lengths = RC.case(50)
    assert {1, 2, 40} <= set(lengths)
    if normalize == 'none':          # unnormalised N(0, 1) charts leave every float range within a few levels: small weights, short sentences
        P, xs, lengths = ROC.small_case(16, [9, 1, 2, 3, 5, 7, 9, 4], seed=77, scale=0.25)
        print('worst relative error %.3e' % _check(P, xs, lengths, 9, normalize, True))
    else:
        print('worst relative error %.3e' % _check(P, xs, lengths, RC.LMAX, normalize, True))


@pytest.mark.parametrize('normalize,share', [('unit', True), ('unit', False), ('none', True)])
def test_masked_outside_pass_with_regions(normalize, share):
    lengths = [7, 1, 2, 4, 7, 3]
    P, xs, _ = ROC.small_case(16, lengths, seed=31, share=share, scale=0.25 if normalize == 'none' else 1.0)
    _check(P, xs, lengths, 7, normalize, share, vl=ROC.vl_inputs(16, lengths, 5, seed=31))


def test_parent_leaves_the_triangle_iff_the_sibling_does():
    """For every L in 2..40, level, pair and length n: for a target inside the triangle of n, parent outside == sibling outside; and
    every such target other than the root (n - 1, 0) keeps a pair inside."""
    for L in range(2, 41):
        off = CL.level_offsets(L)
        lvl = np.zeros(CL.n_cells(L), dtype=np.int64)
        pos = np.zeros(CL.n_cells(L), dtype=np.int64)
        for lv in range(L):
            lvl[off[lv]:off[lv] + L - lv] = lv
            pos[off[lv]:off[lv] + L - lv] = np.arange(L - lv)
        end = lvl + pos                                  # last word of the cell's span
        for level in range(L - 1):
            Lc = L - level
            pidx, sidx = CL.outside_pairs(L, level)
            j = np.tile(np.arange(Lc), Lc - 1)
            for n in range(1, L + 1):
                inside_target = j + level < n
                par_out, sib_out = end[pidx] >= n, end[sidx] >= n
                assert np.array_equal(par_out[inside_target], sib_out[inside_target]), (L, level, n)
                valid = (~sib_out & inside_target).reshape(Lc - 1, Lc).sum(0)          # valid pairs per target position
                for p in range(max(n - level, 0)):
                    if (level, p) != (n - 1, 0):
                        assert valid[p] >= 1, (L, level, n, p)
                    else:
                        assert valid[p] == 0


def test_library_exports_the_ragged_entries():
    from cliora_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'build the library first (python -m cliora_amd.build)'
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('cliora_chart_forward_ragged', 'cliora_ground_eval_ragged'):
        assert hasattr(raw, name), name
    lib = _lib.lib()
    assert len(lib.cliora_chart_forward_ragged.argtypes) == 17 and lib.cliora_chart_forward_ragged.argtypes[14] is ctypes.c_uint64
    assert len(lib.cliora_ground_eval_ragged.argtypes) == 23
    assert lib.cliora_chart_forward_ragged.restype is ctypes.c_int and lib.cliora_ground_eval_ragged.restype is ctypes.c_int


def test_end_to_end_examples_have_no_decisive_near_tie_on_the_oracle():
    """The GPU end-to-end test demands that evaluate_ragged selects, phrase by phrase, what evaluate selects at the exact length, and
    excuses nothing: here the fp64 oracle shows that on its seeded examples no phrase has the two best entries of a decisive row
    within the measured padded-vs-exact difference, so the demand cannot hinge on rounding."""
    net = ROC.vl_net().eval()
    near = 0
    for ex in ROC.examples(ROC.E2E_LENGTHS):
        att = ROC.oracle_atten(net, ex)
        assert att.shape == (len(ex['sentence']), 36)
        near += len(ROC.near_tie_phrases(att, [(s, e) for s, e, _ in ex['VG_GT'][0].values()]))
    assert near == 0


def test_root_level_mask():
    from cliora_amd import ragged
    assert ragged.root_level_mask([1, 3, 3, 40]) == (1 << 0) | (1 << 2) | (1 << 39)
    assert ragged.root_level_mask([0, 65]) == 0
