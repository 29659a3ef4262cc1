"""Mixed-length batches (cliora_amd/ragged.py), the parts that need no GPU: the packer, the padding, the prefix-closure claim on the
CPU oracle, and the new symbol."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import diora_ref as R

import ragged_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lengths(n, seed):
    return np.random.RandomState(seed).randint(1, 41, size=n).tolist()


@pytest.mark.parametrize('max_batch,max_waste', [(64, 0.0), (64, 0.5), (8, 1.0), (64, 4.0), (3, float('inf')), (64, float('inf'))])
def test_pack_partitions_within_bounds(max_batch, max_waste):
    from cliora_amd.ragged import pack, work
    lengths = _lengths(300, 7) + [1, 1, 2, 40, 64]
    packs = pack(lengths, max_batch=max_batch, max_waste=max_waste)
    assert sorted(i for p in packs for i in p) == list(range(len(lengths)))          # every index exactly once
    for p in packs:
        assert 1 <= len(p) <= max_batch
        exact = sum(work(lengths[i]) for i in p)
        padded = len(p) * work(max(lengths[i] for i in p))
        assert padded <= (1.0 + max_waste) * exact if max_waste != float('inf') else True
    assert packs == pack(list(lengths), max_batch=max_batch, max_waste=max_waste)     # deterministic
    if max_waste == float('inf'):
        assert len(packs) == -(-len(lengths) // max_batch)                            # nothing but the size cuts a batch


def test_pack_zero_waste_buckets_by_length_and_work_counts_span_pairs():
    from cliora_amd.ragged import pack, work
    assert [work(n) for n in (1, 2, 3, 4, 20)] == [0, 1, 4, 10, 1330]
    assert all(work(n) == sum((n - lv) * lv for lv in range(1, n)) for n in range(1, 65))
    lengths = [5, 9, 5, 7, 9, 5]
    assert pack(lengths, max_waste=0.0) == [[1, 4], [3], [0, 2, 5]]
    assert pack([], max_waste=0.5) == []
    with pytest.raises(ValueError):
        pack(lengths, max_batch=0)
    with pytest.raises(ValueError):
        pack(lengths, max_waste=-1.0)


def test_pad_batch_shapes():
    from cliora_amd.ragged import pad_batch
    tokens, lengths = pad_batch([[5, 6, 7], [8], [1, 2, 3, 4, 9]], pad_id=0)
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (3, 5)
    assert lengths.dtype == torch.int32 and lengths.tolist() == [3, 1, 5]
    assert tokens.tolist() == [[5, 6, 7, 0, 0], [8, 0, 0, 0, 0], [1, 2, 3, 4, 9]]
    assert pad_batch([[1], [2, 3]], pad_id=-7)[0].tolist() == [[1, -7], [2, 3]]
    with pytest.raises(ValueError):
        pad_batch([[1, 2], []])


def test_ragged_decode_of_padded_oracle_chart_equals_exact_length_cky():
    """Prefix closure on the CPU: the ragged decode, restated in numpy, over the oracle's per-split scores of ONE padded chart gives,
    for every sentence of a mixed set, the spans of the oracle's own CKY over that sentence's exact-length chart."""
    from cliora_amd.ragged import decode_ragged_numpy
    D, lengths, Lmax = 16, [1, 2, 3, 12, 5, 9, 12, 7, 4, 11], 12
    P = R.init_params(D, share=True, seed=31)
    xs = [torch.randn(n, D, generator=torch.Generator().manual_seed(40 + i)) for i, n in enumerate(lengths)]
    pad = R.diora_forward(P, RC.padded(xs, Lmax), outside=False, keep_pairs=True)
    pair_s = {lv: s[..., 0].numpy() for lv, s in pad['pair_s_in'].items()}
    got = decode_ragged_numpy(pair_s, lengths)
    for b, (x, n) in enumerate(zip(xs, lengths)):
        ex = R.diora_forward(P, x[None], outside=False, keep_pairs=True)
        want = R.tree_spans(R.cky_trees(ex['pair_s_in'], 1, n)[0])
        assert got[b] == want, 'sentence %d (length %d)' % (b, n)
        assert len(got[b]) == n - 1 and (n == 1 or got[b][-1] == (0, n - 1))
        assert RC.cky_margin(ex['pair_s_in'], n) > 1e-4         # ... and none of these trees hangs on fp32 rounding
        # the sentence's own cells of the padded chart are the exact-length chart's (to fp32 rounding of differently shaped GEMMs)
        for level in range(1, n):
            np.testing.assert_allclose(pair_s[level][b, :n - level], ex['pair_s_in'][level][0, :, :, 0].numpy(), rtol=0, atol=1e-4)


@pytest.mark.parametrize('D', sorted(RC.CASES))
def test_gpu_cases_have_no_near_tie_in_fp64(D):
    """The yardstick alone meets the GPU test's cap on excused sentences: on the fp64 oracle no cell of any sentence of the seeded
    GPU cases has its two best CKY candidates within the near-tie bound (nor within 1e-6, far above fp32 rounding of a sum of three)."""
    P, xs, lengths = RC.case(D)
    P64 = {k: v.double() for k, v in P.items()}
    assert 1 in lengths and 2 in lengths and RC.LMAX in lengths and max(lengths) == RC.LMAX
    worst = float('inf')
    for x, n in zip(xs, lengths):
        if n < 3:
            continue
        out = R.diora_forward(P64, x[None].double(), outside=False, keep_pairs=True)
        worst = min(worst, RC.cky_margin(out['pair_s_in'], n))
    print('D %d: smallest fp64 CKY margin %.3e' % (D, worst))
    assert worst > max(RC.NEAR_TIE, 1e-6)


def test_ragged_symbol_exported_and_declared():
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert 'int cliora_cky_spans_ragged(' in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'cliora_cky_spans_ragged')
    assert hasattr(lib, 'cliora_phrase_gather')          # the sentence vectors are read through it
