"""The tree sampler (cliora_amd/sample.py, cliora_sample_trees) without a GPU: the numpy Philox against its known-answer vectors, the
fp64 restatement against enumeration of every binary tree (conditional probabilities, log_z, frequencies, log_prob), the draw's
independence of chunking, packing and padding, the host helpers on hand-made examples, and the symbol's declaration, export and
binding.  Yardsticks, pinned cases and bounds: sample_cases.py."""
import ctypes
import math
import os

import numpy as np
import pytest

import posterior_cases as PC
import sample_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_declared_exported_and_bound():
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert 'int cliora_sample_trees(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, const int32_t* ids, int S,' in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'cliora_sample_trees')
    bound = _lib.lib().cliora_sample_trees
    assert len(bound.argtypes) == 13 and bound.restype is ctypes.c_int
    assert bound.argtypes[5] is ctypes.c_uint64 and bound.argtypes[6] is ctypes.c_uint64 and bound.argtypes[7] is ctypes.c_float


def test_philox_known_answers():
    """The three vectors of tests/test_negatives_cpu.py, through the sampler's own numpy Philox."""
    from cliora_amd.sample import philox4x32_10
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = philox4x32_10(*ctr, *key)
        assert tuple(int(x) for x in got) == want


def test_uniform_is_the_negative_samplers_construction():
    """u = (m + 0.5) 2^-53 from the first two words, at counter (level * 256 + pos, sample_lo, sample_hi, sentence id)."""
    from cliora_amd.sample import draw_uniform, philox4x32_10
    seed, sample = 0xa4093822299f31d0, (5 << 32) | 77
    x = philox4x32_10(3 * 256 + 9, 77, 5, 41, seed & 0xffffffff, seed >> 32)
    m = ((int(x[0]) >> 5) << 26) | (int(x[1]) >> 6)
    assert float(draw_uniform(3, 9, sample, 41, seed)) == (m + 0.5) * 2.0 ** -53
    u = draw_uniform(np.arange(4)[:, None], np.arange(4)[None, :], sample, 41, seed)
    assert u.shape == (4, 4) and (u > 0).all() and (u < 1).all() and len(set(u.reshape(-1).tolist())) == 16


@pytest.mark.parametrize('n', range(1, 8))
def test_conditional_probabilities_are_the_enumeration(n):
    """n = 1 .. 7, seeds 0 .. 2, beta in {0, 0.5, 1}, every tree: the product of the restatement's conditional split probabilities is
    exp(beta sum r - log_z) of the enumeration to 1e-12 relative; log_z is the enumerated one; at beta = 0 it is log Catalan(n - 1)."""
    from cliora_amd.sample import inside_numpy, sample_numpy, split_weights
    L = max(n, 2)
    worst = 0.0
    for seed in SC.ENUM_SEEDS:
        pair_s = SC.enum_scores(n, seed)
        for beta in SC.BETAS:
            trees, logp, log_z, _ = SC.enumerate_trees(pair_s, 0, n, beta)
            assert len(trees) == SC.CATALAN[n - 1]
            r, al = inside_numpy(pair_s, 0, n, beta)
            w = {(level, pos): split_weights(r, al, level, pos, beta) for level in range(1, n) for pos in range(n - level)}
            for cell, row in w.items():
                assert abs(row.sum() - 1) <= SC.ENUM_RTOL, (n, seed, beta, cell)
            for t, lp in zip(trees, logp):
                prod = float(np.prod([w[(lv, p)][k] for lv, p, k in t])) if t else 1.0
                err = abs(prod - math.exp(lp)) / math.exp(lp)
                worst = max(worst, err)
                assert err <= SC.ENUM_RTOL, (n, seed, beta, t, err)
            _, _, lz, _ = sample_numpy(pair_s, [n], 1, 0, beta=beta, L=L)
            assert lz[0] == al[n - 1, 0] and abs(lz[0] - log_z) <= SC.ENUM_RTOL * max(1.0, abs(log_z)), (n, seed, beta)
            if beta == 0:
                assert abs(lz[0] - math.log(SC.CATALAN[n - 1])) <= SC.ENUM_RTOL * max(1.0, math.log(SC.CATALAN[n - 1]))
    print('n %d: max relative error of a tree\'s probability = %.3e' % (n, worst))


@pytest.mark.parametrize('score_seed,beta,draw_seed', SC.FREQ_CASES)
def test_frequencies_follow_the_enumerated_probabilities(score_seed, beta, draw_seed):
    """n = 5, 4096 samples: every one of the 14 trees is expected at least 25 times, its frequency lies within 5 binomial standard
    deviations of its enumerated probability, and span_frequencies within the same bound of the enumerated marginals; every sample
    keeps the margin."""
    ok, rarest, margin = SC.frequencies_hold(score_seed, beta, draw_seed)
    print('rarest tree expected %.1f times, smallest margin %.3e' % (rarest, margin))
    assert rarest >= SC.FREQ_MIN_COUNT
    assert ok
    assert margin >= SC.MARGIN


def test_log_prob_is_the_drawn_trees_enumerated_log_probability():
    """n = 2 .. 7, beta in {0, 0.5, 1}, 64 samples: log_prob of every sample is the enumerated log-probability of the tree it drew
    (1e-12 relative), the rows are a tree of the enumeration, (-1, -1) beyond n - 1."""
    from cliora_amd.sample import sample_numpy
    for n in range(2, 8):
        pair_s = SC.enum_scores(n, 1)
        for beta in SC.BETAS:
            trees, logp, log_z, _ = SC.enumerate_trees(pair_s, 0, n, beta)
            index = SC.tree_index(trees)
            spans, log_prob, lz, margin = sample_numpy(pair_s, [n], 64, 99 + n, beta=beta)
            assert spans.shape == (1, 64, n - 1, 2) and spans.dtype == np.int32
            assert margin.min() >= SC.MARGIN
            for s in range(64):
                t = index[SC.span_key(spans[0, s].tolist())]
                assert abs(log_prob[0, s] - logp[t]) <= 1e-12 * max(1.0, abs(logp[t])), (n, beta, s)
            if beta == 0:
                assert np.abs(log_prob + math.log(SC.CATALAN[n - 1])).max() <= 1e-12
    spans, log_prob, lz, margin = sample_numpy(SC.enum_scores(1, 0), [1], 3, 5, L=2)       # one word: no decision, probability 1
    assert spans.shape == (1, 3, 1, 2) and (spans == -1).all() and (log_prob == 0).all() and lz[0] == 0 and np.isinf(margin).all()


def _draw_case():
    L, lengths = PC.RAGGED_L, PC.RAGGED_LENGTHS
    return L, lengths, PC.random_scores(len(lengths), L, SC.DRAW_SCORE_SEED)


def test_chunked_calls_are_one_call():
    """S = 8 is first_sample 0 and 4 with S = 4 each; a 64-bit first_sample reaches the counter's third word."""
    from cliora_amd.sample import sample_numpy
    L, lengths, pair_s = _draw_case()
    for beta in (1.0, 0.5):
        whole = sample_numpy(pair_s, lengths, SC.DRAW_S, SC.DRAW_SEED, beta=beta, L=L)
        assert whole[3].min() >= SC.MARGIN
        lo = sample_numpy(pair_s, lengths, 4, SC.DRAW_SEED, beta=beta, L=L)
        hi = sample_numpy(pair_s, lengths, 4, SC.DRAW_SEED, first_sample=4, beta=beta, L=L)
        assert np.array_equal(whole[0], np.concatenate([lo[0], hi[0]], axis=1))
        assert np.array_equal(whole[1], np.concatenate([lo[1], hi[1]], axis=1)) and np.array_equal(whole[2], lo[2])
    far = sample_numpy(pair_s, lengths, 4, SC.DRAW_SEED, first_sample=1 << 32, L=L)
    assert not np.array_equal(far[0], lo[0]) and far[3].min() >= SC.MARGIN
    other = sample_numpy(pair_s, lengths, 4, SC.DRAW_SEED + 1, L=L)
    assert not np.array_equal(other[0], sample_numpy(pair_s, lengths, 4, SC.DRAW_SEED, L=L)[0])


def test_permuting_sentences_with_their_ids_permutes_the_rows():
    from cliora_amd.sample import sample_numpy
    L, lengths, pair_s = _draw_case()
    ids = [40, 7, 1 << 20, 3, 12]
    base = sample_numpy(pair_s, lengths, SC.DRAW_S, SC.DRAW_SEED, ids=ids, L=L)
    assert base[3].min() >= SC.MARGIN
    perm = [3, 0, 4, 2, 1]
    moved = sample_numpy({lv: s[perm] for lv, s in pair_s.items()}, [lengths[i] for i in perm], SC.DRAW_S, SC.DRAW_SEED,
                         ids=[ids[i] for i in perm], L=L)
    for a, b in zip(base, moved):
        assert np.array_equal(a[perm], b)
    plain = sample_numpy(pair_s, lengths, SC.DRAW_S, SC.DRAW_SEED, L=L)                # ids default to the row
    assert np.array_equal(plain[0], sample_numpy(pair_s, lengths, SC.DRAW_S, SC.DRAW_SEED, ids=range(5), L=L)[0])
    assert not np.array_equal(plain[0][2], base[0][2])


def test_padded_chart_is_each_sentence_alone():
    from cliora_amd.sample import sample_numpy
    L, lengths, pair_s = _draw_case()
    spans, log_prob, log_z, margin = sample_numpy(pair_s, lengths, SC.DRAW_S, SC.DRAW_SEED, L=L)
    for b, n in enumerate(lengths):
        own = {lv: s[b:b + 1, :n - lv] for lv, s in pair_s.items() if lv < n}
        s1, p1, z1, m1 = sample_numpy(own, [n], SC.DRAW_S, SC.DRAW_SEED, ids=[b], L=n)
        assert np.array_equal(spans[b, :, :n - 1], s1[0]) and (spans[b, :, n - 1:] == -1).all()
        assert np.array_equal(log_prob[b], p1[0]) and log_z[b] == z1[0] and np.array_equal(margin[b], m1[0])
    spans, log_prob, log_z, _ = sample_numpy(pair_s, [0, L + 1, 3, 3, 3], 4, 1, L=L)      # lengths outside [1, L]: nothing
    assert (spans[:2] == -1).all() and (log_prob[:2] == 0).all() and (log_z[:2] == 0).all() and (spans[2:, :, :2] >= 0).all()


def test_bad_arguments_are_refused():
    from cliora_amd.sample import MAX_S, sample_numpy
    pair_s = SC.enum_scores(3, 0)
    for S in (0, -1, MAX_S + 1):
        with pytest.raises(ValueError):
            sample_numpy(pair_s, [3], S, 0)
    for beta in (-0.5, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            sample_numpy(pair_s, [3], 2, 0, beta=beta)


def test_span_frequencies_on_a_hand_made_example():
    """Two sentences of 4 words, 4 samples: counts over cells, padding rows ignored, numpy in -> numpy out, a tensor -> a tensor."""
    import torch
    from cliora_amd.posterior import cell_id
    from cliora_amd.sample import span_frequencies
    right = [(2, 3), (1, 3), (0, 3)]
    left = [(0, 1), (0, 2), (0, 3)]
    pad = [(0, 1), (0, 2), (-1, -1)]                                          # a sentence of 3 words in the chart of 4
    spans = np.array([[right, left, left, left], [pad, pad, pad, pad]], dtype=np.int32)
    f = span_frequencies(spans, 4)
    assert isinstance(f, np.ndarray) and f.shape == (2, 10) and f.dtype == np.float32
    want = np.zeros((2, 10), dtype=np.float32)
    want[0, cell_id(4, 3, 0)] = 1.0
    want[0, cell_id(4, 1, 2)] = want[0, cell_id(4, 2, 1)] = 0.25
    want[0, cell_id(4, 1, 0)] = want[0, cell_id(4, 2, 0)] = 0.75
    want[1, cell_id(4, 1, 0)] = want[1, cell_id(4, 2, 0)] = 1.0
    assert np.array_equal(f, want)
    t = span_frequencies(torch.from_numpy(spans), 4)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), want)


def test_expected_f1_on_a_hand_made_example():
    """Sentence 0 (5 words, 4 samples): the gold tree twice, the right-branching one (1 of 3) twice.  Sentence 1: nothing hits."""
    import torch
    from cliora_amd.evaluate import expected_f1, oracle_f1
    from cliora_amd.interchange import SpanF1
    right = [(3, 4), (2, 4), (1, 4), (0, 4)]
    left = [(0, 1), (0, 2), (0, 3), (0, 4)]
    mid = [(0, 1), (2, 3), (2, 4), (0, 4)]
    spans = np.array([[mid, right, right, mid], [left, left, right, mid]], dtype=np.int32)
    gold = [[(0, 1), (2, 3), (2, 4)], [(1, 2), (1, 3)]]
    got = expected_f1(spans, gold)
    f = SpanF1()
    f.add_counts(3, 3, 3)
    f.add_counts(1, 3, 3)
    want0 = (2 * f.sentence[0] + 2 * f.sentence[1]) / 4
    assert abs(got['sentence'][0] - want0) < 1e-12 and got['sentence'][1] == 0.0
    assert abs(got['expected_sent_f1'] - want0 / 2) < 1e-12
    assert expected_f1(torch.from_numpy(spans), gold) == got
    for s in range(4):                                                         # each sample counted as oracle_f1 counts a tree
        one = oracle_f1(spans[:, s:s + 1], np.array([1, 1], dtype=np.int32), gold)
        assert one['best_f1'][0] == f.sentence[0 if s in (0, 3) else 1]
    none = expected_f1(np.full((1, 2, 4, 2), -1, dtype=np.int32), [[(0, 1)]])   # a rejected sentence is skipped
    assert none['sentence'][0] != none['sentence'][0] and none['expected_sent_f1'] != none['expected_sent_f1']
