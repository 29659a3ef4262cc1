"""The k-best decode (cliora_amd/kbest.py, cliora_kbest_spans) without a GPU: the fp32 restatement against enumeration of every binary
tree in fp64, a padded chart against each sentence alone, exact ties against the order of the keys, the best-of-K F1 on a hand-made
example, and the symbols' declaration, export and binding.  Yardsticks and bounds: kbest_cases.py."""
import ctypes
import os

import numpy as np
import pytest

import kbest_cases as KC
import posterior_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_exported_and_bound():
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert 'size_t cliora_kbest_scratch_bytes(const cliora_plan* plan, int K);' in header
    assert 'int cliora_kbest_spans(cliora_plan* plan, void* fwd_workspace, const int32_t* lengths, int K, int32_t* spans_out,' in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'cliora_kbest_spans') and hasattr(raw, 'cliora_kbest_scratch_bytes')
    bound = _lib.lib().cliora_kbest_spans
    assert len(bound.argtypes) == 10 and bound.restype is ctypes.c_int
    query = _lib.fn('cliora_kbest_scratch_bytes')
    assert query.restype is ctypes.c_size_t and len(query.argtypes) == 2


def test_scratch_query_follows_the_lds_limit():
    """0 while 8 C K bytes and the K walk stacks of 4 (L + 1) ints fit 160 KiB, else B tables."""
    from cliora_amd import _lib
    query = _lib.fn('cliora_kbest_scratch_bytes')
    for B, L, K, want in [(64, 40, 8, 0), (64, 40, 16, 0), (64, 64, 8, 0), (64, 64, 9, 0), (64, 64, 10, 1), (3, 65, 4, 0),
                          (3, 128, 2, 0), (3, 128, 3, 1), (3, 128, 8, 1), (3, 128, 16, 1)]:
        plan = _lib.Plan(B, L, 16, forward_only=L > 64)
        Cc = L * (L + 1) // 2
        fits = 8 * Cc * K + 16 * K * (L + 1) <= 160 * 1024
        assert fits == (want == 0), (L, K)
        assert query(plan.handle, K) == (0 if fits else B * Cc * K * 8), (L, K)
    assert query(plan.handle, 0) == 0 and query(plan.handle, 17) == 0        # a bad K has no size; cliora_kbest_spans refuses it


@pytest.mark.parametrize('n', range(1, 9))
def test_kbest_numpy_is_the_enumeration(n):
    """n = 1 .. 8, K in {1, 3, 8, 16}, seeds 0 .. 19: the fp64 totals of consecutive trees among the best K + 1 differ by at least
    1e-4 (no case is excused), and then kbest_numpy returns the same trees in the same order, |score - fp64| <= 1e-5 and count =
    min(K, Catalan(n - 1)).  Measured: kbest_cases.MEASURED_MIN_GAP, MEASURED_MAX_SCORE_ERR."""
    from cliora_amd.kbest import kbest_numpy, tree_count
    L = max(n, 2)
    min_gap, max_err = float('inf'), 0.0
    for seed in KC.ENUM_SEEDS:
        pair_s = KC.enum_scores(n, seed)
        trees, totals = KC.ranked_trees(pair_s, 0, n)
        assert len(trees) == KC.CATALAN[n - 1]
        for K in KC.KS:
            top = totals[:K + 1]
            if len(top) > 1:
                min_gap = min(min_gap, float(np.min(top[:-1] - top[1:])))
                assert np.min(top[:-1] - top[1:]) >= KC.GAP, (n, seed, K)
            spans, scores, count = kbest_numpy(pair_s, [n], K, L)
            want = min(K, KC.CATALAN[n - 1])
            assert spans.shape == (1, K, L - 1, 2) and spans.dtype == np.int32 and scores.dtype == np.float32
            assert count.tolist() == [want] and tree_count(n, K) == want
            for t in range(want):
                assert spans[0, t, :n - 1].tolist() == [list(s) for s in PC.tree_spans(trees[t])], (n, seed, K, t)
                assert (spans[0, t, n - 1:] == -1).all()
            err = float(np.abs(scores[0, :want].astype(np.float64) - totals[:want]).max())
            max_err = max(max_err, err)
            assert err <= KC.SCORE_BOUND, (n, seed, K, err)
            assert (spans[0, want:] == -1).all() and np.isneginf(scores[0, want:]).all()
    print('n %d: smallest fp64 gap among the best K + 1 = %.3e, max |score - fp64| = %.3e' % (n, min_gap, max_err))


def test_rank_zero_is_the_viterbi_decode():
    """Rank 0 of every list is decode_ragged_numpy's tree (first maximum), on scores with exact ties too."""
    from cliora_amd.kbest import kbest_numpy
    from cliora_amd.ragged import decode_ragged_numpy
    for seed in range(4):
        pair_s = PC.random_scores(3, 9, 7000 + seed)
        if seed == 3:
            pair_s = {lv: np.round(s) for lv, s in pair_s.items()}            # integers: ties abound
        want = decode_ragged_numpy(pair_s, [9, 6, 1])
        spans, _, _ = kbest_numpy(pair_s, [9, 6, 1], 5, 9)
        for b, n in enumerate([9, 6, 1]):
            assert spans[b, 0, :n - 1].tolist() == [list(s) for s in want[b]]


def test_padded_chart_is_each_sentence_alone():
    from cliora_amd.kbest import kbest_numpy
    L, lengths = PC.RAGGED_L, PC.RAGGED_LENGTHS
    pair_s = PC.random_scores(len(lengths), L, 4242)
    for K in KC.KS:
        spans, scores, count = kbest_numpy(pair_s, lengths, K, L)
        for b, n in enumerate(lengths):
            own = {lv: s[b:b + 1, :n - lv] for lv, s in pair_s.items() if lv < n}
            s1, v1, c1 = kbest_numpy(own, [n], K, n)
            assert count[b] == c1[0]
            assert np.array_equal(scores[b].view(np.int32), v1[0].view(np.int32))
            assert np.array_equal(spans[b, :, :n - 1], s1[0]) and (spans[b, :, n - 1:] == -1).all()
    spans, scores, count = kbest_numpy(pair_s, [0, L + 1, 3, 3, 3], 4, L)       # lengths outside [1, L]: nothing
    assert count.tolist() == [0, 0, 2, 2, 2] and np.isneginf(scores[:2]).all() and (spans[:2] == -1).all()


@pytest.mark.parametrize('n', [1, 2, 4, 6])
def test_all_zero_scores_give_the_order_of_the_keys(n):
    from cliora_amd.kbest import kbest_numpy
    L = max(n, 2)
    pair_s = {lv: np.zeros((1, L - lv, lv), dtype=np.float32) for lv in range(1, L)}
    for K in KC.KS:
        spans, scores, count = kbest_numpy(pair_s, [n], K, L)
        want = KC.key_order_spans(n, K)
        assert count[0] == len(want) == min(K, KC.CATALAN[n - 1])
        assert (scores[0, :count[0]] == 0).all()
        got = [[tuple(r) for r in spans[0, t, :n - 1].tolist()] for t in range(count[0])]
        assert got == want
        assert len(set(map(tuple, got))) == len(got)                          # no tree twice


def test_oracle_f1_on_a_hand_made_example():
    """Two sentences of 5 words, K 3.  Sentence 0: rank 0 right-branching (1 of 3 gold spans), rank 1 the gold tree, rank 2 padding
    beyond count 2.  Sentence 1: no tree hits; the first is kept."""
    from cliora_amd.evaluate import oracle_f1
    from cliora_amd.interchange import SpanF1
    right = [(3, 4), (2, 4), (1, 4), (0, 4)]
    left = [(0, 1), (0, 2), (0, 3), (0, 4)]
    mid = [(0, 1), (2, 3), (2, 4), (0, 4)]
    pad = [(-1, -1)] * 4
    spans = np.array([[right, mid, pad], [left, right, mid]], dtype=np.int32)
    gold = [[(0, 1), (2, 3), (2, 4)], [(1, 2), (1, 3)]]
    got = oracle_f1(spans, np.array([2, 3], dtype=np.int32), gold)
    assert got['best_rank'] == [1, 0]
    f = SpanF1()
    f.add_counts(3, 3, 3)
    f.add_counts(0, 3, 2)
    assert got['best_f1'] == f.sentence and f.sentence[1] == 0.0 and abs(f.sentence[0] - 1) < 1e-7
    assert got['oracle_corpus_f1'] == f.corpus_f1 == 2 * 0.5 * 0.6 / 1.1 and got['oracle_sent_f1'] == float(np.mean(np.array(f.sentence)))
    g = SpanF1()
    g.add_counts(1, 3, 3)
    g.add_counts(0, 3, 2)
    assert got['corpus_f1'] == g.corpus_f1 == 2 * (1 / 6) * 0.2 / (1 / 6 + 0.2) and got['sent_f1'] == float(np.mean(np.array(g.sentence)))
    import torch
    same = oracle_f1(torch.from_numpy(spans), torch.tensor([2, 3], dtype=torch.int32), gold)
    assert same == got
    none = oracle_f1(spans, np.array([0, 3], dtype=np.int32), gold)             # a rejected sentence is skipped
    assert none['best_rank'] == [-1, 0] and none['oracle_corpus_f1'] == 0.0 and none['corpus_f1'] == 0.0
