"""Negative sampling on the GPU (cliora_amd.sampling; include/cliora_chart.h: cliora_token_counts, cliora_neg_sample): the counts
against the reference's calculate_freq_dist and np.bincount, the race keys and ids against the numpy restatement of
tests/test_negatives_cpu.py, the sampler's contract, its statistics against the reference's sampler (tests/golden/negatives.npz),
and Trainer.step drawing its own negatives."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_negatives_cpu import chi2_ok, draw_stats, pair_probs, race_draws, race_keys, two_sample_ok, weights

pytestmark = pytest.mark.gpu


def _sampler(freq, seed, stream_id=0, power=0.75):
    from cliora_amd.sampling import NegativeSampler
    return NegativeSampler(torch.as_tensor(np.asarray(freq, np.float32)).cuda(), power, seed=seed, stream_id=stream_id)


def _zipf_freq(V, seed, zeros=0):
    rs = np.random.RandomState(seed)
    f = np.floor(1e6 / np.arange(1, V + 1) ** 1.1)[rs.permutation(V)].astype(np.float32)
    if zeros:
        f[rs.choice(V, zeros, replace=False)] = 0
    return f


# ---- counts -----------------------------------------------------------------------------------------------------------------------
def test_counts_are_the_reference_freq_dist():
    from cliora_amd.sampling import calculate_freq_dist
    g = load_golden('negatives.npz')
    ids = g['corpus_ids']
    sents = np.split(ids, np.cumsum(g['corpus_lens'])[:-1])
    got = calculate_freq_dist([list(s) for s in sents], 300, 'cuda')
    assert got.dtype == torch.float32 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), g['freq300'].view(np.uint32))
    got_t = calculate_freq_dist(torch.from_numpy(ids.astype(np.int64)), 300, 'cuda')
    assert torch.equal(got_t, got)


@pytest.mark.parametrize('V', [400000, 9000])
def test_counts_match_bincount_on_2m_tokens(V):
    from cliora_amd.sampling import calculate_freq_dist
    rs = np.random.RandomState(V)
    ids = np.concatenate([rs.randint(0, V, 1500000), rs.randint(0, 50, 500000)])          # a few very frequent ids too
    got = calculate_freq_dist(torch.from_numpy(ids).cuda(), V, 'cuda').cpu().numpy()
    np.testing.assert_array_equal(got, np.bincount(ids, minlength=V).astype(np.float32))


@pytest.mark.parametrize('bad', [-1, 300])
def test_counts_raise_on_out_of_range_ids(bad):
    from cliora_amd.sampling import calculate_freq_dist
    with pytest.raises(ValueError, match='outside'):
        calculate_freq_dist([[1, 2, 3], [4, bad]], 300, 'cuda')


# ---- distribution vector --------------------------------------------------------------------------------------------------------
def test_dist_is_the_reference_dist():
    g = load_golden('negatives.npz')
    s = _sampler(g['freq300'], 1)
    np.testing.assert_allclose(s.dist.cpu().numpy(), g['dist300'], rtol=1e-5)


# ---- exactness against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V,k,S', [(8, 2, 4), (64, 10, 1000), (300, 300, 2), (20000, 100, 8), (400000, 100, 2)])
def test_keys_and_ids_match_the_restatement(V, k, S):
    freq = _zipf_freq(V, V, zeros=0)
    seed, stream_id, offset = 0x1234_5678_9abc_def0 + V, 3, 2 ** 32 - 2          # draw numbers cross a 32-bit boundary
    s = _sampler(freq, seed, stream_id)
    w = s.weights.cpu().numpy()
    ids, E = s.sample_with_keys(S, k, offset=offset)
    ids, E = ids.cpu().numpy(), E.cpu().numpy()
    rid, rE = race_draws(w, k, seed, stream_id, offset + np.arange(S))
    ulp = np.spacing(np.abs(rE))
    assert (np.abs(E - rE) <= 4 * ulp).all()
    Efull = race_keys(w, seed, stream_id, offset + np.arange(S))
    for r in range(S):
        diff = np.nonzero(ids[r] != rid[r])[0]
        for t in diff:                          # only swaps of neighbours whose restated keys are within 1e-14 of each other
            a, b = Efull[r, ids[r, t]], Efull[r, rid[r, t]]
            assert abs(a - b) <= 1e-14 * max(abs(a), abs(b)), (r, t)


# ---- contract -------------------------------------------------------------------------------------------------------------------
def test_rows_distinct_in_range_and_zero_weights_never_drawn():
    V = 5000
    freq = _zipf_freq(V, 7, zeros=1000)
    s = _sampler(freq, 11, power=0.75)
    s.weights[torch.from_numpy(np.nonzero(freq == 0)[0]).cuda()] = 0.0         # eps / V off: the zero counts get weight 0
    s.n_positive = int((s.weights > 0).sum())
    ids = s.sample_many(2000, 100).cpu().numpy()
    assert ids.min() >= 0 and ids.max() < V
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    assert not np.isin(ids, np.nonzero(freq == 0)[0]).any()
    # k of all the positive weights: a permutation of them
    small = _sampler(np.array([3, 0, 1, 2, 0, 9], np.float32), 5)
    small.weights[torch.tensor([1, 4]).cuda()] = 0.0
    small.n_positive = 4
    got = small.sample_many(50, 4).cpu().numpy()
    assert (np.sort(got, axis=1) == np.array([0, 2, 3, 5])).all()
    with pytest.raises(ValueError, match='Fewer non-zero entries in p than size'):
        small.sample(5)


def test_same_seed_same_draws_and_batching_does_not_matter():
    freq = _zipf_freq(20000, 3)
    a, b = _sampler(freq, 99), _sampler(freq, 99)
    x = a.sample_many(1000, 100)
    y = torch.cat([b.sample_many(100, 100) for _ in range(10)])
    assert torch.equal(x, y)
    a.set_seed(99)
    assert torch.equal(a.sample(100), x[0])
    assert torch.equal(a.sample(100), x[1])
    c = _sampler(freq, 99, stream_id=1)
    z = c.sample_many(1000, 100)
    assert (z != x).any(dim=1).float().mean() > 0.99
    d = _sampler(freq, 100)
    assert (d.sample_many(1000, 100) != x).any(dim=1).float().mean() > 0.99


# ---- statistics against the reference ------------------------------------------------------------------------------------------
def test_statistics_match_the_reference_sampler():
    g = load_golden('negatives.npz')
    n = int(g['n_draws'])
    s = _sampler(g['freq64'], 20261016)
    w = weights(g['freq64'])
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    big = s.sample_many(200000, 10).cpu().numpy()
    incl, first = draw_stats(big, 64)
    ok, chi2, df = chi2_ok(first, 200000 * p)
    assert ok, (chi2, df)
    incl_n, first_n = draw_stats(big[:n], 64)
    assert two_sample_ok(incl_n, g['incl64'], n).all()
    assert two_sample_ok(first_n, g['first64'], n).all()
    s8 = _sampler(g['freq8'], 77)
    ids8 = s8.sample_many(n, 2).cpu().numpy()
    pairs = np.zeros((8, 8), np.int64)
    np.add.at(pairs, (ids8[:, 0], ids8[:, 1]), 1)
    ok, chi2, df = chi2_ok(pairs, n * pair_probs(weights(g['freq8'])))
    assert ok, (chi2, df)


# ---- trainer --------------------------------------------------------------------------------------------------------------------
def test_trainer_draws_negatives_when_the_batch_has_none():
    from cliora_amd import harness as H
    from test_gpu_harness import _build
    g = load_golden('net_diora.npz')
    V, K = g['meta']['V'], g['meta']['K']
    freq = _zipf_freq(V, 5)
    results = []
    for explicit in (False, True):
        torch.manual_seed(0)
        net = _build(g, False)
        net.train = lambda mode=True, net=net: torch.nn.Module.train(net, False)          # dropout off, as the fixture
        sampler = _sampler(freq, 4242)
        bm = dict(sentences=torch.from_numpy(g['sentences']).cuda())
        if explicit:
            bm['neg_samples'] = _sampler(freq, 4242).sample(K)
            tr = H.Trainer(net, lr=g['meta']['lr'])
        else:
            tr = H.Trainer(net, lr=g['meta']['lr'], negative_sampler=sampler, k_neg=K)
        loss = tr.step(bm, train=True)['total_loss']
        torch.cuda.synchronize()
        results.append((loss, {k: p.detach().clone() for k, p in net.named_parameters()}, sampler.draws))
    (la, pa, da), (lb, pb, db) = results
    assert np.float32(la).tobytes() == np.float32(lb).tobytes()
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    assert da == 1 and db == 0
