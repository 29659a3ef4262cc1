"""cliora_maxsim_scores, cliora_retrieval_ranks and cliora_score_topk on the GPU: the scores against the fp64 restatement at the
project's per-product bound, the masking of padded rows, the bitwise determinism contract, the status words, the ranks and lists
against their restatements, the reference-made fixture's two logits, and the model-level entry points of cliora_amd.retrieval."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import retrieval_cases as RC

pytestmark = pytest.mark.gpu

EPS = {'bf16x3': 2e-5, 'f32': 1e-6}              # tests/test_gpu_phrases.py: the per-product bound of cliora_knn_ip's arithmetic


def _eps(mode, D):
    return EPS[mode] * (max(1.0, (D / 256.0) ** 0.5) if mode == 'f32' else 1.0)


def _cuda(problem):
    q, q_off, w, keys, k_off = problem
    return torch.from_numpy(q).cuda(), q_off, torch.from_numpy(w).cuda(), torch.from_numpy(keys).cuda(), k_off


def _check(problem, mode, what, **kw):
    """The kernel against maxsim_numpy within eps * sum_t |w_t| |Q_t| max_r |O_r|; equal where the restatement is not finite or the
    caption is empty.  -> (S on the host, the largest error / bound)."""
    from cliora_amd.retrieval import maxsim_numpy, maxsim_scores
    q, q_off, w, keys, k_off = problem
    got = maxsim_scores(*_cuda(problem), **kw).cpu().numpy().astype(np.float64)
    want = maxsim_numpy(q, q_off, w, keys, k_off)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    bound = _eps(mode, q.shape[1]) * RC.error_scale(q, q_off, w, keys, k_off)
    err = np.abs(got - want)
    assert np.array_equal(got[fin & (bound == 0)], want[fin & (bound == 0)])              # empty captions: exact zeros
    sel = fin & (bound > 0)
    ratio = float((err[sel] / bound[sel]).max()) if sel.any() else 0.0
    print('%s [%s]: max err %.3e, max err / bound %.3f' % (what, mode, float(err[sel].max()) if sel.any() else 0.0, ratio))
    assert ratio <= 1.0, (what, ratio)
    return got, ratio


# ---- scores against fp64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', RC.WIDTHS)
def test_scores_against_fp64(mfma_mode, D):
    """Every token count and region count of the cases mixed in one call; 40 images: ten 256-row key steps, several key ranges."""
    problem = RC.grouped_problem(D, RC.TOKEN_COUNTS + (17, 1), RC.REGION_COUNTS * 5, seed=D)
    got, _ = _check(problem, mfma_mode, 'D = %d' % D)
    assert got.shape == (10, 40) and (got[0] == 0.0).all()


def test_padded_rows_never_enter_a_maximum_or_a_sum(mfma_mode):
    """Q <= 0 and O >= 0 elementwise: every true score is negative, so a zero-padded key row that entered a maximum shows as 0.0 and
    a padded query row that entered a sum as a wrong sum.  No count is a multiple of 16."""
    problem = RC.grouped_problem(50, (1, 15, 17, 33, 65, 130), (1, 15, 17, 36, 100, 255, 3, 36), seed=3, sign='negative')
    got, _ = _check(problem, mfma_mode, 'all negative')
    assert (got < 0).all()


@pytest.mark.parametrize('weights', ['zero', 'negative', 'mean'])
def test_weights(mfma_mode, weights):
    q, q_off, w, keys, k_off = RC.grouped_problem(33, (5, 16, 40, 17), (36, 7, 64, 20, 36), seed=8)
    rs = np.random.RandomState(2)
    if weights == 'zero':
        w = np.zeros_like(w)
    elif weights == 'negative':
        w = (-np.abs(rs.randn(w.size)) - 0.1).astype(np.float32)
    got, _ = _check((q, q_off, w, keys, k_off), mfma_mode, weights + ' weights')
    if weights == 'zero':
        assert (got == 0.0).all()
    if weights == 'mean':
        assert (np.abs(got) <= 1.0 + 1e-4).all()          # a mean of cosines


# ---- determinism -----------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_determinism_is_bitwise(mfma_mode, monkeypatch):
    from cliora_amd import _lib, retrieval
    tc, rc = (3, 64, 17, 130, 1, 16, 65, 15, 40, 22), RC.REGION_COUNTS * 3
    q, q_off, w, keys, k_off = _cuda(RC.grouped_problem(100, tc, rc, seed=21))
    S = retrieval.maxsim_scores(q, q_off, w, keys, k_off)
    assert torch.equal(_bits(S), _bits(retrieval.maxsim_scores(q, q_off, w, keys, k_off)))           # two runs
    # a caption alone, and against one image alone
    n = 3
    alone = retrieval.maxsim_scores(q[q_off[n]:q_off[n + 1]], [0, tc[n]], w[q_off[n]:q_off[n + 1]], keys, k_off)
    assert torch.equal(_bits(alone[0]), _bits(S[n]))
    m = 12
    one = retrieval.maxsim_scores(q, q_off, w, keys[k_off[m]:k_off[m + 1]], [0, rc[m]])
    assert torch.equal(_bits(one[:, 0]), _bits(S[:, m]))
    # a workspace budget that forces at least three chunks of captions
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    whole = _lib.fn('cliora_maxsim_workspace_bytes')(len(tc), q.shape[0], len(rc), keys.shape[0], 100)
    keys_only = _lib.fn('cliora_maxsim_workspace_bytes')(0, 0, len(rc), keys.shape[0], 100)
    chunked = retrieval.maxsim_scores(q, q_off, w, keys, k_off, max_workspace_mb=(whole - keys_only) / 3.5 / 2 ** 20)
    monkeypatch.undo()
    assert calls.count('cliora_maxsim_scores') >= 3
    assert torch.equal(_bits(chunked), _bits(S))
    # the same through device offsets
    dev = retrieval.maxsim_scores(q, torch.tensor(q_off, dtype=torch.int32).cuda(), w, keys, torch.tensor(k_off).cuda())
    assert torch.equal(_bits(dev), _bits(S))
    # images permuted: the columns permute
    perm = np.random.RandomState(0).permutation(len(rc))
    pk = torch.cat([keys[k_off[m]:k_off[m + 1]] for m in perm], 0)
    poff = np.concatenate([[0], np.cumsum([rc[m] for m in perm])]).tolist()
    P = retrieval.maxsim_scores(q, q_off, w, pk, poff)
    assert torch.equal(_bits(P), _bits(S[:, torch.from_numpy(perm).cuda()]))


def test_a_nan_stays_in_its_row_or_column(mfma_mode):
    from cliora_amd.retrieval import maxsim_scores
    tc, rc = (3, 64, 17, 20), (36, 1, 100, 17, 36)
    q, q_off, w, keys, k_off = _cuda(RC.grouped_problem(50, tc, rc, seed=4))
    S = maxsim_scores(q, q_off, w, keys, k_off)
    q2 = q.clone()
    q2[q_off[2] + 16, 7] = float('nan')                       # the last token of caption 2 (its second tile)
    Sq = maxsim_scores(q2, q_off, w, keys, k_off)
    assert bool(torch.isnan(Sq[2]).all())
    keep = [0, 1, 3]
    assert torch.equal(_bits(Sq[keep]), _bits(S[keep]))
    k2 = keys.clone()
    k2[k_off[2] + 99, 0] = float('nan')                       # the last region of image 2
    Sk = maxsim_scores(q, q_off, w, k2, k_off)
    assert bool(torch.isnan(Sk[:, 2]).all())
    keep = [0, 1, 3, 4]
    assert torch.equal(_bits(Sk[:, keep]), _bits(S[:, keep]))


# ---- status ------------------------------------------------------------------------------------------------------------------------------
def test_status_words():
    from cliora_amd import _lib, retrieval
    q, q_off, w, keys, k_off = _cuda(RC.grouped_problem(20, (4, 9, 2), (257, 5, 256), seed=6))
    with pytest.raises(_lib.ChartLibError, match='1 image'):
        retrieval.maxsim_scores(q, q_off, w, keys, k_off)
    S, status = retrieval._maxsim(q, q_off, w, keys, k_off, 256)
    assert status.tolist() == [1, 0]
    S = S.cpu()
    assert bool(torch.isnan(S[:, 0]).all()) and bool(torch.isfinite(S[:, 1:]).all())
    bad_q = [0, 4, 2, 15]                                     # caption 1 decreases; caption 2 then holds rows 2..15
    with pytest.raises(_lib.ChartLibError, match='1 group'):
        retrieval.maxsim_scores(q, bad_q, w, keys[257:], [0, 5, 261])
    S, status = retrieval._maxsim(q, bad_q, w, keys[257:], [0, 5, 300], 256)     # and image 1 ends outside the rows
    assert status.tolist() == [0, 2]
    S = S.cpu()
    assert bool(torch.isnan(S[1]).all()) and bool(torch.isnan(S[:, 1]).all()) and bool(torch.isfinite(S[[0, 2], 0]).all())


# ---- ranks and lists -----------------------------------------------------------------------------------------------------------------------
def _rank_cases():
    cases = dict(RC.rank_cases())
    cases['duplicated_columns'] = RC.duplicated_columns_case()
    return cases


@pytest.mark.parametrize('name', sorted(_rank_cases()))
def test_ranks_and_topk_against_numpy(name):
    from cliora_amd.retrieval import retrieval_ranks, retrieval_ranks_numpy, score_topk, score_topk_numpy
    S, io = _rank_cases()[name]
    S32 = S.astype(np.float32)
    St = torch.from_numpy(S32).cuda()
    t2i, i2t, status = retrieval_ranks(St, torch.from_numpy(io))
    want = retrieval_ranks_numpy(S32, io)
    assert t2i.tolist() == want[0].tolist() and i2t.tolist() == want[1].tolist() and int(status) == want[2]
    for k in (1, 3, 64, 128):
        for tr in (False, True):
            D, I = score_topk(St, k, transpose=tr)
            Dw, Iw = score_topk_numpy(S32.T if tr else S32, k)
            assert I.tolist() == Iw.tolist(), (k, tr)
            assert np.array_equal(D.cpu().numpy().astype(np.float64), Dw, equal_nan=True), (k, tr)


def test_ranks_on_a_strided_score_matrix():
    from cliora_amd.retrieval import retrieval_ranks, retrieval_ranks_numpy
    S, io = RC.duplicated_columns_case()
    big = torch.zeros(37, 40).cuda()
    big[:, 3:26] = torch.from_numpy(S.astype(np.float32)).cuda()
    t2i, i2t, _ = retrieval_ranks(big[:, 3:26], torch.from_numpy(io))
    want = retrieval_ranks_numpy(S.astype(np.float32), io)
    assert t2i.tolist() == want[0].tolist() and i2t.tolist() == want[1].tolist()


# ---- the reference's logits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['train', 'eval'])
def test_fixture_logits_through_the_kernel(mfma_mode, which):
    from cliora_amd.retrieval import maxsim_scores, retrieval_ranks, retrieval_ranks_numpy
    q, q_off, w, keys, k_off, want = RC.fixture_problem(load_golden('cliora_small.npz'), which)
    problem = (q.astype(np.float32), q_off, w.astype(np.float32), keys.astype(np.float32), k_off)
    S = maxsim_scores(*_cuda(problem))
    bound = _eps(mfma_mode, q.shape[1]) * RC.error_scale(*problem) + 1e-6          # + the fixture's own fp32 scores against fp64
    err = np.abs(S.cpu().numpy().astype(np.float64) - want)
    print('%s [%s]: max err / bound %.3f' % (which, mfma_mode, float((err / bound).max())))
    assert (err <= bound).all()
    t2i, i2t, _ = retrieval_ranks(S, torch.arange(4))
    wr = retrieval_ranks_numpy(want, np.arange(4))
    assert t2i.tolist() == wr[0].tolist() and i2t.tolist() == wr[1].tolist()


# ---- model level ---------------------------------------------------------------------------------------------------------------------------
def _net(D=48, V=200, E=32, IMG=32, seed=13):
    from cliora_amd import harness as H
    torch.manual_seed(seed)
    net = H.build_net(D, torch.nn.Embedding(V, E), obj_feats=True, img_dim=IMG, k_neg=10, vg_loss=True, use_contr=True)
    g = torch.Generator().manual_seed(seed + 1)
    for p in net.img_encoder.parameters():                    # zero-initialised like the reference: give the regions something to say
        p.data.copy_(0.3 * torch.randn(p.shape, generator=g))
    return net.cuda().eval()


def _logit(vg, L):
    return (vg.double().max(-1).values.sum(-1) / L).cpu().numpy()


def test_model_queries_reproduce_the_module_logits(mfma_mode):
    from cliora_amd import retrieval
    B, L, R, IMG, V = 5, 7, 36, 32, 200
    net = _net()
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(0, V, (B, L), generator=g)
    obj = torch.relu(torch.randn(B, R, IMG, generator=g))
    # eval mode: [inside_h + outside_h | unit(x_word)] against [obj_span | obj_word]
    q, q_off, w = retrieval.caption_queries(net, tokens, mode='eval', obj_feats=obj)
    keys, k_off = retrieval.image_keys(net, obj, mode='eval')
    S = retrieval.maxsim_scores(q, q_off, w, keys, k_off).cpu().numpy().astype(np.float64)
    with torch.no_grad():
        net.eval()
        net(tokens.cuda(), obj.cuda(), None, compute_loss=False)
        want = _logit(net.diora.vg_atten_score, L)
    problem = (q.cpu().numpy(), q_off, w.cpu().numpy(), keys.cpu().numpy(), k_off)
    bound = _eps(mfma_mode, q.shape[1]) * RC.error_scale(*problem)
    print('eval [%s]: max err / bound %.3f' % (mfma_mode, float((np.abs(S - want) / bound).max())))
    assert (np.abs(S - want) <= bound).all()
    # training mode: raw x_word against obj_word
    q, q_off, w = retrieval.caption_queries(net, tokens, mode='word', normalize=False)
    keys, k_off = retrieval.image_keys(net, obj, mode='word')
    S = retrieval.maxsim_scores(q, q_off, w, keys, k_off).cpu().numpy().astype(np.float64)
    with torch.no_grad():
        net.train()
        net(tokens.cuda(), obj.cuda(), None, compute_loss=False)
        want = _logit(net.diora.vg_atten_score, L)
        net.eval()
    problem = (q.cpu().numpy(), q_off, w.cpu().numpy(), keys.cpu().numpy(), k_off)
    bound = _eps(mfma_mode, q.shape[1]) * RC.error_scale(*problem)
    print('train [%s]: max err / bound %.3f' % (mfma_mode, float((np.abs(S - want) / bound).max())))
    assert (np.abs(S - want) <= bound).all()


def test_eval_queries_of_mixed_lengths_match_the_equal_length_ones():
    """A caption's eval-mode rows are the same through the uniform forward and through ragged.forward_ragged, mixed with captions of
    other lengths, up to the padded chart's own difference: its sums run in another order (DESIGN.md section 13 measured 2.3e-5 on
    scores), here on rows that are sums of two unit vectors after at most five levels.  2e-4 is ten of the per-product bounds; a row
    taken from the wrong cell or sentence differs by the order of 1."""
    from cliora_amd import retrieval
    net = _net()
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(0, 200, (3, 6), generator=g)
    obj = torch.relu(torch.randn(5, 36, 32, generator=g))
    q0, off0, _ = retrieval.caption_queries(net, tokens, mode='eval', obj_feats=obj[:3])
    mixed = [tokens[0].tolist(), [4, 9, 2], tokens[1].tolist(), [7, 7, 1, 3, 5, 6, 8, 2, 9], tokens[2].tolist()]
    q1, off1, w1 = retrieval.caption_queries(net, mixed, mode='eval', obj_feats=obj[[0, 3, 1, 4, 2]])
    assert off1 == [0, 6, 9, 15, 24, 30] and abs(float(w1[7]) - 1 / 3) < 1e-7
    for a, b in ((0, 0), (1, 2), (2, 4)):
        d = (q0[off0[a]:off0[a + 1]] - q1[off1[b]:off1[b + 1]]).abs().max()
        assert float(d) <= 2e-4, float(d)


def test_span_queries_cover_each_sentences_own_triangle():
    from cliora_amd import retrieval
    from cliora_amd.posterior import cell_id, span_posteriors
    net = _net()
    g = torch.Generator().manual_seed(6)
    tokens = torch.randint(0, 200, (3, 5), generator=g)
    obj = torch.relu(torch.randn(3, 36, 32, generator=g))
    with torch.no_grad():
        net(tokens.cuda(), obj.cuda(), None, compute_loss=False)
    d = net.diora
    q, off, w = retrieval.span_queries(d)
    assert off == [0, 15, 30, 45] and q.shape == (45, 48)
    c = cell_id(5, 2, 1)                                       # sentence 1, level 2, position 1: row 15 + 5 + 4 + 1
    assert torch.equal(q[15 + 10], d.inside_h[1, c] + d.outside_h[1, c])
    assert torch.equal(w, span_posteriors(d).marginals.reshape(-1))
    keys, k_off = retrieval.image_keys(net, obj, mode='eval')
    S = retrieval.maxsim_scores(q, off, w, keys[:, :48], k_off)            # spans against obj_span
    assert S.shape == (3, 3) and bool(torch.isfinite(S).all())


def test_retrieve_against_a_per_pair_loop():
    """12 captions of mixed lengths over 5 images of mixed region counts: ranks and R@K equal to those of a per-pair fp64 loop whose
    smallest score gap is asserted to be above ten times the kernel's tolerance, so a flipped rank cannot hide as a tie."""
    from cliora_amd import retrieval
    net = _net()
    rs = np.random.RandomState(3)              # seeds chosen for the gap asserted below (17 times the tolerance)
    lens = [3, 9, 17, 5, 1, 12, 8, 20, 6, 4, 33, 7]
    caps = [rs.randint(0, 200, size=n).tolist() for n in lens]
    counts = [36, 5, 17, 64, 20]
    g = torch.Generator().manual_seed(103)
    images = [torch.relu(torch.randn(r, 32, generator=g)) for r in counts]
    image_of = [0, 0, 1, 1, 1, 2, 3, 3, 3, 4, 4, 2]
    out = retrieval.retrieve(net, caps, images, image_of, ks=(1, 2, 5), topk=3)
    want = np.zeros((12, 5))
    scale = np.zeros((12, 5))
    with torch.no_grad():
        for n, c in enumerate(caps):
            xw = net.embed(torch.tensor([c]).cuda())[1][0].double()
            u = xw / xw.norm(dim=-1, keepdim=True).clamp(min=1e-8)
            for m, f in enumerate(images):
                ow = net.img_encoder(f[None].cuda())[1][0].double()
                want[n, m] = float((u @ ow.T).max(-1).values.mean())
                scale[n, m] = float(u.norm(dim=-1).mean() * ow.norm(dim=-1).max())
    tol = float((2e-5 * scale).max())
    got = out['scores'].cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() <= tol
    gaps = [np.diff(np.sort(want, axis=1), axis=1).min(), np.diff(np.sort(want, axis=0), axis=0).min()]
    print('tolerance %.3e, smallest gap in a row %.3e, in a column %.3e' % (tol, gaps[0], gaps[1]))
    assert min(gaps) > 10 * tol
    t2i, i2t, skipped = retrieval.retrieval_ranks_numpy(want, image_of)
    assert out['t2i']['ranks'].tolist() == t2i.tolist() and out['i2t']['ranks'].tolist() == i2t.tolist()
    for k in (1, 2, 5):
        assert out['t2i']['r_at_k'][k] == float((t2i < k).mean()) and out['i2t']['r_at_k'][k] == float((i2t < k).mean())
    assert out['t2i']['median_rank'] == float(np.median(t2i + 1)) and out['i2t']['mean_rank'] == float((i2t + 1).mean())
    assert out['t2i']['skipped'] == 0 and out['i2t']['skipped'] == 0
    D, I = retrieval.score_topk_numpy(want, 3)
    assert out['topk']['t2i'][1].tolist() == I.tolist()
    assert out['topk']['i2t'][1].tolist() == retrieval.score_topk_numpy(want.T, 3)[1].tolist()
    assert np.abs(out['topk']['t2i'][0] - D).max() <= tol


def test_retrieve_in_eval_mode_pairs_each_caption_with_its_image():
    """mode='eval' runs every caption's chart with images[image_of[n]]: the scores are those of caption_queries(mode='eval') on the
    paired features against image_keys(mode='eval'), and the ranks those of that matrix."""
    from cliora_amd import retrieval
    net = _net()
    g = torch.Generator().manual_seed(12)
    caps = [torch.randint(0, 200, (n,), generator=g).tolist() for n in (5, 3, 5, 7)]
    images = torch.relu(torch.randn(3, 36, 32, generator=g))
    image_of = [0, 1, 2, 1]
    out = retrieval.retrieve(net, caps, images, image_of, ks=(1,), mode='eval')
    q, q_off, w = retrieval.caption_queries(net, caps, mode='eval', obj_feats=images[image_of])
    keys, k_off = retrieval.image_keys(net, images, mode='eval')
    assert q.shape == (20, 96) and keys.shape == (108, 96)
    S = retrieval.maxsim_scores(q, q_off, w, keys, k_off)
    assert torch.equal(_bits(out['scores']), _bits(S))
    t2i, i2t, _ = retrieval.retrieval_ranks_numpy(S.cpu().numpy(), image_of)
    assert out['t2i']['ranks'].tolist() == t2i.tolist() and out['i2t']['ranks'].tolist() == i2t.tolist()
