"""The whole-vocabulary loss without a device: the fp64 restatement (cliora_amd.vocab.vocab_nll_numpy) against torch's fp64
cross-entropy and a stable argsort, its edge semantics, the link to the reference's sampled objective, the module's torch fallback
(harness.ReconstructionSoftmaxLoss(full_vocab=True)), the word-prediction metrics, and the workspace formula and refusals of the C
entries through the built library."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocab_cases as VC

EINVAL, ENOMEM = -1, -3
ONE = C.c_void_p(16)              # "some pointer": never dereferenced, every call is refused first
NULL = C.c_void_p(0)


def _argsort_rank(s_row, tok):
    """The place of `tok` in a stable sort by descending score, NaN last: the rank rule stated by sorting."""
    key = np.where(np.isnan(s_row), -np.inf, s_row)
    nan_last = np.isnan(s_row).astype(np.int64)
    order = np.lexsort((np.arange(len(s_row)), -key, nan_last))          # last key first: numbers before NaN, then descending, then index
    return int(np.nonzero(order == tok)[0][0])


@pytest.mark.parametrize('T,V,E', VC.CASES)
def test_numpy_restatement_against_torch_fp64(T, V, E):
    from cliora_amd.vocab import vocab_nll_numpy
    Q, K, tok = VC.make_case(T, V, E)
    w = np.random.RandomState(3).rand(T)
    r = vocab_nll_numpy(Q, K, tok, w, want_grad=True, g=0.7)
    q = torch.from_numpy(Q).double().requires_grad_(True)
    k = torch.from_numpy(K).double().requires_grad_(True)
    logits = q @ k.t()
    nll = F.cross_entropy(logits, torch.from_numpy(tok), reduction='none')
    assert np.abs(r['nll'] - nll.detach().numpy()).max() <= 1e-11
    assert np.abs(r['lse'] - torch.logsumexp(logits, 1).detach().numpy()).max() <= 1e-11
    assert np.abs(r['tgt'] - logits.detach().numpy()[np.arange(T), tok]).max() <= 1e-11
    loss = (torch.from_numpy(w) * nll).sum()
    assert abs(r['loss'] - float(loss.detach())) <= 1e-11 * max(1.0, abs(float(loss.detach())))
    (0.7 * loss).backward()
    for name, t in (('dQ', q), ('dK', k)):
        assert np.abs(r[name] - t.grad.numpy()).max() <= 1e-11 * max(1.0, float(t.grad.abs().max())), name
    s = logits.detach().numpy()
    assert r['rank'].tolist() == [_argsort_rank(s[t], tok[t]) for t in range(T)]
    assert r['status'] == 0
    m = vocab_nll_numpy(Q, K, tok)                            # weights None: the mean
    assert abs(m['loss'] - float(nll.mean())) <= 1e-11 * max(1.0, abs(float(nll.mean())))


@pytest.mark.parametrize('T,V,E', VC.CASES)
def test_cases_keep_their_targets_apart(T, V, E):
    """The rank comparison of the GPU test may leave out a token whose target is within twice the score bound of another logit: at
    most RANK_CLOSE_CAP of a case's tokens, by the fp64 restatement alone and under the wider (split-bf16) bound."""
    Q, K, tok = VC.make_case(T, V, E)
    for mode in ('bf16x3', 'f32'):
        far = VC.separated(Q, K, tok, mode)
        assert int((~far).sum()) <= int(VC.RANK_CLOSE_CAP * T), (mode, int((~far).sum()), T)
    assert np.linalg.norm(Q.astype(np.float64), axis=1).min() >= 1.0 - 1e-6
    if T > 3:
        assert tok[0] == 0 and tok[1] == V - 1 and tok[2] == tok[3]


def test_rank_ties_nan_and_signed_zero():
    from cliora_amd.vocab import vocab_nll_numpy
    K = np.array([[1.0], [2.0], [2.0], [1.0], [2.0], [-0.0], [0.0]])
    Q = np.ones((7, 1))
    r = vocab_nll_numpy(Q, K, np.arange(7))
    assert r['rank'].tolist() == [3, 0, 1, 4, 2, 5, 6]         # equal scores by ascending index; -0 is 0
    Kn = np.array([[1.0], [np.nan], [3.0], [np.nan]])
    r = vocab_nll_numpy(np.ones((4, 1)), Kn, np.arange(4))
    assert r['rank'].tolist() == [1, 2, 0, 3]                  # a NaN logit ranks below every number, NaNs among themselves by index
    s = np.array([1.0, np.nan, 3.0, np.nan])
    assert [_argsort_rank(s, t) for t in range(4)] == [1, 2, 0, 3]


def test_edge_semantics_of_the_restatement():
    from cliora_amd.vocab import vocab_nll_numpy
    rs = np.random.RandomState(0)
    Q, K = rs.randn(6, 5), rs.randn(9, 5)
    tok = np.array([0, 8, 9, -1, 3, 3])
    w = np.array([0.5, 0.25, 0.5, 0.5, 0.0, 0.25])
    Qn = Q.copy()
    Qn[4] = np.nan                                             # a padded row: weight 0
    r = vocab_nll_numpy(Qn, K, tok, w, want_grad=True)
    ref = vocab_nll_numpy(Q[[0, 1, 5]], K, tok[[0, 1, 5]], w[[0, 1, 5]], want_grad=True)
    assert r['status'] == 2 and np.isnan(r['nll'][[2, 3]]).all() and np.isnan(r['tgt'][[2, 3]]).all() and r['rank'][[2, 3]].tolist() == [-1, -1]
    assert np.isfinite(r['lse'][[2, 3]]).all()
    assert r['loss'] == ref['loss']
    assert np.array_equal(r['dQ'][[0, 1, 5]], ref['dQ']) and not r['dQ'][[2, 3, 4]].any()
    assert np.allclose(r['dK'], ref['dK'], rtol=0, atol=1e-15) and np.isfinite(r['dK']).all()
    Qn[0] = np.nan                                             # a NaN query row with weight: its own outputs and the loss
    r = vocab_nll_numpy(Qn, K, tok, w)
    assert np.isnan(r['loss']) and np.isnan(r['nll'][0]) and np.isnan(r['lse'][0]) and r['rank'][0] == 0
    assert np.isfinite(r['nll'][[1, 5]]).all() and np.array_equal(r['rank'][[1, 5]], ref['rank'][[1, 2]])
    # logits of +-300: the maximum is subtracted before every exp
    big = vocab_nll_numpy(np.array([[300.0], [-300.0]]), np.array([[1.0], [-1.0], [0.5]]), np.array([0, 1]))
    assert np.isfinite(big['lse']).all() and np.abs(big['nll']).max() < 1e-60 and big['rank'].tolist() == [0, 0]
    one = vocab_nll_numpy(rs.randn(4, 3), rs.randn(1, 3), np.zeros(4, np.int64))
    assert not one['nll'].any() and not one['rank'].any()      # V = 1
    none = vocab_nll_numpy(np.zeros((0, 3)), rs.randn(5, 3), np.zeros(0, np.int64))
    assert none['loss'] == 0.0 and none['nll'].shape == (0,)   # T = 0


def _net(full, obj=False, V=100, D=32, seed=0):
    from cliora_amd.harness import build_net
    torch.manual_seed(seed)
    return build_net(D, torch.nn.Embedding(V, D), obj_feats=obj, img_dim=24, k_neg=3, full_softmax=full)


class _Chart(object):
    def __init__(self, outside_h):
        self.outside_h = outside_h


def test_link_to_the_sampled_objective():
    """With neg_samples = arange(V) the reference's sampled loss counts the positive once more among the negatives: it is the mean of
    softplus(nll[t]) of the exact loss."""
    from cliora_amd.vocab import vocab_nll_numpy
    net = _net(False).double()
    head = net.reconstruct_softmax_loss
    B, L, V = 4, 5, 100
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(0, V, (B, L), generator=g)
    oh = torch.randn(B, L * (L + 1) // 2, 32, generator=g, dtype=torch.float64)
    sampled = float(head(tokens, torch.arange(V), _Chart(oh)))
    Q = (oh[:, :L].reshape(B * L, -1) @ head.mat).detach().numpy()
    nll = vocab_nll_numpy(Q, head.embeddings.weight.detach().numpy(), tokens.reshape(-1).numpy())['nll']
    assert abs(sampled - float(np.logaddexp(0.0, nll).mean())) <= 1e-6


@pytest.mark.parametrize('obj', [False, True])
def test_full_softmax_module_on_the_cpu(obj):
    from cliora_amd.vocab import vocab_nll_numpy
    net = _net(True, obj=obj).double()
    head = net.reconstruct_softmax_loss
    assert head.full_vocab and head.name == 'reconstruct_softmax_loss' and not _net(False).reconstruct_softmax_loss.full_vocab
    assert head.embeddings.weight.requires_grad == (not obj)
    B, L, V = 4, 5, 100
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, V, (B, L), generator=g)
    oh = torch.randn(B, L * (L + 1) // 2, 32, generator=g, dtype=torch.float64, requires_grad=True)
    loss = head(tokens, None, _Chart(oh))                      # neg_samples is ignored
    logits = (oh[:, :L].reshape(B * L, -1) @ head.mat) @ head.embeddings.weight.t()
    want = F.cross_entropy(logits, tokens.reshape(-1))
    assert abs(float(loss) - float(want)) <= 1e-12
    r = vocab_nll_numpy((oh[:, :L].reshape(B * L, -1) @ head.mat).detach().numpy(), head.embeddings.weight.detach().numpy(), tokens.reshape(-1).numpy())
    assert abs(float(loss) - r['loss']) <= 1e-12
    small = torch.randn(2, 6, 32, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda o: head(tokens[:2, :3], None, _Chart(o)), (small,), eps=1e-6, atol=1e-6)


def test_vocab_nll_torch_path_matches_the_restatement():
    from cliora_amd.vocab import vocab_nll, vocab_nll_numpy
    Q, K, tok = VC.make_case(17, 16, 33)
    tok = tok.copy()
    tok[5] = 16                                                # outside the table
    w = np.random.RandomState(5).rand(17)
    w[7] = 0.0
    q = torch.from_numpy(Q).double().requires_grad_(True)
    k = torch.from_numpy(K).double().requires_grad_(True)
    loss, nll, lse, tgt, rank, status = vocab_nll(q, k, torch.from_numpy(tok), torch.from_numpy(w), want_rank=True)
    r = vocab_nll_numpy(Q, K, tok, w, want_grad=True)
    assert int(status) == 1 and rank.dtype == torch.int32 and rank.tolist() == r['rank'].tolist()
    for a, b in ((nll, r['nll']), (lse, r['lse']), (tgt, r['tgt'])):
        assert np.allclose(a.numpy(), b, rtol=0, atol=1e-11, equal_nan=True)
    assert abs(float(loss) - r['loss']) <= 1e-11
    loss.backward()
    assert np.abs(q.grad.numpy() - r['dQ']).max() <= 1e-11 and np.abs(k.grad.numpy() - r['dK']).max() <= 1e-11
    assert vocab_nll(q, k, torch.from_numpy(tok))[4] is None   # no rank unless asked


def test_word_prediction_metrics():
    from cliora_amd.vocab import word_prediction_metrics
    from cliora_amd import evaluate
    assert evaluate.word_prediction is __import__('cliora_amd.vocab', fromlist=['x']).word_prediction
    nll = np.array([0.5, 1.5, np.nan, 2.5])
    rank = np.array([0, 4, -1, 9])
    m = word_prediction_metrics(nll, rank, ks=(1, 5, 10))
    assert m['tokens'] == 3 and m['out_of_range'] == 1
    assert m['nll'] == 1.5 and abs(m['perplexity'] - np.exp(1.5)) < 1e-12
    assert m['acc@k'] == {1: 1 / 3, 5: 2 / 3, 10: 1.0}
    assert abs(m['mrr'] - (1 + 1 / 5 + 1 / 10) / 3) < 1e-15
    assert sorted(m) == ['acc@k', 'mrr', 'nll', 'out_of_range', 'perplexity', 'tokens']


# ---- the C entries without a device ------------------------------------------------------------------------------------------------
def _refused(name, code, *args):
    from cliora_amd import _lib
    rc = _lib.fn(name)(*args)
    msg = _lib.fn('cliora_last_error')().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith(name + ':'), msg
    return msg


FWD = ('T', 'V', 'E', 'Q', 'ldq', 'K', 'ldk', 'tok', 'w', 'loss', 'nll', 'lse', 'lse_lo', 'tgt', 'rank', 'status', 'ws', 'ws_bytes', 'stream')
BWD = ('T', 'V', 'E', 'Q', 'ldq', 'K', 'ldk', 'tok', 'w', 'lse', 'lse_lo', 'g', 'dQ', 'lddq', 'dK', 'lddk', 'ws', 'ws_bytes', 'stream')


def _args(names, **kw):
    a = {n: ONE for n in names}
    a.update(T=3, V=40, E=20, ldq=20, ldk=20, lddq=20, lddk=20, ws_bytes=1 << 40, stream=NULL)
    a.update(kw)
    return [a[n] for n in names]


@pytest.mark.parametrize('change', [dict(T=-1), dict(V=0), dict(E=0), dict(ldq=19), dict(ldk=19), dict(Q=NULL), dict(K=NULL), dict(tok=NULL),
                                    dict(w=NULL), dict(loss=NULL), dict(nll=NULL), dict(lse=NULL), dict(tgt=NULL), dict(status=NULL),
                                    dict(ws=NULL)])
def test_forward_refusals(change):
    _refused('cliora_vocab_nll_forward', EINVAL, *_args(FWD, **change))


@pytest.mark.parametrize('change', [dict(T=-1), dict(V=0), dict(E=0), dict(ldq=19), dict(ldk=19), dict(lddq=19), dict(lddk=19), dict(Q=NULL),
                                    dict(K=NULL), dict(tok=NULL), dict(w=NULL), dict(lse=NULL), dict(g=NULL), dict(ws=NULL)])
def test_backward_refusals(change):
    _refused('cliora_vocab_nll_backward', EINVAL, *_args(BWD, **change))


def _al(x):
    return (x + 255) // 256 * 256


def _formula(T, V, E, want_backward):
    """The workspace formula as include/cliora_chart.h states it."""
    cd = lambda a, b: (a + b - 1) // b
    F_ = 2048 * cd(E, 32)
    qt, kt, q4, e16 = cd(T, 64), cd(V, 256), cd(T, 256), cd(E, 16)
    r = 2 if kt <= 64 else 16 if kt >= 512 else cd(kt, 32)
    fwd = 2 * _al(4 * qt * F_) + _al(16 * kt * F_) + _al(8 * T * cd(kt, 8)) + _al(4 * T * cd(kt, 8))
    bwd = (_al(16 * q4 * F_) + _al(16 * kt * F_) + _al(4 * T) + _al(16384 * e16 * kt) + _al(16384 * e16 * q4)
           + _al(64 * e16 * max(cd(kt, r) * 64 * qt, cd(q4, 16) * 64 * cd(V, 64))))
    return max(fwd, bwd) if want_backward else fwd


def test_workspace_formula_and_refusal():
    from cliora_amd import _lib
    size = _lib.fn('cliora_vocab_workspace_bytes')
    for T, V, E in VC.CASES + [(0, 1, 1), (1280, 400000, 400), (111826, 400000, 400), (1280, 8000, 1324)]:
        for wb in (0, 1):
            assert size(T, V, E, wb) == _formula(T, V, E, wb), (T, V, E, wb)
    assert size(-1, 5, 5, 0) == 0 and size(5, 0, 5, 0) == 0 and size(5, 5, 0, 1) == 0
    need_f, need_b = size(3, 40, 20, 0), size(3, 40, 20, 1)
    assert 0 < need_f <= need_b
    assert 'cliora_vocab_workspace_bytes' in _refused('cliora_vocab_nll_forward', ENOMEM, *_args(FWD, ws_bytes=need_f - 1))
    assert 'cliora_vocab_workspace_bytes' in _refused('cliora_vocab_nll_backward', ENOMEM, *_args(BWD, ws_bytes=need_b - 1))
    # no buffer of T x V elements: at the test split's size (111 826 tokens, V = 400k, E = 400) everything beside the packed operands
    # is 12 bytes per (token, 2048 words); in training (1 280 tokens) the whole workspace is a few copies of the table
    T, V, E = 111826, 400000, 400
    packed = (2 * 4 * ((T + 63) // 64) + 16 * ((V + 255) // 256)) * 2048 * 13
    assert size(T, V, E, 0) - packed <= 12 * T * 196 + 5 * 256
    assert size(T, V, E, 0) < 4 * T * V // 100
    assert size(1280, V, E, 1) <= 3.1 * (V * 416 * 4) and size(1280, V, E, 1) < 4 * 1280 * V


def test_wrapper_checks_shapes_before_any_call():
    from cliora_amd.vocab import VocabNLL
    q, k = torch.zeros(3, 4), torch.zeros(5, 6)
    with pytest.raises(ValueError):
        VocabNLL.apply(q, k, torch.zeros(3, dtype=torch.long), torch.zeros(3), False)
