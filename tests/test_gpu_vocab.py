"""The whole-vocabulary loss on the device (cliora_amd/vocab.py, csrc/api_vocab.hip, csrc/vocab_kernels.hpp) against its fp64
restatement: values, ranks, gradients, determinism and edge semantics in both MFMA modes, and the module level (Trainer.step,
step_ragged, word_prediction).  Cases, inputs and bounds: tests/vocab_cases.py."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vocab_cases as VC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(T, V, E):
    from cliora_amd.vocab import vocab_nll_numpy
    Q, K, tok = VC.make_case(T, V, E)
    w = (np.random.RandomState(7).rand(T).astype(np.float32) + 0.5) / max(T, 1)
    return Q, K, tok, w, vocab_nll_numpy(Q, K, tok, w, want_grad=True, g=0.75)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _forward(Q, K, tok, w, want_rank=True, fill=None, lo=None):
    """The C entry itself on device tensors -> (loss, nll, lse, tgt, rank, status) as numpy; fill: the workspace's bytes before the call;
    lo: a one-element list that receives lse_lo (a device tensor) when given."""
    from cliora_amd import _lib
    from cliora_amd._lib import ptr
    T, E = Q.shape
    V = K.shape[0]
    nb = _lib.fn('cliora_vocab_workspace_bytes')(T, V, E, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    if fill is not None:
        ws.fill_(fill)
    loss = torch.full((1,), 7.0, device='cuda')
    nll, lse, tgt = (torch.full((T,), 7.0, device='cuda') for _ in range(3))
    rank = torch.full((T,), 7, dtype=torch.int32, device='cuda') if want_rank else None
    status = torch.full((1,), 7, dtype=torch.int32, device='cuda')
    lse_lo = torch.full((T,), 7.0, device='cuda') if lo is not None else None
    _lib.call('cliora_vocab_nll_forward', T, V, E, ptr(Q), E, ptr(K), E, ptr(tok), ptr(w), ptr(loss), ptr(nll), ptr(lse), ptr(lse_lo), ptr(tgt),
              ptr(rank), ptr(status), ptr(ws), nb, _lib.stream())
    if lo is not None:
        lo[0] = lse_lo
    torch.cuda.synchronize()
    return (loss.cpu().numpy()[0], nll.cpu().numpy(), lse.cpu().numpy(), tgt.cpu().numpy(), rank.cpu().numpy() if want_rank else None,
            int(status.cpu()[0]))


def _backward(Q, K, tok, w, lse, g, dq=True, dk=True, fill=None, lse_lo=None):
    from cliora_amd import _lib
    from cliora_amd._lib import ptr
    T, E = Q.shape
    V = K.shape[0]
    nb = _lib.fn('cliora_vocab_workspace_bytes')(T, V, E, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    if fill is not None:
        ws.fill_(fill)
    dQ = torch.full((T, E), 7.0, device='cuda') if dq else None
    dK = torch.full((V, E), 7.0, device='cuda') if dk else None
    gt = torch.tensor([g], dtype=torch.float32, device='cuda')
    _lib.call('cliora_vocab_nll_backward', T, V, E, ptr(Q), E, ptr(K), E, ptr(tok), ptr(w), ptr(lse), ptr(lse_lo), ptr(gt), ptr(dQ), E, ptr(dK), E, ptr(ws),
              nb, _lib.stream())
    torch.cuda.synchronize()
    return (dQ.cpu().numpy() if dq else None), (dK.cpu().numpy() if dk else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


# ---- forward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,V,E', VC.CASES)
def test_forward_against_fp64(mfma_mode, T, V, E):
    from cliora_amd.phrases import knn_ip
    Q, K, tok, w, ref = _case(T, V, E)
    q, k, t, wd = _dev(Q, K, tok, w)
    loss, nll, lse, tgt, rank, status = _forward(q, k, t, wd)
    b = VC.score_bound(mfma_mode, Q, K)
    e_lse, e_tgt, e_nll = np.abs(lse - ref['lse']), np.abs(tgt - ref['tgt']), np.abs(nll - ref['nll'])
    loss_bound = float(np.sum(np.abs(w) * 2 * b)) + 1e-6 * abs(ref['loss'])
    print('vocab fwd %s T %d V %d E %d: err / bound  lse %.3f  tgt %.3f  nll %.3f  loss %.3f' % (
        mfma_mode, T, V, E, (e_lse / b).max(), (e_tgt / b).max(), (e_nll / (2 * b)).max(), abs(loss - ref['loss']) / loss_bound))
    assert status == 0
    assert (e_lse <= b).all() and (e_tgt <= b).all() and (e_nll <= 2 * b).all()
    assert abs(loss - ref['loss']) <= loss_bound
    far = VC.separated(Q, K, tok, mfma_mode)
    assert int((~far).sum()) <= int(VC.RANK_CLOSE_CAP * T)
    assert np.array_equal(rank[far], ref['rank'][far])
    _, best = knn_ip(q, k, 1)                               # the bitwise-target property, on every token
    assert np.array_equal(rank == 0, best.cpu().numpy()[:, 0] == tok)
    no_rank = _forward(q, k, t, wd, want_rank=False)
    assert no_rank[4] is None and np.array_equal(_bits(no_rank[1]), _bits(nll)) and _bits(np.float32(no_rank[0])) == _bits(np.float32(loss))


def test_ties_rank_by_ascending_index(mfma_mode):
    rs = np.random.RandomState(12)
    base = rs.randn(10, 8).astype(np.float32)
    K = base[rs.randint(0, 10, size=600)]                    # 600 words, 10 distinct rows: every logit has about 60 equals
    Q = rs.randn(70, 8).astype(np.float32)
    tok = rs.randint(0, 600, size=70).astype(np.int64)
    w = np.full(70, 1 / 70, np.float32)
    _, _, _, tgt, rank, _ = _forward(*_dev(Q, K, tok, w))
    s = Q.astype(np.float64) @ base.T.astype(np.float64)      # distinct rows are far apart: their order is that of fp64
    src = np.array([int(np.nonzero((base == K[v]).all(1))[0][0]) for v in range(600)])
    want = [int((s[t][src] > s[t][src[tok[t]]]).sum() + (src[:tok[t]] == src[tok[t]]).sum()) for t in range(70)]
    gap = np.abs(s[:, :, None] - s[:, None, :]) + 1e9 * np.eye(10)[None]
    assert gap.min() > 4 * VC.score_bound(mfma_mode, Q, K).max()
    assert rank.tolist() == want


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,V,E', VC.GRAD_CASES)
def test_gradients_against_fp64(mfma_mode, T, V, E):
    Q, K, tok, w, ref = _case(T, V, E)
    q, k, t, wd = _dev(Q, K, tok, w)
    lo = [None]
    lse = _forward(q, k, t, wd, want_rank=False, lo=lo)[2]
    lse_d = torch.from_numpy(lse).cuda()
    assert float(lo[0].abs().max()) <= float(np.spacing(np.abs(lse).max())) / 2
    dQ, dK = _backward(q, k, t, wd, lse_d, 0.75, fill=0xFF, lse_lo=lo[0])
    # the route without the kernels, on the device in fp32, against the same fp64 gradient
    qa, ka = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    (0.75 * (wd * F.cross_entropy(qa @ ka.t(), t, reduction='none')).sum()).backward()
    for name, have, torch_have in (('dQ', dQ, qa.grad), ('dK', dK, ka.grad)):
        tol = VC.grad_tol(mfma_mode, Q, K, name)
        scale = np.abs(ref[name]).max()
        err = np.abs(have - ref[name]).max() / scale
        terr = np.abs(torch_have.cpu().numpy() - ref[name]).max() / scale
        print('vocab grad %s T %d V %d E %d %s: err %.3e  tol %.3e  torch fp32 route %.3e' % (mfma_mode, T, V, E, name, err, tol, terr))
        assert err <= tol, (name, err, tol)
    # each half alone is bitwise the half of the full call
    only_q, none_k = _backward(q, k, t, wd, lse_d, 0.75, dk=False, lse_lo=lo[0])
    none_q, only_k = _backward(q, k, t, wd, lse_d, 0.75, dq=False, lse_lo=lo[0])
    assert none_k is None and none_q is None
    assert np.array_equal(_bits(only_q), _bits(dQ)) and np.array_equal(_bits(only_k), _bits(dK))


def _sum_p_minus_one(Q, K, tok):
    """sum_v p[t][v] - 1 of the recomputed p, for EVERY token, from each half of the backward in one call.  K gets a column of ones and
    Q a zero there, and Q gets the T columns of an identity where K is zero: the scores are unchanged, and with w = 1, g = 1
      dQ[t][E] = sum_v (p[t][v] - [v == tok_t]) 1,        sum_v dK[v][E + 1 + t] = sum_v (p[t][v] - [v == tok_t]) 1."""
    T, E = Q.shape
    V = K.shape[0]
    Qx = np.concatenate([Q, np.zeros((T, 1), np.float32), np.eye(T, dtype=np.float32)], 1)
    Kx = np.concatenate([K, np.ones((V, 1), np.float32), np.zeros((V, T), np.float32)], 1)
    q, k, t, w1 = _dev(Qx, Kx, tok, np.ones(T, np.float32))
    lo = [None]
    lse = torch.from_numpy(_forward(q, k, t, w1, want_rank=False, lo=lo)[2]).cuda()
    dQ, dK = _backward(q, k, t, w1, lse, 1.0, lse_lo=lo[0])
    return dQ[:, E].astype(np.float64), dK[:, E + 1:].astype(np.float64).sum(0)


@pytest.mark.parametrize('T,V,E', VC.GRAD_CASES)
def test_recomputed_probabilities_sum_to_one_on_every_token(mfma_mode, T, V, E):
    Q, K, tok, _, _ = _case(T, V, E)
    from_dq, from_dk = _sum_p_minus_one(Q, K, tok)
    print('vocab sum p - 1 %s T %d V %d E %d: largest |.| from dQ %.3e, from dK %.3e' % (mfma_mode, T, V, E, np.abs(from_dq).max(),
                                                                                        np.abs(from_dk).max()))
    assert from_dq.shape == (T,) and from_dk.shape == (T,)
    assert (np.abs(from_dq) <= 1e-5).all(), np.nonzero(np.abs(from_dq) > 1e-5)[0]
    assert (np.abs(from_dk) <= 1e-5).all(), np.nonzero(np.abs(from_dk) > 1e-5)[0]


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_determinism_and_independence_of_the_rest_of_the_call(mfma_mode):
    T, V, E = 130, 5000, 400
    Q, K, tok, w, _ = _case(T, V, E)
    q, k, t, wd = _dev(Q, K, tok, w)
    a = _forward(q, k, t, wd, fill=0xFF)
    b = _forward(q, k, t, wd, fill=0x00)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(_bits(np.asarray(x)), _bits(np.asarray(y)))
    lse_d = torch.from_numpy(a[2]).cuda()
    dQ, dK = _backward(q, k, t, wd, lse_d, 0.75, fill=0xFF)
    dQ2, dK2 = _backward(q, k, t, wd, lse_d, 0.75, fill=0x00)
    assert np.array_equal(_bits(dQ), _bits(dQ2)) and np.array_equal(_bits(dK), _bits(dK2))
    # permuted, and a subset: every token's outputs and dQ row keep their bits; the subset's loss is the call on the subset
    perm = np.random.RandomState(2).permutation(T)
    qp, tp, wp = _dev(Q[perm], tok[perm], w[perm])
    p = _forward(qp, k, tp, wp)
    for x, y in zip(a[1:5], p[1:5]):
        assert np.array_equal(_bits(x[perm]), _bits(y))
    dQp, _ = _backward(qp, k, tp, wp, torch.from_numpy(p[2]).cuda(), 0.75, dk=False)
    assert np.array_equal(_bits(dQ[perm]), _bits(dQp))
    sub = np.array([5, 64, 17, 129, 70])
    sub.sort()
    qs, ts, wsub = _dev(Q[sub], tok[sub], w[sub])
    s = _forward(qs, k, ts, wsub)
    for x, y in zip(a[1:5], s[1:5]):
        assert np.array_equal(_bits(x[sub]), _bits(y))
    dQs, _ = _backward(qs, k, ts, wsub, torch.from_numpy(s[2]).cuda(), 0.75, dk=False)
    assert np.array_equal(_bits(dQ[sub]), _bits(dQs))
    one = _forward(*_dev(Q[64:65], K, tok[64:65], w[64:65]))
    for x, y in zip(a[1:5], one[1:5]):
        assert np.array_equal(_bits(x[64:65]), _bits(y))
    wz = np.zeros_like(w)
    wz[sub] = w[sub]
    z = _forward(q, k, t, _dev(wz)[0])
    assert _bits(np.float32(z[0])) == _bits(np.float32(s[0]))


# ---- edge semantics -------------------------------------------------------------------------------------------------------------------
def test_edge_semantics(mfma_mode):
    from cliora_amd.vocab import vocab_nll_numpy
    rs = np.random.RandomState(0)
    Q, K = rs.randn(70, 33).astype(np.float32), rs.randn(300, 33).astype(np.float32)
    tok = rs.randint(0, 300, size=70).astype(np.int64)
    w = (rs.rand(70).astype(np.float32) + 0.5) / 70
    tok[[2, 66]] = [300, -1]                                  # ids outside the table
    w[[4, 65]] = 0.0                                          # padded rows ...
    Qn = Q.copy()
    Qn[[4, 65]] = np.nan                                      # ... holding NaN
    keep = np.array([i for i in range(70) if i not in (2, 66, 4, 65)])
    q, k, t, wd = _dev(Qn, K, tok, w)
    loss, nll, lse, tgt, rank, status = _forward(q, k, t, wd, fill=0xFF)          # 0xFF bytes: a workspace of NaNs
    ref = _forward(*_dev(Q[keep], K, tok[keep], w[keep]))
    assert status == 2
    assert np.isnan(nll[[2, 66]]).all() and np.isnan(tgt[[2, 66]]).all() and rank[[2, 66]].tolist() == [-1, -1] and np.isfinite(lse[[2, 66]]).all()
    assert _bits(np.float32(loss)) == _bits(np.float32(ref[0])) and np.isfinite(loss)
    for x, y in zip((nll, lse, tgt, rank), ref[1:5]):
        assert np.array_equal(_bits(x[keep]), _bits(y))
    dQ, dK = _backward(q, k, t, wd, torch.from_numpy(lse).cuda(), 1.0, fill=0xFF)
    rQ, rK = _backward(*_dev(Q[keep], K, tok[keep], w[keep]), torch.from_numpy(ref[2]).cuda(), 1.0)
    assert not dQ[[2, 66, 4, 65]].any() and np.array_equal(_bits(dQ[keep]), _bits(rQ))
    want = vocab_nll_numpy(Q[keep], K, tok[keep], w[keep], want_grad=True)
    qk, kk, tk, wk = _dev(Q[keep], K, tok[keep], w[keep])      # the torch fp32 route on the tokens that count: its error sets the tolerance
    kk.requires_grad_(True)
    (wk * F.cross_entropy(qk @ kk.t(), tk, reduction='none')).sum().backward()
    scale = np.abs(want['dK']).max()
    terr = np.abs(kk.grad.cpu().numpy() - want['dK']).max() / scale
    assert np.isfinite(dK).all() and np.abs(dK - want['dK']).max() <= VC.grad_tol(mfma_mode, Q[keep], K, 'dK', torch_err=terr) * scale
    # a NaN query row that counts: its own outputs and the loss, nobody else's
    Qn[7] = np.nan
    loss2, nll2, lse2, tgt2, rank2, _ = _forward(*_dev(Qn, K, tok, w))
    assert np.isnan(loss2) and np.isnan(nll2[7]) and np.isnan(lse2[7]) and np.isnan(tgt2[7])
    rest = keep[keep != 7]
    for x, y in zip((nll2, lse2, tgt2, rank2), (nll, lse, tgt, rank)):
        assert np.array_equal(_bits(x[rest]), _bits(y[rest]))
    # logits of +-300
    big_q = np.zeros((2, 33), np.float32)
    big_k = np.zeros((3, 33), np.float32)
    big_q[:, 0] = [300.0, -300.0]
    big_k[:, 0] = [1.0, -1.0, 0.5]
    bl, bn, bs, bt, br, _ = _forward(*_dev(big_q, big_k, np.array([0, 1]), np.array([0.5, 0.5], np.float32)))
    assert bt.tolist() == [300.0, 300.0] and bs.tolist() == [300.0, 300.0] and bn.tolist() == [0.0, 0.0] and br.tolist() == [0, 0] and bl == 0.0
    bl, bn, bs, bt, br, _ = _forward(*_dev(big_q, big_k, np.array([1, 0]), np.array([0.5, 0.5], np.float32)))
    assert bn.tolist() == [600.0, 600.0] and br.tolist() == [2, 2] and bl == 600.0
    # V = 1 and T = 0
    l1, n1, s1, t1, r1, _ = _forward(*_dev(Q[:20], K[:1], np.zeros(20, np.int64), w[:20]))
    assert not n1.any() and not r1.any() and l1 == 0.0 and np.array_equal(_bits(s1), _bits(t1))
    l0 = _forward(*_dev(Q[:0], K, tok[:0], w[:0]))
    assert l0[0] == 0.0 and l0[5] == 0
    _, dk0 = _backward(*_dev(Q[:0], K, tok[:0], w[:0]), torch.zeros(0, device='cuda'), 1.0)
    assert dk0.shape == K.shape and not dk0.any()


def test_autograd_function_and_wrapper(mfma_mode):
    from cliora_amd.vocab import vocab_nll
    T, V, E = 65, 256, 300
    Q, K, tok, w, ref = _case(T, V, E)
    q, k, t, wd = _dev(Q, K, tok, w)
    q.requires_grad_(True)
    k.requires_grad_(True)
    loss, nll, lse, tgt, rank, status = vocab_nll(q, k, t, wd, want_rank=True)
    (0.75 * loss).backward()
    assert np.abs(q.grad.cpu().numpy() - ref['dQ']).max() <= VC.grad_tol(mfma_mode, Q, K, 'dQ') * np.abs(ref['dQ']).max()
    assert np.abs(k.grad.cpu().numpy() - ref['dK']).max() <= VC.grad_tol(mfma_mode, Q, K, 'dK') * np.abs(ref['dK']).max()
    assert int(status) == 0 and rank.dtype == torch.int32 and not nll.requires_grad
    frozen = k.detach()                                      # a frozen table: dQ alone, the same bits
    q2 = q.detach().clone().requires_grad_(True)
    (0.75 * vocab_nll(q2, frozen, t, wd)[0]).backward()
    assert torch.equal(q2.grad, q.grad)
    mean = vocab_nll(q.detach(), frozen, t)[0]               # weights None: the mean
    assert abs(float(mean) - float(np.mean(ref['nll']))) <= 2 * VC.score_bound(mfma_mode, Q, K).max()


# ---- module level ---------------------------------------------------------------------------------------------------------------------
def _nets(obj, full=True):
    from cliora_amd import harness as H
    torch.manual_seed(5)
    net = H.build_net(32, torch.nn.Embedding(100, 32), obj_feats=obj, img_dim=48, k_neg=3, full_softmax=full)
    return net.cuda(), H


def _batch(obj, B=4, L=5):
    g = torch.Generator().manual_seed(9)
    bm = dict(sentences=torch.randint(0, 100, (B, L), generator=g).cuda(), neg_samples=torch.randint(0, 100, (3,), generator=g).cuda())
    if obj:
        bm['obj_feats'] = torch.randn(B, 6, 48, generator=g).cuda()
    return bm


@pytest.mark.parametrize('obj', [False, True])
def test_trainer_step_matches_the_torch_fallback(obj, mfma_mode, monkeypatch):
    net, H = _nets(obj)
    other = copy.deepcopy(net)
    start = {k: p.detach().clone() for k, p in net.named_parameters()}
    bm = _batch(obj)
    for n in (net, other):
        n.train = lambda mode=True, n=n: torch.nn.Module.train(n, False)       # dropout off, as tests/test_gpu_harness.py runs its steps
    lr = 2e-3
    got = H.Trainer(net, lr=lr).step(bm, train=True)['total_loss']
    # the fallback: the same step with the loss in torch (F.cross_entropy on the full logits); its gradients, to tell rounding noise
    monkeypatch.setattr(H, 'NATIVE_HEADS', False)
    probe = copy.deepcopy(other)
    probe.eval()
    out = probe(bm['sentences'], bm.get('obj_feats'), bm['neg_samples'])
    out.total().backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in probe.named_parameters()}
    want = H.Trainer(other, lr=lr).step(bm, train=True)['total_loss']
    monkeypatch.setattr(H, 'NATIVE_HEADS', True)
    print('full softmax step %s obj %s: loss %.6f, torch fallback %.6f' % (mfma_mode, obj, got, want))
    assert abs(got - want) <= 2e-4 * max(1.0, abs(want))
    assert net.reconstruct_softmax_loss.embeddings.weight.requires_grad == (not obj)
    tol = 5e-4 if mfma_mode == 'f32' else 1e-3
    moved = 0
    for (k, p), (_, r) in zip(net.named_parameters(), other.named_parameters()):
        if not p.requires_grad:
            assert torch.equal(p, start[k])
            continue
        g = grads[k]
        noise = g.abs() <= 2e-4 * max(1.0, float(g.abs().max()))         # Adam's first step is lr sign(g): below the gradient tolerance the sign is open
        have, ref = p.detach(), r.detach()
        if noise.any():
            assert float((have - start[k])[noise].abs().max()) <= lr * (1 + 1e-3), k
        if (~noise).any():
            assert float((have - ref)[~noise].abs().max()) <= tol * max(1.0, float(ref.abs().max())), k
        moved += int(bool((have != start[k]).any()))
    assert moved >= 5


def test_default_net_keeps_the_sampled_loss():
    """build_net's default is the sampled loss, routed to the kernels it had: the module's value is heads.recon_loss on the same chart,
    bit for bit.  (That those kernels' bits are what they were is held by the goldens of tests/test_gpu_harness.py.)"""
    from cliora_amd import heads
    bm = _batch(False)
    net, H = _nets(False, full=False)
    torch.manual_seed(5)
    plain = H.build_net(32, torch.nn.Embedding(100, 32), obj_feats=False, img_dim=48, k_neg=3).cuda()
    head = plain.reconstruct_softmax_loss
    assert not head.full_vocab and not net.reconstruct_softmax_loss.full_vocab
    plain.eval()
    with torch.no_grad():
        out = plain(bm['sentences'], None, bm['neg_samples'])
        want = heads.recon_loss(head.embeddings.weight, head.mat, plain.diora.outside_h, bm['sentences'], bm['neg_samples'])
    assert torch.equal(out['reconstruct_softmax_loss'], want)
    full, _ = _nets(False)
    full.eval()
    with torch.no_grad():
        assert float(full(bm['sentences'], None, None)['reconstruct_softmax_loss']) != float(want)
    assert int(full.reconstruct_softmax_loss.vocab_status) == 0


def test_step_ragged_is_the_token_weighted_mean(mfma_mode):
    lengths = [2, 5, 5, 7]
    rs = np.random.RandomState(3)
    sentences = [rs.randint(0, 100, size=n).tolist() for n in lengths]
    net, H = _nets(False)
    net.eval()
    want, n_tok = 0.0, float(sum(lengths))
    with torch.no_grad():
        for n in sorted(set(lengths)):
            group = torch.tensor([s for s in sentences if len(s) == n]).cuda()
            out = net(group, None, None)
            want += float(out.total()) * group.numel() / n_tok
    tr = H.Trainer(net, lr=2e-3)
    net.train = lambda mode=True: torch.nn.Module.train(net, False)
    got = tr.step_ragged(sentences)['total_loss']
    print('full softmax step_ragged %s: loss %.6f, per-length mean %.6f' % (mfma_mode, got, want))
    assert abs(got - want) <= 1e-4 * max(1.0, abs(want))


def test_word_prediction_equals_the_numpy_metrics(mfma_mode):
    from cliora_amd.vocab import vocab_nll_numpy, word_prediction, word_prediction_metrics
    from cliora_amd.evaluate import word_prediction as from_evaluate
    assert from_evaluate is word_prediction
    net, _ = _nets(False)
    batches = [_batch(False, 4, 5), _batch(False, 3, 7)]
    m = word_prediction(net, batches, ks=(1, 5, 10))
    head = net.reconstruct_softmax_loss
    nll, rank, close, bound = [], [], 0, 0.0
    with torch.no_grad():
        for bm in batches:
            net(bm['sentences'], None, None, compute_loss=False)
            L = bm['sentences'].shape[1]
            Q = torch.mm(net.diora.outside_h[:, :L].reshape(-1, 32), head.mat).cpu().numpy()
            K = head.embeddings.weight.detach().cpu().numpy()
            tok = bm['sentences'].reshape(-1).cpu().numpy()
            r = vocab_nll_numpy(Q, K, tok)
            close += int((~VC.separated(Q, K, tok, mfma_mode)).sum())
            bound = max(bound, 2.0 * float(VC.score_bound(mfma_mode, Q, K).max()))      # of an nll: twice the score bound
            nll.append(r['nll'])
            rank.append(r['rank'])
    want = word_prediction_metrics(np.concatenate(nll), np.concatenate(rank), ks=(1, 5, 10))
    assert m['tokens'] == want['tokens'] == 41 and m['out_of_range'] == 0
    assert abs(m['nll'] - want['nll']) <= bound and abs(m['perplexity'] - want['perplexity']) <= 2 * bound * want['perplexity']
    if close == 0:                                           # every target further than the score bound from its neighbours: the same ranks
        assert m['acc@k'] == want['acc@k'] and abs(m['mrr'] - want['mrr']) <= 1e-12
    else:
        assert all(abs(m['acc@k'][k] - want['acc@k'][k]) <= close / 41.0 for k in (1, 5, 10))
