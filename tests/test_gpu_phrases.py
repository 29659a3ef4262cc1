"""cliora_phrase_gather, cliora_knn_ip and cliora_knn_filter on the GPU: the gather against torch indexing of the chart, the search
against an fp64 oracle and its determinism contract, and the whole pipeline against what the reference's phrase scripts computed
(tests/golden/phrase_embed.npz)."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = {'bf16x3': 2e-5, 'f32': 1e-6}


def _eps(mode, D):
    """Score tolerance against fp64.  In the f32 mode the products are exact and the error is that of an fp32 sum over D terms,
    which for unit rows grows as sqrt(D): 1e-6 up to D = 256, then with sqrt(D / 256) (measured 1.3e-6 at D = 800)."""
    return EPS[mode] * (max(1.0, (D / 256.0) ** 0.5) if mode == 'f32' else 1.0)


def _offset(L, size):
    C = L * (L + 1) // 2
    n = L - size + 1
    return C - n * (n + 1) // 2


# ---- gather ---------------------------------------------------------------------------------------------------------------
def _chart(B, L, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = L * (L + 1) // 2
    return torch.randn(B, C, D, generator=g).cuda(), torch.randn(B, C, D, generator=g).cuda()


def _rows(B, L, n, seed=1):
    rs = np.random.RandomState(seed)
    rows = []
    for _ in range(n):
        b = rs.randint(B)
        size = rs.randint(1, L + 1)
        rows.append((b, rs.randint(0, L - size + 1), size, None))
    return rows


def test_gather_is_torch_indexing():
    from cliora_amd.phrases import PhraseSet
    B, L, D = 5, 9, 48
    ih, oh = _chart(B, L, D)
    rows = _rows(B, L, 70)
    ps = PhraseSet()
    ps.add_rows(ih, oh, rows[:30], torch.zeros(B, L, dtype=torch.long), ['e%d' % b for b in range(B)])
    ps.add_rows(ih, oh, rows[30:], torch.zeros(B, L, dtype=torch.long), ['e%d' % b for b in range(B)])      # appended at a row offset
    bi = [r[0] for r in rows]
    ci = [_offset(L, r[2]) + r[1] for r in rows]
    want = torch.cat([ih[bi, ci], oh[bi, ci]], 1)
    assert torch.equal(ps.vectors, want)
    assert ps.batch_rows == [30, 40]


def test_gather_normalised_rows_and_zero_rows():
    from cliora_amd.phrases import PhraseSet
    B, L, D = 3, 6, 100
    ih, oh = _chart(B, L, D, seed=3)
    ih[1, 4].zero_()
    oh[1, 4].zero_()
    rows = _rows(B, L, 40, seed=4) + [(1, 4, 1, None)]                  # cell 4 of level 0: the zero row
    ps = PhraseSet()
    ps.add_rows(ih, oh, rows, torch.zeros(B, L, dtype=torch.long), list('abc'), normalize=True)
    bi = [r[0] for r in rows]
    ci = [_offset(L, r[2]) + r[1] for r in rows]
    raw = torch.cat([ih[bi, ci], oh[bi, ci]], 1).double().cpu()
    n = raw.norm(dim=1, keepdim=True)
    want = torch.where(n > 0, raw / n.clamp_min(1e-300), raw).float()
    got = ps.vectors.cpu()
    ulp = (torch.nextafter(want.abs(), torch.tensor(float('inf'))) - want.abs())
    assert bool(((got - want).abs() <= 2 * ulp).all())
    assert bool((got[-1] == 0).all())


def test_gather_strided_chart_views():
    from cliora_amd.phrases import PhraseSet
    B, L, D = 4, 7, 32
    C = L * (L + 1) // 2
    big = torch.randn(B, 2 * C, D + 16, device='cuda')
    ih = big[:, ::2, 8:8 + D]                     # cell stride 2 (D + 16), sentence stride 2C (D + 16)
    oh = torch.randn(C, B, D, device='cuda').transpose(0, 1)
    assert not ih.is_contiguous() and not oh.is_contiguous()
    rows = _rows(B, L, 25, seed=5)
    ps = PhraseSet()
    ps.add_rows(ih, oh, rows, torch.zeros(B, L, dtype=torch.long), list('abcd'))
    bi = [r[0] for r in rows]
    ci = [_offset(L, r[2]) + r[1] for r in rows]
    assert torch.equal(ps.vectors, torch.cat([ih[bi, ci], oh[bi, ci]], 1))


@pytest.mark.parametrize('bad', [(0, 0, 0), (0, 3, 3), (4, 0, 2), (-1, 0, 2), (0, -1, 2)])
def test_gather_refuses_rows_outside_the_chart(bad):
    from cliora_amd import _lib
    from cliora_amd.phrases import PhraseSet
    B, L, D = 4, 5, 16
    ih, oh = _chart(B, L, D)
    ps = PhraseSet()
    with pytest.raises(_lib.ChartLibError, match='outside'):
        ps.add_rows(ih, oh, [(0, 0, 2, None), bad + (None,)], torch.zeros(B, L, dtype=torch.long), list('abcd'))


# ---- search against fp64 ---------------------------------------------------------------------------------------------------
def _check_search(q, keys, k, D, I, eps, ids_equal=None):
    """The contract against fp64 scores: ids unique and valid, D non-increasing, |D - s64(I)| <= eps, nothing left out beats the
    lowest returned score by more than 2 eps, equal D in ascending I.  `ids_equal`: the oracle's ids must match exactly."""
    nq, nk = q.shape[0], keys.shape[0]
    Dh, Ih = D.cpu().double(), I.cpu()
    s64 = (q.double() @ keys.double().T).cpu() if nk else torch.zeros(nq, 0, dtype=torch.float64)
    m = min(k, nk)
    assert bool((Ih[:, m:] == -1).all()) and bool((Dh[:, m:] == float('-inf')).all())
    Iv, Dv = Ih[:, :m], Dh[:, :m]
    assert bool(((Iv >= 0) & (Iv < nk)).all())
    if m:
        assert all(len(set(r)) == m for r in Iv.tolist())
        assert bool((Dv[:, 1:] <= Dv[:, :-1]).all())
        got = s64.gather(1, Iv)
        assert float((Dv - got).abs().max()) <= eps, float((Dv - got).abs().max())
        tie = Dv[:, 1:] == Dv[:, :-1]
        assert bool((Iv[:, 1:] > Iv[:, :-1])[tie].all())
        if m < nk:
            out = s64.scatter(1, Iv, float('-inf'))
            assert bool((out.max(1).values <= Dv[:, -1] + 2 * eps).all())
    if ids_equal is not None:
        want = torch.sort(s64, dim=1, descending=True, stable=True).indices[:, :m]
        assert torch.equal(Iv, want)


@pytest.mark.parametrize('N', [1, 7, 1000])
@pytest.mark.parametrize('D', [32, 100, 800, 1324])
@pytest.mark.parametrize('k', [1, 3, 100, 128])
def test_search_against_fp64(mfma_mode, N, D, k):
    from cliora_amd.phrases import knn_ip
    g = torch.Generator().manual_seed(N * 7 + D + k)
    x = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).cuda()
    Dv, Iv = knn_ip(x, x, k)
    _check_search(x, x, k, Dv, Iv, _eps(mfma_mode, D))


def test_search_well_separated_ids_equal_the_oracle(mfma_mode):
    """Scores on a 1/64 grid far apart from each other: the ids must be the oracle's exactly."""
    from cliora_amd.phrases import knn_ip
    g = torch.Generator().manual_seed(5)
    nq, nk, D, k = 40, 3000, 64, 50
    keys = torch.zeros(nk, D)
    keys[:, 0] = torch.randperm(nk, generator=g).float() / 64.0          # distinct multiples of 1/64: scores exact in both modes
    keys[:, 1:] = (torch.randint(-4, 5, (nk, D - 1), generator=g).float() / 1024.0)
    q = torch.zeros(nq, D)
    q[:, 0] = 1.0
    Dv, Iv = knn_ip(q.cuda(), keys.cuda(), k)
    want = torch.argsort(keys[:, 0], descending=True)[:k]
    assert torch.equal(Iv.cpu(), want.expand(nq, k))
    _check_search(q, keys, k, Dv, Iv, _eps(mfma_mode, D), ids_equal=True)


def test_search_large_against_chunked_fp64(mfma_mode):
    from cliora_amd.phrases import knn_ip
    g = torch.Generator().manual_seed(9)
    N, D, k = 33000, 800, 100
    x = torch.nn.functional.normalize(torch.randn(N, D, generator=g), dim=1).cuda()
    Dv, Iv = knn_ip(x, x, k)
    eps = _eps(mfma_mode, D)
    xd = x.double()
    for r0 in range(0, N, 4096):
        s = xd[r0:r0 + 4096] @ xd.T
        Ir, Dr = Iv[r0:r0 + 4096], Dv[r0:r0 + 4096].double()
        assert bool((Dr[:, 1:] <= Dr[:, :-1]).all())
        got = s.gather(1, Ir)
        assert float((Dr - got).abs().max()) <= eps
        kth = s.topk(k, 1).values[:, -1]
        assert bool((kth <= Dr[:, -1] + 2 * eps).all())
        assert bool((Ir[:, 0] == torch.arange(r0, r0 + Ir.shape[0], device='cuda')).all())      # each row finds itself first
    single = knn_ip(x[12345:12346], x, k)
    assert torch.equal(single[0], Dv[12345:12346]) and torch.equal(single[1], Iv[12345:12346])
    again = knn_ip(x, x, k)
    assert torch.equal(again[0], Dv) and torch.equal(again[1], Iv)


# ---- search edge cases ---------------------------------------------------------------------------------------------------------
def test_search_duplicates_come_in_index_order(mfma_mode):
    from cliora_amd.phrases import knn_ip
    g = torch.Generator().manual_seed(2)
    keys = torch.randn(300, 40, generator=g)
    keys[[17, 90, 250, 299]] = keys[5].clone()
    q = keys[5:6].clone() * 2
    Dv, Iv = knn_ip(q.cuda(), keys.cuda(), 5)
    assert Iv[0].tolist() == [5, 17, 90, 250, 299]
    assert len(set(Dv[0].tolist())) == 1


def test_search_pads_past_the_keys_and_empty_index(mfma_mode):
    from cliora_amd.phrases import PhraseIndex, knn_ip
    x = torch.randn(6, 24, device='cuda')
    Dv, Iv = knn_ip(x, x[:4], 10)
    assert bool((Iv[:, 4:] == -1).all()) and bool(torch.isneginf(Dv[:, 4:]).all())
    assert sorted(Iv[0, :4].tolist()) == [0, 1, 2, 3]
    idx = PhraseIndex(24)
    De, Ie = idx.search(x, 3)
    assert bool((Ie == -1).all()) and bool(torch.isneginf(De).all())


def test_search_nan_row_ranks_last(mfma_mode):
    from cliora_amd.phrases import knn_ip
    g = torch.Generator().manual_seed(4)
    keys = torch.randn(50, 32, generator=g)
    keys[7, 3] = float('nan')
    q = torch.randn(3, 32, generator=g)
    Dv, Iv = knn_ip(q.cuda(), keys.cuda(), 50)
    assert bool((Iv[:, -1] == 7).all()) and bool(torch.isnan(Dv[:, -1]).all())
    assert not bool(torch.isnan(Dv[:, :-1]).any())
    qn = q.clone()
    qn[1, 0] = float('nan')                          # a NaN query: every score NaN, ids in index order
    Dn, In = knn_ip(qn.cuda(), keys.cuda(), 10)
    assert In[1].tolist() == list(range(10)) and bool(torch.isnan(Dn[1]).all())
    assert torch.equal(In[0], Iv[0, :10])


def test_search_refuses_k_above_128():
    from cliora_amd import _lib
    from cliora_amd.phrases import knn_ip
    x = torch.randn(4, 16, device='cuda')
    with pytest.raises(ValueError):
        knn_ip(x, x, 129)
    lib = _lib.lib()
    assert lib.cliora_knn_ip(4, 4, 16, 129, x.data_ptr(), 16, x.data_ptr(), 16, x.data_ptr(), 129, x.data_ptr(), 129,
                             x.data_ptr(), 1 << 20, None) == -1
    assert b'129' in lib.cliora_last_error()


def test_filter_rule():
    from cliora_amd.phrases import knn_filter
    I = torch.tensor([[0, 3, 1, 2, -1, 4], [1, 0, 2, 3, 4, -1], [2, -1, -1, -1, -1, -1]], dtype=torch.int64, device='cuda')
    D = torch.arange(18, dtype=torch.float32, device='cuda').view(3, 6).neg()
    ex = torch.tensor([0, 0, 1, 2, 3], dtype=torch.int32, device='cuda')
    ph = torch.tensor([0, 1, 2, 0, 4], dtype=torch.int32, device='cuda')
    Io, Do, cnt = knn_filter(I, D, ex, ph, 2)
    assert Io.tolist() == [[2, 4], [2, 3], [-1, -1]]      # query 0: 0 same example, 3 same phrase, 1 same example
    assert cnt.tolist() == [2, 2, 0]
    assert Do[0].tolist() == [-3.0, -5.0]


# ---- end to end against the reference -------------------------------------------------------------------------------------
def _fixture():
    return load_golden('phrase_embed.npz')


def _batches(g):
    from test_phrases_cpu import batch_maps
    return batch_maps(g)


def _charts(g, bi):
    return torch.from_numpy(g['b%d__inside_h' % bi]).cuda(), torch.from_numpy(g['b%d__outside_h' % bi]).cuda()


def _pset(g, mode, normalize):
    from cliora_amd.phrases import PhraseSet
    from test_phrases_cpu import idx2word, latent_trees
    ps = PhraseSet()
    for bi, bm in enumerate(_batches(g)):
        if bm['sentences'].shape[1] <= 2:
            continue
        ih, oh = _charts(g, bi)
        ps.add_chart(ih, oh, bm, mode, trees=latent_trees(g, bi), idx2word=idx2word(g), normalize=normalize)
    return ps


def test_neighbours_match_the_reference(mfma_mode):
    from cliora_amd.phrases import nearest_phrases, write_neighbours
    from test_phrases_cpu import idx2word, parse_neighbour_lines
    g = _fixture()
    meta = g['meta']
    ps = _pset(g, 'entities', True)
    nn = nearest_phrases(ps, k_candidates=meta['k_candidates'], k_top=meta['k_top'])
    assert nn.I.tolist() == g['nn_I'].tolist()
    assert float(np.abs(nn.D - g['nn_D']).max()) <= EPS[mfma_mode]
    buf = io.StringIO()
    write_neighbours(buf, ps, nn, idx2word(g))
    got, want = parse_neighbour_lines(buf.getvalue()), parse_neighbour_lines(meta['neighbour_text'])
    assert [(a[0], a[2:]) for a in got] == [(b[0], b[2:]) for b in want]        # everything but the printed score


@pytest.mark.parametrize('mode', ['given', 'all-spans'])
def test_vectors_files_byte_identical(mode, tmp_path):
    from cliora_amd.phrases import write_vectors
    g = _fixture()
    ps = _pset(g, mode, False)
    write_vectors(str(tmp_path), ps)
    key = mode.replace('-', '_')
    assert open(os.path.join(str(tmp_path), 'vectors.csv'), 'rb').read() == bytes(g[key + '__csv'])
    assert open(os.path.join(str(tmp_path), 'vectors.npy'), 'rb').read() == bytes(g[key + '__npy'])


def test_latent_with_the_fixture_weights(mfma_mode, tmp_path):
    """The net itself: harness.Net with the fixture's weights, its own chart and CKY trees on the device."""
    from cliora_amd import harness as H
    from cliora_amd.phrases import embed_phrases, write_vectors
    from test_phrases_cpu import idx2word
    g = _fixture()
    m = g['meta']
    net = H.build_net(m['D'], torch.nn.Embedding(m['V'], m['E']), obj_feats=True, img_dim=m['feat'], k_neg=m['K'], vg_loss=True,
                      use_contr=True, vl_margin=0.2, alpha_contr=1.0, alpha_vg=1.0)
    sd = net.state_dict()
    for k in sd:
        sd[k] = torch.from_numpy(g['param__' + k.replace('.', '__')].copy())
    net.load_state_dict(sd)
    net.cuda()
    bms = []
    for bm in _batches(g):
        bm = dict(bm)
        bm['sentences'] = bm['sentences'].cuda()
        bm['obj_feats'] = bm['obj_feats'].cuda()
        bms.append(bm)
    ps = embed_phrases(net, bms, 'latent', idx2word=idx2word(g))
    write_vectors(str(tmp_path), ps)
    assert open(os.path.join(str(tmp_path), 'vectors.csv'), 'rb').read() == bytes(g['latent__csv'])
    want = np.loadtxt(io.BytesIO(bytes(g['latent__npy'])), dtype=np.float64)
    got = ps.vectors.cpu().double().numpy()
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= 1e-4
