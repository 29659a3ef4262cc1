"""Host side of cliora_amd.phrases against what the reference's phrase scripts computed and wrote (tests/golden/phrase_embed.npz):
the span tables of the four modes, the phrase ids and the neighbour filter restated in numpy, the reference's assertion, and the
two writers byte for byte.  No GPU: the device's gather is restated on the host from the fixture's charts."""
import io
import os

import numpy as np
import pytest
import torch

from conftest import load_golden


def _fixture():
    return load_golden('phrase_embed.npz')


def idx2word(g):
    return {i: 'w%d' % i for i in range(g['meta']['V'])}


def _tree(t):
    return t if not isinstance(t, list) else tuple(_tree(c) for c in t)


def batch_maps(g):
    meta = g['meta']
    out = []
    for bi, (B, L) in enumerate(meta['shapes']):
        f16 = g['b%d__obj_feats' % bi]
        feats = np.zeros(f16.shape[:2] + (meta['feat'],), dtype=np.float32)
        feats[:, :, :meta['feat_cols']] = f16.astype(np.float32)
        ents = [[tuple(e) if e is not None else None for e in lst] for lst in meta['entity_labels'][bi]]
        out.append(dict(sentences=torch.from_numpy(g['b%d__sentences' % bi]), obj_feats=torch.from_numpy(feats),
                        example_ids=meta['example_ids'][bi], entity_labels=ents, trees=[_tree(t) for t in meta['trees'][bi]]))
    return out


def latent_trees(g, bi):
    from cliora_amd.diora import DioraBase
    spans = g['meta']['latent_spans'][bi]
    return None if spans is None else DioraBase.trees_from_spans(np.array(spans, dtype=np.int32))


def parse_neighbour_lines(text):
    """[query] / rank lines -> tuples of their fields."""
    out = []
    for ln in text.splitlines():
        if ln.startswith('[query]'):
            ex, ph = ln[len('[query] example_id='):].split(' phrase=', 1)
            out.append(('query', None, ex, ph))
        else:
            head, rest = ln.split(' example_id=', 1)
            ex, ph = rest.split(' phrase=', 1)
            rank, score = head.split(' ')
            out.append((rank, score, ex, ph))
    return out


def _offset(L, size):
    C = L * (L + 1) // 2
    n = L - size + 1
    return C - n * (n + 1) // 2


def host_set(g, mode, normalize=False):
    """A PhraseSet filled on the host: the rows of every batch by the library's span rules, the vectors by numpy indexing of the
    fixture's charts (float32 normalisation as the reference's faiss.normalize_L2 does it)."""
    from cliora_amd import phrases as P
    ps = P.PhraseSet()
    vecs = []
    for bi, bm in enumerate(batch_maps(g)):
        B, L = bm['sentences'].shape
        if L <= 2:
            continue
        sent = bm['sentences'].tolist()
        if mode == 'entities':
            rows = P.entity_rows(bm['entity_labels'])
        elif mode == 'given':
            rows = P.tree_rows(bm['trees'], sent, idx2word(g))
        elif mode == 'latent':
            rows = P.tree_rows(latent_trees(g, bi), sent, idx2word(g))
        else:
            rows = P.all_cell_rows(B, L)
        ih, oh = g['b%d__inside_h' % bi], g['b%d__outside_h' % bi]
        bidx = [r[0] for r in rows]
        cidx = [_offset(L, r[2]) + r[1] for r in rows]
        vecs.append(np.concatenate([ih[bidx, cidx], oh[bidx, cidx]], 1).reshape(len(rows), -1))
        ps._record(rows, sent, bm['example_ids'])
    x = np.concatenate(vecs, 0).astype(np.float32)
    if normalize:
        nr = np.sqrt(np.sum(x * x, axis=1, dtype=np.float32)).astype(np.float32)
        x[nr > 0] *= (np.float32(1) / nr[nr > 0])[:, None]
    ps.dim = x.shape[1] // 2
    ps._buf = torch.from_numpy(x)
    return ps


def _csv_rows(g, key):
    return bytes(g[key + '__csv']).decode().splitlines()[1:]


@pytest.mark.parametrize('mode', ['given', 'latent', 'all-spans'])
def test_span_tables_are_the_reference_rows(mode):
    g = _fixture()
    ps = host_set(g, mode)
    got = ['%s,%d,%d' % r for r in zip(ps.example_ids, ps.positions, ps.sizes)]
    assert got == _csv_rows(g, mode.replace('-', '_'))


def test_entity_table_is_the_reference_queries():
    g = _fixture()
    ps = host_set(g, 'entities')
    w = idx2word(g)
    got = [('query', None, e, ' '.join(w[t] for t in p)) for e, p in zip(ps.example_ids, ps.phrases)]
    want = [r for r in parse_neighbour_lines(g['meta']['neighbour_text']) if r[0] == 'query']
    assert got == want
    assert all(s >= 2 for s in ps.sizes)
    assert len(ps) == len(g['nn_I'])


def test_entity_rows_skip_none_and_short():
    from cliora_amd.phrases import entity_rows
    ents = [[('a', 0, 3), None, ('b', 1, 1)], [], [None, ('c', 2, 2)]]
    assert entity_rows(ents) == [(0, 0, 3, 'a'), (2, 2, 2, 'c')]
    assert entity_rows(ents, min_size=1) == [(0, 0, 3, 'a'), (0, 1, 1, 'b'), (2, 2, 2, 'c')]


def test_tree_to_spans_and_postprocess():
    from cliora_amd.phrases import tree_rows, tree_to_spans
    assert tree_to_spans((('a', 'b'), ('c', ('d', 'e')))) == [(0, 2), (3, 2), (2, 3), (0, 5)]
    assert tree_to_spans([['a'], ['b', 'c']]) == [(1, 2), (0, 3)]          # a single-word node counts as the word
    w = {1: 'x', 2: 'y', 3: 'z', 4: '.'}
    tree = ((0, 1), (2, 3))
    assert tree_rows([tree], [[1, 2, 3, 4]], w) == [(0, 0, 2, None), (0, 2, 2, None), (0, 0, 4, None)]
    # postprocess: the final '.' leaves its subtree and is re-attached at the top
    assert tree_rows([tree], [[1, 2, 3, 4]], w, postprocess=True) == [(0, 0, 2, None), (0, 0, 3, None), (0, 0, 4, None)]


def test_all_spans_order():
    from cliora_amd.phrases import all_cell_rows
    rows = all_cell_rows(2, 3)
    assert [(b, p, s) for b, p, s, _ in rows][:6] == [(0, 0, 1), (0, 1, 1), (0, 2, 1), (0, 0, 2), (0, 1, 2), (0, 0, 3)]
    assert len(rows) == 12


def test_skipped_batches():
    from cliora_amd.phrases import PhraseSet
    ps = PhraseSet()
    short = dict(sentences=torch.zeros(3, 2, dtype=torch.long), example_ids=list('abc'), entity_labels=[[('x', 0, 2)]] * 3)
    assert ps.add_chart(None, None, short, 'entities') is None
    empty = dict(sentences=torch.zeros(2, 5, dtype=torch.long), example_ids=list('ab'), entity_labels=[[None], []])
    assert ps.add_chart(None, None, empty, 'entities') is None          # the reference crashes on this batch
    with pytest.raises(ValueError):
        ps.add_chart(None, None, dict(empty, sentences=torch.zeros(2, 5, dtype=torch.long)), 'latent')
    assert len(ps) == 0


def test_phrase_ids_and_filter_rule_in_numpy():
    """The kept neighbours of the fixture from its normalised vectors: fp64 scores, (-score, index) order, then the filter."""
    g = _fixture()
    meta = g['meta']
    ps = host_set(g, 'entities', normalize=True)
    first = {}
    assert ps.phrase_ids == [first.setdefault(p, len(first)) for p in ps.phrases]
    x = ps.vectors.numpy().astype(np.float64)
    s = x @ x.T
    ex = np.array([hash(e) for e in ps.example_ids])
    ph = np.array(ps.phrase_ids)
    I = np.full((len(x), meta['k_candidates']), -1)
    for i in range(len(x)):
        order = np.lexsort((np.arange(len(x)), -s[i]))[:meta['k_candidates']]
        I[i, :len(order)] = order
    kept = []
    for i in range(len(x)):
        row = [j for j in I[i] if j >= 0 and ex[j] != ex[i] and ph[j] != ph[i]][:meta['k_top']]
        kept.append(row)
    assert kept == g['nn_I'].tolist()


def test_too_few_candidates_is_the_reference_assertion():
    from cliora_amd.phrases import check_counts
    check_counts(np.array([3, 3]), 3)
    with pytest.raises(AssertionError, match='Did not find enough valid candidates.'):
        check_counts(np.array([3, 2]), 3)


def test_write_neighbours_is_byte_identical():
    from cliora_amd.phrases import Neighbours, write_neighbours
    g = _fixture()
    ps = host_set(g, 'entities', normalize=True)
    buf = io.StringIO()
    write_neighbours(buf, ps, Neighbours(g['nn_I'], g['nn_D']), idx2word(g))
    assert buf.getvalue() == g['meta']['neighbour_text']


@pytest.mark.parametrize('mode', ['given', 'latent', 'all-spans'])
def test_write_vectors_is_byte_identical(mode, tmp_path):
    from cliora_amd.phrases import write_vectors
    g = _fixture()
    ps = host_set(g, mode)
    write_vectors(str(tmp_path), ps)
    key = mode.replace('-', '_')
    assert open(os.path.join(str(tmp_path), 'vectors.csv'), 'rb').read() == bytes(g[key + '__csv'])
    assert open(os.path.join(str(tmp_path), 'vectors.npy'), 'rb').read() == bytes(g[key + '__npy'])
