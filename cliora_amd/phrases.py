"""Phrase vectors and their nearest neighbours on the device, as the reference's two phrase scripts produce them
(cliora/scripts/phrase_embed.py:run, phrase_embed_simple.py:run).

A phrase's vector is ``[inside_h[b, cell] | outside_h[b, cell]]`` of its chart cell.  The reference copies every chart to the host,
indexes it there and searches with ``faiss.IndexFlatIP``.  Here one gather launch per batch appends a batch's vectors to a device
matrix (include/cliora_chart.h: cliora_phrase_gather), the search is the fused MFMA scores + top-k of cliora_knn_ip, which never
writes the score matrix, and the reference's post-search filter is cliora_knn_filter.  What stays on the host is the bookkeeping
(example ids, positions, token tuples, the span order of the trees) and the writers, which produce the reference's bytes.

    from cliora_amd.phrases import embed_phrases, nearest_phrases, write_neighbours
    pset = embed_phrases(net, batches, 'entities', normalize=True)      # net: harness.Net; batches: batch_map dicts
    nn = nearest_phrases(pset, k_candidates=100, k_top=3)
    write_neighbours(sys.stdout, pset, nn, idx2word)
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import ptr_or_null as _p, stream as _stream
from .interchange import postprocess as _postprocess, replace_leaves

MODES = ('entities', 'given', 'latent', 'all-spans')
MAX_K = 128


# ---- spans of one batch ---------------------------------------------------------------------------------------------
def tree_to_spans(tree):
    """(pos, size) of every node of a tree of words with two or more children, children before parents: phrase_embed_simple.py:62-76
    (a node holding a single word counts as that word; other single-child nodes pass through)."""
    spans = []

    def helper(tr, pos=0):
        if isinstance(tr, str) or len(tr) == 1 and isinstance(tr[0], str):
            return 1
        if len(tr) == 1:
            return helper(tr[0], pos)
        size = 0
        for x in tr:
            size += helper(x, pos + size)
        spans.append((pos, size))
        return size

    helper(tree)
    return spans


def entity_rows(entity_labels, min_size=2):
    """(sentence, pos, size, label) of batch_map['entity_labels'] (phrase_embed.py:58-76, 209-213): (label, pos, size) entries,
    ``None`` entries skipped, sizes below `min_size` dropped."""
    rows = []
    for i, lst in enumerate(entity_labels):
        for el in lst:
            if el is None:
                continue
            label, pos, size = el[0], el[1], el[2]
            if size >= min_size:
                rows.append((i, int(pos), int(size), label))
    return rows


def tree_rows(trees, sentences, idx2word=None, postprocess=False):
    """(sentence, pos, size, None) per span of each tree, in the order of phrase_embed_simple.py:174-181: leaves replaced by the
    sentence's words, ``postprocess`` re-attaches a final punctuation mark at the top, then tree_to_spans."""
    rows = []
    for ii, tr in enumerate(trees):
        words = [idx2word[i] if idx2word is not None else str(i) for i in sentences[ii]]
        tr = replace_leaves(tr, words)
        if postprocess:
            tr = _postprocess(tr, words)
        rows.extend((ii, pos, size, None) for pos, size in tree_to_spans(tr))
    return rows


def all_cell_rows(B, L):
    """Every cell, sentence-major, then level, then position (phrase_embed_simple.py:243-257: inside_h.view(-1, D))."""
    return [(b, pos, level + 1, None) for b in range(B) for level in range(L) for pos in range(L - level)]


# ---- the phrase set ----------------------------------------------------------------------------------------------------
class PhraseSet(object):
    """Phrase vectors on the device and what the writers need on the host.

    vectors: (N, 2D) fp32 CUDA tensor (a view of a buffer that grows by doubling); example_ids, positions, sizes, labels,
    phrases (token-id tuples) and phrase_ids (one integer per distinct tuple, in order of first appearance): host lists of N;
    batch_rows: the rows each added batch contributed (vectors.npy is written per batch, as the reference does)."""

    def __init__(self, dim=None, device=None):
        self.dim = dim
        self.device = torch.device(device) if device is not None else None
        self._buf = None
        self.n = 0
        self.example_ids, self.positions, self.sizes, self.labels, self.phrases, self.phrase_ids = [], [], [], [], [], []
        self.batch_rows = []
        self._pid = {}

    @property
    def vectors(self):
        if self._buf is None:
            return torch.empty((0, 2 * (self.dim or 0)), dtype=torch.float32, device=self.device or 'cuda')
        return self._buf[:self.n]

    def __len__(self):
        return self.n

    def _reserve(self, n, device):
        if self._buf is not None and self._buf.shape[0] >= n:
            return
        cap = max(n, 1024, 2 * (self._buf.shape[0] if self._buf is not None else 0))
        buf = torch.empty((cap, 2 * self.dim), dtype=torch.float32, device=device)
        if self._buf is not None and self.n:
            buf[:self.n].copy_(self._buf[:self.n])
        self._buf = buf

    def add_rows(self, inside_h, outside_h, rows, sentences, example_ids, normalize=False):
        """Append one batch: rows (sentence, pos, size, label) of the (B, C, D) charts inside_h / outside_h (fp32 CUDA, any sentence /
        cell strides, unit stride along D).  One gather launch; a row outside the chart raises."""
        B, Cc, D = inside_h.shape
        L = int(round((np.sqrt(8 * Cc + 1) - 1) / 2))
        if L * (L + 1) // 2 != Cc or outside_h.shape != inside_h.shape:
            raise ValueError('charts %s / %s are not (B, L(L+1)/2, D)' % (tuple(inside_h.shape), tuple(outside_h.shape)))
        if inside_h.dtype != torch.float32 or outside_h.dtype != torch.float32 or inside_h.stride(2) != 1 or outside_h.stride(2) != 1:
            raise ValueError('charts must be fp32 with unit stride along D')
        if self.dim is None:
            self.dim = D
        if D != self.dim:
            raise ValueError('chart width %d, phrase set width %d' % (D, self.dim))
        dev = inside_h.device
        if self.device is None:
            self.device = dev
        N = len(rows)
        with torch.cuda.device(dev):
            self._reserve(self.n + N, dev)
            tab = torch.from_numpy(np.array([r[:3] for r in rows], dtype=np.int32).reshape(-1, 3)).to(dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call('cliora_phrase_gather', B, L, D, _p(inside_h), inside_h.stride(0), inside_h.stride(1), _p(outside_h),
                      outside_h.stride(0), outside_h.stride(1), N, _p(tab), int(bool(normalize)), _p(self._buf),
                      self._buf.stride(0), self.n, _p(status), _stream())
            bad = int(status.item()) if N else 0
        if bad:
            raise _lib.ChartLibError('cliora_phrase_gather rejected %d phrase(s) outside their sentence' % bad)
        self._record(rows, sentences, example_ids)
        return N

    def _record(self, rows, sentences, example_ids):
        """The host lists of rows whose vectors were just appended."""
        sent = sentences.tolist() if hasattr(sentences, 'tolist') else [list(s) for s in sentences]
        for b, pos, size, label in rows:
            tok = tuple(sent[b][pos:pos + size])
            self.example_ids.append(example_ids[b])
            self.positions.append(pos)
            self.sizes.append(size)
            self.labels.append(label)
            self.phrases.append(tok)
            self.phrase_ids.append(self._pid.setdefault(tok, len(self._pid)))
        self.batch_rows.append(len(rows))
        self.n += len(rows)

    def add_chart(self, inside_h, outside_h, batch_map, mode, trees=None, idx2word=None, normalize=False, min_size=2, postprocess=False):
        """One batch whose chart is computed: its rows by `mode` (MODES), then the gather.  'latent' needs the batch's CKY `trees`
        (nested tuples of word positions, DioraBase.trees_from_spans); 'given' reads batch_map['trees'].  Returns the rows added,
        or None when the batch is skipped: a sentence length <= 2 (both scripts), or 'entities' with no entity labels at all (the
        reference crashes there: get_cell_index returns two values to a four-way unpack)."""
        sentences = batch_map['sentences']
        B, L = int(sentences.shape[0]), int(sentences.shape[1])
        if L <= 2:
            return None
        sent = sentences.tolist()
        if mode == 'entities':
            if not any(el is not None for lst in batch_map['entity_labels'] for el in lst):
                return None
            rows = entity_rows(batch_map['entity_labels'], min_size)
        elif mode == 'given':
            rows = tree_rows(batch_map['trees'], sent, idx2word, postprocess)
        elif mode == 'latent':
            if trees is None:
                raise ValueError("mode 'latent' needs the batch's CKY trees")
            rows = tree_rows(trees, sent, idx2word, postprocess)
        elif mode == 'all-spans':
            rows = all_cell_rows(B, L)
        else:
            raise ValueError('mode %r: one of %s' % (mode, ', '.join(MODES)))
        return self.add_rows(inside_h, outside_h, rows, sent, batch_map['example_ids'], normalize)


def embed_phrases(net, batches, mode, normalize=False, min_size=2, postprocess=False, idx2word=None):
    """phrase_embed.py:run (mode 'entities', lines 187-226) / phrase_embed_simple.py:run ('given', 'latent', 'all-spans', lines
    231-288) on a harness.Net: eval mode, outside pass on, one forward without losses and one gather per batch.  Batches with
    sentences of length <= 2 are skipped, as in both scripts; so is an 'entities' batch without entity labels (the reference
    crashes on it).  `idx2word` gives the words the trees' postprocessing looks at (ids as strings without it)."""
    if mode not in MODES:
        raise ValueError('mode %r: one of %s' % (mode, ', '.join(MODES)))
    diora = net.diora
    diora.outside = True
    net.eval()
    dev = next(net.parameters()).device
    pset = PhraseSet(device=dev)
    with torch.no_grad():
        for bm in batches:
            sentences = bm['sentences']
            if sentences.shape[1] <= 2:
                continue
            obj = bm.get('obj_feats') if net.obj_feats else None
            net(sentences.to(dev), obj.to(dev) if obj is not None else None, None, compute_loss=False)
            trees = diora.trees_from_spans(diora.cky_spans_device().cpu()) if mode == 'latent' else None
            pset.add_chart(diora.inside_h, diora.outside_h, bm, mode, trees=trees, idx2word=idx2word, normalize=normalize,
                           min_size=min_size, postprocess=postprocess)
    return pset


def embed_phrases_ragged(net, sentences, mode, example_ids=None, entity_labels=None, trees=None, obj_feats=None, normalize=False,
                         min_size=2, postprocess=False, idx2word=None, max_batch=64, max_waste=None, pad_id=0, max_len=64,
                         max_long_batch=8):
    """``embed_phrases`` for sentences of any lengths, given in any order: packed into right-padded charts and run with the outside
    pass made each sentence's own (cliora_amd.ragged.forward_ragged); cliora_phrase_gather addresses a cell by (sentence, pos, size)
    within the padded chart's L, so it reads the padded charts as they are.  -> PhraseSet whose rows follow the caller's order of
    sentences (within a sentence the order of `embed_phrases`), as one batch.

    sentences: lists of token ids; example_ids: one per sentence (default: its index); entity_labels (mode 'entities') / trees
    (mode 'given'): one entry per sentence, as batch_map['entity_labels'][b] / batch_map['trees'][b]; obj_feats: (N, R, img_dim) for a
    CLIORA net.  'all-spans' means the cells of each sentence's own triangle.  Sentences of length <= 2 are skipped, as both scripts
    skip such batches.  Every row must lie inside its sentence (checked on the host).  max_len: the longest sentence taken, 64 or up to
    128; a pack topped by a sentence of more than 64 words then holds at most `max_long_batch` sentences (``ragged.forward_ragged``)."""
    from . import ragged
    if mode not in MODES:
        raise ValueError('mode %r: one of %s' % (mode, ', '.join(MODES)))
    if mode == 'entities' and entity_labels is None:
        raise ValueError("mode 'entities' needs entity_labels")
    if mode == 'given' and trees is None:
        raise ValueError("mode 'given' needs the sentences' trees")
    diora = net.diora
    dev = next(net.parameters()).device
    keep = [i for i, s_ in enumerate(sentences) if len(s_) > 2]
    sents = [list(sentences[i]) for i in keep]
    feats = obj_feats[torch.as_tensor(keep, dtype=torch.int64)] if obj_feats is not None else None
    ids = list(example_ids) if example_ids is not None else list(range(len(sentences)))
    parts = {}                          # position in `sentences` -> (its rows with the sentence renumbered, its vectors on the device)

    def per_pack(idx, lens, d):
        local = [sents[j] for j in idx]
        if mode == 'entities':
            rows = entity_rows([entity_labels[keep[j]] for j in idx], min_size)
        elif mode == 'given':
            rows = tree_rows([trees[keep[j]] for j in idx], local, idx2word, postprocess)
        elif mode == 'latent':
            spans, status = ragged.cky_spans_ragged(d, lens)
            host = torch.cat([spans.reshape(-1), status, d._ragged_status]).cpu().numpy()
            if host[-2:].any():
                raise _lib.ChartLibError('the padded chart rejected %d sentence length(s)' % int(host[-2:].max()))
            sp = host[:-2].reshape(spans.shape)
            cky = [d.trees_from_spans(sp[b:b + 1, :len(local[b]) - 1])[0] for b in range(len(idx))]
            rows = tree_rows(cky, local, idx2word, postprocess)
        else:
            rows = [(b, pos, level + 1, None) for b in range(len(idx)) for level in range(len(local[b]))
                    for pos in range(len(local[b]) - level)]
        for b, pos, size, _ in rows:
            if pos < 0 or size < 1 or pos + size > len(local[b]):
                raise ValueError('phrase (pos %d, size %d) lies outside its sentence of length %d' % (pos, size, len(local[b])))
        ih, oh = d.inside_h, d.outside_h
        B, _, D = ih.shape
        N = len(rows)
        with torch.cuda.device(dev):
            out = torch.empty((N, 2 * D), dtype=torch.float32, device=dev)
            tab = torch.from_numpy(np.array([r[:3] for r in rows], dtype=np.int32).reshape(-1, 3)).to(dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.call('cliora_phrase_gather', B, d._plan.L, D, _p(ih), ih.stride(0), ih.stride(1), _p(oh), oh.stride(0), oh.stride(1), N,
                      _p(tab), int(bool(normalize)), _p(out), out.stride(0), 0, _p(status), _stream())
            bad = torch.stack([status[0], d._ragged_status[0]]).cpu().tolist() if N else [0, int(d._ragged_status.item())]
        if any(bad):
            raise _lib.ChartLibError('the padded chart rejected %d phrase(s) / %d sentence length(s)' % tuple(bad))
        by_sent = {}
        for r, row in enumerate(rows):
            by_sent.setdefault(row[0], []).append(r)
        for b, rr in by_sent.items():
            i = keep[idx[b]]
            parts[i] = ([(i,) + rows[r][1:] for r in rr], out[torch.as_tensor(rr, dtype=torch.int64, device=dev)])

    ragged.forward_ragged(net, sents, obj_feats=feats, per_pack=per_pack, max_batch=max_batch,
                          max_waste=ragged.DEFAULT_MAX_WASTE if max_waste is None else max_waste, pad_id=pad_id, max_len=max_len,
                          max_long_batch=max_long_batch)
    pset = PhraseSet(dim=diora.size, device=dev)
    order = sorted(parts)
    if order:
        all_rows = [r for i in order for r in parts[i][0]]
        with torch.cuda.device(dev):
            pset._reserve(len(all_rows), dev)
            pset._buf[:len(all_rows)].copy_(torch.cat([parts[i][1] for i in order], 0))
        pset._record(all_rows, [list(s_) for s_ in sentences], ids)
    return pset


# ---- search --------------------------------------------------------------------------------------------------------------
def knn_ip(q, keys, k):
    """cliora_knn_ip: (D, I) = faiss.IndexFlatIP search of the rows of q among the rows of keys (fp32 CUDA, unit column stride, any
    row stride); D (nq, k) fp32 descending, I (nq, k) int64, -1 / -inf past the keys.  Uses the library's MFMA mode."""
    if not 1 <= k <= MAX_K:
        raise ValueError('k = %d: cliora_knn_ip supports 1 <= k <= %d' % (k, MAX_K))
    if q.dim() != 2 or keys.dim() != 2 or q.shape[1] != keys.shape[1]:
        raise ValueError('queries %s and keys %s must be (n, D) of one width' % (tuple(q.shape), tuple(keys.shape)))
    for t in (q, keys):
        if t.dtype != torch.float32 or not t.is_cuda or (t.shape[0] > 1 and t.stride(1) != 1):
            raise ValueError('queries and keys must be fp32 CUDA rows with unit stride along D')
    nq, D = q.shape
    nk = keys.shape[0]
    dev = q.device
    with torch.cuda.device(dev):
        Dout = torch.empty((nq, k), dtype=torch.float32, device=dev)
        Iout = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if nq == 0:
            return Dout, Iout
        ws = torch.empty(max(1, _lib.fn('cliora_knn_ip_workspace_bytes')(nq, nk, D, k)), dtype=torch.uint8, device=dev)
        ldq = q.stride(0) if nq > 1 else D
        ldk = keys.stride(0) if nk > 1 else D
        _lib.call('cliora_knn_ip', nq, nk, D, k, _p(q), ldq, _p(keys) if nk else C.c_void_p(0), ldk, _p(Dout), k, _p(Iout), k,
                  _p(ws), ws.numel(), _stream())
    return Dout, Iout


class PhraseIndex(object):
    """The faiss-shaped wrapper of cliora_knn_ip (phrase_embed.py:136-152): ``add(vecs)`` device rows, ``search(q, k) -> (D, I)``."""

    def __init__(self, dim):
        self.dim = dim
        self._parts = []
        self._keys = None

    @property
    def ntotal(self):
        return sum(p.shape[0] for p in self._parts)

    def add(self, vecs):
        if vecs.dim() != 2 or vecs.shape[1] != self.dim:
            raise ValueError('vectors %s, index width %d' % (tuple(vecs.shape), self.dim))
        self._parts.append(vecs)
        self._keys = None

    def keys(self):
        if self._keys is None:
            if not self._parts:
                return None
            self._keys = self._parts[0] if len(self._parts) == 1 else torch.cat(self._parts, 0)
        return self._keys

    def search(self, q, k):
        keys = self.keys()
        if keys is None:
            keys = torch.empty((0, self.dim), dtype=torch.float32, device=q.device)
        return knn_ip(q, keys, k)


class Neighbours(object):
    """Host result of nearest_phrases: I (N, k_top) int64 and D (N, k_top) float32, the kept candidates of every phrase."""

    def __init__(self, I, D):
        self.I, self.D = I, D


def knn_filter(I, D, example_ids, phrase_ids, k_top):
    """cliora_knn_filter on device tensors: (I_out, D_out, count)."""
    nq, kc = I.shape
    dev = I.device
    with torch.cuda.device(dev):
        Io = torch.empty((nq, k_top), dtype=torch.int64, device=dev)
        Do = torch.empty((nq, k_top), dtype=torch.float32, device=dev)
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        _lib.call('cliora_knn_filter', nq, kc, _p(I), I.stride(0) if nq else kc, _p(D), D.stride(0) if nq else kc, _p(example_ids),
                  _p(phrase_ids), example_ids.numel(), k_top, _p(Io), _p(Do), _p(cnt), _stream())
    return Io, Do, cnt


def nearest_phrases(pset, k_candidates=100, k_top=3):
    """phrase_embed.py:232-263: every phrase searched against all of them (the vectors as they are: embed with normalize=True
    for the reference's cosine similarity), then per phrase the first k_top candidates of another example and another token
    tuple.  Raises the reference's assertion when a phrase has fewer."""
    vecs = pset.vectors
    D, I = knn_ip(vecs, vecs, k_candidates)
    ex = {}
    ex_ids = torch.tensor([ex.setdefault(e, len(ex)) for e in pset.example_ids], dtype=torch.int32).to(vecs.device)
    ph_ids = torch.tensor(pset.phrase_ids, dtype=torch.int32).to(vecs.device)
    Io, Do, cnt = knn_filter(I, D, ex_ids, ph_ids, k_top)
    host = torch.cat([Io.view(torch.int32).view(-1), Do.view(torch.int32).view(-1), cnt]).cpu().numpy()   # one copy
    n = Io.numel()
    Ih = host[:2 * n].view(np.int64).reshape(Io.shape)
    Dh = host[2 * n:3 * n].view(np.float32).reshape(Do.shape)
    check_counts(host[3 * n:], k_top)
    return Neighbours(Ih, Dh)


def check_counts(count, k_top):
    """phrase_embed.py:263: every phrase must have k_top kept neighbours."""
    assert bool((np.asarray(count) == k_top).all()), 'Did not find enough valid candidates.'


# ---- writers ---------------------------------------------------------------------------------------------------------------
def write_neighbours(f, pset, nn, idx2word):
    """The lines phrase_embed.py:265-270 prints: a [query] line per phrase, then its kept neighbours by rank."""
    def stringify(phrase):
        return ' '.join([idx2word[idx] for idx in phrase])

    ex, ph = pset.example_ids, pset.phrases
    for i in range(len(ph)):
        f.write('[query] example_id={} phrase={}\n'.format(ex[i], stringify(ph[i])))
        for rank, (j, score) in enumerate(zip(nn.I[i].tolist(), nn.D[i])):
            f.write('rank={} score={:.3f} example_id={} phrase={}\n'.format(rank, score, ex[j], stringify(ph[j])))


def write_vectors(path, pset):
    """vectors.csv (example_id,position,size) and vectors.npy -- TEXT, np.savetxt's, one block per batch appended as
    phrase_embed_simple.py:220-288 writes them.  One device-to-host copy of the vectors."""
    with open(os.path.join(path, 'vectors.csv'), 'w') as f:
        f.write('example_id,position,size\n')
        for e, p, s in zip(pset.example_ids, pset.positions, pset.sizes):
            f.write('%s,%s,%s\n' % (e, p, s))
    host = pset.vectors.cpu().numpy()
    with open(os.path.join(path, 'vectors.npy'), 'ab') as f:
        r = 0
        for n in pset.batch_rows:
            np.savetxt(f, host[r:r + n])
            r += n
