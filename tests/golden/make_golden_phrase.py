#!/usr/bin/env python
"""Generate phrase_embed.npz by RUNNING the reference's own phrase scripts: cliora/scripts/phrase_embed.py:run (entity phrases,
nearest neighbours) and cliora/scripts/phrase_embed_simple.py:run in its modes 'given', 'latent' and 'all-spans'.

Runs only in the build container (needs the reference checkout); the GPU box never executes this.
Usage:  python tests/golden/make_golden_phrase.py

Both scripts are executed from their text with stand-ins for what they import and this container lacks:
  * `train`: get_validation_dataset / get_validation_iterator / build_net -- a word table, the batches below, and the reference
    Trainer of make_golden_eval (cliora.net.trainer.build_net) with its seeded weights;
  * `faiss`: a STAND-IN, not faiss: IndexFlatIP scores in float64 with numpy and orders a query's keys by (-score, index), returning
    float32 scores and -1 / -inf past the keys; normalize_L2 scales float32 rows in place by 1 / sqrt(sum of squares in float32);
  * `tqdm`: the identity;
  * cliora.analysis.cky.ParsePredictor: phrase_embed_simple's TreeHelper constructs it with a `word2idx` keyword that the reference's
    class does not take (cky.py:9); the stand-in drops it.
Captured: the printed neighbour lines and the candidate lists behind them, vectors.csv and vectors.npy of each mode, per batch the
inputs, the reference chart's inside_h / outside_h and the CKY trees, and the net's state.  The generator asserts that the candidate
scores the neighbour walk looks at are more than 1e-4 apart, apart from exact duplicates (the same sentence under two example ids,
the same span labelled twice), so that the device's fp32 order must agree.
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_eval as MGE                             # noqa: E402  (reference on sys.path, the reference trainer and weights)
from make_golden import save, state_np, META               # noqa: E402
import cliora.analysis.cky as ref_cky                      # noqa: E402

SCRIPTS = os.path.join(os.path.dirname(MGE.REF_PARSE))
D, V, E, K, FEAT, R = MGE.D, MGE.V, MGE.E, MGE.K, MGE.FEAT, MGE.R
SHAPES = [(4, 6), (3, 2), (5, 8), (4, 5)]                  # (B, L); L = 2 is skipped by both scripts
DUP = (2, 0, 3)                                            # batch 2: sentence 3 is sentence 0 under another example id
K_CANDIDATES, K_TOP = 100, 3


def make_inputs(seed):
    rs = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed + 1)
    batches = []
    for bi, (B, L) in enumerate(SHAPES):
        sent = torch.randint(1, V, (B, L), generator=g)
        feats = torch.zeros(B, R, FEAT)
        feats[:, :, :64] = torch.randn(B, R, 64, generator=g).half().float()
        ents = []
        for b in range(B):
            lst = []
            for _ in range(rs.randint(2, 5)):
                size = int(rs.randint(1, L + 1))
                pos = int(rs.randint(0, L - size + 1))
                lst.append(('L%d' % rs.randint(3), pos, size))
            if b == 1:
                lst.insert(1, None)                        # a None entry (skipped)
            ents.append(lst)
        trees = [MGE.rand_tree(rs, 0, L) for _ in range(B)]
        if bi == DUP[0]:
            sent[DUP[2]] = sent[DUP[1]]
            feats[DUP[2]] = feats[DUP[1]]
            ents[DUP[2]] = list(ents[DUP[1]])
            trees[DUP[2]] = trees[DUP[1]]
        bm = dict(example_ids=['%d_%d' % (bi, b) for b in range(B)], sentences=sent, image_feats=torch.zeros(B, 1),
                  neg_samples=torch.randperm(V, generator=g)[:K], obj_feats=feats, boxes=torch.zeros(B, R, 4),
                  obj_cates=torch.zeros(B, R), GT=[[(0, L - 1)]] * B, batch_size=B, length=L, entity_labels=ents, trees=trees)
        batches.append(bm)
    return batches


class FlatIP(object):
    """Stand-in for faiss.IndexFlatIP: float64 scores, (-score, index) order, float32 D, -1 / -inf past the keys."""
    searches = []

    def __init__(self, dim):
        self.dim, self.x = dim, np.zeros((0, dim))

    def add(self, v):
        self.x = np.concatenate([self.x, np.asarray(v, dtype=np.float64)], 0)

    def search(self, q, k):
        s = np.asarray(q, dtype=np.float64) @ self.x.T
        n = self.x.shape[0]
        I = -np.ones((s.shape[0], k), dtype=np.int64)
        Dv = np.full((s.shape[0], k), -np.inf, dtype=np.float32)
        for i in range(s.shape[0]):
            order = np.lexsort((np.arange(n), -s[i]))[:k]
            I[i, :len(order)] = order
            Dv[i, :len(order)] = s[i, order]
        FlatIP.searches.append((s, I, Dv, self.x))
        return Dv, I


def normalize_L2(x):
    nr = np.sqrt(np.sum(x * x, axis=1, dtype=np.float32)).astype(np.float32)
    nz = nr > 0
    x[nz] *= (np.float32(1) / nr[nz])[:, None]


def run_script(name, opts, bms, emb, word2idx):
    faiss = types.ModuleType('faiss')
    faiss.IndexFlatIP, faiss.normalize_L2 = FlatIP, normalize_L2
    tq = types.ModuleType('tqdm')
    tq.tqdm = lambda it, *a, **k: it

    class Iterator(object):
        def get_iterator(self, random_seed=None):
            return iter(bms)

    train = types.ModuleType('train')
    train.argument_parser = train.parse_args = train.configure = lambda *a, **k: None
    train.get_validation_dataset = lambda o: dict(word2idx=word2idx, embeddings=emb)
    train.get_validation_iterator = lambda o, ds: Iterator()
    train.build_net = lambda o, embeddings, *a: MGE.make_trainer(embeddings)
    cky = types.ModuleType('cliora.analysis.cky')
    cky.ParsePredictor = lambda net, word2idx=None: ref_cky.ParsePredictor(net)
    saved = {n: sys.modules.get(n) for n in ('faiss', 'tqdm', 'train', 'cliora.analysis.cky')}
    sys.modules.update({'faiss': faiss, 'tqdm': tq, 'train': train, 'cliora.analysis.cky': cky})
    try:
        ns = {'__name__': 'phrase_fixture'}
        exec(compile(open(os.path.join(SCRIPTS, name)).read(), name, 'exec'), ns)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            ns['run'](opts)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return buf.getvalue()


def main(seed=31):
    torch.manual_seed(0)
    emb = torch.nn.Embedding(V, E)
    torch.nn.init.normal_(emb.weight, generator=torch.Generator().manual_seed(93))
    word2idx = {'w%d' % i: i for i in range(V)}
    bms = make_inputs(seed)
    arrs = dict(state_np(MGE.make_trainer(emb).net, 'param__'))
    # the reference chart and CKY trees of every batch (the same weights every script builds)
    tr = MGE.make_trainer(emb)
    diora = tr.net.diora
    MGE.override_init_with_batch(diora)
    MGE.override_inside_hook(diora)
    latent = []
    for bi, bm in enumerate(bms):
        p = 'b%d__' % bi
        arrs[p + 'sentences'] = bm['sentences'].numpy()
        arrs[p + 'obj_feats'] = bm['obj_feats'][:, :, :64].numpy().astype(np.float16)
        if bm['length'] <= 2:
            latent.append(None)
            continue
        with torch.no_grad():
            tr.step(bm, train=False, compute_loss=False)
        arrs[p + 'inside_h'] = diora.inside_h.numpy().copy()
        arrs[p + 'outside_h'] = diora.outside_h.numpy().copy()
        trees = MGE.ParsePredictor(net=diora).parse_batch(bm)
        latent.append([MGE.get_spans(MGE.get_actions(str(t))) for t in trees])
    d = arrs['b%d__inside_h' % DUP[0]], arrs['b%d__outside_h' % DUP[0]]
    for h in d:
        assert np.array_equal(h[DUP[1]], h[DUP[2]]), 'the duplicated sentence must have a bitwise equal chart'
    meta = dict(META, D=D, R=R, V=V, E=E, K=K, feat=FEAT, feat_cols=64, shapes=SHAPES, k_candidates=K_CANDIDATES, k_top=K_TOP,
                example_ids=[bm['example_ids'] for bm in bms], entity_labels=[bm['entity_labels'] for bm in bms],
                trees=[json.loads(json.dumps(bm['trees'])) for bm in bms], latent_spans=latent)
    opts = MGE.options(None)
    opts.k_candidates, opts.k_top, opts.hidden_dim = K_CANDIDATES, K_TOP, D
    # phrase_embed.py:run -- entity phrases, normalised, neighbours
    FlatIP.searches = []
    text = run_script('phrase_embed.py', opts, bms, emb, word2idx)
    text = ''.join(ln + '\n' for ln in text.splitlines() if ln.startswith(('[query] ', 'rank=')))     # the trainer prints too
    (s64, I, Dv, keys), = FlatIP.searches
    # the candidate walk of phrase_embed.py:250-263 restated, to record the kept ids and check the gaps it depends on
    qlines = [ln for ln in text.splitlines() if ln.startswith('[query]')]
    ex = [e for bm in bms if bm['length'] > 2 for e in (bm['example_ids'][i] for i, lst in enumerate(bm['entity_labels'])
                                                          for el in lst if el is not None and el[2] >= 2)]
    phr = [ln.split(' phrase=', 1)[1] for ln in qlines]
    assert len(ex) == len(phr) == I.shape[0]
    nn_I, nn_D = [], []
    for i in range(I.shape[0]):
        kept, walked = [], []
        for j, sc in zip(I[i].tolist(), Dv[i].tolist()):
            walked.append(j)
            if ex[i] == ex[j] or phr[i] == phr[j]:
                continue
            kept.append((j, sc))
            if len(kept) == K_TOP:
                break
        nxt = I[i][len(walked)] if len(walked) < I.shape[1] and I[i][len(walked)] >= 0 else None
        seq = walked + ([int(nxt)] if nxt is not None else [])
        for a, b in zip(seq, seq[1:]):
            gap = s64[i, a] - s64[i, b]
            assert gap > 1e-4 or (gap == 0 and np.array_equal(keys[a], keys[b])), (i, a, b, gap)
        nn_I.append([j for j, _ in kept])
        nn_D.append([sc for _, sc in kept])
    arrs['nn_I'] = np.array(nn_I, dtype=np.int64)
    arrs['nn_D'] = np.array(nn_D, dtype=np.float32)
    meta['neighbour_text'] = text
    # phrase_embed_simple.py:run in three modes
    for mode in ('given', 'latent', 'all-spans'):
        with tempfile.TemporaryDirectory() as tmp:
            opts.parse_mode, opts.experiment_path, opts.postprocess = mode, tmp, False
            run_script('phrase_embed_simple.py', opts, bms, emb, word2idx)
            key = mode.replace('-', '_')
            arrs[key + '__csv'] = np.frombuffer(open(os.path.join(tmp, 'vectors.csv'), 'rb').read(), dtype=np.uint8)
            arrs[key + '__npy'] = np.frombuffer(open(os.path.join(tmp, 'vectors.npy'), 'rb').read(), dtype=np.uint8)
    arrs['meta'] = np.array(json.dumps(meta))
    save('phrase_embed.npz', **arrs)
    print('entity phrases', I.shape[0], 'rows given', arrs['given__csv'].tobytes().count(b'\n') - 1,
          'latent', arrs['latent__csv'].tobytes().count(b'\n') - 1, 'all-spans', arrs['all_spans__csv'].tobytes().count(b'\n') - 1)


if __name__ == '__main__':
    main()
