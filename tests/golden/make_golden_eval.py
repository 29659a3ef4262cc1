#!/usr/bin/env python
"""Generate eval_parse.npz by RUNNING the reference's own evaluation loop, cliora/scripts/parse.py:run (lines 101-291).

Runs only in the build container (needs the reference checkout); the GPU box never executes this.
Usage:  python tests/golden/make_golden_eval.py

parse.py is executed from its text with three stand-ins for what it imports and this container lacks:
  * torchvision.ops.box_iou -- torchvision's formula in its operation order, wrapped to record every call (one per gold phrase);
  * the `train` module's get_validation_dataset / get_validation_iterator / build_net -- a word table, the batches below, and the
    reference Trainer of cliora.net.trainer.build_net with fixed weights;
  * tqdm -- the identity.
Captured: the printed metrics and mean losses, parse.jsonl, and per phrase the selected word / box (recomputed from atten_score with the
script's own rule, checked against the box handed to box_iou) and hit.  Stored: inputs and outputs only.
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                  # noqa: E402  (reference on sys.path, cv2 stub, helpers)
from make_golden import ref_trainer, seeded_params, state_np, save, META      # noqa: E402
from cliora.analysis.cky import ParsePredictor            # noqa: E402
from cliora.analysis.utils import override_init_with_batch, override_inside_hook, get_actions, get_spans  # noqa: E402

REF_PARSE = os.path.join(os.path.dirname(MG.ref_trainer.__file__), '..', 'scripts', 'parse.py')
D, R, V, E, K, FEAT = 16, 36, 50, 32, 6, 2048
SHAPES = [(4, 5), (3, 2), (5, 8), (4, 11)]          # (B, L) per batch; L = 2 is skipped by the script


def box_iou(a, b):
    """torchvision.ops.box_iou (boxes xyxy), same operation order."""
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(a[:, None, :2], b[:, :2])
    rb = torch.min(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = area1[:, None] + area2 - inter
    return inter / union


def options(exp_path):
    return argparse.Namespace(lr=2e-3, hidden_dim=D, k_neg=K, normalize='unit', cuda=False, local_rank=0, share=True, arch='mlp',
                              obj_feats=True, multigpu=False, emb='none', margin=1.0, vl_margin=0.2, hinge_margin=1.0, alpha_contr=1.0,
                              vg_loss=True, alpha_vg=1.0, use_contr=True, use_contr_ce=False, visualize=False, load_model_path=None,
                              experiment_name='eval-fixture', experiment_path=exp_path, seed=11, postprocess=False)


def make_trainer(emb):
    tr = ref_trainer.build_net(options(None), emb)
    net = tr.net
    seeded_params(net, 91)
    g = torch.Generator().manual_seed(92)
    with torch.no_grad():
        for p in net.img_encoder.parameters():        # zero-initialised in the reference (utils.py:45-50); only the first 64 feature
            p.copy_(0.05 * torch.randn(p.shape, generator=g))          # columns carry data, the rest of the weight is zero
            if p.dim() == 2:
                p[:, 64:] = 0
    return tr


def rand_tree(rs, lo, hi):
    if hi - lo == 1:
        return lo
    k = rs.randint(lo + 1, hi)
    return (rand_tree(rs, lo, k), rand_tree(rs, k, hi))


def make_inputs():
    rs = np.random.RandomState(17)
    g = torch.Generator().manual_seed(18)
    batches = []
    for bi, (B, L) in enumerate(SHAPES):
        sent = torch.randint(1, V, (B, L), generator=g)
        feats = torch.zeros(B, R, FEAT)
        feats[:, :, :64] = torch.randn(B, R, 64, generator=g).half().float()
        feats[0, 6:12] = feats[0, 0:6]                     # duplicated regions: identical score columns, argmax ties
        feats[1, 1::2] = feats[1, 0:1]
        boxes = torch.zeros(B, R, 4)
        for b in range(B):                                 # distinct integer boxes per sentence, one of zero area
            seen = set()
            for r in range(R):
                while True:
                    x1, y1 = rs.randint(0, 300, size=2)
                    w, h = rs.randint(1, 200, size=2)
                    bx = (float(x1), float(y1), float(x1 + w), float(y1 + h))
                    if r == R - 1:
                        bx = (float(x1), float(y1), float(x1), float(y1 + h))
                    if bx not in seen:
                        break
                seen.add(bx)
                boxes[b, r] = torch.tensor(bx)
        gt = []
        for b in range(B):
            spans = get_spans(get_actions(str(rand_tree(rs, 0, L)))) if L > 1 else [(0, 0)]
            body = list(spans[:-1])
            if body and b % 2 == 0:
                body.insert(int(rs.randint(0, len(body) + 1)), body[int(rs.randint(0, len(body)))])     # a duplicate gold span
            gt.append(body + [spans[-1]])
        phrases = []
        for b in range(B):
            ph = [(0, L)]                                   # the whole sentence (never a CCRA hit: the root is no predicted span)
            ph += [(s, s + 1) for s in rs.choice(L, size=min(2, L), replace=False)]
            for _ in range(rs.randint(0, 4)):
                s = rs.randint(0, L)
                ph.append((s, rs.randint(s + 1, L + 1)))
            if bi == 3 and b == 3:
                ph = []                                     # a sentence without phrases
            phrases.append([(int(s), int(e)) for s, e in ph])
        batches.append(dict(sent=sent, feats=feats, boxes=boxes, gt=gt, phrases=phrases, neg=torch.randperm(V, generator=g)[:K]))
    return batches


def select(att, s, e):
    """parse.py:180-185 on one sentence's (L, R) scores."""
    words = att[s:e]
    wid = words.max(1)[0].max(0)[1]
    return int(wid) + s, int(words[wid].max(0)[1])


def gt_box_for(kind, pb, rs):
    x1, y1, x2, y2 = pb
    w = x2 - x1
    if kind == 'exact':                      # IoU exactly 0.5: no hit
        return [x1, y1, x1 + 2 * w, y2]
    if kind == 'above':
        return [x1, y1, x1 + 2 * w - 0.5, y2]
    if kind == 'below':
        return [x1, y1, x1 + 2 * w + 0.5, y2]
    if kind == 'same':
        return [x1, y1, x2, y2]
    if kind == 'zero':                        # zero-area gold box (against a zero-area selection: 0 / 0 = NaN, no hit)
        return [x1, y1, x1, y2]
    return [float(v) for v in rs.randint(400, 600, size=2)] + [700.0, 700.0]     # disjoint


def main():
    torch.manual_seed(0)
    emb = torch.nn.Embedding(V, E)
    torch.nn.init.normal_(emb.weight, generator=torch.Generator().manual_seed(93))
    inp = make_inputs()
    # pass 1: the reference net's attention scores and trees, to place the gold boxes around the boxes it selects
    tr = make_trainer(emb)
    diora = tr.net.diora
    override_init_with_batch(diora)
    override_inside_hook(diora)
    diora.outside = True
    tr.net.eval()
    rs = np.random.RandomState(23)
    kinds = ['exact', 'above', 'below', 'same', 'zero', 'far']
    sel, bms = [], []
    for bi, x in enumerate(inp):
        B, L = x['sent'].shape
        bm = dict(example_ids=['%d_%d' % (bi, b) for b in range(B)], sentences=x['sent'], image_feats=torch.zeros(B, 1),
                  neg_samples=x['neg'], obj_feats=x['feats'], boxes=x['boxes'], obj_cates=torch.zeros(B, R), GT=x['gt'],
                  batch_size=B, length=L)
        if L > 2:
            with torch.no_grad():
                tr.step(bm, None, train=False, compute_loss=True)
            att = diora.atten_score.detach().cpu()
            x['atten'] = att.numpy().copy()
            x['spans'] = np.array([get_spans(get_actions(str(t))) for t in ParsePredictor(net=diora).parse_batch(bm)], dtype=np.int32)
        vg = []
        for b in range(B):
            target = {}
            for j, (s, e) in enumerate(x['phrases'][b]):
                if L > 2:
                    wid, box = select(att[b], s, e)
                    kind = kinds[(bi + b + j) % len(kinds)]
                    if kind == 'zero' and j % 2 == 0:       # the selected box made zero-area as well: the NaN case
                        pb = x['boxes'][b, box]
                        x['boxes'][b, box, 2] = pb[0]
                    gbox = gt_box_for(kind, x['boxes'][b, box].tolist(), rs)
                    sel.append((bi, b, s, e, wid, box))
                else:
                    gbox = [1.0, 2.0, 30.0, 40.0]
                target['phr%d' % j] = (s, e, gbox)
            vg.append((target, None))
        bm['VG_GT'] = vg
        bms.append(bm)
    # pass 2: parse.py:run itself
    calls = []

    def rec_iou(a, b):
        out = box_iou(a, b)
        calls.append((a[0].tolist(), b[0].tolist(), float(out.max()), bool(out.max() > 0.5)))
        return out

    tv = types.ModuleType('torchvision')
    tv.ops = types.ModuleType('torchvision.ops')
    tv.ops.box_iou = rec_iou
    tq = types.ModuleType('tqdm')
    tq.tqdm = lambda it, *a, **k: it
    word2idx = {'w%d' % i: i for i in range(V)}

    class Iterator(object):
        def get_iterator(self, random_seed=None):
            return iter(bms)

    train = types.ModuleType('train')
    train.argument_parser = train.parse_args = train.configure = lambda *a, **k: None
    train.get_validation_dataset = lambda o: dict(word2idx=word2idx, embeddings=emb)
    train.get_validation_iterator = lambda o, ds: Iterator()
    train.build_net = lambda o, embeddings: make_trainer(embeddings)
    saved = {n: sys.modules.get(n) for n in ('torchvision', 'torchvision.ops', 'tqdm', 'train')}
    sys.modules.update({'torchvision': tv, 'torchvision.ops': tv.ops, 'tqdm': tq, 'train': train})
    try:
        ns = {'__name__': 'parse_fixture'}
        exec(compile(open(REF_PARSE).read(), 'parse.py', 'exec'), ns)
        with tempfile.TemporaryDirectory() as tmp:
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ns['run'](options(tmp))
            lines = open(os.path.join(tmp, 'parse.jsonl')).read().splitlines()
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    text = buf.getvalue()
    print(text)
    num = r'([-+0-9.eEnaif]+)'
    m1 = re.search(r'corpus_f1:%s \t sent_f1:%s \t grounding acc:%s \t ccra:%s' % (num, num, num, num), text)
    m2 = re.search(r'recon_loss: %s ; vg_loss: %s; contr_loss: %s; total_loss: %s' % (num, num, num, num), text)
    metrics = [float(v) for v in m1.groups()] + [float(v) for v in m2.groups()]
    assert len(calls) == len(sel), (len(calls), len(sel))
    hits = []
    for (bi, b, s, e, wid, box), (pb, gb, iou, hit) in zip(sel, calls):
        assert pb == inp[bi]['boxes'][b, box].tolist()      # the box the script compared is the one the rule above selects
        hits.append(hit)
    arrs = dict(state_np(make_trainer(emb).net, 'param__'))
    for bi, x in enumerate(inp):
        p = 'b%d__' % bi
        arrs[p + 'sentences'] = x['sent'].numpy()
        arrs[p + 'obj_feats'] = x['feats'][:, :, :64].numpy().astype(np.float16)     # the other columns are zero
        arrs[p + 'boxes'] = x['boxes'].numpy()
        arrs[p + 'neg_samples'] = x['neg'].numpy()
        if 'atten' in x:
            arrs[p + 'atten_score'] = x['atten']
            arrs[p + 'spans'] = x['spans']
    sel_a = np.array(sel, dtype=np.int32).reshape(-1, 6)
    arrs['phrase_sel'] = sel_a                                  # batch, sentence, start, end, word, box
    arrs['phrase_hit'] = np.array(hits, dtype=np.int32)
    arrs['phrase_iou'] = np.array([c[2] for c in calls], dtype=np.float32)
    vg_json = [[[[s, e, box] for (s, e, box) in [v for v in bm['VG_GT'][b][0].values()]] for b in range(len(bm['VG_GT']))] for bm in bms]
    arrs['meta'] = np.array(json.dumps(dict(META, D=D, R=R, V=V, E=E, K=K, feat=FEAT, feat_cols=64, shapes=SHAPES,
                                            example_ids=[bm['example_ids'] for bm in bms], GT=[bm['GT'] for bm in bms], VG_GT=vg_json,
                                            metrics=metrics, parse_jsonl=lines)))
    save('eval_parse.npz', **arrs)
    print('phrases', len(sel), 'hits', sum(hits), 'nan', int(np.isnan(arrs['phrase_iou']).sum()),
          'exact 0.5', int((arrs['phrase_iou'] == 0.5).sum()))


if __name__ == '__main__':
    main()
