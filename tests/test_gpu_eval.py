"""cliora_ground_eval and cliora_amd.evaluate on the GPU against what the reference's parse.py:run computed (tests/golden/eval_parse.npz)
and against a plain torch restatement of the selection rule at the c3 shape (B 64, L 20, R 36)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_eval_cpu import _gt, _host_result, _vg_gt

pytestmark = pytest.mark.gpu


def _strided(att):
    """atten as DioraMLP.atten_score holds it: the permuted diagonal of a (B, B, L, R) tensor."""
    B = att.shape[0]
    vg = torch.randn((B,) + tuple(att.shape), device=att.device)
    for i in range(B):
        vg[i, i] = att[i]
    return torch.diagonal(vg, 0, 0, 1).permute(2, 0, 1)


@pytest.mark.parametrize('layout', ['contiguous', 'strided'])
def test_kernel_matches_the_reference_selection(layout):
    from cliora_amd.evaluate import Targets, ground
    g = load_golden('eval_parse.npz')
    meta = g['meta']
    for bi, (B, L) in enumerate(meta['shapes']):
        if L <= 2:
            continue
        att = torch.from_numpy(g['b%d__atten_score' % bi]).cuda()
        if layout == 'strided':
            att = _strided(att)
            assert not att.is_contiguous()
        tg = Targets(_vg_gt(meta, bi), _gt(meta, bi), B, L)
        spans = torch.from_numpy(g['b%d__spans' % bi]).cuda()
        res = ground(att, torch.from_numpy(g['b%d__boxes' % bi]).cuda(), tg, spans)
        want = _host_result(g, bi)
        assert np.array_equal(res.spans, g['b%d__spans' % bi])
        for f in ('word', 'box', 'hit', 'ccr'):
            assert np.array_equal(getattr(res, f), getattr(want, f)), (bi, f)
        assert np.array_equal(res.sent, want.sent), bi
        assert np.array_equal(res.span_xyxy, want.span_xyxy), bi


def _net(g):
    from cliora_amd import harness as H
    m = g['meta']
    net = H.build_net(m['D'], torch.nn.Embedding(m['V'], m['E']), obj_feats=True, img_dim=m['feat'], k_neg=m['K'], vg_loss=True,
                      use_contr=True, vl_margin=0.2, alpha_contr=1.0, alpha_vg=1.0)
    sd = net.state_dict()
    for k in sd:
        sd[k] = torch.from_numpy(g['param__' + k.replace('.', '__')].copy())
    net.load_state_dict(sd)
    return net.cuda()


def _batches(g):
    meta = g['meta']
    out = []
    for bi, (B, L) in enumerate(meta['shapes']):
        f16 = g['b%d__obj_feats' % bi]
        feats = np.zeros(f16.shape[:2] + (meta['feat'],), dtype=np.float32)
        feats[:, :, :meta['feat_cols']] = f16.astype(np.float32)
        out.append(dict(sentences=torch.from_numpy(g['b%d__sentences' % bi]).cuda(), obj_feats=torch.from_numpy(feats).cuda(),
                        boxes=torch.from_numpy(g['b%d__boxes' % bi]).cuda(), neg_samples=torch.from_numpy(g['b%d__neg_samples' % bi]).cuda(),
                        VG_GT=_vg_gt(meta, bi), GT=_gt(meta, bi), example_ids=meta['example_ids'][bi]))
    return out


def test_evaluate_end_to_end_matches_parse_run(mfma_mode, tmp_path):
    """The four metrics exactly, the losses to test_gpu_harness's tolerance for the reference losses, parse.jsonl line for line.
    In the split-bf16 mode the attention scores are not the reference's to the last bit, so a phrase whose two best words or regions
    lie within that rounding could choose differently: there the grounding numbers may move by one phrase and pred_boxes are not
    compared; the exact-fp32 mode asserts all of it exactly.  Tree spans and F1 are exact in both (as the CKY tests require)."""
    from cliora_amd.evaluate import evaluate
    g = load_golden('eval_parse.npz')
    meta = g['meta']
    path = os.path.join(str(tmp_path), 'parse.jsonl')
    got = evaluate(_net(g), _batches(g), {i: 'w%d' % i for i in range(meta['V'])}, out_path=path)
    want = meta['metrics']
    names = ('corpus_f1', 'sent_f1', 'ground_acc', 'ccra', 'recon_loss', 'vg_loss', 'contr_loss', 'total_loss')
    assert got['corpus_f1'] == want[0] and got['sent_f1'] == want[1]
    one = 1.0 / len(g['phrase_sel'])
    for k in (2, 3):
        if mfma_mode == 'f32':
            assert got[names[k]] == want[k], (names[k], got[names[k]], want[k])
        else:
            assert abs(got[names[k]] - want[k]) <= one + 1e-9, (names[k], got[names[k]], want[k])
    tol = 5e-4 if mfma_mode == 'f32' else 1e-3
    for k in range(4, 8):
        assert abs(got[names[k]] - want[k]) <= tol * max(1.0, abs(want[k])), (names[k], got[names[k]], want[k])
    lines = open(path).read().splitlines()
    assert len(lines) == len(meta['parse_jsonl'])
    for a, b in zip(lines, meta['parse_jsonl']):
        ja, jb = json.loads(a), json.loads(b)
        if mfma_mode != 'f32':
            ja.pop('pred_boxes'), jb.pop('pred_boxes')
        assert ja == jb


def _torch_select(att, s, e):
    """The selection rule with plain torch ops on the device: first word of [s, e) with the largest row maximum, then the first
    region of that row attaining it (first indices made explicit: CUDA/HIP max does not promise the first)."""
    rows = att[s:e]
    rmax = rows.max(1).values
    R = rows.shape[1]
    first = torch.where(rows == rmax[:, None], torch.arange(R, device=att.device), R).min(1).values
    m = rmax.max()
    w = int(torch.where(rmax == m, torch.arange(e - s, device=att.device), e - s).min())
    return s + w, int(first[w])


def _torch_iou(a, g):
    a1 = (a[2] - a[0]) * (a[3] - a[1])
    a2 = (g[2] - g[0]) * (g[3] - g[1])
    wh = (torch.min(a[2:], g[2:]) - torch.max(a[:2], g[:2])).clamp(min=0)
    inter = wh[0] * wh[1]
    return inter / (a1 + a2 - inter)


def test_c3_batch_matches_a_torch_restatement():
    from cliora_amd.evaluate import Targets, ground
    B, L, R = 64, 20, 36
    gen = torch.Generator().manual_seed(5)
    rs = np.random.RandomState(6)
    att = torch.softmax(torch.randn(B, L, R, generator=gen), -1)
    att[:, :, 20:30] = att[:, :, 0:10]                      # duplicated regions: exact ties
    att = att.cuda()
    xy = torch.randint(0, 300, (B, R, 2), generator=gen).float()
    wh = torch.randint(0, 150, (B, R, 2), generator=gen).float()    # some zero widths / heights
    boxes = torch.cat([xy, xy + wh], -1).cuda()

    def tree(lo, hi, out):
        if hi - lo == 1:
            return
        k = rs.randint(lo + 1, hi)
        tree(lo, k, out), tree(k, hi, out)
        out.append((lo, hi - 1))
    spans = []
    for b in range(B):
        sp = []
        tree(0, L, sp)
        spans.append(sp)
    vg, gt = [], []
    for b in range(B):
        n = 0 if b == 0 else (L - 1 if b == 1 else rs.randint(1, 10))
        target = {}
        for j in range(n):
            s = rs.randint(0, L)
            e = rs.randint(s + 1, L + 1)
            if rs.rand() < 0.5:
                s, e = spans[b][rs.randint(0, L - 2)]
                e += 1
            bx = boxes[b, rs.randint(0, R)].tolist()
            target[j] = (s, e, [bx[0], bx[1], bx[2] + float(rs.randint(0, 40)), bx[3]])
        vg.append((target, None))
        g_sp = [tuple(spans[b][k]) for k in rs.choice(L - 1, size=rs.randint(0, L), replace=True)]
        gt.append(g_sp + [(0, L - 1)])
    tg = Targets(vg, gt, B, L)
    d_spans = torch.tensor(spans, dtype=torch.int32).cuda()
    res = ground(_strided(att), boxes, tg, d_spans)
    assert tg.P == len(res.word) and tg.phr_off[1] == 0 and tg.phr_off[2] - tg.phr_off[1] == L - 1
    for k, (b, s, e) in enumerate(tg.phrases):
        w, box = _torch_select(att[b], s, e)
        iou = _torch_iou(boxes[b, box], torch.tensor(tg.phr_box[k]).cuda())
        hit = int(bool(iou > 0.5))
        pred = set(spans[b][:-1])
        ccr = int(bool(hit) and (e - 1 == s or (s, e - 1) in pred))
        assert (res.word[k], res.box[k], res.hit[k], res.ccr[k]) == (w, box, hit, ccr), (k, b, s, e)
    for b in range(B):
        pred, gold = set(spans[b][:-1]), set(gt[b][:-1])
        assert res.sent[b].tolist() == [len(pred & gold), len(pred), len(gold)], b
        for k, (s, e) in enumerate(spans[b]):
            _, box = _torch_select(att[b], s, e + 1)
            assert res.span_xyxy[b, k].tolist() == boxes[b, box].tolist(), (b, k)
