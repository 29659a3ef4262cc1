"""Host side of cliora_amd.evaluate against what the reference's parse.py:run computed and wrote (tests/golden/eval_parse.npz):
the CSR tables of VG_GT / GT, the metric formulas on the per-phrase results and tree spans recorded in the fixture, and the
parse.jsonl lines with pred_boxes.  No GPU: the device's part (box selection, IoU, counts) is restated on the host here from the
fixture's attention scores, by the reference's rule."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def _fixture():
    return load_golden('eval_parse.npz')


def _vg_gt(meta, bi):
    return [({'p%d' % j: (s, e, box) for j, (s, e, box) in enumerate(sent)}, None) for sent in meta['VG_GT'][bi]]


def _gt(meta, bi):
    return [[tuple(s) for s in sent] for sent in meta['GT'][bi]]


def _host_result(g, bi):
    """GroundResult of batch bi as the kernel must produce it, from the fixture (selected word / box, hit) and the reference's rule."""
    from cliora_amd.evaluate import GroundResult, Targets
    meta = g['meta']
    B, L = meta['shapes'][bi]
    tg = Targets(_vg_gt(meta, bi), _gt(meta, bi), B, L)
    spans = g['b%d__spans' % bi]
    sel = g['phrase_sel']
    rows = np.nonzero(sel[:, 0] == bi)[0]
    hit = g['phrase_hit'][rows]
    phr = np.zeros((len(rows), 4), dtype=np.int32)
    for k, r in enumerate(rows):
        _, b, s, e, w, box = sel[r].tolist()
        pred = set(map(tuple, spans[b][:-1].tolist()))
        phr[k] = (w, box, hit[k], int(bool(hit[k]) and (e - 1 == s or (s, e - 1) in pred)))
    sent = np.zeros((B, 3), dtype=np.int32)
    for b in range(B):
        pred, gold = set(map(tuple, spans[b][:-1].tolist())), set(tg.gold[b])
        sent[b] = (len(pred & gold), len(pred), len(gold))
    att = torch.from_numpy(g['b%d__atten_score' % bi])
    boxes = g['b%d__boxes' % bi]
    xyxy = np.zeros((B, L - 1, 4), dtype=np.float32)
    for b in range(B):
        for k, (s, e) in enumerate(spans[b].tolist()):
            words = att[b, s:e + 1]
            wid = int(words.max(1)[0].max(0)[1])
            xyxy[b, k] = boxes[b, int(words[wid].max(0)[1])]
    return GroundResult(tg, spans, phr, sent, xyxy)


def test_targets_csr_packing():
    from cliora_amd.evaluate import Targets
    vg = [({'a': (0, 3, [1, 2, 3, 4]), 'b': (2, 3, [5., 6., 7., 8.])}, None), ({}, None), ({'c': (1, 5, (0, 0, 1, 1))}, None)]
    gt = [[(0, 1), (0, 1), (0, 4)], [(2, 3), (0, 4)], [(0, 4)]]
    tg = Targets(vg, gt, 3, 5)
    assert tg.phrases == [(0, 0, 3), (0, 2, 3), (2, 1, 5)]
    assert tg.phr_off.tolist() == [0, 2, 2, 3]
    assert tg.phr_span.tolist() == [[0, 3], [2, 3], [1, 5]]
    assert tg.phr_box.dtype == np.float32 and tg.phr_box.tolist() == [[1, 2, 3, 4], [5, 6, 7, 8], [0, 0, 1, 1]]
    assert tg.gold == [[(0, 1), (0, 1)], [(2, 3)], []]          # GT[b][:-1], duplicates kept (the kernel counts the set)
    assert tg.gold_off.tolist() == [0, 2, 3, 3] and tg.gold_span.tolist() == [[0, 1], [0, 1], [2, 3]]
    packed = tg.packed()
    assert packed.dtype == np.int32 and packed.size == 4 + 6 + 12 + 4 + 6
    assert packed[10:22].view(np.float32).tolist() == tg.phr_box.ravel().tolist()
    empty = Targets(None, None, 2, 4)
    assert empty.P == 0 and empty.G == 0 and empty.phr_off.tolist() == [0, 0, 0]


@pytest.mark.parametrize('start,end', [(2, 2), (3, 2), (0, 6), (-1, 2)])
def test_targets_reject_phrases_outside_the_sentence(start, end):
    from cliora_amd.evaluate import Targets
    with pytest.raises(ValueError):
        Targets([({'a': (start, end, [0, 0, 1, 1])}, None)], [[(0, 4)]], 1, 5)


def test_fixture_metrics_from_the_recorded_results():
    """Counts -> corpus F1, sentence F1, grounding accuracy, CCRA: the numbers the reference's run printed."""
    from cliora_amd.evaluate import Evaluator
    g = _fixture()
    ev = Evaluator()
    for bi, (B, L) in enumerate(g['meta']['shapes']):
        if L <= 2:
            continue
        ev.add(_host_result(g, bi))
    got = ev.result()
    want = g['meta']['metrics']
    for k, name in enumerate(('corpus_f1', 'sent_f1', 'ground_acc', 'ccra')):
        assert abs(got[name] - want[k]) <= 1e-12, (name, got[name], want[k])
    assert ev.total_num == len(g['phrase_sel'])


def test_fixture_parse_jsonl_lines():
    from cliora_amd.diora import DioraBase
    from cliora_amd.evaluate import batch_records
    g = _fixture()
    meta = g['meta']
    idx2word = {i: 'w%d' % i for i in range(meta['V'])}
    lines = []
    for bi, (B, L) in enumerate(meta['shapes']):
        if L <= 2:
            continue
        res = _host_result(g, bi)
        trees = DioraBase.trees_from_spans(res.spans)
        lines += batch_records(res, trees, g['b%d__sentences' % bi].tolist(), meta['example_ids'][bi], idx2word, True)
    want = meta['parse_jsonl']
    assert len(lines) == len(want)
    for a, b in zip(lines, want):
        assert json.loads(a) == json.loads(b)
        assert list(json.loads(a)) == list(json.loads(b))         # key order too


def test_ground_eval_symbol_exported_and_declared():
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert 'int cliora_ground_eval(' in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'cliora_ground_eval')
