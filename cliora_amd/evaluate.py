"""Evaluation of a trained net the way the reference's parse script reports it (cliora/scripts/parse.py:101-291, run by
test_cliora.sh): corpus and sentence span F1, phrase grounding accuracy, CCRA (gold noun phrases grounded correctly AND
constituents of the predicted tree), the mean eval losses, and ``parse.jsonl`` with a ``pred_boxes`` field.

The reference does the grounding as a host loop over every phrase and predicted span, each a ``.max()`` over a CPU copy of
``atten_score`` plus a ``box_iou``.  Here one launch per batch does it on the device (include/cliora_chart.h: cliora_ground_eval),
reading ``atten_score`` in place and the tree spans of the CKY decode where they were written; the host gets ONE copy of every
output.  What stays on the host is what must be bitwise the reference's: the float formulas of the metrics (Python doubles,
``SpanF1`` semantics, ``np.mean`` of the sentence F1s) and the order of the span sets in ``parse.jsonl``.

    from cliora_amd.evaluate import evaluate
    m = evaluate(net, batches, idx2word, out_path='parse.jsonl')     # net: harness.Net; batches: batch_map dicts
    m['corpus_f1'], m['sent_f1'], m['ground_acc'], m['ccra']
"""

import numpy as np
import torch

from . import _lib
from .interchange import SpanF1, parse_record
from .vocab import word_prediction      # the exact held-out word prediction (nll, perplexity, acc@k, mrr): its own pass, its own result

METRICS = ('corpus_f1', 'sent_f1', 'ground_acc', 'ccra', 'recon_loss', 'vg_loss', 'contr_loss', 'total_loss')
LOSS_NAMES = ('reconstruct_softmax_loss', 'vg_loss', 'contrastive_loss')     # harness.Net's loss names, as in the reference's Net


# ---- inputs: VG_GT / GT as CSR tables -------------------------------------------------------------------------------
class Targets(object):
    """The gold phrases (VG_GT) and gold constituents (GT[b][:-1]) of one batch as CSR tables.

    phrases: (sentence, start, end) per phrase, ``end`` exclusive, in the reference's order (the items of each sentence's dict);
    phr_off (B+1), phr_span (P, 2), phr_box (P, 4) float32; gold_off (B+1), gold_span (G, 2); gold: the Python list per sentence."""

    def __init__(self, vg_gt, gt, B, L, lengths=None):
        """lengths: per sentence, for a batch of mixed lengths padded to L (a phrase must then lie inside its own sentence)."""
        self.B, self.L = B, L
        self.phrases, spans, boxes = [], [], []
        phr_off = [0]
        for b in range(B):
            if vg_gt is not None:
                target, _noun_mask = vg_gt[b]
                for _, anno in target.items():
                    start, end, box = anno
                    start, end = int(start), int(end)
                    n = L if lengths is None else int(lengths[b])
                    if not (0 <= start < end <= n):
                        raise ValueError('sentence %d: phrase [%d, %d) is empty or outside the sentence of length %d' % (b, start, end, n))
                    if len(box) != 4:
                        raise ValueError('sentence %d: gold box %r is not (x1, y1, x2, y2)' % (b, box))
                    self.phrases.append((b, start, end))
                    spans.append((start, end))
                    boxes.append([float(v) for v in box])
            phr_off.append(len(spans))
        self.gold = [list(gt[b][:-1]) for b in range(B)] if gt is not None else [[] for _ in range(B)]
        gold_off, gold_span = [0], []
        for g in self.gold:
            gold_span.extend((int(s), int(e)) for s, e in g)
            gold_off.append(len(gold_span))
        self.phr_off = np.array(phr_off, dtype=np.int32)
        self.phr_span = np.array(spans, dtype=np.int32).reshape(-1, 2)
        self.phr_box = np.array(boxes, dtype=np.float32).reshape(-1, 4)
        self.gold_off = np.array(gold_off, dtype=np.int32)
        self.gold_span = np.array(gold_span, dtype=np.int32).reshape(-1, 2)

    @property
    def P(self):
        return len(self.phrases)

    @property
    def G(self):
        return len(self.gold_span)

    def packed(self):
        """The five tables as one int32 array (the boxes' bits included): one host-to-device copy."""
        return np.concatenate([self.phr_off, self.phr_span.ravel(), self.phr_box.view(np.int32).ravel(), self.gold_off,
                               self.gold_span.ravel()])


# ---- outputs ------------------------------------------------------------------------------------------------------------
class GroundResult(object):
    """Host view of one batch's outputs: spans (B, L-1, 2) the tree spans, root last; per phrase word / box / hit / ccr (P,);
    sent (B, 3) = |pred & gold|, |pred|, |gold| over span sets (pred without its root); span_xyxy (B, L-1, 4) float32, the box of
    every predicted span, or None (text-only DIORA)."""

    def __init__(self, targets, spans, phr, sent, span_xyxy):
        self.targets, self.phrases = targets, targets.phrases
        self.spans, self.sent, self.span_xyxy = spans, sent, span_xyxy
        phr = np.asarray(phr, dtype=np.int32).reshape(-1, 4)
        self.word, self.box, self.hit, self.ccr = phr[:, 0], phr[:, 1], phr[:, 2], phr[:, 3]


def ground_batch(diora, batch_map, spans=None, decode='viterbi'):
    """cliora_ground_eval for the batch the chart module last ran on: packs batch_map's VG_GT / GT into CSR tables, launches once
    on the current stream and copies every output back in one transfer.  `spans`: the (B, L-1, 2) int32 device spans of
    ``diora.cky_spans_device()``; None decodes them here, into the output buffer.  Text-only DIORA (``atten_score`` None): F1 counts
    only, the phrases are not read (the reference skips them too).  decode: which tree is decoded when `spans` is None -- 'viterbi'
    (cky_spans_device), 'mbr' (mbr_spans_device, cliora_amd.posterior) or 'hard' (hard_spans_device: the tree a hard chart's own
    selections spell, uniform batches only; refused on a module whose last forward was not hard)."""
    from . import ragged
    if decode == 'hard':
        if getattr(diora, 'selection', None) is None:
            raise ValueError("decode='hard' needs a hard chart: the module's last forward ran with hard=False")
    else:
        ragged.decode_entry(decode)
    plan = diora._plan
    B, L = plan.B * len(diora._wss), plan.L
    atten = getattr(diora, 'atten_score', None)
    tg = Targets(batch_map.get('VG_GT') if atten is not None else None, batch_map.get('GT'), B, L)
    boxes = batch_map['boxes'] if atten is not None else None
    if spans is None:
        spans = {'mbr': diora.mbr_spans_device, 'hard': diora.hard_spans_device}.get(decode, diora.cky_spans_device)
    return ground(atten, boxes, tg, spans, device=diora._wss[0].device)


def ground(atten, boxes, targets, spans, device=None, lengths=None, extra_status=()):
    """One cliora_ground_eval launch.  atten: (B, L, R) fp32 CUDA tensor, any strides (None: counts only); boxes (B, R, 4); targets:
    a Targets; spans: (B, L-1, 2) int32 device tensor, or a callable that writes them into the tensor it is given (the decode).
    lengths: int32 device tensor (B,) of a batch of mixed lengths padded to L -- cliora_ground_eval_ragged; the rows of `spans` beyond
    a sentence's n - 1 come back as (-1, -1).  extra_status: names and one-element int32 device tensors, or callables returning one
    once the decode has run (the status words of the forward and the decode): they ride in the same device-to-host copy and must
    be 0."""
    B, L = targets.B, targets.L
    P, G, NS = targets.P, targets.G, L - 1
    R = atten.shape[2] if atten is not None else 0
    dev = atten.device if atten is not None else device
    # output buffer: [status | sent B*3 | phrases P*4 | spans B*NS*2 | span boxes B*NS*4 (fp32 bits)]
    extra_status = list(extra_status)
    sizes = [1, B * 3, P * 4, B * NS * 2, B * NS * 4 if atten is not None else 0, len(extra_status)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    with torch.cuda.device(dev):
        out = torch.empty(offs[-1], device=dev, dtype=torch.int32)
        sec = [out[offs[i]:offs[i + 1]] for i in range(len(sizes))]
        d_spans = sec[3].view(B, NS, 2)
        if callable(spans):
            spans(out=d_spans)
        else:
            d_spans.copy_(spans)
        tab = torch.from_numpy(targets.packed()).to(dev)
        o = np.cumsum([0, B + 1, P * 2, P * 4, B + 1, G * 2]).tolist()
        phr_off, phr_span, phr_box, gold_off, gold_span = (tab[o[i]:o[i + 1]] for i in range(5))
        if atten is not None:
            boxes = boxes.to(device=dev, dtype=torch.float32).contiguous()
            if atten.shape != (B, L, R) or atten.dtype != torch.float32 or boxes.shape != (B, R, 4):
                raise ValueError('atten_score %s / boxes %s do not match B %d, L %d' % (tuple(atten.shape), tuple(boxes.shape), B, L))
            sb, sl, sr = atten.stride()
        else:
            boxes, sb, sl, sr = None, 0, 0, 0
        p, st = _lib.ptr_or_null, _lib.stream()
        if lengths is None:
            _lib.call('cliora_ground_eval', B, L, R, p(atten), sb, sl, sr, p(boxes), P, p(phr_off), p(phr_span), p(phr_box), p(d_spans), G,
                      p(gold_off), p(gold_span), p(sec[2]), None, p(sec[4]), p(sec[1]), p(sec[0]), st)
        else:
            lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
            if lengths.numel() != B:
                raise ValueError('lengths holds %d sentences, not %d' % (lengths.numel(), B))
            _lib.call('cliora_ground_eval_ragged', B, L, R, p(lengths), p(atten), sb, sl, sr, p(boxes), P, p(phr_off), p(phr_span),
                      p(phr_box), p(d_spans), G, p(gold_off), p(gold_span), p(sec[2]), None, p(sec[4]),
                      p(sec[1]), p(sec[0]), st)
        for k, (_, t) in enumerate(extra_status):
            sec[5][k:k + 1].copy_((t() if callable(t) else t).reshape(1))
        host = out.cpu().numpy()
    h = [host[offs[i]:offs[i + 1]] for i in range(len(sizes))]
    if h[0][0] and lengths is None:
        raise _lib.ChartLibError('cliora_ground_eval rejected %d phrase(s) / span(s) outside their sentence' % int(h[0][0]))
    if h[0][0]:
        raise _lib.ChartLibError('cliora_ground_eval_ragged rejected %d sentence length(s) outside 1..%d, or phrase(s) / span(s) outside '
                                 'their sentence' % (int(h[0][0]), L))
    for k, (name, _) in enumerate(extra_status):
        if h[5][k]:
            raise _lib.ChartLibError('%s rejected %d sentence length(s)' % (name, int(h[5][k])))
    xyxy = h[4].view(np.float32).reshape(B, NS, 4) if atten is not None else None
    return GroundResult(targets, h[3].reshape(B, NS, 2), h[2], h[1].reshape(B, 3), xyxy)


# ---- accumulation and the reference's formulas --------------------------------------------------------------------------
class Evaluator(object):
    """Accumulates the numbers parse.py:run reports (parse.py:146-264) over batches; ``result()`` applies its formulas (:282-291)."""

    def __init__(self):
        self.f1 = SpanF1()
        self.recall_num = self.ccr_num = self.total_num = 0.
        self.num_data = 0
        self._loss = None            # float64 device sums: recon, vg, contrastive, total

    def add_losses(self, out):
        """One batch's Net.forward(..., compute_loss=True) output: summed on the device, read once by result()."""
        if not hasattr(out, 'parts'):
            raise TypeError('add_losses wants the LossDict of harness.Net.forward(..., compute_loss=True)')
        tot = out.total()
        zero = torch.zeros((), device=tot.device, dtype=torch.float32)
        row = torch.stack([out[n].reshape(()) if n in out else zero for n in LOSS_NAMES] + [tot.reshape(())]).double()
        self._loss = row if self._loss is None else self._loss + row
        self.num_data += 1

    def add_counts(self, sent, hit=(), ccr=()):
        """Per sentence (tp, |pred|, |gold|); per phrase the hit and ccr flags."""
        for tp, npred, ngold in np.asarray(sent).reshape(-1, 3).tolist():
            self.f1.add_counts(tp, npred, ngold)
        hit = np.asarray(hit).reshape(-1)
        self.recall_num += int(hit.sum())
        self.ccr_num += int(np.asarray(ccr).sum())
        self.total_num += hit.size

    def add(self, res):
        self.add_counts(res.sent, res.hit, res.ccr)

    def losses(self):
        if self._loss is None:
            return [float('nan')] * 4
        return [v / self.num_data for v in self._loss.cpu().tolist()]

    def result(self):
        tp, fp, fn = self.f1.tp, self.f1.fp, self.f1.fn
        prec = tp / (tp + fp) if tp + fp else 0.
        recall = tp / (tp + fn) if tp + fn else 0.
        corpus_f1 = 2 * prec * recall / (prec + recall) if prec + recall > 0 else 0.
        sent_f1 = float(np.mean(np.array(self.f1.sentence))) if self.f1.sentence else float('nan')
        ground_acc = self.recall_num / (self.total_num + 1e-8)
        ccra = self.ccr_num / (self.total_num + 1e-8)
        return dict(zip(METRICS, [corpus_f1, sent_f1, ground_acc, ccra] + self.losses()))


def oracle_f1(spans_k, count, gold):
    """Best-of-K ("oracle") span F1 on the host.  spans_k (B, K, L-1, 2) and count (B,): the k-best trees of cliora_amd.kbest (arrays
    or tensors; (-1, -1) rows are padding); gold: per sentence its constituents, the root excluded.  Each tree is counted as
    ``SpanF1.add_counts`` counts a sentence -- span sets, the predicted root (the tree's last row) dropped as cliora_ground_eval
    drops it -- and a sentence keeps its tree with the highest sentence F1, the first on a tie.  -> dict: best_rank and best_f1 per
    sentence, and the corpus figures of the kept trees, oracle_corpus_f1 and oracle_sent_f1, beside rank 0's own (corpus_f1,
    sent_f1).  A sentence with count 0 is skipped (best_rank -1, best_f1 nan)."""
    spans_k = spans_k.cpu().numpy() if isinstance(spans_k, torch.Tensor) else np.asarray(spans_k)
    count = count.cpu().numpy() if isinstance(count, torch.Tensor) else np.asarray(count)
    first, best = SpanF1(), SpanF1()
    best_rank, best_f1 = [], []
    for b in range(spans_k.shape[0]):
        g = set((int(s), int(e)) for s, e in gold[b])
        keep = None
        for t in range(int(count[b])):
            rows = [tuple(r) for r in spans_k[b, t].tolist() if r[0] >= 0]
            pred = set(rows[:-1])
            one = SpanF1()
            one.add_counts(len(pred & g), len(pred), len(g))
            if t == 0:
                first.add_counts(len(pred & g), len(pred), len(g))
            if keep is None or one.sentence[0] > keep[1]:
                keep = (t, one.sentence[0], len(pred & g), len(pred))
        if keep is None:
            best_rank.append(-1)
            best_f1.append(float('nan'))
            continue
        best.add_counts(keep[2], keep[3], len(g))
        best_rank.append(keep[0])
        best_f1.append(keep[1])
    mean = lambda f: float(np.mean(np.array(f.sentence))) if f.sentence else float('nan')
    return dict(best_rank=best_rank, best_f1=best_f1, oracle_corpus_f1=best.corpus_f1, oracle_sent_f1=mean(best),
                corpus_f1=first.corpus_f1, sent_f1=mean(first))


def oracle_f1_given_brackets(diora, entity_labels, gold, k, lengths=None):
    """``oracle_f1`` over the k best trees that keep the annotated phrases: the upper bound on a model's span F1 once the gold noun
    phrases are given.  diora: a chart module after its forward; entity_labels: batch_map['entity_labels'], turned into required
    brackets by ``constrained.brackets_from_entity_labels`` (crossing phrases dropped, so some tree always qualifies); gold, k: as
    ``oracle_f1`` and ``kbest.kbest_spans`` take them; lengths: an int32 tensor (B,) for a right-padded batch.  A rejected sentence (a
    phrase outside its sentence) raises.  -> oracle_f1's dict: corpus_f1 / sent_f1 are the best constrained tree's."""
    from . import constrained
    required = constrained.brackets_from_entity_labels(entity_labels)
    kb = constrained.constrained_kbest(diora, constrained.pack_brackets(required), k, lengths)
    constrained.refuse_rejected(int(kb.status.sum().item()), 'cliora_kbest_spans_constrained')
    return oracle_f1(kb.spans, kb.count, gold)


def expected_f1(spans_s, gold):
    """Expected span F1 under sampled trees, on the host.  spans_s (B, S, L-1, 2): the trees of cliora_amd.sample (an array or a
    tensor; (-1, -1) rows are padding); gold: per sentence its constituents, the root excluded.  Each sample is counted as
    ``oracle_f1`` counts a tree -- span sets, the predicted root (its last row) dropped -- and a sentence's figure is the mean of its
    samples' sentence F1: a Monte-Carlo estimate of the expectation of F1 under the distribution the trees were drawn from.
    -> dict: sentence (per sentence; nan for one without a sampled tree, which is skipped) and expected_sent_f1, their mean."""
    spans_s = spans_s.cpu().numpy() if isinstance(spans_s, torch.Tensor) else np.asarray(spans_s)
    sentence = []
    for b in range(spans_s.shape[0]):
        g = set((int(s), int(e)) for s, e in gold[b])
        one = SpanF1()
        for t in range(spans_s.shape[1]):
            rows = [tuple(r) for r in spans_s[b, t].tolist() if r[0] >= 0]
            if not rows:
                continue
            pred = set(rows[:-1])
            one.add_counts(len(pred & g), len(pred), len(g))
        sentence.append(float(np.mean(np.array(one.sentence))) if one.sentence else float('nan'))
    kept = [f for f in sentence if f == f]
    return dict(sentence=sentence, expected_sent_f1=float(np.mean(np.array(kept))) if kept else float('nan'))


def batch_records(res, trees, sentences, example_ids, idx2word, with_boxes, post=False):
    """The batch's parse.jsonl lines (parse.py:215-280).  pred_spans / gold_spans in the iteration order of the reference's Python
    sets, built the same way (from the span list in reduce order, from GT[b][:-1]); pred_boxes in the order of pred_spans."""
    lines = []
    spans = res.spans.tolist()
    for b, tree in enumerate(trees):
        order = [tuple(s) for s in spans[b][:-1]]
        pred = set(order)
        gold = set(res.targets.gold[b])
        boxes = []
        if with_boxes:
            first = {}
            for k, s in enumerate(order):
                first.setdefault(s, k)
            boxes = [res.span_xyxy[b, first[s]].tolist() for s in pred]
        words = [idx2word[i] for i in sentences[b]]
        lines.append(parse_record(example_ids[b], tree, words, gold, pred, boxes, post=post))
    return lines


def evaluate(net, batches, idx2word, out_path=None, postprocess=False, decode='viterbi'):
    """parse.py:run (lines 101-291) on a harness.Net: eval mode, outside pass on, batches of length <= 2 skipped; returns the eight
    numbers it prints (METRICS) and writes parse.jsonl to `out_path` when given.  decode: 'viterbi' (the reference's tree) or 'mbr'
    (the minimum-Bayes-risk tree of cliora_amd.posterior: F1, CCRA and the records are then those of that tree) or 'hard' (the tree
    a hard chart's selections spell, hard_spans_device; refused on a module that is not hard)."""
    diora = net.diora
    if decode == 'hard' and not getattr(diora, 'hard', False):
        raise ValueError("decode='hard' needs a hard chart module (DioraMLP(hard=True), build_net(hard=True))")
    diora.outside = True
    net.eval()
    ev = Evaluator()
    dev = next(net.parameters()).device
    f = open(out_path, 'w') if out_path else None
    try:
        with torch.no_grad():
            for bm in batches:
                sentences = bm['sentences']
                if sentences.shape[1] <= 2:
                    continue
                obj = bm.get('obj_feats') if net.obj_feats else None
                out = net(sentences.to(dev), obj.to(dev) if obj is not None else None, bm['neg_samples'].to(dev), compute_loss=True)
                ev.add_losses(out)
                res = ground_batch(diora, bm, decode=decode)
                ev.add(res)
                if f is not None:
                    trees = diora.trees_from_spans(res.spans)
                    with_boxes = getattr(diora, 'all_atten_score', None) is not None
                    for line in batch_records(res, trees, sentences.cpu().tolist(), bm['example_ids'], idx2word, with_boxes, postprocess):
                        f.write(line + '\n')
    finally:
        if f is not None:
            f.close()
    return ev.result()


def evaluate_ragged(net, examples, idx2word, out_path=None, postprocess=False, max_batch=64, max_waste=None, pad_id=0,
                    return_details=False, decode='viterbi', max_len=64, max_long_batch=8):
    """``evaluate`` for examples of any lengths, given in any order: the sentences are packed into right-padded charts
    (cliora_amd.ragged), each pack costs one forward with the outside pass (cliora_chart_forward_ragged), one cliora_cky_spans_ragged,
    one cliora_ground_eval_ragged and one device-to-host copy, and the results come back in the caller's order.

    examples: dicts with 'sentence' (token ids), 'example_id', 'GT' (gold constituents, the root last, as batch_map['GT'][b]) and,
    for a CLIORA net, 'VG_GT' ((phrase dict, noun mask) as batch_map['VG_GT'][b]), 'boxes' (R, 4) and 'obj_feats' (R, img_dim).
    Examples of length <= 2 are skipped, as ``evaluate`` skips such batches.  Returns the first four METRICS (corpus_f1, sent_f1,
    ground_acc, ccra); parse.jsonl goes to `out_path` in the caller's order.  The four loss fields are left out: the reference defines
    the eval losses per uniform-length batch (the reconstruction loss reads every leaf of the batch and shares its negatives, the
    contrastive and VG losses compare the sentences of a batch with each other), and their ops take no per-sentence lengths.  return_details: also a list with, per
    example, None (skipped) or a dict of spans (n-1, 2), sent (3,), hit / ccr / word / box per phrase and span_xyxy (n-1, 4).
    decode: 'viterbi' or 'mbr', as ``evaluate``, or 'hard' on a hard net (the packs then run cliora_chart_forward_ragged_hard and the
    trees are those of cliora_hard_spans_ragged; refused on a net that is not hard).  max_len: the longest sentence taken, 64 or up to 128 (an unfiltered test set); a
    pack topped by a sentence of more than 64 words then holds at most `max_long_batch` sentences (``ragged.forward_ragged``)."""
    from . import ragged
    diora = net.diora
    if decode == 'hard':                # before decode_entry, which keeps refusing the name: a hard net's own padded chart and walk
        if not getattr(diora, 'hard', False):
            raise ValueError("decode='hard' needs a hard chart module (DioraMLP(hard=True), build_net(hard=True))")
        entry, forward_entry = 'cliora_hard_spans_ragged', 'cliora_chart_forward_ragged_hard'
    else:
        entry, forward_entry = ragged.decode_entry(decode), 'cliora_chart_forward_ragged'
    keep =[i for i, ex in enumerate(examples) if len(ex['sentence']) > 2]
    sents = [list(examples[i]['sentence']) for i in keep]
    vl = bool(net.obj_feats)
    feats = torch.stack([torch.as_tensor(examples[i]['obj_feats']) for i in keep]) if vl and keep else None
    details = [None] * len(examples)
    lines = [None] * len(examples)

    def per_pack(idx, lens, d):
        ex = [examples[keep[j]] for j in idx]
        B, L = len(idx), d._plan.L
        ns = [len(e['sentence']) for e in ex]
        atten = d.atten_score if vl else None
        tg = Targets([e['VG_GT'] for e in ex] if vl else None, [e['GT'] for e in ex], B, L, lengths=ns)
        boxes = torch.stack([torch.as_tensor(e['boxes'], dtype=torch.float32) for e in ex]) if vl else None
        cky_status = []

        def decode_into(out):
            if decode == 'hard':
                cky_status.append(ragged.hard_spans_ragged(d, lens, out=out)[1])
            else:
                cky_status.append(ragged.decode_spans_ragged(d, lens, decode, out=out)[1])

        res = ground(atten, boxes, tg, decode_into, device=d._wss[0].device, lengths=lens,
                     extra_status=[(forward_entry, d._ragged_status), (entry, lambda: cky_status[0])])
        off = tg.phr_off
        for b, j in enumerate(idx):
            n = ns[b]
            sl = slice(int(off[b]), int(off[b + 1]))
            det = dict(spans=res.spans[b, :n - 1].copy(), sent=res.sent[b].copy(), hit=res.hit[sl].copy(), ccr=res.ccr[sl].copy(),
                       word=res.word[sl].copy(), box=res.box[sl].copy(),
                       span_xyxy=res.span_xyxy[b, :n - 1].copy() if res.span_xyxy is not None else None)
            details[keep[j]] = det
            if out_path:
                one = GroundResult(Targets(None, [ex[b]['GT']], 1, n), det['spans'][None], np.zeros((0, 4), np.int32), det['sent'][None],
                                   det['span_xyxy'][None] if det['span_xyxy'] is not None else None)
                tree = diora.trees_from_spans(det['spans'][None])
                lines[keep[j]] = batch_records(one, tree, [list(ex[b]['sentence'])], [ex[b]['example_id']], idx2word, vl, postprocess)[0]

    ragged.forward_ragged(net, sents, obj_feats=feats, per_pack=per_pack, max_batch=max_batch,
                          max_waste=ragged.DEFAULT_MAX_WASTE if max_waste is None else max_waste, pad_id=pad_id, max_len=max_len,
                          max_long_batch=max_long_batch)
    ev = Evaluator()
    for det in details:                 # in the caller's order: the sentence F1s are averaged in it
        if det is not None:
            ev.add_counts(det['sent'], det['hit'], det['ccr'])
    if out_path:
        with open(out_path, 'w') as f:
            for line in lines:
                if line is not None:
                    f.write(line + '\n')
    m = {k: v for k, v in ev.result().items() if k in METRICS[:4]}
    return (m, details) if return_details else m


def _inside_only(nets):
    """Context of chart_divergence: every net in eval mode with its outside pass off; modes and flags restored on exit."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        was = [(n.training, n.diora.outside) for n in nets]
        try:
            for n in nets:
                n.eval()
                n.diora.outside = False
            with torch.no_grad():
                yield
        finally:
            for n, (training, outside) in zip(nets, was):
                n.diora.outside = outside
                n.train(training)
    return cm()


def _divergence_result(ab, ba):
    ab, ba = (np.concatenate(v) if v else np.zeros(0, dtype=np.float32) for v in (ab, ba))
    return dict(kl_ab=float(ab.mean()) if ab.size else 0.0, kl_ba=float(ba.mean()) if ba.size else 0.0, per_sentence_ab=ab, per_sentence_ba=ba)


def _pair_divergence(a, b, ab, ba, lengths=None):
    """KL(a || b) and KL(b || a) of two chart modules after their forwards, appended per sentence; one device-to-host copy."""
    from .query import host_copy
    from .structured import tree_kl
    r1 = tree_kl(a, b, lengths=lengths, student_grad=False)
    r2 = tree_kl(b, a, lengths=lengths, student_grad=False)
    k1, k2, s1, s2 = host_copy(r1.kl, r2.kl, r1.status, r2.status)
    if int(s1.sum()) or int(s2.sum()):
        raise _lib.ChartLibError('cliora_tree_kl rejected %d sentence length(s)' % max(int(s1.sum()), int(s2.sum())))
    ab.append(k1.copy())
    ba.append(k2.copy())


def chart_divergence(net_a, net_b, batches):
    """How far two nets' parse distributions lie apart on the same batches (cliora_amd.structured.tree_kl):
    both nets run their inside pass in eval mode under no_grad on each batch_map ('sentences', and 'obj_feats' for a net with
    regions), then KL(a || b) and KL(b || a) per sentence -- two launches and ONE device-to-host copy per batch.  The nets may differ
    in width, regions, weight sharing, soft or hard; batches of one length each, up to 64 words.
    -> dict(kl_ab, kl_ba: the means over all sentences; per_sentence_ab, per_sentence_ba: fp32 arrays in the batches' order)."""
    ab, ba = [], []
    with _inside_only((net_a, net_b)):
        for bm in batches:
            for net in (net_a, net_b):
                dev = next(net.parameters()).device
                obj = bm.get('obj_feats') if net.obj_feats else None
                net(bm['sentences'].to(dev), obj.to(dev) if obj is not None else None, None, compute_loss=False)
            _pair_divergence(net_a.diora, net_b.diora, ab, ba)
    return _divergence_result(ab, ba)


def chart_divergence_ragged(net_a, net_b, sentences, obj_feats=None, max_batch=64, max_waste=None, pad_id=0):
    """``chart_divergence`` for sentences of any lengths in 1..64, given in any order: they are packed into right-padded charts
    (cliora_amd.ragged.pack), both nets run the inside pass of each pack -- prefix-closed, so each sentence's own triangle holds its
    own scores -- and the divergence reads each triangle through the pack's lengths.  obj_feats: (N, R, img_dim) for the nets that
    have regions.  The per-sentence arrays come back in the caller's order."""
    from . import ragged
    lengths = ragged._check_batch(net_a, sentences, obj_feats if net_a.obj_feats else None, ragged.MAX_L, 'inside')[1]
    ragged._check_batch(net_b, sentences, obj_feats if net_b.obj_feats else None, ragged.MAX_L, 'inside')
    ab, ba, order = [], [], []
    with _inside_only((net_a, net_b)):
        for idx in (ragged.pack(lengths, max_batch, ragged.DEFAULT_MAX_WASTE if max_waste is None else max_waste) if lengths else ()):
            for net in (net_a, net_b):
                _, lens = next(ragged._forward_packs(net, sentences, lengths, [idx], pad_id, obj_feats if net.obj_feats else None, None))
            _pair_divergence(net_a.diora, net_b.diora, ab, ba, lengths=lens)
            order += list(idx)
    res = _divergence_result(ab, ba)
    back = np.argsort(np.asarray(order, dtype=np.int64), kind='stable')
    res['per_sentence_ab'], res['per_sentence_ba'] = res['per_sentence_ab'][back], res['per_sentence_ba'][back]
    return res
