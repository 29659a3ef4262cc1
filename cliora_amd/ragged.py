"""Sentences of different lengths parsed in one padded chart, decoded per sentence.

Every other entry point of the library takes a batch whose sentences have one length, the reference's own rule (it buckets by exact
length and never pads).  A caller who holds "these 40 captions" then pays one chain of dependent level launches and one CKY launch
per distinct length.  The inside pass is prefix-closed: cell (level, pos) with pos + level < n reads only cells of words [0, n).  So a
sentence of length n padded on the right to Lmax has, in its own triangle of the padded chart, the inside vectors, inside scores and
per-split scores a chart of length n would hold, and the CKY tree needs only those.  ``cliora_cky_spans_ragged`` (include/
cliora_chart.h) decodes each sentence from its own triangle; ``cliora_phrase_gather`` reads the inside vector of its own root cell.

The OUTSIDE pass is not prefix-closed (in a padded chart every cell has parents that reach beyond the sentence), but masking makes
it the sentence's own without touching a level kernel (``cliora_chart_forward_ragged``): a pair (parent,
sibling) of a cell of the triangle leaves the triangle iff its sibling does and its score adds inside_s[sibling], so -1e30 written
into inside_s beyond each triangle after the inside pass zeroes those pairs' softmax weights, and each sentence's root cell
(n - 1, 0) receives the seed rows after its level.  ``forward_ragged`` runs both passes that way, for text-only and CLIORA nets;
``evaluate.evaluate_ragged`` and ``phrases.embed_phrases_ragged`` are built on it.  Those entries are inference only.  They take
sentences of up to 64 words unless ``max_len`` is raised, to 128 at the most: a pack topped by a sentence of
more than 64 words runs on a forward-only plan through ``cliora_chart_forward_ragged_wide``, whose root-level mask is two words, and
holds at most ``max_long_batch`` sentences (such a plan's workspace is large: 1 300.8 MiB at B 8 / L 128 / D 400).

TRAINING through the same padded chart: ``forward_ragged_train`` runs each pack as one autograd node
(``diora.RaggedChartFunction``: cliora_chart_forward_ragged_train / cliora_chart_backward_ragged -- the cotangents are masked to
each triangle and each sentence's root cell is cut out of the outside backward, so the unchanged backward chains compute each
sentence's own gradient), ``reconstruction_loss_ragged`` is the reconstruction loss over the valid tokens, and
``harness.Trainer.step_ragged`` one optimizer step over all packs.  A CLIORA net trains the same way when given the region
features of every sentence (``obj_feats=``): the ``_vl`` forms of the two entries, and the VG and contrastive losses over each
sentence's own words and triangle (``harness.VGLoss`` / ``ContrastiveLoss`` with ``lengths``).

A HARD (S-DIORA) net -- ``build_net(hard=True)``, or a trained net whose ``diora.hard`` is set -- runs the same entries (DESIGN.md
section 29): ``forward_ragged``, ``forward_ragged_train`` and ``Trainer.step_ragged`` route its packs through
``cliora_chart_forward_ragged_hard`` (the module's ``_ragged_hard`` / ``_ragged_hard_train`` slots; ``diora.selection`` then holds the
pack's padded selection arrays, -1 wherever no cell of a sentence selects), ``parse_ragged_hard`` reads each sentence's tree off its
own inside selections (``cliora_hard_spans_ragged``), and ``evaluate.evaluate_ragged(decode='hard')`` scores those trees.

    from cliora_amd.ragged import parse_ragged, encode_ragged, forward_ragged
    trees = parse_ragged(net, sentences)        # net: harness.Net; sentences: lists of token ids, any lengths 1..64
    trees = parse_ragged(net, sentences, max_len=128)            # ... 1..128: the inside pass alone needs no root-level mask
    vecs = encode_ragged(net, sentences)        # (N, D) inside vectors of the sentences' roots, on the device
    trees = parse_ragged(vl_net, sentences, obj_feats=feats)     # a CLIORA net: region features (N, R, img_dim), one row per sentence
    forward_ragged(net, sentences, per_pack=lambda idx, lens, diora: ...)    # both passes; diora holds the pack's padded charts
    forward_ragged(net, sentences, per_pack=..., max_len=128)                # ... of sentences of 1..128 words
    for idx, lens, diora in forward_ragged_train(net, sentences): ...        # the same, one pack at a time, with autograd live
    for idx, lens, diora in forward_ragged_train(vl_net, sentences, obj_feats=feats): ...      # a CLIORA net with its images
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr_or_null as _p, stream as _stream
from .query import ChartQuery, host_copy, per_sentence, walk_spans

MAX_L = 64                # csrc/plan.hpp: CLIORA_MAX_L -- the default of max_len, the training charts, one word of the root-level mask
MAX_L_INSIDE = _lib.MAX_L_FWD    # csrc/plan.hpp: CLIORA_MAX_L_FWD -- what max_len may be raised to, for the inside-only and the both-pass entries
# Sentences in a pack topped by one of more than 64 words, for the both-pass entries: the batch the figures of a long plan's forward
# workspace are quoted for (1 300.8 MiB at B 8 / L 128 / D 400, 1 418 MiB with 36 regions); it grows with B.
DEFAULT_MAX_LONG_BATCH = 8
# Padded work a pack may carry beyond its sentences' own work, as a fraction of the latter.  Measured choice (tools/ragged_bench.py,
# profiles/ragged_bench.json): the best of the sweep on 64 mixed sentences (5.3x the bucketed path), within
# 2 % of the best on 1 000.
DEFAULT_MAX_WASTE = 2.0


def work(length):
    """Span pairs of one sentence's inside pass: sum over levels of (L - level) * level = (L^3 - L) / 6 compose rows."""
    length = int(length)
    return (length ** 3 - length) // 6


def pad_batch(sentences, pad_id=0):
    """-> (tokens (B, Lmax) int64, lengths (B,) int32), each sentence padded on the right with `pad_id`."""
    lengths = [len(s) for s in sentences]
    if not lengths:
        return torch.zeros((0, 0), dtype=torch.int64), torch.zeros((0,), dtype=torch.int32)
    if min(lengths) < 1:
        raise ValueError('an empty sentence has no chart')
    tokens = np.full((len(lengths), max(lengths)), pad_id, dtype=np.int64)
    for i, s in enumerate(sentences):
        tokens[i, :lengths[i]] = np.asarray(s, dtype=np.int64)
    return torch.from_numpy(tokens), torch.tensor(lengths, dtype=torch.int32)


def pack(lengths, max_batch=64, max_waste=DEFAULT_MAX_WASTE, max_long_batch=None):
    """Cut the sentences into batches that each share one padded chart: -> list of index lists.

    The indices are sorted by length (longest first, ties by index) and cut greedily: a batch takes the next sentence while it holds
    fewer than `max_batch` and its padded work, len(batch) * work(longest), stays within (1 + max_waste) times the sum of its
    sentences' own work().  max_waste = 0 buckets by exact work (sentences of length 1 cost nothing and ride along with each other
    only), float('inf') fills every batch.  max_long_batch: a batch whose longest sentence has more than 64 words (it runs on a
    forward-only plan, whose workspace is large) takes at most that many sentences; None: no such cap.  Pure and deterministic."""
    if max_batch < 1:
        raise ValueError('max_batch must be at least 1')
    if max_long_batch is not None and max_long_batch < 1:
        raise ValueError('max_long_batch must be at least 1')
    if not max_waste >= 0:
        raise ValueError('max_waste must be >= 0')
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    packs, cur, exact, top, cap = [], [], 0, 0, max_batch
    for i in order:
        w = work(lengths[i])
        if cur and (len(cur) >= cap or (len(cur) + 1) * top > (1.0 + max_waste) * (exact + w)):
            packs.append(cur)
            cur, exact = [], 0
        if not cur:
            top = w
            cap = min(max_batch, max_long_batch) if max_long_batch is not None and int(lengths[i]) > MAX_L else max_batch
        cur.append(i)
        exact += w
    if cur:
        packs.append(cur)
    return packs


def decode_ragged_numpy(pair_s, lengths, L=None):
    """The decode of cliora_cky_spans_ragged restated in numpy, for tests: `pair_s[level]` (B, Lmax - level, level) are the per-split
    inside scores of the PADDED chart; sentence b is decoded from levels 1 .. n-1 at positions pos < n - level, candidate
    (val_l + val_r) + (s - max s) in fp32, first maximum wins.  -> per sentence the list of (start, end), children before parents;
    with L, the padded chart's length, also the chosen splits: (spans, split (B, C) int32, -1 at the leaves and outside each triangle)."""
    out = []
    split = None if L is None else np.full((len(lengths), L * (L + 1) // 2), -1, dtype=np.int32)
    for b, n in enumerate(int(x) for x in lengths):
        val = {(0, p): np.float32(1.0) for p in range(n)}
        bp = {}
        for level in range(1, n):
            s = np.asarray(pair_s[level][b], dtype=np.float32)
            for pos in range(n - level):
                row = s[pos, :level]
                rel = row - row.max()
                cand = np.array([(val[(k, pos)] + val[(level - k - 1, pos + k + 1)]) + rel[k] for k in range(level)], dtype=np.float32)
                k = int(np.argmax(cand))
                val[(level, pos)], bp[(level, pos)] = cand[k], k
                if split is not None:
                    split[b, L * (L + 1) // 2 - (L - level) * (L - level + 1) // 2 + pos] = k
        out.append(walk_spans(n, lambda level, pos: bp[(level, pos)]))
    return out if split is None else (out, split)


def cky_spans_ragged(diora, lengths, split_out=False, out=None):
    """cliora_cky_spans_ragged on a chart module after its forward over a right-padded batch.

    lengths: int32 tensor (B,), one per sentence of the chart.  -> (spans, status) or (spans, status, split): spans (B, L-1, 2) int32
    with (-1, -1) beyond each sentence's n - 1 rows; status (number of workspaces,) int32 counting the lengths outside [1, L], which
    the caller must check; split (B, C) int32, -1 at the leaves and outside each triangle.  Device tensors; nothing is synchronised.
    out: a contiguous int32 tensor (B, L-1, 2) on the chart's device to decode into (cliora_amd.evaluate: its output buffer)."""
    q = ChartQuery(diora)
    q.check_int32('lengths', lengths)
    spans, status = q.spans(out), q.status(zeroed=False)
    split = q.empty(torch.int32, q.plan.C) if split_out else None
    q.launch('cliora_cky_spans_ragged', per_sentence(q.moved(lengths)), per_sentence(split), per_sentence(spans), status=status)
    return (spans, status, split) if split_out else (spans, status)


def root_rows(diora, lengths):
    """(B, D) inside vectors of the sentences' own root cells (n - 1, 0) of a padded chart: one cliora_phrase_gather launch over the
    device table (b, 0, lengths[b]), whose outside half is pointed at the inside chart and dropped (the outside pass is off)."""
    ih = diora.chart.inside_h
    B, Cc, D = ih.shape
    L = diora._plan.L
    dev = ih.device
    with torch.cuda.device(dev):
        n = lengths.to(dev).to(torch.int32)
        tab = torch.stack([torch.arange(B, dtype=torch.int32, device=dev), torch.zeros_like(n), n], 1).contiguous()
        out = torch.empty((B, 2 * D), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call('cliora_phrase_gather', B, L, D, _p(ih), ih.stride(0), ih.stride(1), _p(ih), ih.stride(0), ih.stride(1), B, _p(tab),
                  0, _p(out), out.stride(0), 0, _p(status), _stream())
        bad = int(status.item())
    if bad:
        raise _lib.ChartLibError('%d sentence length(s) outside 1..%d' % (bad, L))
    return out[:, :D]


def root_level_mask(lengths, max_len=MAX_L):
    """Bit t set iff some sentence has n - 1 == t: the outside levels after which cliora_chart_forward_ragged seeds a root.  A
    Python int of up to max_len bits (64, or 128 for cliora_chart_forward_ragged_wide, which takes it as two words:
    ``diora.ragged_chart`` splits it); a length outside 1..max_len sets no bit."""
    max_len = int(max_len)
    if not 1 <= max_len <= MAX_L_INSIDE:
        raise ValueError('max_len must be in 1..%d' % MAX_L_INSIDE)
    m = 0
    for n in lengths:
        if 1 <= int(n) <= max_len:
            m |= 1 << (int(n) - 1)
    return m


def _check_batch(net, sentences, obj_feats, max_len, kind):
    """What every entry here checks before any pack runs: which module this is and whether it may have regions, the sentences, the
    length limit.  kind: 'inside' (the inside pass alone), 'both' (both passes, inference) or 'train' (forward_ragged_train), which
    picks the messages.  -> (the net has regions, the sentences' lengths)."""
    from .cliora import DioraMLP as VLDiora
    from .diora import DioraMLP as TextDiora
    diora, train = net.diora, kind == 'train'
    vl = isinstance(diora, VLDiora)
    if (vl and obj_feats is None) or not (vl or isinstance(diora, TextDiora)):
        if train:
            raise NotImplementedError('training through a padded chart of mixed lengths is text-only DIORA (cliora_amd.diora.DioraMLP), got %s%s'
                                      % (type(diora).__name__, ' without obj_feats' if vl else ''))
        if vl:
            raise NotImplementedError(
                'the vision-language module scores regions against inside_h + outside_h of every cell: pass the region features of '
                'every sentence (obj_feats=) to run it on a padded chart')
        raise NotImplementedError('ragged batches need cliora_amd.diora.DioraMLP or cliora_amd.cliora.DioraMLP, got %s'
                                  % type(diora).__name__)
    if not vl and obj_feats is not None:
        raise ValueError('obj_feats given to a text-only net')
    if train and not torch.is_grad_enabled():
        raise _lib.ChartLibError('forward_ragged_train needs gradients enabled; forward_ragged runs the same batch for inference')
    lengths = [len(s) for s in sentences]
    if not lengths:
        return vl, lengths
    if min(lengths) < 1:
        raise ValueError('an empty sentence has no chart')
    if vl and len(obj_feats) != len(sentences):
        raise ValueError('obj_feats holds %d sentences, not %d' % (len(obj_feats), len(sentences)))
    if not 1 <= int(max_len) <= MAX_L_INSIDE:
        raise ValueError('max_len must be in 1..%d' % MAX_L_INSIDE)
    if max(lengths) > max_len:
        if train:
            raise _lib.ChartLibError('L > %d is not supported by the padded training chart (got a sentence of %d words)' % (MAX_L, max(lengths)))
        if kind == 'both' and max_len == MAX_L:
            raise _lib.ChartLibError('L > %d is not supported by the both-pass padded chart (its root-level mask holds %d levels; got a '
                                     'sentence of %d words): run longer sentences through the uniform-length entry points'
                                     % (MAX_L, MAX_L, max(lengths)))
        raise _lib.ChartLibError('L > %d is not supported (got a sentence of %d words)%s' % (
            max_len, max(lengths), ': pass max_len=%d for sentences of up to %d words' % (MAX_L_INSIDE, MAX_L_INSIDE)
            if max_len < MAX_L_INSIDE and max(lengths) <= MAX_L_INSIDE else ''))
    return vl, lengths


def _forward_packs(net, sentences, lengths, packs, pad_id, obj_feats, slot, max_len=MAX_L):
    """The one loop over the packs, a generator: per pack pad, embed, encode the pack's regions (obj_feats, else None) and run the
    chart module's forward -- with (lengths on the device, root-level mask) in the module's slot `slot` ('_ragged', '_ragged_train';
    for a hard module '_ragged_hard', '_ragged_hard_train' in their place) around it, cleared whatever happens; slot None: the
    module's ordinary forward -- then yield (indices, lengths on the device)."""
    diora = net.diora
    dev = next(net.parameters()).device
    if slot is not None and getattr(diora, 'hard', False):      # a hard module's own slots: cliora_chart_forward_ragged_hard
        slot = {'_ragged': '_ragged_hard', '_ragged_train': '_ragged_hard_train'}[slot]
    for idx in packs:
        tokens, lens = pad_batch([sentences[i] for i in idx], pad_id)
        x_span, x_word = net.embed(tokens.to(dev))
        o_span = o_word = None
        if obj_feats is not None:
            o_span, o_word = net.img_encoder(obj_feats[torch.as_tensor(idx, dtype=torch.int64)].to(dev))
        lens = lens.to(dev)
        if slot is not None:
            diora.__dict__[slot] = (lens, root_level_mask((lengths[i] for i in idx), max_len))
        try:
            diora(x_span, x_word, o_span, o_word)
        finally:
            if slot is not None:
                diora.__dict__[slot] = None
        yield idx, lens


def _run_packs(net, sentences, max_batch, max_waste, pad_id, per_pack, obj_feats=None, outside=False, max_len=MAX_L, max_long_batch=None):
    """pack -> per pack: pad, embed (and encode the regions), chart forward, `per_pack(indices, lengths_on_device)`.  outside False:
    the inside pass alone through the module's ordinary forward; True: both passes through cliora_chart_forward_ragged (a pack of
    L > 64: cliora_chart_forward_ragged_wide).  max_len: the longest sentence taken (64, or up to 128); a longer one is refused before
    any pack has run.  max_long_batch: ``pack``'s."""
    diora = net.diora
    _, lengths = _check_batch(net, sentences, obj_feats, max_len, 'both' if outside else 'inside')
    if not lengths:
        return
    was_training, had_outside = net.training, diora.outside
    net.eval()
    diora.outside = bool(outside)
    try:
        with torch.no_grad():
            for idx, lens in _forward_packs(net, sentences, lengths, pack(lengths, max_batch, max_waste, max_long_batch), pad_id, obj_feats,
                                            '_ragged' if outside else None, max_len):
                per_pack(idx, lens)
    finally:
        diora.outside = had_outside
        net.train(was_training)


def forward_ragged(net, sentences, obj_feats=None, per_pack=None, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, max_len=MAX_L,
                   max_long_batch=DEFAULT_MAX_LONG_BATCH):
    """Both passes over sentences of any lengths in 1..max_len (64; up to 128 when asked for: a pack whose longest sentence has more
    than 64 words runs on a forward-only plan through cliora_chart_forward_ragged_wide and, with max_len > 64, holds at most
    `max_long_batch` sentences): packs them (``pack``), runs each pack as one right-padded chart through
    cliora_chart_forward_ragged in eval mode under no_grad, and calls ``per_pack(indices, lengths, diora)`` after each -- `indices`
    the pack's positions in `sentences`, `lengths` their int32 lengths on the device, `diora` the chart module holding the pack's
    state: the four charts, valid on each sentence's own triangle (cells beyond it are unspecified), and for a CLIORA net
    atten_score[b, :n_b] / vg_atten_score.  `diora._ragged_status` is the call's status word, still on the device: the callback (or
    whoever reads the pack's results) must find it 0.  obj_feats: (N, R, img_dim) region features, one row per sentence, for a
    CLIORA net.  Returns the packs.  Training mode and the module's `outside` are restored afterwards."""
    packs = []

    def each(idx, lens):
        packs.append(idx)
        if per_pack is not None:
            per_pack(idx, lens, net.diora)

    _run_packs(net, sentences, max_batch, max_waste, pad_id, each, obj_feats=obj_feats, outside=True, max_len=max_len,
               max_long_batch=max_long_batch if int(max_len) > MAX_L else None)
    return packs


def forward_ragged_train(net, sentences, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, obj_feats=None):
    """forward_ragged with autograd live, sentences of any lengths in 1..64: a generator that packs them (``pack``) and, one pack at a
    time, pads, embeds and runs the pack as one right-padded chart through ``diora.RaggedChartFunction``, then yields
    ``(indices, lengths, diora)`` -- `indices` the pack's positions in `sentences`, `lengths` their int32 lengths on the device,
    `diora` the chart module holding the pack's charts in the autograd graph: valid on each sentence's own triangle; cells beyond it
    are unspecified and their cotangents are ignored.  Text-only DIORA, or a CLIORA net with obj_feats (N, R, img_dim), one row of
    region features per sentence: each pack then encodes its images, and the module also holds vg_atten_score and all_atten_score of
    the pack, to be read through the length-aware losses (harness.VGLoss / ContrastiveLoss with `lengths`).  The status word is read
    after each forward (one synchronisation per pack) and a rejected length raises.  The structured losses of the module
    (bracket_nll, tree_objective, ...) read each sentence's own triangle.  Gradients must be enabled; the net's mode is the caller's."""
    diora = net.diora
    vl, lengths = _check_batch(net, sentences, obj_feats, MAX_L, 'train')
    for idx, lens in _forward_packs(net, sentences, lengths, pack(lengths, max_batch, max_waste), pad_id, obj_feats, '_ragged_train'):
        bad = int(diora._ragged_status.item())
        if bad:
            raise _lib.ChartLibError('cliora_chart_forward_ragged_%s rejected %d sentence length(s)'
                                     % ('hard' if getattr(diora, 'hard', False) else 'train_vl' if vl else 'train', bad))
        yield idx, lens, diora


class _LeafRows(object):
    """What a reconstruction loss reads of a chart module (outside_h), holding the valid leaf rows as sentences of one word."""
    __slots__ = ('outside_h',)

    def __init__(self, outside_h):
        self.outside_h = outside_h


def reconstruction_loss_ragged(net, pack_sentences, neg_samples, diora=None):
    """The reconstruction loss (harness.ReconstructionSoftmaxLoss) of a padded chart over its VALID tokens: the leaf rows
    outside_h[b, :n_b] and their tokens are gathered and presented to the loss as N_valid sentences of one word, so the mean is over
    the sum of the lengths and no padded position contributes.  pack_sentences: the token lists of the chart's sentences, in its
    order.  -> a 0-d tensor in the graph."""
    diora = net.diora if diora is None else diora
    oh = diora.chart.outside_h
    lens = [len(s) for s in pack_sentences]
    if len(lens) != oh.shape[0]:
        raise ValueError('pack_sentences holds %d sentences, the chart %d' % (len(lens), oh.shape[0]))
    rows = torch.from_numpy(np.repeat(np.arange(len(lens), dtype=np.int64), lens)).to(oh.device)
    pos = torch.from_numpy(np.concatenate([np.arange(n, dtype=np.int64) for n in lens])).to(oh.device)
    tokens = torch.from_numpy(np.concatenate([np.asarray(s, dtype=np.int64) for s in pack_sentences])).to(oh.device)
    cells = oh[rows, pos].unsqueeze(1)                   # (N_valid, 1, D): the leaf cell of a one-word chart is its cell 0
    return net.reconstruct_softmax_loss(tokens.view(-1, 1), neg_samples, _LeafRows(cells))


def decode_entry(decode):
    """The one check of a decode's name: 'viterbi' or 'mbr' -> the C entry that decodes a padded chart that way, for messages."""
    if decode not in ('viterbi', 'mbr'):
        raise ValueError("decode must be 'viterbi' or 'mbr', not %r" % (decode,))
    return 'cliora_span_posteriors' if decode == 'mbr' else 'cliora_cky_spans_ragged'


def decode_spans_ragged(diora, lengths, decode='viterbi', out=None):
    """The span decode of a padded chart by name: 'viterbi' (cliora_cky_spans_ragged) or 'mbr' (cliora_span_posteriors' MBR tree,
    cliora_amd.posterior).  -> (spans, status, the entry's name for messages), spans decoded into `out` when given."""
    entry = decode_entry(decode)
    if decode == 'viterbi':
        return cky_spans_ragged(diora, lengths, out=out) + (entry,)
    from . import posterior
    post = posterior.span_posteriors(diora, lengths, mbr=True, out=out)
    return post.spans, post.status, entry


def parse_ragged(net, sentences, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, obj_feats=None, max_len=MAX_L, decode='viterbi',
                 max_long_batch=None):
    """Best binary tree of every sentence (nested tuples of word positions as ``DioraBase.cky()``; 0 for a single word), in the
    caller's order.  net: a harness.Net; sentences: sequences of token ids of any lengths in 1..max_len (64; up to 128 when asked for:
    a pack whose longest sentence has more than 64 words runs on a forward-only plan); obj_feats: the region features
    (N, R, img_dim) of a CLIORA net, one row per sentence.  Runs in eval mode under no_grad with the outside pass off (both restored
    afterwards; the module's chart is left as the last pack's, outside_h unwritten).  One device-to-host copy per pack.
    decode: 'viterbi' (the reference's tree) or 'mbr' (the tree with the most expected correct brackets, cliora_amd.posterior).
    max_long_batch: ``pack``'s cap on a pack topped by a sentence of more than 64 words (None: none)."""
    diora = net.diora
    trees = [None] * len(sentences)
    decode_entry(decode)                             # a bad name is refused before any pack has run

    def decode_pack(idx, lens):
        spans, status, entry = decode_spans_ragged(diora, lens, decode)
        rows, status = host_copy(spans, status)                             # the pack's one device-to-host copy
        if status.any():
            raise _lib.ChartLibError('%s rejected %d sentence length(s)' % (entry, int(status.sum())))
        for b, i in enumerate(idx):
            trees[i] = diora.trees_from_spans(rows[b:b + 1, :len(sentences[i]) - 1])[0]

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, obj_feats=obj_feats, max_len=max_len, max_long_batch=max_long_batch)
    return trees


def hard_spans_ragged(diora, lengths, out=None):
    """cliora_hard_spans_ragged on a hard chart module after its forward over a right-padded batch: the tree each sentence's own
    inside selections spell.  lengths: int32 tensor (B,).  -> (spans (B, L-1, 2) int32 with (-1, -1) beyond each sentence's n - 1 rows,
    status (1,) int32 counting the lengths outside [1, L], which the caller must check).  Device tensors; nothing is synchronised."""
    return diora.hard_spans_device(out=out, lengths=lengths)


def parse_ragged_hard(net, sentences, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, max_len=MAX_L_INSIDE, max_long_batch=None):
    """The hard (S-DIORA) tree of every sentence -- the one its own inside selections spell, no CKY pass -- in the caller's order, as
    ``parse_ragged`` returns trees.  net: a harness.Net whose chart module is hard (build_net(hard=True), or .hard set).  Packs like
    ``parse_ragged`` and runs the inside pass alone through the module's ordinary hard forward on the padded batch (the inside pass
    is prefix-closed, hard or soft: DESIGN.md section 29), then cliora_hard_spans_ragged; sentences of up to 128 words.  One
    device-to-host copy per pack."""
    diora = net.diora
    if not getattr(diora, 'hard', False):
        raise ValueError('parse_ragged_hard needs a hard chart module (DioraMLP(hard=True), build_net(hard=True)); parse_ragged decodes a soft one')
    trees = [None] * len(sentences)

    def decode_pack(idx, lens):
        rows, status = host_copy(*hard_spans_ragged(diora, lens))                # the pack's one device-to-host copy
        if status.any():
            raise _lib.ChartLibError('cliora_hard_spans_ragged rejected %d sentence length(s)' % int(status.sum()))
        for b, i in enumerate(idx):
            trees[i] = diora.trees_from_spans(rows[b:b + 1, :len(sentences[i]) - 1])[0]

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, max_len=max_len, max_long_batch=max_long_batch)
    return trees


def parse_ragged_kbest(net, sentences, k, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, obj_feats=None, max_len=MAX_L_INSIDE):
    """The k best binary trees of every sentence (cliora_amd.kbest), in the caller's order: per sentence the list of its
    (tree, score), best first -- min(k, Catalan(n - 1)) nested tuples as ``parse_ragged`` returns them (0 for a single word), each
    with the sum of its potentials.  Packs like ``parse_ragged`` and runs the inside pass only, so sentences of up to 128 words are
    taken (max_len).  One device-to-host copy per pack."""
    from . import kbest
    diora = net.diora
    out = [None] * len(sentences)
    k = int(k)
    if not 1 <= k <= kbest.MAX_K:                    # refused before any pack has run
        raise ValueError('k must be in 1..%d' % kbest.MAX_K)

    def decode_pack(idx, lens):
        kb = kbest.kbest_spans(diora, k, lens)
        rows, scores, count, status = host_copy(kb.spans, kb.scores, kb.count, kb.status)
        if status.any():
            raise _lib.ChartLibError('cliora_kbest_spans rejected %d sentence length(s)' % int(status.sum()))
        for b, i in enumerate(idx):
            trees = diora.trees_from_spans(rows[b, :count[b], :len(sentences[i]) - 1])
            out[i] = list(zip(trees, scores[b, :count[b]].tolist()))

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, obj_feats=obj_feats, max_len=max_len)
    return out


def parse_ragged_samples(net, sentences, S, seed, beta=1.0, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, obj_feats=None,
                         max_len=MAX_L_INSIDE):
    """S binary trees of every sentence drawn from its posterior over parses (cliora_amd.sample), in the caller's order: per sentence
    the list of its S (tree, log_prob) -- nested tuples as ``parse_ragged`` returns them, ``[(0, 0.0)] * S`` for a single word.  A
    sentence's id in the draw is its index in `sentences`, so its samples do not depend on the pack it lands in.  Packs like
    ``parse_ragged`` and runs the inside pass only, so sentences of up to 128 words are taken (max_len).  One device-to-host copy
    per pack."""
    from . import sample
    diora = net.diora
    out = [None] * len(sentences)
    S = int(S)
    if not 1 <= S <= sample.MAX_S:                   # refused before any pack has run
        raise ValueError('S must be in 1..%d' % sample.MAX_S)
    if not (beta >= 0 and np.isfinite(beta)):
        raise ValueError('beta must be finite and >= 0')

    def decode_pack(idx, lens):
        ts = sample.sample_spans(diora, S, seed, lens, ids=torch.tensor(idx, dtype=torch.int32), beta=beta)
        rows, log_prob, status = host_copy(ts.spans, ts.log_prob, ts.status)
        if status.any():
            raise _lib.ChartLibError('cliora_sample_trees rejected %d sentence length(s)' % int(status.sum()))
        for b, i in enumerate(idx):
            trees = diora.trees_from_spans(rows[b, :, :len(sentences[i]) - 1])
            out[i] = list(zip(trees, log_prob[b].tolist()))

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, obj_feats=obj_feats, max_len=max_len)
    return out


def _ragged_brackets(sentences, required, forbidden):
    """required / forbidden as the ragged entries take them -> one list of spans per sentence each; refused before any pack has run."""
    from . import constrained
    required = [list(r) for r in required]
    forbidden = [[] for _ in sentences] if forbidden is None else [list(f) for f in forbidden]
    if len(required) != len(sentences) or len(forbidden) != len(sentences):
        raise ValueError('required and forbidden hold one list of spans per sentence (%d)' % len(sentences))
    if max([len(r) + len(f) for r, f in zip(required, forbidden)] or [0]) > constrained.MAX_M:
        raise ValueError('at most %d brackets per sentence' % constrained.MAX_M)
    return required, forbidden


def parse_ragged_constrained(net, sentences, required, forbidden=None, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, obj_feats=None,
                             max_len=MAX_L_INSIDE):
    """The best binary tree of every sentence under its brackets (cliora_amd.constrained), in the caller's order: per sentence
    (tree, log_prob) -- the tree nested tuples as ``parse_ragged`` returns them (0 for a single word), None when no tree keeps every
    span of required[i] and none of forbidden[i] (per-sentence lists of (start, end), inclusive word positions); log_prob the log of
    the joint probability of the brackets under the sentence's posterior over parses, -inf with None.  A sentence's result does not
    depend on the pack it lands in.  Packs like ``parse_ragged`` and runs the inside pass only, so sentences of up to 128 words are
    taken (max_len).  One device-to-host copy per pack; a bracket outside its sentence raises ChartLibError."""
    from . import constrained
    diora = net.diora
    out = [None] * len(sentences)
    required, forbidden = _ragged_brackets(sentences, required, forbidden)

    def decode_pack(idx, lens):
        brackets = constrained.pack_brackets([required[i] for i in idx], [forbidden[i] for i in idx])
        spans, feasible, log_prob, rejected = constrained.host_results(constrained.constrained_parse(diora, brackets, lens))
        constrained.refuse_rejected(rejected)
        for b, i in enumerate(idx):
            tree = diora.trees_from_spans(spans[b:b + 1, :len(sentences[i]) - 1])[0] if feasible[b] else None
            out[i] = (tree, float(log_prob[b]))

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, obj_feats=obj_feats, max_len=max_len)
    return out


def parse_ragged_kbest_constrained(net, sentences, k, required, forbidden=None, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0,
                                   obj_feats=None, max_len=MAX_L_INSIDE):
    """``parse_ragged_kbest`` among the trees that keep every span of required[i] and none of forbidden[i] (per-sentence lists of
    (start, end), inclusive word positions; cliora_amd.constrained.constrained_kbest), in the caller's order: per sentence the list of
    its (tree, score), best first -- min(k, the number of qualifying trees) of them, [] where none qualifies.  A sentence's result does
    not depend on the pack it lands in.  Sentences of up to 128 words are taken (max_len).  One device-to-host copy per pack; a
    bracket outside its sentence raises ChartLibError."""
    from . import constrained, kbest
    diora = net.diora
    out = [None] * len(sentences)
    k = int(k)
    if not 1 <= k <= kbest.MAX_K:                    # refused before any pack has run
        raise ValueError('k must be in 1..%d' % kbest.MAX_K)
    required, forbidden = _ragged_brackets(sentences, required, forbidden)

    def decode_pack(idx, lens):
        brackets = constrained.pack_brackets([required[i] for i in idx], [forbidden[i] for i in idx])
        kb = constrained.constrained_kbest(diora, brackets, k, lens)
        rows, scores, count, status = host_copy(kb.spans, kb.scores, kb.count, kb.status)
        constrained.refuse_rejected(int(status.sum()), 'cliora_kbest_spans_constrained')
        for b, i in enumerate(idx):
            trees = diora.trees_from_spans(rows[b, :count[b], :len(sentences[i]) - 1])
            out[i] = list(zip(trees, scores[b, :count[b]].tolist()))

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, obj_feats=obj_feats, max_len=max_len)
    return out


def parse_ragged_samples_constrained(net, sentences, S, seed, required, forbidden=None, beta=1.0, max_batch=64, max_waste=DEFAULT_MAX_WASTE,
                                     pad_id=0, obj_feats=None, max_len=MAX_L_INSIDE):
    """``parse_ragged_samples`` from each sentence's posterior over parses given its brackets (required / forbidden as
    ``parse_ragged_kbest_constrained`` takes them; cliora_amd.constrained.constrained_samples), in the caller's order: per sentence the
    list of its S (tree, log_prob), log_prob the log of the draw's probability among the qualifying trees; [] where no tree qualifies.
    A sentence's id in the draw is its index in `sentences`, so its samples do not depend on the pack it lands in.  Sentences of up to
    128 words are taken (max_len).  One device-to-host copy per pack; a bracket outside its sentence raises ChartLibError."""
    from . import constrained, sample
    diora = net.diora
    out = [None] * len(sentences)
    S = int(S)
    if not 1 <= S <= sample.MAX_S:                   # refused before any pack has run
        raise ValueError('S must be in 1..%d' % sample.MAX_S)
    if not (beta >= 0 and np.isfinite(beta)):
        raise ValueError('beta must be finite and >= 0')
    required, forbidden = _ragged_brackets(sentences, required, forbidden)

    def decode_pack(idx, lens):
        brackets = constrained.pack_brackets([required[i] for i in idx], [forbidden[i] for i in idx])
        ts = constrained.constrained_samples(diora, brackets, S, seed, lens, ids=torch.tensor(idx, dtype=torch.int32), beta=beta)
        rows, log_prob, feasible, status = host_copy(ts.spans, ts.log_prob, ts.feasible, ts.status)
        constrained.refuse_rejected(int(status.sum()), 'cliora_sample_trees_constrained')
        for b, i in enumerate(idx):
            trees = diora.trees_from_spans(rows[b, :, :len(sentences[i]) - 1]) if feasible[b] else []
            out[i] = list(zip(trees, log_prob[b].tolist()))

    _run_packs(net, sentences, max_batch, max_waste, pad_id, decode_pack, obj_feats=obj_feats, max_len=max_len)
    return out


def encode_ragged(net, sentences, max_batch=64, max_waste=DEFAULT_MAX_WASTE, pad_id=0, obj_feats=None, max_len=MAX_L, max_long_batch=None):
    """(N, D) fp32 on the device: row i = inside_h of sentence i's root cell (its own length's root, not the padded chart's), the
    vector DIORA users read off the root.  Same plumbing as parse_ragged, max_len and max_long_batch included."""
    diora = net.diora
    dev = next(net.parameters()).device
    out = torch.empty((len(sentences), diora.size), dtype=torch.float32, device=dev)

    def gather(idx, lens):
        out[torch.tensor(idx, dtype=torch.int64, device=dev)] = root_rows(diora, lens)

    _run_packs(net, sentences, max_batch, max_waste, pad_id, gather, obj_feats=obj_feats, max_len=max_len, max_long_batch=max_long_batch)
    return out
