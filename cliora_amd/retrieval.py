"""Caption-image retrieval on the device: the image-text matching logit of a trained CLIORA model over a whole split.

``VGLoss`` trains ``logits[a][c] = mean_l max_r <word_l of caption a, region_r of image c>`` inside one batch (cliora.py:460-464,
trainer.py:145-152).  Over a test split the same score is a weighted late-interaction ("MaxSim") product of grouped rows,

    S[n][m] = sum over the tokens t of caption n of  w[t] * max over the regions r of image m of <Q[t], O[r]>,

which cliora_maxsim_scores computes without writing a (tokens x regions) or (tokens x images) intermediate (include/cliora_chart.h,
DESIGN.md section 26), cliora_retrieval_ranks turns into the ranks behind Recall@K and the median rank, and cliora_score_topk into
the retrieved lists.  With ``Q = x_word, w = 1/L`` it is the training-mode logit; with ``Q = [(inside_h + outside_h)[leaves] |
unit(x_word)]`` against ``O = [obj_span | obj_word]`` the eval-mode one (a maximum over regions of a sum of two inner products is the
inner product of the concatenations); with span rows and posterior weights a span-level score.

    out = retrieve(net, captions, images, image_of)          # net: harness.Net with obj_feats; captions: lists of token ids
    out['t2i']['r_at_k'][1], out['i2t']['median_rank']

``maxsim_numpy``, ``retrieval_ranks_numpy`` and ``score_topk_numpy`` restate the kernels in fp64 for the tests, as ``kbest_numpy`` and
``sample_numpy`` restate theirs.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr_or_null as _p, stream as _stream

MAX_REGIONS = 256        # csrc/retrieval_kernels.hpp MAXSIM_MAX_REGIONS: an image lies inside one 256-row key step
MAX_K = 128
TINY = 1e-8              # utils.py:11, the floor of UnitNorm


# ---- fp64 restatements -------------------------------------------------------------------------------------------------------
def maxsim_numpy(q, q_off, w, keys, k_off, max_regions=MAX_REGIONS):
    """S (N, M) fp64 from the definition: an empty caption gives 0.0, an empty image -inf (0.0 against an empty caption), a NaN
    poisons its group's maximum, an image of more than `max_regions` regions or a group with a decreasing / out-of-range offset gives NaN."""
    q, keys, w = np.asarray(q, dtype=np.float64), np.asarray(keys, dtype=np.float64), np.asarray(w, dtype=np.float64)
    q_off, k_off = [int(x) for x in q_off], [int(x) for x in k_off]
    N, M = len(q_off) - 1, len(k_off) - 1
    S = np.zeros((N, M), dtype=np.float64)

    def bad(a, b, total):
        return a < 0 or b < a or b > total

    for n in range(N):
        qa, qb = q_off[n], q_off[n + 1]
        for m in range(M):
            ka, kb = k_off[m], k_off[m + 1]
            if bad(qa, qb, q.shape[0]) or bad(ka, kb, keys.shape[0]) or kb - ka > max_regions:
                S[n, m] = np.nan
            elif qb == qa:
                S[n, m] = 0.0
            elif kb == ka:
                S[n, m] = -np.inf
            else:
                with np.errstate(invalid='ignore'):
                    v = (q[qa:qb] @ keys[ka:kb].T).max(axis=1)
                    S[n, m] = float((w[qa:qb] * v).sum())
    return S


def _before(sa, ia, sb, ib):
    """a orders before b under knn_key: descending score, ascending index on ties, NaN below every number (elementwise, broadcasting)."""
    na, nb = np.isnan(sa), np.isnan(sb)
    with np.errstate(invalid='ignore'):
        gt, eq = sa > sb, sa == sb
    return (~na & nb) | (~na & ~nb & gt) | (((na & nb) | (~na & ~nb & eq)) & (ia < ib))


def retrieval_ranks_numpy(S, image_of):
    """(rank_t2i (N), rank_i2t (M), skipped) as cliora_retrieval_ranks defines them."""
    S = np.asarray(S, dtype=np.float64)
    N, M = S.shape
    image_of = np.asarray(image_of, dtype=np.int64)
    t2i, i2t, skipped = np.full(N, -1, dtype=np.int64), np.full(M, -1, dtype=np.int64), 0
    cols, rows = np.arange(M), np.arange(N)
    for n in range(N):
        g = int(image_of[n])
        if not 0 <= g < M:
            skipped += 1
            continue
        t2i[n] = int((_before(S[n], cols, S[n, g], g) & (cols != g)).sum())
    for m in range(M):
        mine = image_of == m
        best = -1
        for n in rows[mine]:
            c = int((_before(S[:, m], rows, S[n, m], n) & ~mine).sum())
            best = c if best < 0 else min(best, c)
        i2t[m] = best
    return t2i, i2t, skipped


def score_topk_numpy(S, k):
    """(D (rows, k) fp64, I (rows, k) int64): the k best of every row in knn_key's order, -inf / -1 past the columns."""
    S = np.asarray(S, dtype=np.float64)
    rows, cols = S.shape
    D, I = np.full((rows, k), -np.inf), np.full((rows, k), -1, dtype=np.int64)
    idx = np.arange(cols)
    for r in range(rows):
        place = _before(S[r][None, :], idx[None, :], S[r][:, None], idx[:, None]).sum(axis=1)      # how many order before each
        order = np.argsort(place, kind='stable')[:k]
        D[r, :len(order)], I[r, :len(order)] = S[r, order], order
    return D, I


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
def _offsets(off, dev):
    """-> (int32 device tensor, host list or None)."""
    if isinstance(off, torch.Tensor):
        if off.dim() != 1 or off.numel() < 1 or off.dtype not in (torch.int32, torch.int64):
            raise ValueError('offsets must be a 1-d int32 / int64 tensor of (groups + 1) entries')
        return off.to(device=dev, dtype=torch.int32).contiguous(), None
    host = [int(x) for x in off]
    if len(host) < 1:
        raise ValueError('offsets hold (groups + 1) entries')
    return torch.tensor(host, dtype=torch.int32).to(dev), host


def _ws_bytes(N, NT, M, MR, D):
    return _lib.fn('cliora_maxsim_workspace_bytes')(N, NT, M, MR, D)


def _maxsim(q, q_off, w, keys, k_off, max_workspace_mb):
    """The launches of maxsim_scores: -> (S, status (2,) int32 on the device, nothing synchronised unless the call has to be chunked
    and the caption offsets were given as a device tensor)."""
    if q.dim() != 2 or keys.dim() != 2 or q.shape[1] != keys.shape[1]:
        raise ValueError('queries %s and keys %s must be (rows, D) of one width' % (tuple(q.shape), tuple(keys.shape)))
    if w.dim() != 1 or w.shape[0] != q.shape[0]:
        raise ValueError('weights %s: one per query row (%d)' % (tuple(w.shape), q.shape[0]))
    for t in (q, keys, w):
        if t.dtype != torch.float32 or not t.is_cuda or t.device != q.device:
            raise ValueError('queries, weights and keys must be fp32 CUDA tensors on one device')
    for t in (q, keys):
        if t.shape[0] > 1 and t.stride(1) != 1:
            raise ValueError('queries and keys must have unit stride along D')
    if q.shape[1] < 1:
        raise ValueError('D = 0')
    w = w.contiguous()
    dev = q.device
    NT, D = q.shape
    MR = keys.shape[0]
    qo, qo_host = _offsets(q_off, dev)
    ko, _ = _offsets(k_off, dev)
    N, M = qo.numel() - 1, ko.numel() - 1
    ldq = q.stride(0) if NT > 1 else D
    ldo = keys.stride(0) if MR > 1 else D
    budget = int(max_workspace_mb * (1 << 20))
    with torch.cuda.device(dev):
        S = torch.empty((N, M), dtype=torch.float32, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        if N == 0 or M == 0:
            return S, status

        def run(n0, n1, r0, r1, off, st):
            ws = torch.empty(max(1, _ws_bytes(n1 - n0, r1 - r0, M, MR, D)), dtype=torch.uint8, device=dev)
            _lib.call('cliora_maxsim_scores', n1 - n0, r1 - r0, M, MR, D, C.c_void_p(q.data_ptr() + 4 * r0 * ldq) if r1 > r0 else C.c_void_p(0),
                      ldq, _p(off), C.c_void_p(w.data_ptr() + 4 * r0) if r1 > r0 else C.c_void_p(0), _p(keys), ldo, _p(ko),
                      C.c_void_p(S.data_ptr() + 4 * n0 * M), M, _p(st), _p(ws), ws.numel(), _stream())

        # the budget bounds what grows with the captions (their packed rows, their tiles' partials); the packed images are needed whatever the split
        limit = _ws_bytes(0, 0, M, MR, D) + budget
        if _ws_bytes(N, NT, M, MR, D) <= limit:
            run(0, N, 0, NT, qo, status)
            return S, status
        # chunks of captions: a caption's row of S does not depend on what else is in its call, so the result is bitwise the same
        if qo_host is None:
            qo_host = qo.cpu().tolist()
        bad = sum(1 for a, b in zip(qo_host[:-1], qo_host[1:]) if a < 0 or b < a or b > NT)
        if bad:
            raise _lib.ChartLibError('cliora_maxsim_scores: %d caption(s) with a decreasing offset or one outside [0, %d]' % (bad, NT))
        def fit(n0):                             # the largest n1 whose workspace fits (at least one caption)
            lo, hi = n0 + 1, N
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if _ws_bytes(mid - n0, qo_host[mid] - qo_host[n0], M, MR, D) <= limit:
                    lo = mid
                else:
                    hi = mid - 1
            return lo

        n0, left = 0, 0
        while n0 < N:                            # how many chunks a greedy fill takes ...
            n0, left = fit(n0), left + 1
        n0 = 0
        while n0 < N:                            # ... and that many of about equal numbers of rows
            n1 = fit(n0)
            if left > 1:
                even = qo_host[n0] + -(-(qo_host[N] - qo_host[n0]) // left)
                n1 = max(n0 + 1, min(n1, next((n for n in range(n0 + 1, n1 + 1) if qo_host[n] >= even), n1)))
            left = max(1, left - 1)
            st = torch.zeros(2, dtype=torch.int32, device=dev)
            run(n0, n1, qo_host[n0], qo_host[n1], qo[n0:n1 + 1] - qo_host[n0], st)
            status = torch.maximum(status, st)   # the images are the same in every chunk, and the captions were checked above
            n0 = n1
    return S, status


def _status_message(status):
    return ('cliora_maxsim_scores rejected %d image(s) of more than %d regions and %d group(s) with a decreasing or out-of-range offset'
            % (int(status[0]), MAX_REGIONS, int(status[1])))


def maxsim_scores(q, q_off, w, keys, k_off, max_workspace_mb=256):
    """S (N, M) fp32 = cliora_maxsim_scores.  q (NT, D) / keys (MR, D): fp32 CUDA rows with unit stride along D (any row stride);
    w (NT) fp32; q_off (N + 1) / k_off (M + 1): group offsets, an int tensor (host or device) or a host list.  Uses the library's MFMA
    mode.  `max_workspace_mb` bounds the part of the workspace that grows with the captions (the packed images are needed in any case): a
    call above it is split over the captions into chunks of about equal numbers of rows; the result is bitwise independent of the split.  Raises ChartLibError when the call's status is non-zero (one synchronisation)."""
    S, status = _maxsim(q, q_off, w, keys, k_off, max_workspace_mb)
    st = status.cpu().tolist()
    if any(st):
        raise _lib.ChartLibError(_status_message(st))
    return S


def retrieval_ranks(S, image_of):
    """cliora_retrieval_ranks: -> (rank_t2i (N) int32, rank_i2t (M) int32, status (1) int32), device tensors, nothing synchronised."""
    if S.dim() != 2 or S.dtype != torch.float32 or not S.is_cuda or (S.shape[1] > 1 and S.stride(1) != 1):
        raise ValueError('scores must be an fp32 CUDA matrix with unit column stride')
    N, M = S.shape
    dev = S.device
    io = torch.as_tensor(image_of).to(device=dev, dtype=torch.int32).contiguous()
    if io.shape != (N,):
        raise ValueError('image_of %s: one image per caption (%d)' % (tuple(io.shape), N))
    with torch.cuda.device(dev):
        t2i = torch.empty(N, dtype=torch.int32, device=dev)
        i2t = torch.empty(M, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call('cliora_retrieval_ranks', N, M, _p(S), S.stride(0) if N > 1 else max(M, 1), _p(io), _p(t2i), _p(i2t), _p(status), _stream())
    return t2i, i2t, status


def score_topk(S, k, transpose=False):
    """cliora_score_topk: (D (rows, k) fp32, I (rows, k) int64), the k best entries of every row of S -- of every column with
    transpose=True (the captions per image) -- in the order of the ranks; -inf / -1 past the entries there are."""
    if not 1 <= k <= MAX_K:
        raise ValueError('k = %d: cliora_score_topk supports 1 <= k <= %d' % (k, MAX_K))
    if S.dim() != 2 or S.dtype != torch.float32 or not S.is_cuda:
        raise ValueError('scores must be an fp32 CUDA matrix')
    V = S.t() if transpose else S
    rows, cols = V.shape
    dev = S.device
    with torch.cuda.device(dev):
        Dout = torch.empty((rows, k), dtype=torch.float32, device=dev)
        Iout = torch.empty((rows, k), dtype=torch.int64, device=dev)
        _lib.call('cliora_score_topk', rows, cols, k, _p(V), V.stride(0), V.stride(1), _p(Dout), _p(Iout), _stream())
    return Dout, Iout


# ---- queries and keys of a model ----------------------------------------------------------------------------------------------------
def _unit(x):
    return x / x.norm(p=2, dim=-1, keepdim=True).clamp(min=TINY)          # utils.py:12-14


def _ragged_rows(x, lengths):
    """The valid rows of a right-padded (B, L, W) tensor, sentence-major: -> ((sum lengths, W), offsets as a host list)."""
    B, L = x.shape[0], x.shape[1]
    lens = [int(n) for n in lengths]
    if len(lens) != B or any(n < 0 or n > L for n in lens):
        raise ValueError('lengths must hold one value in 0..%d per row' % L)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if all(n == L for n in lens):
        return x.reshape(B * L, x.shape[2]), off.tolist()
    idx = np.concatenate([b * L + np.arange(n) for b, n in enumerate(lens)]) if off[-1] else np.zeros(0, dtype=np.int64)
    return x.reshape(B * L, x.shape[2])[torch.from_numpy(idx).to(x.device)], off.tolist()


def _pad_tokens(tokens, lengths, pad_id=0):
    """tokens: a (B, L) tensor (with `lengths` or full) or lists of ids -> ((B, L) int64 host tensor, lengths list)."""
    if isinstance(tokens, torch.Tensor):
        B, L = tokens.shape
        return tokens, [L] * B if lengths is None else [int(n) for n in lengths]
    lens = [len(s) for s in tokens]
    out = torch.full((len(lens), max(lens + [1])), pad_id, dtype=torch.int64)
    for b, s in enumerate(tokens):
        out[b, :len(s)] = torch.as_tensor(list(s), dtype=torch.int64)
    return out, lens


def image_keys(net, obj_feats, counts=None, mode='word'):
    """The region rows of the images: -> (keys (sum counts, W) fp32, k_off host list of M + 1).  mode 'word': ``obj_word`` of
    net.img_encoder (W = D), the regions the trained logit scores words against; 'eval': ``[obj_span | obj_word]`` (W = 2D).
    obj_feats: (M, R, img_dim) region features, right-padded when `counts` gives each image's own number of regions, or a list of
    (r_m, img_dim) tensors.  Rows beyond an image's count never reach the kernel."""
    if mode not in ('word', 'eval'):
        raise ValueError("mode %r: 'word' or 'eval'" % (mode,))
    dev = next(net.parameters()).device
    if not isinstance(obj_feats, torch.Tensor):
        counts = [int(f.shape[0]) for f in obj_feats]
        R = max(counts + [1])
        feats = torch.zeros((len(counts), R, obj_feats[0].shape[-1] if counts else 1), dtype=torch.float32)
        for m_, f in enumerate(obj_feats):
            feats[m_, :f.shape[0]] = f.float()
        obj_feats = feats
    M, R = obj_feats.shape[0], obj_feats.shape[1]
    with torch.no_grad():
        o_span, o_word = net.img_encoder(obj_feats.to(dev))
        rows = o_word if mode == 'word' else torch.cat([o_span, o_word], -1)
        return _ragged_rows(rows.float(), [R] * M if counts is None else counts)


def caption_queries(net, tokens, lengths=None, mode='word', normalize=True, obj_feats=None):
    """The word rows of the captions: -> (q (sum lengths, W) fp32, q_off host list of N + 1, w (sum lengths) fp32 = 1 / length).
    tokens: lists of token ids of any lengths, or a (B, L) tensor, right-padded when `lengths` is given.

    mode 'word': ``unit(x_word)`` of every valid word, the eval convention of cliora.py:463; normalize=False: the raw ``x_word`` of the
    trained logit (cliora.py:460).  It depends on no image: this is the mode retrieval figures are quoted on.

    mode 'eval': ``[(inside_h + outside_h)[leaf] | unit(x_word)]`` (W = 2D) after an eval forward of each caption WITH ITS OWN IMAGE
    (obj_feats: (N, R, img_dim), row n the image paired with caption n; mixed lengths run through ragged.forward_ragged).  Against
    ``image_keys(mode='eval')`` it reproduces the reference's eval attention logit (cliora.py:463-464).  The chart of a CLIORA model
    attends to its image, so these queries HAVE SEEN THE PAIRED IMAGE: they are for analysis of the attention, not for retrieval
    figures."""
    if mode not in ('word', 'eval'):
        raise ValueError("mode %r: 'word' or 'eval'" % (mode,))
    dev = next(net.parameters()).device
    padded, lens = _pad_tokens(tokens, lengths)
    with torch.no_grad():
        if mode == 'word':
            x_word = net.embed(padded.to(dev))[1].float()
            q, off = _ragged_rows(_unit(x_word) if normalize else x_word, lens)
        else:
            if obj_feats is None:
                raise ValueError("mode 'eval' runs each caption's chart with its own image: pass obj_feats (N, R, img_dim)")
            if min(lens + [1]) < 1:
                raise ValueError('an empty caption has no chart')
            diora = net.diora
            was_training, had_outside = net.training, diora.outside
            try:
                if len(set(lens)) == 1 and lens[0] == padded.shape[1]:
                    net.eval()
                    diora.outside = True
                    net(padded.to(dev), obj_feats.to(dev), None, compute_loss=False)
                    L = lens[0]
                    x_word = net.embed(padded.to(dev))[1].float()
                    q = torch.cat([diora.inside_h[:, :L] + diora.outside_h[:, :L], _unit(x_word)], -1)
                    q, off = _ragged_rows(q, lens)
                else:
                    from . import ragged
                    sents = [padded[b, :n].tolist() for b, n in enumerate(lens)]
                    parts = {}

                    def per_pack(idx, lens_dev, d):
                        tok, _ = ragged.pad_batch([sents[i] for i in idx], 0)
                        x_word = net.embed(tok.to(dev))[1].float()
                        Lp = tok.shape[1]
                        rows = torch.cat([d.inside_h[:, :Lp] + d.outside_h[:, :Lp], _unit(x_word)], -1)
                        for b, i in enumerate(idx):
                            parts[i] = rows[b, :lens[i]].clone()
                        parts.setdefault('status', []).append(d._ragged_status)

                    ragged.forward_ragged(net, sents, obj_feats=obj_feats, per_pack=per_pack)
                    bad = int(torch.stack([s.reshape(-1)[0] for s in parts.pop('status')]).max().item())
                    if bad:
                        raise _lib.ChartLibError('the padded chart rejected %d sentence length(s)' % bad)
                    q = torch.cat([parts[i] for i in range(len(sents))], 0)
                    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
            finally:
                diora.outside = had_outside
                net.train(was_training)
        inv = [1.0 / n if n else 0.0 for n in lens]
        w = torch.tensor(np.repeat(np.asarray(inv, dtype=np.float32), lens)).to(dev)
    return q.contiguous(), off, w


def span_queries(diora, lengths=None, weights=None):
    """After a forward of a chart module: the rows ``inside_h + outside_h`` of each sentence's own triangle, sentence-major, then level,
    then position -> (q (spans, D), q_off host list of B + 1, w (spans)).  lengths: None (every sentence has L words) or one length per
    sentence of a right-padded batch (host list or tensor).  weights: (B, C) per cell; default the span posteriors
    (posterior.span_posteriors), which makes the score of a sentence against an image the posterior-weighted sum of its spans' best
    regions -- for text-only charts as well, against any region matrix of the chart's width."""
    from .posterior import cell_id, span_posteriors
    ih, oh = diora.inside_h, diora.outside_h
    B, Cc, _ = ih.shape
    L = int(round((np.sqrt(8 * Cc + 1) - 1) / 2))
    lens = [L] * B if lengths is None else [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if any(n < 1 or n > L for n in lens) or len(lens) != B:
        raise ValueError('lengths must hold one value in 1..%d per sentence' % L)
    if weights is None:
        ldev = None if lengths is None else torch.as_tensor(lens, dtype=torch.int32).to(ih.device)
        weights = span_posteriors(diora, ldev).marginals
    cells = np.array([b * Cc + cell_id(L, level, pos) for b, n in enumerate(lens) for level in range(n) for pos in range(n - level)],
                     dtype=np.int64)
    off = np.concatenate([[0], np.cumsum([n * (n + 1) // 2 for n in lens])]).tolist()
    idx = torch.from_numpy(cells).to(ih.device)
    with torch.no_grad():
        q = (ih.reshape(B * Cc, -1)[idx] + oh.reshape(B * Cc, -1)[idx]).float()
        w = weights.reshape(-1)[idx].float()
    return q.contiguous(), off, w.contiguous()


# ---- the evaluation -----------------------------------------------------------------------------------------------------------------
def _direction(ranks, ks):
    r = np.asarray(ranks, dtype=np.int64)
    ok = r[r >= 0]
    return {'r_at_k': {int(k): (float((ok < k).mean()) if ok.size else float('nan')) for k in ks},
            'median_rank': float(np.median(ok + 1)) if ok.size else float('nan'),
            'mean_rank': float((ok + 1).mean()) if ok.size else float('nan'),
            'skipped': int((r < 0).sum()), 'ranks': r}


def retrieve(net, captions, images, image_of, ks=(1, 5, 10), mode='word', topk=0, counts=None, max_workspace_mb=256):
    """Text-to-image and image-to-text retrieval of `captions` (lists of token ids of any lengths, or a (N, L) tensor) over `images`
    ((M, R, img_dim), right-padded with `counts`, or a list of (r_m, img_dim) tensors); image_of[n] is the image caption n was written
    for.  One MaxSim pass, one ranks launch, one copy to the host.  ->

        {'t2i': {'r_at_k': {k: fraction}, 'median_rank', 'mean_rank' (1-based), 'skipped', 'ranks' (0-based, -1 = skipped)},
         'i2t': the same per image (skipped: images without captions), 'scores': S (N, M) on the device,
         'topk': {'t2i': (D, I), 'i2t': (D, I)} host arrays of the `topk` best images per caption / captions per image, with topk > 0}

    mode 'word' scores unit word vectors against obj_word and depends on no pairing; mode 'eval' runs each caption's chart with its own
    image (images[image_of], a tensor of one region count) and is for analysis only: see ``caption_queries``."""
    paired = None
    if mode == 'eval':
        if not isinstance(images, torch.Tensor) or counts is not None:
            raise ValueError("mode 'eval' needs the images as one (M, R, img_dim) tensor")
        paired = images[torch.as_tensor(image_of, dtype=torch.int64)]
    q, q_off, w = caption_queries(net, captions, mode=mode, obj_feats=paired)
    keys, k_off = image_keys(net, images, counts=counts, mode=mode)
    S, status = _maxsim(q, q_off, w, keys, k_off, max_workspace_mb)
    t2i, i2t, rstatus = retrieval_ranks(S, image_of)
    N, M = S.shape
    parts = [status, rstatus, t2i, i2t]
    lists = []
    if topk:
        lists = [score_topk(S, topk), score_topk(S, topk, transpose=True)]
        for D_, I_ in lists:
            parts += [D_.view(torch.int32).reshape(-1), I_.view(torch.int32).reshape(-1)]
    host = torch.cat(parts).cpu().numpy()               # the one copy
    if host[:2].any():
        raise _lib.ChartLibError(_status_message(host[:2]))
    out = {'t2i': _direction(host[3:3 + N], ks), 'i2t': _direction(host[3 + N:3 + N + M], ks), 'scores': S}
    if topk:
        o, res = 3 + N + M, {}
        for name, rows in (('t2i', N), ('i2t', M)):
            n = rows * topk
            res[name] = (host[o:o + n].view(np.float32).reshape(rows, topk), host[o + n:o + 3 * n].view(np.int64).reshape(rows, topk))
            o += 3 * n
        out['topk'] = res
    return out
