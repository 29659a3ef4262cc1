"""Minimal training harness around the native chart modules: the callers either side of the path.

The reference's CLI cannot run on the GPU box (torchvision / h5py / datasets absent), so this
module restates what sits around ``self.diora(...)`` in cliora/net/trainer.py: ``Embed`` (:204-224),
``ImageEncoder`` (net/utils.py:37-55), the three losses (:25-171), ``Net.forward`` (:272-304) and
the update rule of ``Trainer._step`` / ``gradient_update`` (:450-455, 483-501: backward,
clip_grad_norm_ 5.0, Adam).  On the GPU every one of them runs on this library's kernels
(cliora_amd/heads.py -> csrc/api_heads.hip: gather + fp32-MFMA projections, the fused
reconstruction / VG / contrastive heads, one clip + Adam launch sequence over a flat buffer);
the torch formulas below them are what runs on CPU tensors (the CPU tests) and what the kernels
are checked against.  Module and parameter names follow the reference so that its checkpoints
(``trainer.py:383-398``) load by key.  Pinned by tests/golden/net_*.npz.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import heads
from .diora import DioraMLP as TextDiora, check_lengths      # check_lengths: also imported from here (harness.check_lengths)
from .cliora import DioraMLP as VLDiora

NATIVE_HEADS = True        # False: the torch formulas everywhere (A/B and tests)


def _native(*tensors):
    return NATIVE_HEADS and all(t is None or t.is_cuda for t in tensors)


def _normal_(module):
    for p in module.parameters():
        if p.requires_grad:
            p.data.normal_()


def _lane_reads(lane, t, made_here):
    """`t` is about to be read on `lane`.  When it was made here, on the current stream, after the lane forked (a copy of non-contiguous
    tokens, the fp32 conversion of the region features), the lane waits for it, and its memory is not reused before the lane's reads
    (the word projection's forward and backward) are done."""
    if made_here:
        lane.wait_stream(torch.cuda.current_stream(t.device))
        t.record_stream(lane)


class Embed(nn.Module):
    """Two bias-free projections of the word embedding: span input and word input."""

    def __init__(self, embeddings, input_size, size):
        super().__init__()
        self.input_size, self.size, self.embeddings = input_size, size, embeddings
        self.mat = nn.Parameter(torch.empty(size, input_size))
        self.mat1 = nn.Parameter(torch.empty(size, input_size))
        _normal_(self)

    def forward(self, tokens, word_lane=None):
        """word_lane: a stream for the WORD projection (the second output), whose only reader is then the word-region scorer on the same
        stream (cliora_amd.cliora.DioraMLP.word_lane); None: both on the current stream.  Afterwards `word_on_lane` says whether the word
        projection was produced on word_lane (the native path only: a table width that is not a multiple of 16 takes the torch path, on
        the current stream)."""
        B, L = tokens.shape
        w = self.embeddings.weight
        self.word_on_lane = False
        if _native(w, tokens) and w.shape[1] % 16 == 0:
            idx = tokens.reshape(-1)
            span = heads.proj(w, idx, self.mat).view(B, L, -1)
            if word_lane is None:
                return span, heads.proj(w, idx, self.mat1).view(B, L, -1)
            _lane_reads(word_lane, idx, not tokens.is_contiguous())
            self.word_on_lane = True
            with torch.cuda.stream(word_lane):
                return span, heads.proj(w, idx, self.mat1).view(B, L, -1)
        e = self.embeddings(tokens.reshape(-1))
        return (e @ self.mat.t()).view(B, L, -1), (e @ self.mat1.t()).view(B, L, -1)


class ImageEncoder(nn.Module):
    """Two linear maps of the region features; zero-initialised like the reference (utils.py:45-50)."""

    def __init__(self, input_size, size):
        super().__init__()
        self.fc, self.fc_vis = nn.Linear(input_size, size), nn.Linear(input_size, size)
        for p in self.parameters():
            p.data.zero_()

    def forward(self, obj_feats, word_lane=None):
        x = obj_feats.float()
        self.word_on_lane = False                         # see Embed.forward
        if _native(x) and x.shape[-1] % 16 == 0:
            lead = x.shape[:-1]
            span = heads.proj(x, None, self.fc.weight, self.fc.bias).view(*lead, -1)
            if word_lane is None:
                return span, heads.proj(x, None, self.fc_vis.weight, self.fc_vis.bias).view(*lead, -1)
            _lane_reads(word_lane, x, x is not obj_feats)
            self.word_on_lane = True
            with torch.cuda.stream(word_lane):
                return span, heads.proj(x, None, self.fc_vis.weight, self.fc_vis.bias).view(*lead, -1)
        return self.fc(x), self.fc_vis(x)


class ReconstructionSoftmaxLoss(nn.Module):
    name = 'reconstruct_softmax_loss'

    def __init__(self, embeddings, input_size, size, k_neg=3, full_vocab=False):
        """full_vocab: the exact loss over the whole table instead of the sampled one (cliora_amd.vocab): the mean over the tokens of
        logsumexp_v <mat^T o_t, emb[v]> - <mat^T o_t, emb[tok_t]>; neg_samples is then ignored."""
        super().__init__()
        self.k_neg, self.embeddings, self.full_vocab = k_neg, embeddings, bool(full_vocab)
        self.vocab_status = None             # full_vocab on the device: the last call's count of ids outside the table (forward)
        self.mat = nn.Parameter(torch.empty(size, input_size))
        _normal_(self)

    def forward(self, tokens, neg_samples, diora):
        B, L = tokens.shape
        w = self.embeddings.weight
        if self.full_vocab:
            q = diora.outside_h[:, :L].reshape(B * L, -1) @ self.mat                 # B*L,E: the gradient to mat and outside_h flows through this product
            from . import vocab
            if _native(w, tokens, q) and vocab.supported(q, w, tokens):
                # An id outside the table raises in the torch formula below.  Here it is left out of the sum (while 1 / T still counts
                # it) and counted in vocab_status, a one-element int32 tensor on the device: reading it is a synchronisation, so it is
                # the caller's to check, once per epoch or when a loss looks wrong.
                loss, _, _, _, _, self.vocab_status = vocab.vocab_nll(q, w, tokens.reshape(-1))
                return loss
            return F.cross_entropy(q @ w.t(), tokens.reshape(-1))
        if _native(w, tokens, neg_samples, diora.outside_h) and w.shape[1] % 16 == 0:
            return heads.recon_loss(w, self.mat, diora.outside_h, tokens, neg_samples)
        pos = self.embeddings(tokens) @ self.mat.t()                     # B,L,D
        neg = self.embeddings(neg_samples) @ self.mat.t()                # K,D
        cell = diora.outside_h[:, :L]                                    # B,L,D  leaf outside vectors
        logits = torch.cat([(pos * cell).sum(-1, keepdim=True), cell @ neg.t()], -1).view(B * L, -1)
        return F.cross_entropy(logits, torch.zeros(B * L, dtype=torch.long, device=logits.device))


class FusedContrastive(torch.autograd.Function):
    """cliora_contrastive_loss: the hinge + span-marginal weighting of trainer.py:103-128 on the region maxima (B, B, C), value and
    gradient in one launch (the backward scales the stored gradients by the incoming cotangent)."""

    @staticmethod
    def forward(ctx, smax, ins, outs, margin, alpha, lengths=None, status_out=None):
        """lengths (int32 device tensor (B,)): cliora_contrastive_loss_ragged over the sentences' own triangles of a padded chart; its
        status word (the count of lengths outside 1..L) is copied into status_out[0], a one-element list, still on the device."""
        from . import _lib
        B, _, Cc = smax.shape
        smax, ins, outs = smax.contiguous().float(), ins.contiguous().float(), outs.contiguous().float()
        dev = smax.device
        loss = torch.empty(1, device=dev)
        d_smax, d_ins, d_outs = torch.empty_like(smax), torch.empty_like(ins), torch.empty_like(outs)
        p = _lib.ptr
        with _lib.device_guard(smax):
            if lengths is None:
                nbytes = _lib.fn('cliora_contrastive_workspace_bytes')(B, Cc)
                ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
                _lib.call('cliora_contrastive_loss', B, Cc, p(smax), p(ins), p(outs), float(margin), float(alpha), p(loss), p(d_smax), p(d_ins),
                          p(d_outs), p(ws), nbytes, _lib.stream())
            else:
                lengths = check_lengths(lengths, B, dev)
                nbytes = RAGGED_STATUS_BYTES + _lib.fn('cliora_contrastive_workspace_bytes')(B, 2 * Cc)
                ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
                _lib.call('cliora_contrastive_loss_ragged', B, Cc, p(smax), p(ins), p(outs), p(lengths), float(margin), float(alpha), p(loss),
                          p(d_smax), p(d_ins), p(d_outs), p(ws), nbytes, _lib.stream())
                if status_out is not None:
                    status_out[0] = ws[:4].view(torch.int32)
        ctx.save_for_backward(d_smax, d_ins, d_outs)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d_smax, d_ins, d_outs = ctx.saved_tensors
        return d_smax * g, d_ins * g, d_outs * g, None, None, None, None


RAGGED_STATUS_BYTES = heads.RAGGED_STATUS_BYTES


def triangle_masks(lengths, L):
    """Of a padded chart of length L whose sentence x has lengths[x] words, in closed form from (n_x, level,
    pos) and on the lengths' device: own (B, C) bool, the cells (level, pos) with pos + level < n_x; half (B, C) bool, the owned cells
    whose number in the sentence's OWN chart, level n_x - level (level - 1) / 2 + pos, is below C_x // 2; root (B,) int64, the padded
    chart's row of the cell (n_x - 1, 0)."""
    level = torch.cat([torch.full((L - k,), k, dtype=torch.int64) for k in range(L)]).to(lengths.device)
    pos = torch.cat([torch.arange(L - k, dtype=torch.int64) for k in range(L)]).to(lengths.device)
    n = lengths.long().view(-1, 1)
    own = pos + level < n
    half = own & (level * n - level * (level - 1) // 2 + pos < (n * (n + 1) // 2) // 2)
    lv = n.view(-1) - 1
    return own, half, lv * L - lv * (lv - 1) // 2


class ContrastiveLoss(nn.Module):
    name = 'contrastive_loss'
    fused = True            # native kernel when the scores are on the GPU and B <= 128 (False: the torch ops below)

    def __init__(self, margin=1.0, alpha_contr=0.01):
        super().__init__()
        self.margin, self.alpha, self.floor = margin, alpha_contr, 1e-8

    def forward(self, diora, lengths=None):
        """lengths (int32 (B,), on the scores' device): the sentences of a right-padded chart have these many words, and the loss is
        DESIGN.md section 23's over their own triangles; `self.status` then holds the fused kernel's status word, on the device."""
        ins, outs = diora.inside_s.squeeze(-1), diora.outside_s.squeeze(-1)
        B, C = ins.shape
        smax = diora.all_atten_score.max(-1).values                      # B(text),B(image),C
        if lengths is not None:
            if self.fused and smax.is_cuda and B <= 128:
                status = [None]
                v = FusedContrastive.apply(smax, ins, outs, self.margin, self.alpha, lengths, status)
                self.__dict__['status'] = status[0]
                return v
            return self.forward_ragged_torch(smax, ins, outs, lengths)
        if self.fused and smax.is_cuda and B <= 128:
            return FusedContrastive.apply(smax, ins, outs, self.margin, self.alpha)
        sc = smax.permute(2, 0, 1)                                       # C,B(text),B(image)
        pos = torch.diagonal(sc, 0, 1, 2).unsqueeze(-1)                  # C,B,1
        off_diag = ~torch.eye(B, dtype=torch.bool, device=sc.device)
        txt = (self.margin + sc - pos).clamp(min=self.floor) * off_diag
        img = (self.margin + sc - pos.transpose(1, 2)).clamp(min=self.floor) * off_diag
        per_span = (txt.mean(2) + img.mean(1)).t()                       # B,C
        marginal = torch.exp(ins + outs - ins[:, -1:])
        return (marginal * per_span)[:, :C // 2].sum(-1).mean() * self.alpha

    def forward_ragged_torch(self, smax, ins, outs, lengths):
        """The mixed-length loss in torch ops.  Whatever the inputs hold beyond a triangle is replaced by 0 BEFORE any arithmetic (a
        mask applied after the exp would let a NaN there into the gradients), and every sum selects its terms."""
        B, C = ins.shape
        L = int(round(((8 * C + 1) ** 0.5 - 1) / 2))
        own, half, root = triangle_masks(check_lengths(lengths, B, ins.device), L)
        zero = smax.new_zeros(())
        s = torch.where(own[:, None, :], smax, zero)                     # s[a, c, cell]: text a's cell against image c
        ins, outs = torch.where(own, ins, zero), torch.where(own, outs, zero)
        pos = torch.diagonal(s, 0, 0, 1).t()                             # B,C: s[x, x, cell]
        off_diag = ~torch.eye(B, dtype=torch.bool, device=s.device)[:, :, None]
        txt = torch.where(off_diag, (self.margin + s - pos[:, None, :]).clamp(min=self.floor), zero).sum(1) / B       # over the images y != x
        img = torch.where(off_diag & own[:, None, :], (self.margin + s - pos[None, :, :]).clamp(min=self.floor), zero).sum(0) / B   # texts a != x owning the cell
        marginal = torch.exp(torch.where(half, ins + outs - ins.gather(1, root.view(-1, 1)), zero))
        return torch.where(half, marginal * (txt + img), zero).sum() / B * self.alpha


class VGLoss(nn.Module):
    name = 'vg_loss'

    def __init__(self, alpha_vg=0.1):
        super().__init__()
        self.alpha = alpha_vg

    def forward(self, vg_atten_score, lengths=None):
        """lengths (int32 (B,), on the scores' device): sentence a of the right-padded batch has lengths[a] words, and its logits are the
        mean over those; `self.status` then holds the fused kernel's status word, on the device."""
        B, _, L, _ = vg_atten_score.shape
        if lengths is not None:
            lengths = check_lengths(lengths, B, vg_atten_score.device)
            if _native(vg_atten_score):
                status = [None]
                v = heads.vg_loss(vg_atten_score, self.alpha, lengths, status)
                self.__dict__['status'] = status[0]
                return v
            word = torch.arange(L, device=lengths.device) < lengths.view(-1, 1)            # B,L
            v = torch.where(word[:, None, :, None], vg_atten_score, vg_atten_score.new_zeros(()))      # zeros before any arithmetic
            logits = v.max(-1).values.sum(-1) / lengths.view(-1, 1)
            return self.alpha * F.cross_entropy(logits, torch.arange(B, device=logits.device))
        if _native(vg_atten_score):
            return heads.vg_loss(vg_atten_score, self.alpha)
        logits = vg_atten_score.max(-1).values.sum(-1) / L
        return self.alpha * F.cross_entropy(logits, torch.arange(B, device=logits.device))


class LossDict(dict):
    """What Net.forward returns: the named losses, plus -- built only when somebody asks for it -- the reference's `total_loss`, the (1, n)
    row of the losses (trainer.py:300-303).  Asking includes `in`, get(), keys(), items() and values(): they show the reference's `ret`
    (the named losses, then total_loss), which its prepare_result walks (trainer.py:457-461).  Plain iteration lists what is built.  `total()` is the scalar
    the reference roots its backward at, `total_loss.mean(dim=0).sum()` (trainer.py:487), as the plain sum of the parts: the same value
    and the same gradients without the cat / mean / sum launches and their four backward launches per step."""
    parts = ()

    def __missing__(self, key):
        if key != 'total_loss' or not self.parts:
            raise KeyError(key)
        v = torch.cat([p.view(1, 1) for p in self.parts], 1)
        self[key] = v
        return v

    def _full(self):
        if self.parts and not dict.__contains__(self, 'total_loss'):
            self.__missing__('total_loss')
        return self

    def __contains__(self, key):
        return dict.__contains__(self._full() if key == 'total_loss' else self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        return dict.keys(self._full())

    def items(self):
        return dict.items(self._full())

    def values(self):
        return dict.values(self._full())

    def total(self):
        t = self.parts[0]
        for p in self.parts[1:]:
            t = t + p
        return t


class Net(nn.Module):
    def __init__(self, embed, image_encoder, diora, obj_feats, loss_funcs=(), bracket_loss_weight=0.0, risk_loss_weight=0.0,
                 entropy_loss_weight=0.0, hinge_loss_weight=0.0, hinge_margin=1.0, hinge_penalty=float('inf'), teacher=None,
                 kl_loss_weight=0.0, kl_direction='forward'):
        super().__init__()
        self.obj_feats = obj_feats
        # != 0 with a teacher: a training step adds weight * parse_divergence(teacher, self.diora, kl_direction).
        # The teacher is a chart module of this net's width (a CLIORA one needs a net with regions) that is NOT a submodule: its
        # parameters are in no optimizer and no state_dict of the net, and net.train() never reaches it.  Each step runs its inside
        # pass alone on the net's own x_span, under no_grad.
        if kl_direction not in ('forward', 'reverse', 'symmetric'):
            raise ValueError("kl_direction must be 'forward', 'reverse' or 'symmetric'")
        self.__dict__['teacher'] = teacher
        self.kl_loss_weight, self.kl_direction = float(kl_loss_weight), kl_direction
        # > 0: a batch that carries entity_labels adds weight * bracket_nll of its annotated phrases (cliora_amd.structured) to the total
        self.bracket_loss_weight = float(bracket_loss_weight)
        # > 0: such a batch adds weight * the mean expected cost under span_costs of ALL its phrases, crossing ones included (minus the
        # expected number of them recovered); != 0, either sign: a training step adds weight * the mean entropy of the parse distribution
        self.risk_loss_weight, self.entropy_loss_weight = float(risk_loss_weight), float(entropy_loss_weight)
        # > 0: such a batch adds weight * bracket_hinge of its phrases: the structured hinge (perceptron at margin
        # 0) with an infinite penalty, over the laminar subset of the phrases; the ramp loss with a finite one, crossing phrases kept
        self.hinge_loss_weight, self.hinge_margin, self.hinge_penalty = float(hinge_loss_weight), float(hinge_margin), float(hinge_penalty)
        self.overlap_word_branch = True      # vision-language training steps: the word branch on the library's caller lane (forward())
        if obj_feats:
            self.img_encoder = image_encoder
        self.embed, self.diora = embed, diora
        self.loss_func_names = [m.name for m in loss_funcs]
        for m in loss_funcs:
            setattr(self, m.name, m)

    def forward(self, tokens, obj_feats=None, neg_samples=None, compute_loss=True, entity_labels=None):
        # The word branch of a vision-language training step -- Embed's word projection, ImageEncoder's fc_vis, the word-region scorer and,
        # in the backward, their gradients and the region matrix's half of the region-max backward -- shares nothing with the chart
        # (cliora.py:459-461, trainer.py:139-171): it runs on the library's caller lane beside the chart's forward and backward
        # (autograd runs a node's backward on its forward's stream and orders the streams itself; the lane joins the current stream
        # before the VG loss reads the scores, and again when backward() returns).
        lane = None
        if (self.overlap_word_branch and self.obj_feats and self.training and torch.is_grad_enabled() and tokens.is_cuda and heads.NATIVE_LANES
                and getattr(self.diora, 'lazy_region_scores', False)):
            from . import _lib
            # the lane reads the tokens (word projection) and the fp32 region features (fc_vis): make them final BEFORE the fork, so
            # that the lane's wait below covers a copy of non-contiguous tokens and the conversion of fp16 / fp64 features
            t1, f1 = tokens.contiguous(), obj_feats.float()
            made = [t for t, t0 in ((t1, tokens), (f1, obj_feats)) if t is not t0]
            tokens, obj_feats = t1, f1
            lane = _lib.side_stream(tokens.device)
            lane.wait_stream(torch.cuda.current_stream(tokens.device))     # the step's inputs and the parameters of the last update
            for t in made:              # freed in the backward, while the lane may still read them
                t.record_stream(lane)
        if lane is not None:
            x_span, x_word = self.embed(tokens, word_lane=lane)
        else:
            x_span, x_word = self.embed(tokens)
        # the scorer skips its wait for the current stream only when EVERY word input was produced on the lane (Embed / ImageEncoder
        # take the torch path, on the current stream, at widths that are not multiples of 16)
        on_lane = lane is not None and getattr(self.embed, 'word_on_lane', False)
        o_span = o_word = None
        if self.obj_feats:
            o_span, o_word = self.img_encoder(obj_feats, word_lane=lane) if lane is not None else self.img_encoder(obj_feats)
            on_lane = on_lane and getattr(self.img_encoder, 'word_on_lane', False)
        flags = hasattr(self.diora, 'word_lane')
        if flags:
            self.diora.word_lane, self.diora.word_inputs_on_lane = lane, on_lane
        try:
            self.diora(x_span, x_word, o_span, o_word)
        finally:                        # per call: a later direct call of the chart module must not inherit them
            if flags:
                self.diora.word_lane, self.diora.word_inputs_on_lane = None, False
        if compute_loss and self.uses_teacher():
            self.run_teacher(x_span, x_word, o_span, o_word)
        if not compute_loss:
            return {'total_loss': torch.ones(1, 1, device=x_span.device)}
        ret, parts = LossDict(), []
        for name in self.loss_func_names:
            fn = getattr(self, name)
            if 'reconstruct' in name:
                v = fn(tokens, neg_samples, self.diora)
            elif 'contrastive' in name:
                v = fn(self.diora)
            else:
                v = fn(self.diora.vg_atten_score)
            ret[name] = v
            parts.append(v)
        for name, v in self.structured_losses(entity_labels, tokens.shape[1], tokens.device):
            ret[name] = v
            parts.append(v)
        ret.parts = parts
        return ret

    def uses_teacher(self):
        """Whether this step adds the divergence from the teacher: a training step of a net with a teacher and a weight."""
        return self.kl_loss_weight != 0 and self.teacher is not None and self.training and torch.is_grad_enabled()

    def run_teacher(self, x_span, x_word=None, o_span=None, o_word=None):
        """The teacher's inside pass alone on the chart inputs of this net's own forward (detached), under no_grad, in the mode the
        teacher is in; regions only for a teacher that takes them.  A padded pack runs the same way: the inside pass is prefix-closed."""
        from .cliora import DioraMLP as VLDiora
        teacher = self.teacher
        vl = isinstance(teacher, VLDiora)
        if vl and o_span is None:
            raise ValueError('a CLIORA teacher needs a net with regions (obj_feats)')
        det = lambda t: t.detach() if t is not None else None
        had_outside = teacher.outside
        teacher.outside = False
        try:
            with torch.no_grad():
                teacher(det(x_span), det(x_word), *((det(o_span), det(o_word)) if vl else ()))
        finally:
            teacher.outside = had_outside

    def structured_losses(self, entity_labels, L, device):
        """The weighted structured terms of the chart self.diora holds (cliora_amd.structured), as (name, 0-d tensor) in the order they
        join the total: bracket_nll, hinge and risk for a batch that carries entity_labels, entropy for a training step, kl for a
        training step of a net with a teacher (whose forward on the same inputs has run: ``run_teacher``).  L: the chart's length."""
        out = []
        if entity_labels is not None and self.bracket_loss_weight > 0:
            from .constrained import brackets_from_entity_labels
            out.append(('bracket_nll', self.bracket_loss_weight * self.diora.bracket_nll(brackets_from_entity_labels(entity_labels))))
        if entity_labels is not None and self.hinge_loss_weight > 0:
            from .constrained import brackets_from_entity_labels
            req = brackets_from_entity_labels(entity_labels, drop_crossing=self.hinge_penalty == float('inf'))
            out.append(('hinge', self.hinge_loss_weight * self.diora.bracket_hinge(req, margin=self.hinge_margin, penalty=self.hinge_penalty)))
        use_risk = entity_labels is not None and self.risk_loss_weight > 0
        use_entropy = self.entropy_loss_weight != 0 and self.training and torch.is_grad_enabled()
        if use_risk or use_entropy:                             # one node for both: one kernel launch each way
            from .constrained import brackets_from_entity_labels
            from .structured import span_costs
            cost = None
            if use_risk:
                cost = span_costs(brackets_from_entity_labels(entity_labels, drop_crossing=False), L=L, device=device)
            risk, entropy = self.diora.tree_objective(cost)
            if use_risk:
                out.append(('risk', self.risk_loss_weight * risk.mean()))
            if use_entropy:
                out.append(('entropy', self.entropy_loss_weight * entropy.mean()))
        if self.uses_teacher():
            out.append(('kl', self.kl_loss_weight * self.diora.parse_divergence(self.teacher, direction=self.kl_direction)))
        return out


def select_diora(arch, obj_feats):
    """The module class `build_net` takes for --arch / --obj_feats (trainer.py:518-526).  The reference knows 'mlp' (cliora.DioraMLP with
    obj_feats, diora.DioraMLP without) and raises NotImplementedError for everything else; BASELINE config 5 names the TreeLSTM, which the
    reference ships only as commented text (vg.py:28-76): 'treelstm' selects this library's reconstruction of it (text-only; parity
    unpinned, cliora_amd/treelstm.py), any other name raises like the reference."""
    if arch == 'mlp':
        return VLDiora if obj_feats else TextDiora
    if arch == 'treelstm':
        if obj_feats:
            raise NotImplementedError('arch=treelstm is text-only (the reference has no vision-language TreeLSTM)')
        from .treelstm import DioraTreeLSTM
        return DioraTreeLSTM
    raise NotImplementedError('arch=%r (trainer.py:518-526 knows mlp; this library adds treelstm)' % (arch,))


def build_net(size, embeddings, obj_feats=False, img_dim=2048, k_neg=100, share=True, normalize='unit',
              vg_loss=False, use_contr=False, vl_margin=0.2, alpha_contr=1.0, alpha_vg=1.0, arch='mlp', bracket_loss_weight=0.0,
              risk_loss_weight=0.0, entropy_loss_weight=0.0, full_softmax=False, hard=False, hinge_loss_weight=0.0, hinge_margin=1.0,
              hinge_penalty=float('inf'), teacher=None, kl_loss_weight=0.0, kl_direction='forward'):
    """What trainer.py:504-582 assembles, on the native chart modules.  full_softmax: the reconstruction loss is the exact one over the
    whole table (ReconstructionSoftmaxLoss(full_vocab=True)) instead of the reference's sampled loss.  hard: the chart module encodes
    every cell's single best split (S-DIORA, `--arch hard` of the reference's training script; text-only DioraMLP).  teacher,
    kl_loss_weight, kl_direction: Net's -- a frozen chart module whose parse distribution each training step is pulled towards."""
    embed = Embed(embeddings, embeddings.weight.shape[1], size)
    enc = ImageEncoder(img_dim, size)
    diora = select_diora(arch, obj_feats)(size, outside=True, normalize=normalize, compress=False, share=share)
    if hard:
        diora.hard = True            # forward refuses it on a module that is not the text-only DioraMLP
    losses = [ReconstructionSoftmaxLoss(embeddings, embeddings.weight.shape[1], size, k_neg=k_neg, full_vocab=full_softmax)]
    if vg_loss:
        losses.append(VGLoss(alpha_vg))
    if obj_feats and use_contr:
        losses.append(ContrastiveLoss(vl_margin, alpha_contr))
    if obj_feats:
        embeddings.weight.requires_grad = False              # trainer.py:541
    return Net(embed, enc, diora, obj_feats, losses, bracket_loss_weight=bracket_loss_weight, risk_loss_weight=risk_loss_weight,
               entropy_loss_weight=entropy_loss_weight, hinge_loss_weight=hinge_loss_weight, hinge_margin=hinge_margin,
               hinge_penalty=hinge_penalty, teacher=teacher, kl_loss_weight=kl_loss_weight, kl_direction=kl_direction)


class Trainer(object):
    def __init__(self, net, lr=2e-3, reducer=None, negative_sampler=None, k_neg=100):
        self.net = net
        self.negative_sampler = negative_sampler             # cliora_amd.sampling.NegativeSampler or None (batch_iterator.py:158-160)
        self.k_neg = k_neg
        self.params = [p for p in net.parameters() if p.requires_grad]
        self.reducer = reducer                               # cliora_amd.parallel.FlatGradAllReduce or None
        self.defer_table_grads = True
        self._loss_host, self._loss_ev, self._loss_pending = None, None, False      # pinned scalar + event of the per-step loss read (step(sync=True))
        self.fused = _native(*self.params)                   # clip + Adam as three launches over one flat buffer (heads.FusedClipAdam)
        if self.fused:
            self.optimizer = heads.FusedClipAdam(self.params, lr=lr, betas=(0.9, 0.999), eps=1e-8, max_norm=5.0, reducer=reducer)
        else:
            self.optimizer = torch.optim.Adam(self.params, lr=lr, betas=(0.9, 0.999), eps=1e-8)

    def step(self, batch_map, train=True, compute_loss=True, sync=True):
        """One training / evaluation step (trainer.py:437-501).  sync=True returns the loss as a Python float like the reference's
        `.item()` (trainer.py:463) -- a device synchronisation per step; sync=False returns the 0-d tensor and lets the host run
        ahead of the device (read it when logging)."""
        self.net.train(train)
        neg_samples = batch_map.get('neg_samples')
        if neg_samples is None and self.negative_sampler is not None:       # drawn on the current stream, ahead of the forward
            neg_samples = self.negative_sampler.sample(self.k_neg)
        with torch.set_grad_enabled(train):
            if ((getattr(self.net, 'bracket_loss_weight', 0.0) > 0 or getattr(self.net, 'risk_loss_weight', 0.0) > 0
                 or getattr(self.net, 'hinge_loss_weight', 0.0) > 0) and train and compute_loss
                    and batch_map.get('entity_labels') is not None):
                out = self.net(batch_map['sentences'], batch_map.get('obj_feats'), neg_samples, compute_loss,
                               entity_labels=batch_map['entity_labels'])
            else:
                out = self.net(batch_map['sentences'], batch_map.get('obj_feats'), neg_samples, compute_loss)
        total = out.total() if isinstance(out, LossDict) else out['total_loss'].mean(dim=0).sum()
        # sync=True returns the loss as a Python float like the reference's `.item()` (trainer.py:463).  Its value is final once the FORWARD is:
        # it is copied to pinned host memory here, behind the forward, and read at the end of the step by waiting for THAT copy only -- the
        # host then goes on to enqueue the next step while this one's backward and update still run, instead of waiting for them too.
        loss_ev = None
        if sync and total.is_cuda:
            if self._loss_host is None:
                self._loss_host = torch.empty((), dtype=torch.float32, pin_memory=True)
                self._loss_ev = torch.cuda.Event()
            if self._loss_pending:                        # the previous step's copy into the same pinned scalar (already waited for by its step)
                self._loss_ev.synchronize()
            self._loss_host.copy_(total.detach(), non_blocking=True)
            self._loss_ev.record(torch.cuda.current_stream(total.device))
            self._loss_pending = True
            loss_ev = self._loss_ev
        if train:
            self._backward_and_update(total)
        if loss_ev is not None:
            loss_ev.synchronize()
            self._loss_pending = False
            return {'total_loss': float(self._loss_host)}
        return {'total_loss': float(total.detach()) if sync else total.detach()}

    def _backward_and_update(self, total):
        """backward, all-reduce, clip 5.0 + Adam (trainer.py:483-501) from the step's scalar loss."""
        self.optimizer.zero_grad()
        # this step owns its gradients from backward to the update, so the embedding table's gradient is assembled once, in the flat
        # buffer, from every lookup's rows (heads.DeferredTableGrads) instead of one dense scatter per lookup + dense adds
        defer = heads.DeferredTableGrads(self.optimizer.grads) if (self.fused and self.defer_table_grads) else None
        heads._deferred = defer
        heads._step_lanes = lanes = set() if self.fused else None
        try:
            total.backward()
        finally:
            heads._deferred = None
            heads._step_lanes = None
        for lane in (lanes or ()):               # leaf gradients that backward nodes left to the caller lane (heads._step_lane)
            torch.cuda.current_stream(lane.device).wait_stream(lane)
        if defer is not None:
            defer.flush()
        if self.reducer is not None:
            self.reducer.all_reduce_mean()
        if self.fused:
            self.optimizer.step(gathered=self.reducer is not None and self.optimizer.grads is self.reducer)
        else:
            torch.nn.utils.clip_grad_norm_(self.params, 5.0)
            self.optimizer.step()

    def step_ragged(self, sentences, neg_samples=None, entity_labels=None, max_batch=64, max_waste=None, pad_id=0, obj_feats=None):
        """One optimizer step over sentences of any lengths in 1..64: the sentences are packed into right-padded charts
        (cliora_amd.ragged.forward_ragged_train), each pack's losses are weighted, and one backward and one update follow.  The
        reconstruction term (and the structured terms with it) is weighted by the pack's share of the TOKENS -- over the step it is
        ONE mean over all tokens, what ``step`` gives for a batch of one length.  obj_feats: (N, R, img_dim) region features, one row
        per sentence, for a CLIORA net, which then trains whatever of vg_loss and contrastive_loss it carries too (DESIGN.md section
        23), each weighted by the pack's share of the SENTENCES: each is a mean over the pack's sentences and compares sentences of
        that pack only.  entity_labels: per sentence, as batch_map['entity_labels'], for the bracket / risk terms.  Returns the loss
        as a Python float."""
        from . import ragged
        if 'reconstruct_softmax_loss' not in self.net.loss_func_names:
            raise NotImplementedError('step_ragged trains the reconstruction loss of a net (with the vision-language losses it carries)')
        net = self.net
        net.train(True)
        if neg_samples is None and self.negative_sampler is not None:
            neg_samples = self.negative_sampler.sample(self.k_neg)
        n_tokens, n_sentences = float(sum(len(s) for s in sentences)), float(len(sentences))
        total = None
        # a net with a teacher: the teacher runs on each pack's own chart inputs, taken as the pack's forward receives them
        seen, hook = [], None
        if net.kl_loss_weight != 0 and net.teacher is not None:
            hook = net.diora.register_forward_pre_hook(lambda _, args: seen.append(args))
        try:
            with torch.enable_grad():
                for idx, lens, diora in ragged.forward_ragged_train(net, sentences, max_batch=max_batch, pad_id=pad_id, obj_feats=obj_feats,
                                                                    max_waste=ragged.DEFAULT_MAX_WASTE if max_waste is None else max_waste):
                    group = [sentences[i] for i in idx]
                    labels = [entity_labels[i] for i in idx] if entity_labels is not None else None
                    part = ragged.reconstruction_loss_ragged(net, group, neg_samples, diora)
                    if hook is not None:                  # inside pass alone on the padded pack; the student's holder has the lengths
                        net.run_teacher(*seen[-1])
                        del seen[:]
                    for _, v in net.structured_losses(labels, diora._plan.L, part.device):      # each sentence's own triangle (the holder's lengths)
                        part = part + v
                    part = part * (sum(len(s) for s in group) / n_tokens)
                    for name in net.loss_func_names:
                        if 'contrastive' in name:
                            part = part + getattr(net, name)(diora, lens) * (len(idx) / n_sentences)
                        elif 'reconstruct' not in name:
                            part = part + getattr(net, name)(diora.vg_atten_score, lens) * (len(idx) / n_sentences)
                    total = part if total is None else total + part
        finally:
            if hook is not None:
                hook.remove()
        if total is None:
            raise ValueError('step_ragged: no sentence')
        self._backward_and_update(total)
        return {'total_loss': float(total.detach())}
