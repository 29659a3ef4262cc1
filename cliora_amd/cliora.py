"""MI355X-native drop-in for ``cliora.net.cliora.DioraMLP`` (cliora/net/cliora.py:205-488):
the vision-language chart model.  Same constructor and
``forward(x_span, x_word, obj_embed_span, obj_embed_word) -> None``; besides the six charts it
leaves ``all_atten_score (B,B,C,R)``, ``vg_atten_score (B,B,L,R)`` and ``atten_score (B,L,R)``
on the module (cliora.py:453-468).

Two autograd nodes, both HIP behind the C ABI: the chart (with the AttentionHead residual at
the leaves and in every inside aggregate, cliora.py:28-42, 71-80, 140-157) and the
span-region / word-region scorers.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import ptr, stream
from .diora import DioraBase, ComposeMLP, Bilinear, _cont

DROPOUT_P = 0.1   # AttentionHead: nn.Dropout(0.1), cliora.py:32


class VLScoreFunction(torch.autograd.Function):
    """cliora_vl_scores_forward / _backward: the einsum('abx,cdx->acbd') scorers of cliora.py:453-466."""

    @staticmethod
    def forward(ctx, plan, training, inside_h, outside_h, obj_span, x_word, obj_word, want_all):
        """x_word / obj_word None: all_atten only; want_all False (training mode only): vg_atten only."""
        B, L, Cc, R = plan.B, plan.L, plan.C, plan.R
        tens = [_cont(t) for t in (inside_h, outside_h, obj_span, x_word, obj_word)]
        dev = tens[0].device
        with _lib.device_guard(tens[0]):
            all_att = torch.empty((B, B, Cc, R), device=dev, dtype=torch.float32) if want_all else None
            vg = torch.empty((B, B, L, R), device=dev, dtype=torch.float32) if x_word is not None else None
            nbytes = _lib.fn('cliora_plan_vl_workspace_bytes')(plan.handle)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            _lib.call('cliora_vl_scores_forward', plan.handle, *map(ptr, tens), int(training), ptr(all_att), ptr(vg), ptr(ws), nbytes, stream())
        ctx.plan, ctx.training, ctx.nbytes = plan, int(training), nbytes
        ctx.have_words = x_word is not None
        ctx.save_for_backward(*[t for t in tens if t is not None])
        ctx.set_materialize_grads(False)
        return all_att, vg

    @staticmethod
    def backward(ctx, d_all, d_vg):
        plan = ctx.plan
        if ctx.have_words:
            inside_h, outside_h, obj_span, x_word, obj_word = ctx.saved_tensors
        else:
            (inside_h, outside_h, obj_span), x_word, obj_word = ctx.saved_tensors, None, None
        need = ctx.needs_input_grad          # (plan, training, inside_h, outside_h, obj_span, x_word, obj_word, want_all)
        with _lib.device_guard(inside_h):
            d_all, d_vg = _cont(d_all), _cont(d_vg)
            d_sum = torch.empty_like(inside_h) if (need[2] or need[3]) else None
            d_obj_span = torch.empty_like(obj_span) if need[4] else None
            d_x_word = torch.empty_like(x_word) if (x_word is not None and need[5]) else None
            d_obj_word = torch.empty_like(obj_word) if (obj_word is not None and need[6]) else None
            ws = torch.empty(ctx.nbytes, device=inside_h.device, dtype=torch.uint8)
            _lib.call('cliora_vl_scores_backward', plan.handle, ptr(inside_h), ptr(outside_h), ptr(obj_span), ptr(x_word), ptr(obj_word),
                      ctx.training, ptr(d_all), ptr(d_vg), ptr(d_sum), ptr(d_obj_span), ptr(d_x_word), ptr(d_obj_word), ptr(ws),
                      ctx.nbytes, stream())
        return None, None, d_sum, d_sum, d_obj_span, d_x_word, d_obj_word, None


def _max_backward(ctx, d_max, want_sum, want_obj):
    """cliora_vl_scores_max_backward on the current stream for the outputs wanted (the entry takes either as NULL) -> (d_sum, d_obj)."""
    inside_h, outside_h, obj_span, arg = ctx.saved_tensors
    with _lib.device_guard(inside_h):
        d_sum = torch.empty_like(inside_h) if want_sum else None
        d_obj = torch.empty_like(obj_span) if want_obj else None
        ws = torch.empty(ctx.nbytes, device=inside_h.device, dtype=torch.uint8)
        _lib.call('cliora_vl_scores_max_backward', ctx.plan.handle, ptr(inside_h), ptr(outside_h), ptr(obj_span), ptr(d_max), ptr(arg),
                  ptr(d_sum), ptr(d_obj), ptr(ws), ctx.nbytes, stream())
    return d_sum, d_obj


class VLMaxFunction(torch.autograd.Function):
    """cliora_vl_scores_max_forward / _backward: max over the R regions of einsum('abx,cdx->acbd', inside_h + outside_h, obj)
    (cliora.py:457 followed by trainer.py:101) without the (B, B, C, R) tensor.  The backward computes the gradients its inputs need:
    applied to a detached region matrix it owns the gradient of the CHART rows only (d inside_h = d outside_h = d_sum_h), and VLMaxObj
    the region matrix's (region_max)."""

    @staticmethod
    def forward(ctx, plan, inside_h, outside_h, obj_span):
        B, Cc = plan.B, plan.C
        tens = [t.contiguous().float() for t in (inside_h, outside_h, obj_span)]
        dev = tens[0].device
        with _lib.device_guard(tens[0]):
            vmax = torch.empty((B, B, Cc), device=dev, dtype=torch.float32)
            arg = torch.empty((B, B, Cc), device=dev, dtype=torch.int32)
            nbytes = _lib.fn('cliora_plan_vl_workspace_bytes')(plan.handle)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            _lib.call('cliora_vl_scores_max_forward', plan.handle, *map(ptr, tens), ptr(vmax), ptr(arg), ptr(ws), nbytes, stream())
        ctx.plan, ctx.nbytes = plan, nbytes
        ctx.save_for_backward(*tens, arg)
        ctx.mark_non_differentiable(arg)
        return vmax, arg

    @staticmethod
    def backward(ctx, d_max, _d_arg):
        need = ctx.needs_input_grad          # (plan, inside_h, outside_h, obj_span)
        if d_max is None:
            return None, None, None, None
        d_sum, d_obj = _max_backward(ctx, d_max.contiguous().float(), need[1] or need[2], need[3])
        return None, d_sum, d_sum, d_obj


class VLMaxObj(torch.autograd.Function):
    """The region matrix's half of the region-max scorer's backward, on the library's caller lane, so that the chart backward -- which
    needs d_sum_h -- does not wait for the 0.1-0.2 ms of the region-matrix half.  forward: no work (hands `vmax` through); it is called
    under the caller lane's stream so that autograd runs the backward there (a node's backward runs on its forward's stream).  JoinGrad
    hands the one cotangent to this node and to VLMaxFunction."""

    @staticmethod
    def forward(ctx, plan, obj_span, inside_h, outside_h, vmax, arg):
        ctx.plan = plan
        ctx.nbytes = _lib.fn('cliora_plan_vl_workspace_bytes')(plan.handle)
        ctx.save_for_backward(inside_h, outside_h, obj_span, arg)
        return vmax.view_as(vmax)

    @staticmethod
    def backward(ctx, d_max):
        if d_max is None:
            return None, None, None, None, None, None
        d_max = d_max.contiguous().float()
        lane = torch.cuda.current_stream(d_max.device)
        for t in (*ctx.saved_tensors, d_max):       # made on the current stream, read here on the lane (see forward)
            t.record_stream(lane)
        return None, _max_backward(ctx, d_max, False, True)[1], None, None, None, None


class JoinGrad(torch.autograd.Function):
    """a (values) with b as a second path for the cotangent: forward returns a, backward hands the same cotangent to a's and b's producers."""

    @staticmethod
    def forward(ctx, a, b):
        return a.view_as(a)

    @staticmethod
    def backward(ctx, g):
        return g, g


def region_max(plan, inside_h, outside_h, obj_span, lane):
    """(max over regions, its region) of the span-region scores; with a lane: the region matrix's gradient as a node of its own there."""
    if lane is None or not obj_span.requires_grad or not torch.is_grad_enabled():
        return VLMaxFunction.apply(plan, inside_h, outside_h, obj_span)
    vmax_a, arg = VLMaxFunction.apply(plan, inside_h, outside_h, obj_span.detach())
    with torch.cuda.stream(lane):
        vmax_b = VLMaxObj.apply(plan, obj_span, inside_h.detach(), outside_h.detach(), vmax_a.detach(), arg)
    return JoinGrad.apply(vmax_a, vmax_b), arg


class RegionMax(tuple):
    """What `all_atten_score.max(-1)` returns: (values, indices) with the field names of torch.return_types.max."""
    values = property(lambda self: self[0])
    indices = property(lambda self: self[1])


class LazyRegionScores:
    """`all_atten_score` of cliora.py:457 -- einsum('abx,cdx->acbd', inside_h + outside_h, obj_span), (B, B, C, R) -- in training
    mode, before anyone has asked for it.  Its one consumer there, ContrastiveLoss (trainer.py:101), takes `.max(-1).values`:
    that runs the fused scorer (the GEMM's epilogue keeps the maximum and its region per (sentence, image, span); the 124 MB
    tensor at B 64 / L 20 / R 36 is never written or differentiated through).  Anything else -- indexing, torch functions,
    tensor attributes -- materialises the dense tensor once through the ordinary scorer and behaves like it."""

    def __init__(self, plan, inside_h, outside_h, obj_span, lane=None):
        self._plan, self._args, self._lane = plan, (inside_h, outside_h, obj_span), lane
        self._dense, self._max = None, None
        self.shape = torch.Size((plan.B, plan.B, plan.C, plan.R))
        self.device, self.dtype = inside_h.device, torch.float32

    def size(self, dim=None):
        return self.shape if dim is None else self.shape[dim]

    def dim(self):
        return 4

    def max(self, dim=None, keepdim=False):
        if dim in (-1, 3) and not keepdim and self._dense is None:
            if self._max is None:
                vmax, arg = region_max(self._plan, *self._args, self._lane)
                self._max = RegionMax((vmax, arg.long()))
            return self._max
        return self.materialize().max() if dim is None else self.materialize().max(dim, keepdim)

    def materialize(self):
        if self._dense is None:
            ih, oh, obj = self._args
            self._dense = VLScoreFunction.apply(self._plan, True, ih, oh, obj, None, None, True)[0]
        return self._dense

    def __getattr__(self, name):                    # only reached for names not defined above
        if name.startswith('_'):                    # private / dunder probes (copy, pickle, ...) must not materialise or recurse
            raise AttributeError(name)
        return getattr(self.materialize(), name)

    def __getitem__(self, idx):
        return self.materialize()[idx]

    def __len__(self):
        return self.shape[0]

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        un = lambda a: a.materialize() if isinstance(a, LazyRegionScores) else a
        return func(*[un(a) for a in args], **{k: un(v) for k, v in (kwargs or {}).items()})


def _delegate(name):
    def op(self, *a, **k):
        return getattr(self.materialize(), name)(*a, **k)
    op.__name__ = name
    return op


for _n in ('__add__', '__radd__', '__sub__', '__rsub__', '__mul__', '__rmul__', '__truediv__', '__rtruediv__', '__neg__', '__pow__',
           '__matmul__', '__lt__', '__le__', '__gt__', '__ge__', '__eq__', '__ne__', '__iter__', '__repr__', '__array__'):
    setattr(LazyRegionScores, _n, _delegate(_n))
LazyRegionScores.__hash__ = object.__hash__


class AttentionHead(nn.Module):
    """Parameter-free; kept for the module tree and the dropout rate (cliora.py:28-42)."""

    def __init__(self, q_dim, k_dim, v_dim, h_dim):
        super().__init__()
        self.h_dim = h_dim
        self.dropout = nn.Dropout(DROPOUT_P)


class VLComposeMLP(ComposeMLP):
    pass


class DioraMLP(DioraBase):
    vision_language = True

    def init_parameters(self):
        self.atten_head = AttentionHead(self.size, self.size, self.size, self.size)
        self.inside_score_func = Bilinear(self.size)
        self.inside_compose_func = VLComposeMLP(self.size, leaf=True)
        if self.share:
            self.outside_score_func = self.inside_score_func
            self.outside_compose_func = self.inside_compose_func
        else:
            self.outside_score_func = Bilinear(self.size)
            self.outside_compose_func = VLComposeMLP(self.size)
        if self.compress:
            self.root_mat_out = nn.Parameter(torch.empty(self.size, self.size))
        else:
            self.root_vector_out_h = nn.Parameter(torch.empty(self.size))
        self.root_vector_out_c = None
        self.dropout_mask = None      # tests inject a (B, C, R) pre-scaled mask here; None = draw one per forward
        self.lazy_region_scores = True   # training mode: all_atten_score is a LazyRegionScores (False: always the dense tensor)
        # The library's caller lane (include/cliora_chart.h: cliora_device_side_stream) for the work of a training step that the chart does not
        # wait for: the word-region scorer (its inputs may already live there: harness.Net puts the word projections on it) and the region
        # matrix's half of the region-max backward.  None (default) = everything on the current stream; harness.Net sets it per forward.
        self.word_lane = None
        # True: x_word / obj_embed_word were produced ON the lane (harness.Net.forward), so the scorer needs no wait for the current stream --
        # it then runs beside the chart's forward instead of behind it
        self.word_inputs_on_lane = False

    def get_chart_wrapper(self):
        return self

    def _regions(self, obj_embed_span):
        if obj_embed_span is None:
            raise ValueError('the CLIORA module needs obj_embed_span (use cliora_amd.diora.DioraMLP for text only)')
        return obj_embed_span.shape[1]

    def _drop_mask(self, plan, dev):
        if not self.training:
            return None
        mask = self.dropout_mask
        if mask is None:   # same distribution as nn.Dropout(0.1) on the (.., R) probabilities
            mask = F.dropout(torch.ones((plan.B, plan.C, plan.R), device=dev), DROPOUT_P, True)
        return mask

    def _chart_inputs(self, plan, x_span, obj_embed_span):
        return obj_embed_span, self._drop_mask(plan, x_span.device)

    def forward(self, x_span, x_word, obj_embed_span=None, obj_embed_word=None):
        super().forward(x_span, x_word, obj_embed_span, obj_embed_word)
        plan, ch = self._plan, self.chart
        ih, oh = ch.inside_h, ch.outside_h
        ch.outside_c = torch.zeros_like(oh)       # made with every forward here (the text-only module leaves it to its first reader)
        # cliora.py:453-468
        if self.training and self.lazy_region_scores:
            # training: vg_atten does not read all_atten (cliora.py:459-461) and the contrastive loss only wants its region max
            # (a padded chart of mixed lengths, _ragged_train: everything on the current stream)
            lane = self.word_lane if x_span.is_cuda and self.__dict__.get('_ragged_train') is None else None
            if lane is not None:
                # the word-region scorer on the caller lane: neither its forward nor its backward (0.2 ms at c3) is on the chart's path; the
                # chart rows and the span region matrix are not read by it (detached: no gradient edge into the chart either)
                cur = torch.cuda.current_stream(x_span.device)
                if not self.word_inputs_on_lane:      # inputs produced on this stream: the lane waits for them (and for the whole chart before them)
                    lane.wait_stream(cur)
                    for t in (x_word, obj_embed_word):      # ... and their memory is not reused before the scorer's backward there is done
                        if t is not None:
                            t.record_stream(lane)
                with torch.cuda.stream(lane):
                    _, vg = VLScoreFunction.apply(plan, True, ih.detach(), oh.detach(), obj_embed_span.detach(), x_word, obj_embed_word, False)
                cur.wait_stream(lane)                 # whoever reads vg next on this stream (the VG loss) finds it complete
                vg.record_stream(cur)
            else:
                _, vg = VLScoreFunction.apply(plan, True, ih, oh, obj_embed_span, x_word, obj_embed_word, False)
            all_att = LazyRegionScores(plan, ih, oh, obj_embed_span, lane)
        else:
            all_att, vg = VLScoreFunction.apply(plan, self.training, ih, oh, obj_embed_span, x_word, obj_embed_word, True)
        self.__dict__.update(all_atten_score=all_att, vg_atten_score_word=vg, vg_atten_score=vg,
                             atten_score=torch.diagonal(vg, 0, 0, 1).permute(2, 0, 1))
        return None
