"""MI355X-native drop-in for ``cliora.net.diora.DioraMLP`` (cliora/net/diora.py:205-471).

Same constructor, same ``forward(x_span, x_word, obj_embed_span=None,
obj_embed_word=None) -> None`` with results left on attributes, same parameter
names (state_dict keys), same hooks -- but the whole chart recursion (leaf
transform, inside pass, outside pass) and its backward run as hand-written HIP
kernels behind the C ABI of include/cliora_chart.h.  torch only owns the device
memory, the stream and the autograd edge.  There is no CPU fallback: without
the HIP library (or on CPU tensors) ``forward`` raises.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from .index import Index


from ._lib import ptr as _ptr, stream as _stream, param_struct as _param_struct      # noqa: F401  (re-exports: the tests import them from here)
from .query import ChartQuery, host_copy, per_sentence, span_buffer, workspace_slices      # noqa: F401  (re-exports, as above)


def _grad_out(t):
    """Output tensor for the gradient of the parameter that `t` (its detached view) belongs to: the parameter's slice of a live
    flat all-reduce buffer (cliora_amd.parallel: the backward then writes straight into what RCCL reduces), else a fresh tensor."""
    global _grad_buffer_for
    if _grad_buffer_for is None:
        from .parallel import grad_buffer_for as _g
        _grad_buffer_for = _g
    v = _grad_buffer_for(t)
    return v if v is not None else torch.empty_like(t)


_grad_buffer_for = None


def chart_buffers(plan, dev, flags, *widths):
    """The chart outputs of one forward -- an uninitialised fp32 (B, C, w) per width -- and its workspace, with the per-pair tail when
    `flags` asks for the hooks' states.  -> (outputs, workspace, its bytes)."""
    outs = [torch.empty((plan.B, plan.C, w), device=dev, dtype=torch.float32) for w in widths]
    nbytes = plan.fwd_bytes + (plan.pair_bytes if flags & _lib.FWD_PAIR_STATES else 0)
    return outs, torch.empty(nbytes, device=dev, dtype=torch.uint8), nbytes


def _cont(g):
    return g.contiguous().float() if g is not None else None


class ChartWorkspaces(list):
    """The holder of a forward's workspace(s), made anew by every forward of a chart module, with the slot through which
    cliora_amd.structured hands the chart node a cotangent on the inside split scores: `split_cot` is a one-element list that the
    node of that forward shares (ChartFunction keeps it in its ctx), so a cotangent left there can reach that forward's backward only.
    `lengths`: the int32 device lengths of a padded training chart of mixed lengths (RaggedChartFunction), else None; the structured
    losses read each sentence's own triangle through them.  `selection`: the (sel_in, sel_out) int32 (B, C) device tensors a hard chart
    (cliora_chart_forward_hard) writes its selected splits into, set by the module before the node runs, else None."""
    __slots__ = ('split_cot', 'lengths', 'selection')

    def __init__(self):
        super().__init__()
        self.split_cot = [None]
        self.lengths = None
        self.selection = None


def check_lengths(lengths, B, dev):
    """The lengths of a padded chart's sentences as the C entries take them: int32, (B,), on the chart's device."""
    if lengths.dtype != torch.int32 or lengths.numel() != B or lengths.device != dev:
        raise ValueError('lengths must be an int32 tensor of %d sentences on %s' % (B, dev))
    return lengths.contiguous()


def _chart_forward(entry, plan, flags, x_span, obj_span, drop_mask, params, lengths=None, root_levels=None, selection=None):
    """The call of a chart forward entry, for every route: the inputs made contiguous fp32, the parameters detached, the outputs and
    the workspace allocated (chart_buffers), inside_c zeroed for a plan with regions, then `entry` under the tensors' device.  With
    `lengths` (a padded chart of mixed lengths) the entry also gets them, `root_levels` as the entry takes it and a fresh status
    word.  With `selection` (a hard chart, text-only: `entry` is cliora_chart_forward_hard) the entry gets the two selection arrays
    in place of the regions' arguments.
    -> (x_span, lengths, obj_span, drop_mask, ptens, the four charts, inside_c or None, workspace, status or None)."""
    if not x_span.is_cuda:
        raise _lib.ChartLibError('the chart path runs on the GPU only (got a CPU tensor)')
    D, dev, vl, status, tail = plan.D, x_span.device, obj_span is not None, None, ()
    if lengths is not None:
        lengths = check_lengths(lengths, plan.B, dev)
    x_span, obj_span, drop_mask = x_span.contiguous().float(), _cont(obj_span), _cont(drop_mask)
    ptens = {n: (p.detach().contiguous() if p is not None else None) for n, p in zip(_lib.PARAM_FIELDS, params)}
    with _lib.device_guard(x_span):
        outs, ws, nbytes = chart_buffers(plan, dev, flags, *((D, 1, D, 1, D) if vl else (D, 1, D, 1)))
        inside_c = outs.pop().zero_() if vl else None
        if lengths is not None:
            status = torch.empty(1, device=dev, dtype=torch.int32)
            tail = (_ptr(lengths), root_levels, _ptr(status))
        pst = _param_struct(ptens)
        if selection is not None:         # (with lengths: cliora_chart_forward_ragged_hard, root_levels as two host words)
            _lib.call(entry, plan.handle, C.byref(pst), _ptr(x_span), *map(_ptr, outs), *map(_ptr, selection), _ptr(ws), nbytes, flags,
                      *tail, _stream())
        else:
            _lib.call(entry, plan.handle, C.byref(pst), _ptr(x_span), _ptr(obj_span), _ptr(drop_mask), *map(_ptr, outs), _ptr(inside_c),
                      _ptr(ws), nbytes, flags, *tail, _stream())
    return x_span, lengths, obj_span, drop_mask, ptens, outs, inside_c, ws, status


def _chart_backward(ctx, x_span, obj_span, charts, cots, lengths=None):
    """The call of a chart backward entry for the node `ctx`: the gradient outputs and the workspace allocated, the split cotangent of
    a structured loss of the same forward taken (once), then cliora_chart_backward -- cliora_chart_backward_split when there is a split
    cotangent -- or, with `lengths`, cliora_chart_backward_ragged[_vl], which masks the cotangents into buffers of their own.
    -> (d_x, d_obj or None, the parameters' gradients in _lib.PARAM_FIELDS order)."""
    plan = ctx.plan
    with _lib.device_guard(x_span):
        d_x = torch.empty_like(x_span)
        d_obj = torch.empty_like(obj_span) if ctx.vl else None
        pst = _param_struct(ctx.ptens)
        g = {n: (_grad_out(t) if t is not None else None) for n, t in ctx.ptens.items()}
        wsb = torch.empty(plan.bwd_bytes, device=x_span.device, dtype=torch.uint8)
        gst = _param_struct(g)
        d_split = ctx.split_cot[0] if ctx.split_cot is not None else None
        if d_split is not None:
            ctx.split_cot[0] = None                       # a bracket loss of this forward left it: taken once
        cots = [_cont(d) for d in cots]
        if lengths is None:
            entry, split, tail = 'cliora_chart_backward' + ('_split' if d_split is not None else ''), d_split is not None, ()
        else:
            masked = [torch.empty_like(d) if d is not None else None for d in cots]      # the library masks the cotangents into these
            entry, split = 'cliora_chart_backward_ragged' + ('_vl' if ctx.vl else ''), True
            tail = (_ptr(lengths), ctx.root_levels, *map(_ptr, masked))
        _lib.call(entry, plan.handle, C.byref(pst), _ptr(x_span), _ptr(obj_span), _ptr(ctx.drop_mask), *map(_ptr, charts),
                  *map(_ptr, cots), *((_ptr(d_split),) if split else ()), _ptr(ctx.ws), plan.fwd_bytes, _ptr(wsb), plan.bwd_bytes, _ptr(d_x),
                  _ptr(d_obj), C.byref(gst), ctx.run_outside, *tail, _stream())
    return d_x, d_obj, tuple(g[n] for n in _lib.PARAM_FIELDS)


class ChartFunction(torch.autograd.Function):
    """One autograd node for the whole inside-outside chart, text-only (obj_span None) or with image regions (a plan of R > 0).

    forward  -> cliora_chart_forward   (replaces diora.py:283-398 as executed by DioraBase.forward); cliora_chart_forward_hard when the
                holder carries selection arrays (a hard chart: same workspace, same backward)
    backward -> cliora_chart_backward  (replaces what autograd replays through those lines), or cliora_chart_backward_split when a
                bracket loss of the same forward left a cotangent on the split scores (cliora_amd.structured)
    Inputs: plan, holder (list that receives the forward workspace), run_outside, x_span, obj_span, drop_mask, then the parameter
    tensors in _lib.PARAM_FIELDS order (None for the out_* set when the weights are shared).  Without obj_span the library gets NULL
    for obj_span, drop_mask, inside_c and d_obj_span, and the fifth output, inside_c, is None.
    Every C-ABI call runs under the tensors' device (the plan's index tables and the kernels' LDS attribute are per device).
    """

    @staticmethod
    def forward(ctx, plan, holder, run_outside, x_span, obj_span, drop_mask, *params):
        run_outside, vl = int(run_outside), obj_span is not None
        selection = getattr(holder, 'selection', None)
        x_span, _, obj_span, drop_mask, ptens, outs, inside_c, ws, _ = _chart_forward(
            'cliora_chart_forward' + ('_hard' if selection is not None else ''), plan, run_outside, x_span, obj_span, drop_mask, params,
            selection=selection)
        ctx.plan, ctx.run_outside, ctx.ws, ctx.ptens, ctx.drop_mask, ctx.vl = plan, run_outside & 1, ws, ptens, drop_mask, vl
        ctx.split_cot = getattr(holder, 'split_cot', None)      # cliora_amd.structured leaves d_split there (a plain list: no such input)
        ctx.save_for_backward(x_span, *((obj_span,) if vl else ()), *outs)
        ctx.set_materialize_grads(False)
        if vl:
            ctx.mark_non_differentiable(inside_c)
        holder.clear()
        holder.append(ws)
        return (*outs, inside_c)

    @staticmethod
    def backward(ctx, d_ih, d_is, d_oh, d_os, _d_ic):
        saved = ctx.saved_tensors
        d_x, d_obj, grads = _chart_backward(ctx, saved[0], saved[1] if ctx.vl else None, saved[-4:], (d_ih, d_is, d_oh, d_os))
        return (None, None, None, d_x, d_obj, None) + grads


class RaggedChartFunction(torch.autograd.Function):
    """ChartFunction for a right-padded batch of mixed lengths (DESIGN.md sections 22 and 23).

    forward  -> cliora_chart_forward_ragged_train   (the padded chart's schedule with the backward's state written)
    backward -> cliora_chart_backward_ragged        (the split cotangent of a structured loss of the same forward included)
    With image regions (obj_span given, a plan of R > 0) the `_vl` forms of the two entries: the (B, C, R) dropout mask is taken and
    d obj_span returned.  When the holder carries selection arrays (a hard padded chart) the forward is
    cliora_chart_forward_ragged_hard and the backward the same cliora_chart_backward_ragged.
    Inputs: plan, holder, run_outside, lengths (int32 device tensor (B,)), root_levels (the bit mask of {n - 1}), x_span, obj_span,
    drop_mask (both None for text-only DIORA), then the parameter tensors in _lib.PARAM_FIELDS order.  Outputs: the four charts --
    valid on each sentence's own triangle, unspecified beyond it, where their cotangents are ignored -- the status word (1,) int32
    on the device, which the caller must read, and inside_c (None without regions)."""

    @staticmethod
    def forward(ctx, plan, holder, run_outside, lengths, root_levels, x_span, obj_span, drop_mask, *params):
        run_outside, vl = int(run_outside), obj_span is not None
        selection = getattr(holder, 'selection', None)
        if selection is not None:         # a hard padded chart (text-only): one entry for inference and training, the mask as two words
            entry, mask = 'cliora_chart_forward_ragged_hard', split_root_levels(root_levels)
        else:
            entry, mask = 'cliora_chart_forward_ragged_train' + ('_vl' if vl else ''), int(root_levels)
        x_span, lengths, obj_span, drop_mask, ptens, outs, inside_c, ws, status = _chart_forward(
            entry, plan, run_outside, x_span, obj_span, drop_mask, params, lengths, mask, selection=selection)
        ctx.plan, ctx.run_outside, ctx.ws, ctx.ptens, ctx.root_levels = plan, run_outside & 1, ws, ptens, int(root_levels)
        ctx.drop_mask, ctx.vl = drop_mask, vl
        ctx.split_cot = getattr(holder, 'split_cot', None)
        ctx.save_for_backward(x_span, lengths, *((obj_span,) if vl else ()), *outs)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(status, *((inside_c,) if vl else ()))
        holder.clear()
        holder.append(ws)
        holder.lengths = lengths
        return (*outs, status, inside_c)

    @staticmethod
    def backward(ctx, d_ih, d_is, d_oh, d_os, _d_status, _d_ic):
        saved = ctx.saved_tensors
        d_x, d_obj, grads = _chart_backward(ctx, saved[0], saved[2] if ctx.vl else None, saved[-4:], (d_ih, d_is, d_oh, d_os), saved[1])
        return (None, None, None, None, None, d_x, d_obj, None) + grads


def split_root_levels(mask):
    """A root-level mask of up to 128 bits as cliora_chart_forward_ragged_wide takes it: two 64-bit words in host memory, bit t & 63 of
    word t >> 6 for level t."""
    mask = int(mask)
    return (C.c_uint64 * 2)(mask & 0xFFFFFFFFFFFFFFFF, (mask >> 64) & 0xFFFFFFFFFFFFFFFF)


def ragged_chart(plan, holder, outside, x_span, obj_span, params, lengths, root_levels, hard_dense=False):
    """cliora_chart_forward_ragged (include/cliora_chart.h): both passes of a right-padded batch of mixed lengths, inference only, so no
    autograd node.  lengths: int32 device tensor (B,); root_levels: the bit mask of {n - 1}, a Python int.  A long plan (L > 64) runs
    through cliora_chart_forward_ragged_wide, which takes the mask as two 64-bit words; a short plan through the entry it always ran
    through.  A holder that carries selection arrays (a hard chart, text-only) runs cliora_chart_forward_ragged_hard at either length
    (hard_dense: CLIORA_FWD_HARD_DENSE).  -> inside_h, inside_s, outside_h, outside_s, inside_c (None for a text-only plan), status
    (1,) int32 on the device, which the caller must read."""
    entry, mask, flags = 'cliora_chart_forward_ragged', int(root_levels), int(bool(outside)) | _lib.FWD_NO_BACKWARD
    selection = getattr(holder, 'selection', None)
    if plan.L > _lib.MAX_L or selection is not None:
        if mask < 0 or mask >> _lib.MAX_L_FWD:
            raise ValueError('root_levels holds a bit at or above %d' % _lib.MAX_L_FWD)
        entry, mask = 'cliora_chart_forward_ragged_wide', split_root_levels(mask)
    if selection is not None:
        entry, flags = 'cliora_chart_forward_ragged_hard', flags | (_lib.FWD_HARD_DENSE if hard_dense else 0)
    _, _, _, _, _, outs, inside_c, ws, status = _chart_forward(entry, plan, flags, x_span.detach(),
                                                               obj_span.detach() if obj_span is not None else None, None, params, lengths,
                                                               mask, selection=selection)
    holder.clear()
    holder.append(ws)
    return (*outs, inside_c, status)


# --------------------------------------------------------------------------------------
# Parameter containers with the reference's module tree, so state_dict keys match
# (diora.py:26-97, 453-471).  Their forward() is never used on the product path.
# --------------------------------------------------------------------------------------
class ComposeMLP(nn.Module):
    def __init__(self, size, ninput=2, leaf=False):
        super().__init__()
        self.size, self.ninput = size, ninput
        if leaf:
            self.leaf_fc = nn.Linear(size, size)
        self.h_fcs = nn.Sequential(nn.Linear(2 * size, size), nn.ReLU(), nn.Linear(size, size), nn.ReLU())


class Bilinear(nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = size
        self.mat = nn.Parameter(torch.empty(size, size))


class Chart(object):
    """Attribute bag with the six chart tensors (diora.py:7-23).  DioraMLP's cell states are identically zero (diora.py:60-61, 70):
    they are created when first read (two fill launches and ~20 us of host time per step otherwise, for tensors nothing on the
    training path reads)."""
    __slots__ = ('inside_h', 'inside_s', 'outside_h', 'outside_s', '_ic', '_oc')

    def __init__(self):
        self._ic = self._oc = None

    @property
    def inside_c(self):
        if self._ic is None:
            self._ic = torch.zeros_like(self.inside_h)
        return self._ic

    @inside_c.setter
    def inside_c(self, v):
        self._ic = v

    @property
    def outside_c(self):
        if self._oc is None:
            self._oc = torch.zeros_like(self.outside_h)
        return self._oc

    @outside_c.setter
    def outside_c(self, v):
        self._oc = v


class DioraBase(nn.Module):
    vision_language = False
    # hard (S-DIORA) charts: every cell encodes its single best split.  A plain settable attribute; only the
    # text-only cliora_amd.diora.DioraMLP takes it (forward refuses the rest).  hard_dense: the same chart through the dense compose
    # kernels (CLIORA_FWD_HARD_DENSE: the on-device cross-check and the benchmark's baseline, not a tuning switch).
    hard = False
    hard_dense = False

    def __init__(self, size, word_mat=None, cate_mat=None, outside=True, normalize='unit', compress=False, share=True):
        super().__init__()
        assert normalize in ('none', 'unit'), 'Does not support "{}".'.format(normalize)
        self.size = size
        self.share = share
        self.outside = outside
        self.normalize = normalize
        self.compress = compress
        self.ninput = 2
        self.index = None
        self.charts = None
        # cliora_amd.ragged sets (lengths on the device, root-level mask) around an eval forward over a right-padded batch of mixed
        # lengths: the chart then runs through cliora_chart_forward_ragged (L > 64: _wide) and leaves its status word in _ragged_status
        self.__dict__['_ragged'] = None
        # cliora_amd.ragged sets the same pair around a TRAINING forward over such a batch (forward_ragged_train): the chart then is a
        # RaggedChartFunction node (text-only DIORA, or CLIORA with its regions)
        self.__dict__['_ragged_train'] = None
        # ... and, around the forward of a HARD module over such a batch, these two in their place: the chart
        # then runs through cliora_chart_forward_ragged_hard.  A hard module keeps refusing the two slots above (_check_hard).
        self.__dict__['_ragged_hard'] = None
        self.__dict__['_ragged_hard_train'] = None
        self.init_parameters()
        self.reset_parameters()
        self.reset()

    def init_parameters(self):
        raise NotImplementedError

    def reset_parameters(self):
        # every parameter ~ N(0, 1): diora.py:234-237
        for p in self.parameters():
            if p.requires_grad:
                p.data.normal_()

    # ---- attribute surface read by the losses / CKY / eval scripts
    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def is_cuda(self):
        d = self.device
        return d.index is not None and d.index >= 0

    inside_h = property(lambda self: self.chart.inside_h)
    inside_c = property(lambda self: self.chart.inside_c)
    inside_s = property(lambda self: self.chart.inside_s)
    outside_h = property(lambda self: self.chart.outside_h)
    outside_c = property(lambda self: self.chart.outside_c)
    outside_s = property(lambda self: self.chart.outside_s)

    def cuda(self, device=None):
        super().cuda(device)
        if self.index is not None:
            self.index.cuda = True
        return self

    def get(self, chart, level):
        L = self.length - level
        offset = self.index.get_offset(self.length)[level]
        return chart[:, offset:offset + L]

    def inside_hook(self, level, h, c, s):
        pass

    def outside_hook(self, level, h, c, s):
        pass

    def init_with_batch(self, h, c):
        # the native forward has already filled the chart; kept as an overridable method because
        # analysis/utils.py:67-76 wraps it with types.MethodType to attach its score store
        d = self.__dict__
        d['batch_size'], d['length'] = h.shape[0], h.shape[1]

    def reset(self):
        # plain attributes, written straight into the instance dict: nn.Module.__setattr__ walks its parameter / buffer / module
        # registries for every assignment (~3.5 us each; a configs[0]-sized step is bound by the host)
        self.__dict__.update(batch_size=None, length=None, chart=None, atten_score=None, all_atten_score=None, vg_atten_score=None,
                             _wss=None, _plan=None, _ragged_status=None, selection=None)

    def _check_long(self, L, needs_grad, hooks):
        """64 < L <= 128 runs on a forward-only plan (include/cliora_chart.h): every refusal before any launch.  A padded chart of mixed
        lengths (_ragged) is taken at these lengths too (cliora_chart_forward_ragged_wide)."""
        if L <= _lib.MAX_L:
            return
        if needs_grad or self.training:
            raise _lib.ChartLibError('L = %d > %d is inference only (the backward stops at %d words): call it in eval mode under '
                                     'torch.no_grad()' % (L, _lib.MAX_L, _lib.MAX_L))
        if hooks:
            raise _lib.ChartLibError('L = %d > %d: inside_hook / outside_hook overrides get no per-pair states (a long plan sizes no '
                                     'per-pair rows)' % (L, _lib.MAX_L))
        if self.compress:
            raise _lib.ChartLibError('L = %d > %d: compress = True is not supported' % (L, _lib.MAX_L))

    def _check_hard(self, hooks):
        """What a hard chart does not take: every refusal before any launch."""
        if self.vision_language:
            raise NotImplementedError('hard=True: cliora_amd.cliora.DioraMLP is not supported (the attention re-normalises an inside cell '
                                      'between its aggregate and the scoring); a hard chart is text-only cliora_amd.diora.DioraMLP')
        if self.plan_arch != 0:
            raise NotImplementedError('hard=True: DioraTreeLSTM is not supported; a hard chart is text-only cliora_amd.diora.DioraMLP')
        if self.compress:
            raise NotImplementedError('hard=True: compress = True is not supported')
        if hooks:
            raise NotImplementedError('hard=True: inside_hook / outside_hook overrides get no per-pair states (a hard level composes one '
                                      'pair per cell)')
        if self.__dict__.get('_ragged') is not None or self.__dict__.get('_ragged_train') is not None:
            raise NotImplementedError('hard=True: a padded chart of mixed lengths is not supported')

    def _check_padded(self, hooks):
        """What no padded chart of mixed lengths takes, for inference or with a backward."""
        if hooks:
            raise NotImplementedError('inside_hook / outside_hook overrides get no per-pair states from a padded chart of mixed lengths')
        if self.compress:
            raise NotImplementedError('compress = True is not supported on a padded chart of mixed lengths')

    def _check_ragged(self, needs_grad, hooks):
        if needs_grad or self.training:
            raise _lib.ChartLibError('a padded chart of mixed lengths is inference only: call it in eval mode under torch.no_grad()')
        self._check_padded(hooks)

    def _check_ragged_train(self, L, hooks):
        """A padded chart of mixed lengths with a backward: every refusal before any launch."""
        if self.plan_arch != 0:
            raise NotImplementedError('training through a padded chart of mixed lengths is text-only DIORA (cliora_amd.diora.DioraMLP) '
                                      'or CLIORA (cliora_amd.cliora.DioraMLP), not the TreeLSTM')
        if L > _lib.MAX_L:
            raise _lib.ChartLibError('L = %d > %d: a padded chart of mixed lengths trains through at most %d words' % (L, _lib.MAX_L, _lib.MAX_L))
        self._check_padded(hooks)

    def _run_ragged_train(self, plan, holder, x_span, obj_embed_span, params, ragged):
        """_run_chart through RaggedChartFunction (with regions, DESIGN.md section 23: the mask's rows are those of the PADDED chart);
        the status word is left in _ragged_status."""
        flags = int(bool(self.outside)) | (_lib.FWD_HARD_DENSE if holder.selection is not None and self.hard_dense else 0)
        *charts, self.__dict__['_ragged_status'], inside_c = RaggedChartFunction.apply(
            plan, holder, flags, *ragged, x_span, *self._chart_inputs(plan, x_span, obj_embed_span), *params)
        return (*charts, inside_c, None)

    def _hook_overridden(self, name):
        return name in self.__dict__ or getattr(type(self), name) is not getattr(DioraBase, name)

    def _param_tensors(self):
        # through the module / parameter registries directly: attribute access on an nn.Module falls back to __getattr__ for every
        # submodule and parameter (always the live objects: nothing is cached)
        mods, pars = self._modules, self._parameters
        ic = mods['inside_compose_func']._modules
        fc, h0, h2 = ic['leaf_fc']._parameters, ic['h_fcs']._modules['0']._parameters, ic['h_fcs']._modules['2']._parameters
        t = dict(leaf_w=fc['weight'], leaf_b=fc['bias'], in_w1=h0['weight'], in_b1=h0['bias'], in_w2=h2['weight'], in_b2=h2['bias'],
                 in_mat=mods['inside_score_func']._parameters['mat'])
        if self.compress:           # diora.py:342-343, 466-467: the outside root is inside_h[root] @ root_mat_out
            t['root_mat'] = pars['root_mat_out']
        else:
            t['root_h'] = pars['root_vector_out_h']
        if not self.share:
            oc = mods['outside_compose_func']._modules['h_fcs']._modules
            o0, o2 = oc['0']._parameters, oc['2']._parameters
            t.update(out_w1=o0['weight'], out_b1=o0['bias'], out_w2=o2['weight'], out_b2=o2['bias'],
                     out_mat=mods['outside_score_func']._parameters['mat'])
        return [t.get(n) for n in _lib.PARAM_FIELDS]

    # ---- what a subclass supplies to forward(): the plan's arch, and the three methods below (with _param_tensors)
    plan_arch = 0

    def _regions(self, obj_embed_span):
        """The plan's R for this module's kind of call; refuses an obj_embed_span it cannot take."""
        if obj_embed_span is not None:
            raise NotImplementedError('text-only DIORA module; use cliora_amd.cliora.DioraMLP with image regions')
        return 0

    def _chart_inputs(self, plan, x_span, obj_embed_span):
        """(obj_span, drop_mask) of this module's kind of chart call, on every route: none here (_regions has refused the regions)."""
        return None, None

    def _run_chart(self, plan, holder, flags, x_span, obj_embed_span, params):
        """The one call that runs the chart -> (inside_h, inside_s, outside_h, outside_s, inside_c, outside_c); a cell state None is
        identically zero (Chart creates it when first read)."""
        return ChartFunction.apply(plan, holder, flags, x_span, *self._chart_inputs(plan, x_span, obj_embed_span), *params) + (None,)

    def _run_ragged(self, plan, holder, x_span, obj_embed_span, params, ragged):
        """_run_chart through cliora_chart_forward_ragged (cliora_amd.ragged); the status word is left in _ragged_status."""
        obj_span, _ = self._chart_inputs(plan, x_span, obj_embed_span)      # eval mode (_check_ragged): no dropout mask
        *charts, self.__dict__['_ragged_status'] = ragged_chart(plan, holder, self.outside, x_span, obj_span, params, *ragged,
                                                                hard_dense=self.hard_dense)
        return (*charts, None)

    def forward(self, x_span, x_word=None, obj_embed_span=None, obj_embed_word=None):
        if self.index is None:
            self.index = Index(cuda=self.is_cuda)
        self.reset()
        R = self._regions(obj_embed_span)
        B, L, D = x_span.shape
        assert D == self.size
        dev_index = x_span.device.index if x_span.is_cuda else -1
        holder = ChartWorkspaces()
        # eval / torch.no_grad: nothing will ask for the backward, so the per-pair state is not written -- unless a hook
        # override wants the per-split tensors (analysis/utils.py:67-95)
        params = self._param_tensors()
        needs_grad = torch.is_grad_enabled() and (x_span.requires_grad or (obj_embed_span is not None and obj_embed_span.requires_grad)
                                                  or any(t is not None and t.requires_grad for t in params))
        hooks = self._hook_overridden('inside_hook') or self._hook_overridden('outside_hook')
        if self.hard:
            self._check_hard(hooks)
        self._check_long(L, needs_grad, hooks)
        plan = _lib.get_plan(B, L, D, self.share, self.normalize, R, dev_index, arch=self.plan_arch)
        flags = int(bool(self.outside)) | (0 if needs_grad else _lib.FWD_NO_BACKWARD) | (_lib.FWD_PAIR_STATES if hooks else 0)
        ragged, ragged_train = self.__dict__.get('_ragged'), self.__dict__.get('_ragged_train')
        hard_slots = self.__dict__.get('_ragged_hard'), self.__dict__.get('_ragged_hard_train')
        if hard_slots != (None, None):     # a hard padded chart: the same two routes, the selection arrays on the holder
            if not self.hard:
                raise NotImplementedError('_ragged_hard / _ragged_hard_train are a hard module\'s slots (hard=False: _ragged / _ragged_train)')
            ragged, ragged_train = hard_slots
            sel = torch.empty((2, B, plan.C), dtype=torch.int32, device=x_span.device)      # every entry is written by the call
            holder.selection = (sel[0], sel[1])
        if ragged is not None:
            self._check_ragged(needs_grad, hooks)
            charts = self._run_ragged(plan, holder, x_span, obj_embed_span, params, ragged)
        elif ragged_train is not None and needs_grad:
            self._check_ragged_train(L, hooks)
            charts = self._run_ragged_train(plan, holder, x_span, obj_embed_span, params, ragged_train)
        elif ragged_train is not None:
            raise _lib.ChartLibError('a padded training chart of mixed lengths needs gradients enabled; cliora_amd.ragged.forward_ragged '
                                     'runs the same batch for inference')
        else:
            if self.hard:          # the selections, -1 where the call writes none (leaves, the outside root, no outside pass)
                sel = torch.full((2, B, plan.C), -1, dtype=torch.int32, device=x_span.device)
                holder.selection = (sel[0], sel[1])
                flags |= _lib.FWD_HARD_DENSE if self.hard_dense else 0
            charts = self._run_chart(plan, holder, flags, x_span, obj_embed_span, params)
        ch = Chart()
        ch.inside_h, ch.inside_s, ch.outside_h, ch.outside_s, ch.inside_c, ch.outside_c = charts      # a zero cell state: on first read (Chart)
        d = self.__dict__
        d['chart'], d['_wss'], d['_plan'], d['selection'] = ch, holder, plan, holder.selection
        if self._hook_overridden('init_with_batch'):      # analysis/utils.py:67-76 wraps it: then it gets the reference's arguments
            self.init_with_batch(ch.inside_h[:, :L], ch.inside_c[:, :L])
        else:
            d['batch_size'], d['length'] = B, L
        if hooks:
            self._serve_hooks(L)
        return None

    # ---- un-aggregated per-split tensors the hooks receive (diora.py:295-334)
    def _level_views(self, entry, ws, level):
        """(scores (rows,), compose outputs (rows, ld)) of one level as fp32 views of the workspace `ws`; entry: cliora_inside_pair_states or
        cliora_outside_pair_states."""
        ps, ph, rows, ldh = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.call(entry, self._plan.handle, _ptr(ws), level, C.byref(ps), C.byref(ph), C.byref(rows), C.byref(ldh))
        wsf = ws.view(torch.float32)
        so, ho = (ps.value - ws.data_ptr()) // 4, (ph.value - ws.data_ptr()) // 4
        n, ld = rows.value, ldh.value
        return wsf[so:so + n], wsf[ho:ho + n * ld].view(n, ld)

    def pair_states(self, level):
        """(h, s) of one inside level: h (B*Lc*N, D) compose outputs, s (B, Lc, N, 1) split scores."""
        plan = self._plan
        hs, ss = [], []
        for ws in self._wss:
            s, h = self._level_views('cliora_inside_pair_states', ws, level)
            ss.append(s.view(plan.B, plan.L - level, level, 1))
            hs.append(h[:, :plan.D])
        if len(hs) == 1:
            return hs[0], ss[0]
        return torch.cat(hs, 0), torch.cat(ss, 0)

    def pair_states_out(self, level):
        """(h, s) of one outside level in the REFERENCE's order (diora.py:364-398): h (B*N*Lc, D) compose outputs,
        s (B, N, Lc, 1) split scores, N = L-level-1 (parent, sibling) splits of the Lc = L-level target cells."""
        plan = self._plan
        L = plan.L
        Lc, N = L - level, L - level - 1
        ii = torch.arange(N).view(N, 1)
        jj = torch.arange(Lc).view(1, Lc).expand(N, Lc)
        nn_ = torch.where(jj < N - ii, L - 2 - ii - level, N - ii - 1)          # our split of the reference's (i, j)
        hs, ss = [], []
        for ws in self._wss:
            s, h = self._level_views('cliora_outside_pair_states', ws, level)
            jd, nd = jj.to(ws.device), nn_.to(ws.device)
            ss.append(s.view(plan.B, Lc, N)[:, jd, nd].unsqueeze(-1))                           # (B, N, Lc, 1)
            hs.append(h.view(plan.B, Lc, N, -1)[:, jd, nd][..., :plan.D].reshape(plan.B * N * Lc, plan.D))
        if len(hs) == 1:
            return hs[0], ss[0]
        return torch.cat(hs, 0), torch.cat(ss, 0)

    def _serve_hooks(self, L):
        """inside_hook / outside_hook overrides get the per-split states the reference passes them (diora.py:331, 398),
        after the native passes have run."""
        if self._hook_overridden('inside_hook'):
            for level in range(1, L):
                h, s = self.pair_states(level)
                self.inside_hook(level, h, torch.zeros_like(h), s)
        if self.outside and self._hook_overridden('outside_hook'):
            for level in range(L - 2, -1, -1):
                h, s = self.pair_states_out(level)
                self.outside_hook(level, h, torch.zeros_like(h), s)

    def cky_spans(self):
        """Constituent spans of the best binary tree per sentence (analysis/cky.py:31-99 decoded on the GPU, cliora_cky_spans): an int32
        array (B, L-1, 2) of (start, end) word positions, children before parents, the root last -- what the reference derives on the
        host with ``get_spans(get_actions(tree))`` (analysis/utils.py:3-49) and scores F1 on (scripts/train.py:184-204).  One
        device-to-host copy, no recursion."""
        plan = self._plan
        if plan.L < 2:                                   # one word: no constituent
            import numpy as np
            return np.zeros((plan.B * len(self._wss), 0, 2), dtype=np.int32)
        return self.cky_spans_device().cpu().numpy()

    def cky_spans_device(self, out=None):
        """cky_spans left on the device: an int32 tensor (B, L-1, 2) on the chart's GPU, written into `out` when given (a contiguous
        int32 tensor of that shape; cliora_amd.evaluate decodes into its batch's output buffer)."""
        q = ChartQuery(self)
        spans = q.spans(out)
        if q.plan.L > 1:
            q.launch('cliora_cky_spans', None, per_sentence(spans))
        return spans

    # ---- the tree of a hard chart: it falls out of the selections, no CKY pass
    def _hard_selection(self):
        if self.__dict__.get('selection') is None:
            raise _lib.ChartLibError('the last forward was not a hard chart (DioraMLP(hard=True), or set .hard): there are no selections')
        return self.selection

    def hard_spans_device(self, out=None, lengths=None):
        """The spans of the tree the hard chart's inside selections spell (cliora_hard_spans), in the layout of cky_spans_device: an
        int32 tensor (B, L-1, 2) on the chart's GPU, written into `out` when given.  lengths (int32 tensor (B,)): the chart is a
        right-padded batch of mixed lengths -- cliora_hard_spans_ragged walks each sentence from its own root, rows beyond its n - 1
        are (-1, -1) -- and the result is (spans, status): status (1,) int32 on the device counts the lengths outside [1, L], which
        the caller must check."""
        sel_in, _ = self._hard_selection()
        plan = self._plan
        spans, _ = span_buffer(self, out)
        with torch.cuda.device(spans.device):
            if lengths is not None:
                lengths = check_lengths(lengths.to(spans.device), plan.B, spans.device)
                status = torch.empty(1, dtype=torch.int32, device=spans.device)
                _lib.call('cliora_hard_spans_ragged', plan.handle, _ptr(sel_in), _ptr(lengths), _ptr(spans) if plan.L > 1 else None,
                          _ptr(status), _stream())
                return spans, status
            if plan.L > 1:
                _lib.call('cliora_hard_spans', plan.handle, _ptr(sel_in), _ptr(spans), _stream())
        return spans

    def hard_spans(self, lengths=None):
        """hard_spans_device as an int32 array (B, L-1, 2): one device-to-host copy.  With lengths (a padded chart of mixed lengths)
        a length outside [1, L] raises."""
        self._hard_selection()
        if lengths is not None:
            spans, status = host_copy(*self.hard_spans_device(lengths=lengths))
            if status.any():
                raise _lib.ChartLibError('cliora_hard_spans_ragged rejected %d sentence length(s)' % int(status.sum()))
            return spans
        if self._plan.L < 2:
            import numpy as np
            return np.zeros((self._plan.B, 0, 2), dtype=np.int32)
        return self.hard_spans_device().cpu().numpy()

    def hard_tree(self, lengths=None):
        """The hard chart's tree per sentence as nested tuples of word positions, as cky() returns the Viterbi tree.  With lengths:
        of each sentence's own triangle of a padded chart."""
        if lengths is None:
            return self.trees_from_spans(self.hard_spans())
        spans = self.hard_spans(lengths)
        return [self.trees_from_spans(spans[b:b + 1, :int(n) - 1])[0] for b, n in enumerate(lengths.tolist())]

    @property
    def inside_tree(self):
        """What the reference's TreesFromDiora.parse_batch reads (analysis/diora_tree.py:47-64): inside_tree[(b, 0)][(L-1, 0)] is the
        list of the (level, pos) cells of sentence b's tree above the leaves."""
        from .hard import inside_tree_from_spans
        return inside_tree_from_spans(self.hard_spans())

    @staticmethod
    def trees_from_spans(spans):
        """Nested tuples of word positions (what ``ParsePredictor.parse_batch`` returns, e.g. ``(0, ((1, 2), 3))``) from the
        children-before-parents span lists of cky_spans: a stack per sentence, no recursion."""
        trees = []
        for sent in spans.tolist():
            if not sent:
                trees.append(0)
                continue
            stack = []                                   # (start, end, tree) of the finished constituents
            for s, e in sent:
                if stack and stack[-1][1] == e and stack[-1][0] > s:
                    rs, _, right = stack.pop()
                else:
                    rs, right = e, e                     # the right child is the word e itself
                if stack and stack[-1][0] == s and stack[-1][1] == rs - 1:
                    left = stack.pop()[2]
                else:
                    left = s
                stack.append((s, e, (left, right)))
            trees.append(stack[-1][2])
        return trees

    def cky(self):
        """Best binary tree per sentence (analysis/cky.py:31-99) decoded on the GPU.

        Returns nested tuples of word positions, e.g. ``(0, ((1, 2), 3))`` -- a view of the device-built span lists (cky_spans)."""
        return self.trees_from_spans(self.cky_spans())

    def span_posteriors(self, lengths=None, mbr=False):
        """Span posteriors, log-partition and (mbr=True) the minimum-Bayes-risk tree of the last forward: the sum-product pass over
        the potentials cky() maximises (cliora_amd.posterior.span_posteriors).  Device tensors."""
        from . import posterior
        return posterior.span_posteriors(self, lengths=lengths, mbr=mbr)

    def mbr_spans_device(self, out=None):
        """Spans of the MBR tree -- the tree with the most expected correct brackets under the span posteriors -- in the layout of
        cky_spans_device: an int32 tensor (B, L-1, 2) on the chart's GPU, written into `out` when given."""
        from . import posterior
        return posterior.span_posteriors(self, mbr=True, out=out).spans

    def mbr(self):
        """MBR tree per sentence as nested tuples of word positions, as cky() returns the Viterbi tree."""
        if self._plan.L < 2:
            return [0] * (self._plan.B * len(self._wss))
        return self.trees_from_spans(self.mbr_spans_device().cpu().numpy())

    def kbest_spans_device(self, k, lengths=None):
        """The k best trees of the last forward, rank 0 the tree of cky() (cliora_amd.kbest.kbest_spans):
        -> KBest(spans (B, k, L-1, 2), scores (B, k), count (B,), status).  Device tensors."""
        from . import kbest
        return kbest.kbest_spans(self, k, lengths=lengths)

    def kbest(self, k):
        """Per sentence the list of its (tree, score), best first: min(k, Catalan(L - 1)) nested tuples of word positions as cky()
        returns them, each with the sum of its potentials (<= 0; exp(score - log_z) is the tree's posterior mass)."""
        kb = self.kbest_spans_device(k)
        spans, scores, count = host_copy(kb.spans, kb.scores, kb.count)
        return [list(zip(self.trees_from_spans(spans[b, :count[b]]), scores[b, :count[b]].tolist())) for b in range(len(count))]

    def sample_spans_device(self, S, seed, lengths=None, ids=None, first_sample=0, beta=1.0):
        """S trees per sentence drawn from the posterior over parses of the last forward, the distribution whose mode is cky()
        (cliora_amd.sample.sample_spans): -> TreeSamples(spans (B, S, L-1, 2), log_prob (B, S), log_z (B,),
        status).  Device tensors."""
        from . import sample
        return sample.sample_spans(self, S, seed, lengths=lengths, ids=ids, first_sample=first_sample, beta=beta)

    def sample_trees(self, S, seed, beta=1.0):
        """Per sentence the list of its S sampled (tree, log_prob): nested tuples of word positions as cky() returns them, each with
        the log of its probability under the distribution it was drawn from.  One device-to-host copy."""
        ts = self.sample_spans_device(S, seed, beta=beta)
        spans, log_prob = host_copy(ts.spans, ts.log_prob)
        return [list(zip(self.trees_from_spans(spans[b]), log_prob[b].tolist())) for b in range(spans.shape[0])]

    def cky_constrained(self, required, forbidden=None):
        """Best binary tree per sentence among those that keep every span of required[b] as a constituent and none of forbidden[b]
        (per-sentence lists of (start, end), inclusive word positions; cliora_amd.constrained): nested tuples
        as cky() returns them, None for a sentence no tree qualifies for.  One device-to-host copy."""
        from . import constrained
        cp = constrained.constrained_parse(self, constrained.pack_brackets(required, forbidden))
        spans, feasible, _, rejected = constrained.host_results(cp)
        constrained.refuse_rejected(rejected)
        return [self.trees_from_spans(spans[b:b + 1])[0] if feasible[b] else None for b in range(len(feasible))]

    def bracket_log_prob(self, required, forbidden=None):
        """Per sentence the log of the probability, under the posterior over parses of the last forward, that every span of
        required[b] is a constituent and none of forbidden[b] is -- jointly, which the per-span marginals cannot give: a list of
        floats <= 0, -inf where no tree qualifies.  One device-to-host copy."""
        from . import constrained
        cp = constrained.constrained_parse(self, constrained.pack_brackets(required, forbidden))
        log_prob, status = host_copy(cp.log_prob, cp.status)
        constrained.refuse_rejected(int(status.sum()))
        return log_prob.tolist()

    def kbest_constrained(self, k, required, forbidden=None):
        """kbest() among the trees that keep every span of required[b] as a constituent and none of forbidden[b] (per-sentence lists
        of (start, end) as cky_constrained takes them; cliora_amd.constrained.constrained_kbest): per sentence
        the list of its (tree, score), best first -- min(k, the number of qualifying trees) of them, [] where none qualifies; rank 0
        is cky_constrained's tree.  One device-to-host copy."""
        from . import constrained
        kb = constrained.constrained_kbest(self, constrained.pack_brackets(required, forbidden), k)
        spans, scores, count, status = host_copy(kb.spans, kb.scores, kb.count, kb.status)
        constrained.refuse_rejected(int(status.sum()), 'cliora_kbest_spans_constrained')
        return [list(zip(self.trees_from_spans(spans[b, :count[b]]), scores[b, :count[b]].tolist())) for b in range(len(count))]

    def sample_trees_constrained(self, S, seed, required, forbidden=None, beta=1.0):
        """sample_trees() from the posterior over parses given the brackets (cliora_amd.constrained.constrained_samples, DESIGN.md
        section 25): per sentence the list of its S sampled (tree, log_prob), every tree keeping the brackets and log_prob the log of
        its probability among the trees that do; [] where no tree qualifies.  One device-to-host copy."""
        from . import constrained
        ts = constrained.constrained_samples(self, constrained.pack_brackets(required, forbidden), S, seed, beta=beta)
        spans, log_prob, feasible, status = host_copy(ts.spans, ts.log_prob, ts.feasible, ts.status)
        constrained.refuse_rejected(int(status.sum()), 'cliora_sample_trees_constrained')
        return [list(zip(self.trees_from_spans(spans[b]), log_prob[b].tolist())) if feasible[b] else [] for b in range(len(feasible))]

    def _check_spans(self, required, forbidden):
        L = self._plan.L
        for lst in list(required) + list(forbidden or ()):
            for s, e in lst:
                if not 0 <= int(s) <= int(e) < L:
                    raise ValueError('bracket (%d, %d) is not 0 <= start <= end < %d' % (s, e, L))

    def bracket_nll(self, required, forbidden=None, reduction='mean'):
        """The loss -log_prob of the brackets, in the autograd graph of the last forward (cliora_amd.structured.bracket_nll; DESIGN.md
        section 20): required / forbidden as cky_constrained takes them -- per-sentence lists of (start, end); a gold tree is its inner
        brackets.  The mean (or 'sum') over the sentences some tree qualifies for.  A span outside its sentence raises here, on the
        host; nothing is synchronised."""
        from . import constrained, structured
        self._check_spans(required, forbidden)
        return structured.bracket_nll(self, constrained.pack_brackets(required, forbidden), reduction=reduction)

    def bracket_hinge(self, required, forbidden=None, margin=1.0, penalty=float('inf'), reduction='mean'):
        """The max-margin loss of the brackets, in the autograd graph of the last forward (cliora_amd.structured.bracket_hinge;
        DESIGN.md section 30): the score of the best cost-augmented tree minus that of the best tree that respects the brackets.
        required / forbidden as bracket_nll takes them.  margin > 0, penalty inf: structured hinge; margin 0: perceptron; a finite
        penalty: ramp, which takes crossing brackets too.  A span outside its sentence raises here, on the host; nothing is
        synchronised."""
        from . import constrained, structured
        self._check_spans(required, forbidden)
        return structured.bracket_hinge(self, constrained.pack_brackets(required, forbidden), margin=margin, penalty=penalty,
                                        reduction=reduction)

    def tree_objective(self, cost=None):
        """(risk, entropy) of the distribution over parses of the last forward, two (B,) tensors in its autograd graph
        (cliora_amd.structured.tree_objective): the expected value of the per-cell cost -- fp32 (B, C) in the cell
        order of inside_s, ``structured.span_costs``; None = 0 -- and the entropy.  Nothing is synchronised."""
        from . import structured
        return structured.tree_objective(self, cost)

    def parse_entropy(self, reduction='mean'):
        """The entropy of the distribution over parses, its mean (or 'sum') over the batch: a 0-d tensor in the graph."""
        from . import structured
        return structured.parse_entropy(self, reduction=reduction)

    def expected_cost(self, cost, reduction='mean'):
        """The expected cost of the parse (cost as tree_objective takes it), its mean (or 'sum') over the batch: a 0-d tensor in the
        graph.  With ``structured.span_costs`` of the annotated phrases: minus the expected number of them recovered."""
        from . import structured
        return structured.expected_cost(self, cost, reduction=reduction)

    def parse_kl(self, teacher):
        """(kl, cross_entropy) of this chart's distribution over parses against the one of `teacher` -- any chart module after a
        forward on the same sentences (same B and L) --, two (B,) tensors in the autograd graph of the last forward
        (cliora_amd.structured.parse_kl): KL(teacher || self) and -sum_T p_teacher(T) log p_self(T).  A teacher
        whose forward kept backward state gets its gradient too.  Nothing is synchronised."""
        from . import structured
        return structured.parse_kl(teacher, self)

    def parse_divergence(self, teacher, direction='forward', reduction='mean'):
        """The divergence from `teacher`'s distribution over parses, its mean (or 'sum') over the batch: a 0-d tensor in the graph.
        direction 'forward': KL(teacher || self); 'reverse': KL(self || teacher); 'symmetric': their sum."""
        from . import structured
        return structured.parse_divergence(teacher, self, direction=direction, reduction=reduction)


class DioraMLP(DioraBase):
    def __init__(self, *args, hard=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.hard = bool(hard)

    def init_parameters(self):
        self.inside_score_func = Bilinear(self.size)
        self.inside_compose_func = ComposeMLP(self.size, leaf=True)
        if self.share:
            self.outside_score_func = self.inside_score_func
            self.outside_compose_func = self.inside_compose_func
        else:
            self.outside_score_func = Bilinear(self.size)
            self.outside_compose_func = ComposeMLP(self.size)
        if self.compress:
            self.root_mat_out = nn.Parameter(torch.empty(self.size, self.size))
        else:
            self.root_vector_out_h = nn.Parameter(torch.empty(self.size))
        self.root_vector_out_c = None
