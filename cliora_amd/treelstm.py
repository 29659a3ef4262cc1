"""``DioraTreeLSTM`` on the MI355X chart engine (BASELINE config 5).

PARITY UNPINNED.  This tree of the reference cannot build a TreeLSTM model: ``build_net`` raises
for any ``--arch`` but ``mlp`` (cliora/net/trainer.py:518-526) and the composition exists only as
commented-out text (cliora/net/vg.py:28-76).  What is implemented is that text on the
``DioraBase`` skeleton (cliora/net/diora.py:205-450) the way the original DIORA wires it: inside and
outside functions shared or (``share=False``, diora.py:459-464) a second compose / score module for the
outside pass, ``constant`` = 1 inside and 0 outside (diora.py:174), and ``root_vector_out_c`` a
parameter (the hint at diora.py:470-471).  The oracle's restatement is
checked against the commented text executed in memory (tests/golden/treelstm_recon.npz).

Parameters: ``inside_compose_func.W (3D,D)``, ``.U (5D,2D)``, ``.B (5D)``, ``inside_score_func.mat``,
``root_vector_out_h``, ``root_vector_out_c``; ``outside_*`` alias the inside modules, or with ``share=False`` are
``outside_compose_func.{U, B}`` and ``outside_score_func.mat`` of their own.
"""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import ptr
from .diora import DioraBase, Bilinear, _grad_out, chart_buffers


class TreeLSTM(nn.Module):
    def __init__(self, size, ninput=2, leaf=False):
        super().__init__()
        self.size, self.ninput = size, ninput
        if leaf:
            self.W = nn.Parameter(torch.empty(3 * size, size))
        self.U = nn.Parameter(torch.empty(5 * size, ninput * size))
        self.B = nn.Parameter(torch.empty(5 * size))


class LSTMChartFunction(torch.autograd.Function):
    """cliora_lstm_forward / cliora_lstm_backward; six chart outputs (h, c, s for inside and outside)."""

    NAMES = ('lstm_w', 'lstm_u', 'lstm_b', 'in_mat', 'root_h', 'root_c', 'lstm_u_out', 'lstm_b_out', 'out_mat')

    @staticmethod
    def forward(ctx, plan, holder, run_outside, x_span, *params):
        if not x_span.is_cuda:
            raise _lib.ChartLibError('the chart path runs on the GPU only (got a CPU tensor)')
        D = plan.D
        x_span = x_span.contiguous().float()
        ptens = {n: p.detach().contiguous() for n, p in zip(LSTMChartFunction.NAMES, params) if p is not None}
        with _lib.device_guard(x_span):
            outs, ws, nbytes = chart_buffers(plan, x_span.device, 0, D, D, 1, D, D, 1)      # the per-split rows are part of fwd_bytes
            pst = _lib.param_struct(ptens)
            _lib.call('cliora_lstm_forward', plan.handle, C.byref(pst), ptr(x_span), *map(ptr, outs), ptr(ws), nbytes, int(run_outside),
                      _lib.stream())
        ctx.plan, ctx.run_outside, ctx.ws, ctx.ptens = plan, int(run_outside) & 1, ws, ptens
        ctx.save_for_backward(x_span, *outs)
        ctx.set_materialize_grads(False)
        holder.clear()
        holder.append(ws)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *cots):
        plan, saved = ctx.plan, ctx.saved_tensors
        x_span = saved[0]
        with _lib.device_guard(x_span):
            cots = [g.contiguous().float() if g is not None else None for g in cots]
            grads = {n: _grad_out(t) for n, t in ctx.ptens.items()}
            d_x = torch.empty_like(x_span)
            wsb = torch.empty(plan.bwd_bytes, device=x_span.device, dtype=torch.uint8)
            pst, gst = _lib.param_struct(ctx.ptens), _lib.param_struct(grads)
            _lib.call('cliora_lstm_backward', plan.handle, C.byref(pst), *map(ptr, saved), *map(ptr, cots), ptr(ctx.ws), plan.fwd_bytes,
                      ptr(wsb), plan.bwd_bytes, ptr(d_x), C.byref(gst), ctx.run_outside, _lib.stream())
        return (None, None, None, d_x) + tuple(grads.get(n) for n in LSTMChartFunction.NAMES)


class DioraTreeLSTM(DioraBase):
    def init_parameters(self):
        if self.compress:
            raise NotImplementedError('DioraTreeLSTM with compress=True is not built (the reference never enables compress: trainer.py:552)')
        self.inside_score_func = Bilinear(self.size)
        self.inside_compose_func = TreeLSTM(self.size, leaf=True)
        if self.share:
            self.outside_score_func = self.inside_score_func
            self.outside_compose_func = self.inside_compose_func
        else:                       # diora.py:462-464
            self.outside_score_func = Bilinear(self.size)
            self.outside_compose_func = TreeLSTM(self.size)
        self.root_vector_out_h = nn.Parameter(torch.empty(self.size))
        self.root_vector_out_c = nn.Parameter(torch.empty(self.size))

    plan_arch = 1

    def _check_long(self, L, needs_grad, hooks):
        pass            # a TreeLSTM plan refuses L > 64 itself (_lib.Plan)

    def _regions(self, obj_embed_span):
        if obj_embed_span is not None:
            raise NotImplementedError('DioraTreeLSTM is text-only')
        return 0

    def _param_tensors(self):
        cf, of = self.inside_compose_func, self.outside_compose_func
        outer = (None, None, None) if self.share else (of.U, of.B, self.outside_score_func.mat)
        return (cf.W, cf.U, cf.B, self.inside_score_func.mat, self.root_vector_out_h, self.root_vector_out_c) + outer

    def _run_chart(self, plan, holder, flags, x_span, obj_embed_span, params):
        # eval / torch.no_grad without a hook override: the per-split rows h_n, c_n are not written (flag bits of cliora_chart_forward).
        # hooks: per-split h (the pair rows the backward keeps anyway) and scores, in the reference's layout and order
        # (diora.py:331, 398); the per-split cell states are not kept: c is passed as zeros, as for DioraMLP
        ih, ic, is_, oh, oc, os_ = LSTMChartFunction.apply(plan, holder, flags, x_span, *params)
        return ih, is_, oh, os_, ic, oc

    def _run_ragged(self, plan, holder, x_span, obj_embed_span, params, ragged):
        raise NotImplementedError('DioraTreeLSTM has no padded chart of mixed lengths')
