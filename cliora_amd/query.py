"""After-forward chart queries: the one launcher of their C entries, and the one host walk of their restatements.

Every question asked of a chart after its forward -- the best tree of a padded chart, the posteriors, the K best trees, samples, the
constrained forms, the bracket gradient, the expectation, the margin loss, the divergence from a second chart -- is one C entry of include/cliora_chart.h that starts
(plan, forward workspace, ...) and ends (..., status, stream), called once per forward workspace of the chart module on that
workspace's B sentences.  ``ChartQuery`` is what such a call reads of the module, the checks of the per-sentence arguments and the
loop over the workspaces; a query is its checks, its output allocations, one ``launch`` and its result tuple.

``walk`` is the traversal every decode kernel ends with -- the node's decision, the whole left subtree, the whole right subtree, then
the node emitted -- which the numpy restatements of those kernels (the yardsticks of the GPU tests) share.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import ptr_or_null as _p, stream as _stream


class per_sentence(object):
    """A per-sentence tensor among a launch's arguments: each workspace gets its own B rows (NULL for None and for an empty tensor)."""
    __slots__ = ('t',)

    def __init__(self, t):
        self.t = t

    def at(self, i, sl):
        return _p(self.t[sl]) if self.t is not None else None


class per_workspace(object):
    """A buffer of `count` elements per workspace, back to back: workspace i gets the address of element i * count."""
    __slots__ = ('t', 'count')

    def __init__(self, t, count):
        self.t, self.count = t, count

    def at(self, i, sl):
        return C.c_void_p(self.t.data_ptr() + self.t.element_size() * i * self.count)


class workspace_of(object):
    """The forward workspace of a SECOND chart among a launch's arguments (``ChartQuery.second``): workspace i of its holder."""
    __slots__ = ('q',)

    def __init__(self, q):
        self.q = q

    def at(self, i, sl):
        return C.c_void_p(self.q.parts[i][0].data_ptr())


class ChartQuery(object):
    """What an after-forward query reads of a chart module (anything that carries `_plan` and `_wss`): plan, parts -- per forward
    workspace (workspace, the slice of its B sentences in the module's outputs) --, nws, rows = B * nws, dev, and holder, the module's
    `_wss` itself (a ``diora.ChartWorkspaces`` has the `lengths` of a padded training chart)."""
    __slots__ = ('plan', 'holder', 'parts', 'nws', 'rows', 'dev')

    def __init__(self, diora):
        plan, wss = diora._plan, diora._wss
        B = plan.B
        self.plan, self.holder, self.nws, self.rows, self.dev = plan, wss, len(wss), B * len(wss), wss[0].device
        self.parts = [(ws, slice(i * B, (i + 1) * B)) for i, ws in enumerate(wss)]

    def second(self, other, who):
        """The arguments that name a second chart in this query's launch: -> (its plan handle, ``workspace_of`` it).  The two charts
        must agree in B, L, the number of workspaces and the device -- then their slices agree too; refused before any device call."""
        a, b = self.plan, other.plan
        if (a.B, a.L, self.nws, self.dev) != (b.B, b.L, other.nws, other.dev):
            raise ValueError('%s: the two charts differ: B %d L %d, %d workspace(s) on %s against B %d L %d, %d workspace(s) on %s'
                             % (who, a.B, a.L, self.nws, self.dev, b.B, b.L, other.nws, other.dev))
        return b.handle, workspace_of(other)

    def lengths_or_holders(self, lengths):
        """The default of the structured queries: the lengths of a padded training chart of mixed lengths, each sentence's own triangle."""
        return getattr(self.holder, 'lengths', None) if lengths is None else lengths

    # ---- the checks of the per-sentence arguments, each raised before any device call
    def check_int32(self, name, t):
        """lengths / ids: int32, one per sentence of the chart."""
        if t is not None and (t.dtype != torch.int32 or t.numel() != self.rows):
            raise ValueError('%s must be int32, one per sentence of the chart (%d)' % (name, self.rows))

    def check_brackets(self, brackets):
        """-> M, the bracket rows per sentence (0 for None)."""
        if brackets is None:
            return 0
        if brackets.dtype != torch.int32 or brackets.dim() != 3 or brackets.shape[0] != self.rows or brackets.shape[2] != 3:
            raise ValueError('brackets must be int32 (%d, M, 3)' % self.rows)
        return int(brackets.shape[1])                          # a bad M is the library's to refuse, with its message

    def check_weights(self, name, w):
        if w is not None and w.numel() != self.rows:
            raise ValueError('%s must hold one value per sentence of the chart (%d)' % (name, self.rows))

    def check_cost(self, cost):
        if cost is not None and (cost.dim() != 2 or tuple(cost.shape) != (self.rows, self.plan.C)):
            raise ValueError('cost must be (%d, %d): one value per cell of the chart' % (self.rows, self.plan.C))

    def spans(self, out=None):
        """The span output of a decode: an int32 tensor (rows, L-1, 2) on the chart's device -- `out`, checked, when given, else a
        fresh one."""
        L, shape = self.plan.L, (self.rows, self.plan.L - 1, 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.dev)
        elif out.shape != shape or out.dtype != torch.int32 or not out.is_contiguous() or out.device != self.dev:
            raise ValueError('out must be a contiguous int32 tensor (%d, %d, 2) on %s' % (shape[0], L - 1, self.dev))
        return out

    # ---- the arguments on the chart's device, the outputs
    def moved(self, t):
        return t.to(self.dev).contiguous() if t is not None else None

    def moved_weights(self, w):
        return w.to(self.dev).contiguous().float().reshape(-1) if w is not None else None

    def default_ids(self, ids):
        """The samplers' sentence ids on the device: the caller's, else the row in the chart over every workspace (one workspace: NULL,
        which is the library's word for the same)."""
        if ids is None:
            return torch.arange(self.rows, dtype=torch.int32, device=self.dev) if self.nws > 1 else None
        return self.moved(ids)

    def empty(self, dtype, *tail):
        """An uninitialised output of one row per sentence of the chart."""
        return torch.empty((self.rows,) + tail, dtype=dtype, device=self.dev)

    def status(self, zeroed=True):
        """One status word per workspace.  (The entries differ in whether their caller zeroes it: each keeps what it did.)"""
        return (torch.zeros if zeroed else torch.empty)(self.nws, dtype=torch.int32, device=self.dev)

    def split_buffer(self):
        """The d_split output of a structured query: cliora_plan_split_score_count fp32 per workspace, back to back.
        -> (the launch's argument, the (count * nws,) view the caller returns)."""
        count = int(_lib.fn('cliora_plan_split_score_count')(self.plan.handle))
        buf = torch.empty(max(count * self.nws, 1), dtype=torch.float32, device=self.dev)    # (one word: no row, but the library wants an address)
        return per_workspace(buf, count), buf[:count * self.nws]

    def launch(self, entry, *args, status=None):
        """The loop over the workspaces: `entry`(plan, workspace i, *args, [status word i,] stream) under the chart's device.  args,
        in the entry's ABI order: ``per_sentence(t)`` a per-sentence tensor, ``per_workspace(t, count)``, ``workspace_of(q)`` (a second
        chart: ``second``), a tensor as it is (scratch: NULL for None and for an empty one), anything else a plain scalar."""
        with torch.cuda.device(self.dev):
            for i, (ws, sl) in enumerate(self.parts):
                call = [a.at(i, sl) if isinstance(a, (per_sentence, per_workspace, workspace_of)) else _p(a) if torch.is_tensor(a) else a for a in args]
                if status is not None:
                    call.append(C.c_void_p(status[i:i + 1].data_ptr()))
                _lib.call(entry, self.plan.handle, C.c_void_p(ws.data_ptr()), *call, _stream())


def workspace_slices(diora):
    """Per forward workspace of a chart module: (workspace, the slice of its B sentences in the module's outputs)."""
    return ChartQuery(diora).parts


def span_buffer(diora, out=None):
    """The span output of a decode over a chart module's workspaces (``ChartQuery.spans``).  -> (spans, workspace_slices(diora))."""
    q = ChartQuery(diora)
    return q.spans(out), q.parts


def host_copy(*tensors):
    """The int32 / fp32 tensors of one device as numpy arrays of their own dtypes and shapes, after ONE device-to-host copy: they
    travel concatenated, as 32-bit words."""
    host = torch.cat([t.reshape(-1).view(torch.int32) for t in tensors]).cpu().numpy()
    ends = [0]
    for t in tensors:
        ends.append(ends[-1] + t.numel())
    return [host[a:b].view(str(t.dtype)[len('torch.'):]).reshape(t.shape) for t, a, b in zip(tensors, ends, ends[1:])]


# ---- the restatements' side -----------------------------------------------------------------------------------------------------------
def walk(n, choose, state=None):
    """The kernels' walk over a sentence of n words from its root cell (n - 1, 0), with an explicit stack: at a cell above the leaves
    ``choose(level, pos, state) -> (split, left state, right state)`` is called, ONCE, before anything below the cell -- so the calls
    come in pre-order, left subtree first: the order in which a sampler draws and sums its log-probability --, then the whole left
    subtree (split, pos), the whole right subtree (level - split - 1, pos + split + 1), then the cell is emitted.
    -> [(start, end, split, state)], children before parents, the root last; [] for one word."""
    out, stack = [], [(n - 1, 0, 0, None, state)] if n > 1 else []
    while stack:
        level, pos, phase, k, st = stack.pop()
        if level == 0:
            continue
        if phase == 0:
            k, left, right = choose(level, pos, st)
            k = int(k)
            stack += [(level, pos, 2, k, st), (level - k - 1, pos + k + 1, 0, None, right), (k, pos, 0, None, left)]
        else:
            out.append((pos, pos + level, k, st))
    return out


def walk_spans(n, split_of):
    """``walk`` over plain backpointers split_of(level, pos) -> [(start, end)], children before parents."""
    return [row[:2] for row in walk(n, lambda level, pos, _: (split_of(level, pos), None, None))]


def sentences_of(pair_s, lengths, L=None, brackets=False):
    """What a restatement starts with: -> (lengths as ints, the chart's length -- `L`, else inferred from level 1 of `pair_s`, or the
    one word there is --[, the brackets as an array, (B, 0, 3) for None])."""
    lengths = [int(x) for x in lengths]
    if L is None:
        L = np.asarray(pair_s[1]).shape[1] + 1 if max(lengths) > 1 else max(lengths)
    if brackets is False:
        return lengths, L
    return lengths, L, np.zeros((len(lengths), 0, 3), dtype=np.int32) if brackets is None else np.asarray(brackets)
