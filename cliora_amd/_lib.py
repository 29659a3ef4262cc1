"""ctypes binding of include/cliora_chart.h (the C-ABI shared library).

The product path has NO CPU fallback: if the HIP library is missing or a call
fails, this raises.  Build it with ``python -m cliora_amd.build`` (or
``__graft_entry__.build()``).
"""
import collections
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CLIORA_CHART_LIB') or os.path.join(HERE, 'libcliora_chart.so')   # override: kernel experiments only

NORM = {'none': 0, 'unit': 1}
MAX_L = 64               # csrc/plan.hpp CLIORA_MAX_L: the longest sentence of anything with a backward, of TreeLSTM / compress plans, of the ragged entries that take the root-level mask as one word
MAX_L_FWD = 128          # csrc/plan.hpp CLIORA_MAX_L_FWD: the longest sentence of a forward-only ("long") DioraMLP / CLIORA plan
FWD_NO_BACKWARD = 2      # include/cliora_chart.h: flag bits of cliora_chart_forward's run_outside word
FWD_PAIR_STATES = 4
FWD_HARD_DENSE = 16      # cliora_chart_forward_hard only: the one-hot weights through the dense compose kernels (cross-check / baseline)
KCLASS = {'compose_fwd': 0, 'compose_bwd': 1, 'wgrad': 2}

PARAM_FIELDS = ('leaf_w', 'leaf_b', 'in_w1', 'in_b1', 'in_w2', 'in_b2', 'in_mat',
                'out_w1', 'out_b1', 'out_w2', 'out_b2', 'out_mat', 'root_h',
                'lstm_w', 'lstm_u', 'lstm_b', 'root_c', 'lstm_u_out', 'lstm_b_out', 'root_mat')


class Params(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PARAM_FIELDS]


class ChartLibError(RuntimeError):
    pass


vp, i32, i64, u64, sz, f32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_size_t, C.c_float
pp, pvp, psz = C.POINTER(Params), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)

# The C ABI of include/cliora_chart.h as data: symbol -> (result type, argument types).  lib() applies it to every symbol the loaded
# library has; fn() refuses an absent one.  tests/test_abi_table.py holds the arities against the header's prototypes.
ABI = {
    'cliora_plan_create': (i32, [i32] * 6 + [pvp]),
    'cliora_plan_create_ex': (i32, [i32] * 7 + [pvp]),
    'cliora_plan_destroy': (None, [vp]),
    'cliora_plan_fwd_workspace_bytes': (sz, [vp]),
    'cliora_plan_bwd_workspace_bytes': (sz, [vp]),
    'cliora_plan_pair_states_bytes': (sz, [vp]),
    'cliora_plan_device_bytes': (sz, [vp]),
    'cliora_plan_fwd_offset': (sz, [vp, C.c_char_p]),
    'cliora_plan_table': (i32, [vp, C.c_char_p, C.POINTER(C.POINTER(C.c_int32)), psz]),
    'cliora_chart_forward': (i32, [vp, pp] + [vp] * 8 + [vp, sz, i32, vp]),
    'cliora_chart_forward_hard': (i32, [vp, pp] + [vp] * 7 + [vp, sz, i32, vp]),
    'cliora_hard_spans': (i32, [vp, vp, vp, vp]),
    'cliora_chart_forward_ragged_hard': (i32, [vp, pp] + [vp] * 7 + [vp, sz, i32, vp, vp, vp, vp]),
    'cliora_hard_spans_ragged': (i32, [vp] * 6),
    'cliora_chart_backward': (i32, [vp, pp] + [vp] * 11 + [vp, sz, vp, sz, vp, vp, pp, i32, vp]),
    'cliora_chart_backward_split': (i32, [vp, pp] + [vp] * 12 + [vp, sz, vp, sz, vp, vp, pp, i32, vp]),
    'cliora_chart_forward_ragged': (i32, [vp, pp] + [vp] * 8 + [vp, sz, i32, vp, u64, vp, vp]),
    'cliora_chart_forward_ragged_wide': (i32, [vp, pp] + [vp] * 8 + [vp, sz, i32, vp, vp, vp, vp]),
    'cliora_chart_forward_ragged_train': (i32, [vp, pp] + [vp] * 8 + [vp, sz, i32, vp, u64, vp, vp]),
    'cliora_chart_backward_ragged': (i32, [vp, pp] + [vp] * 12 + [vp, sz, vp, sz, vp, vp, pp, i32, vp, u64] + [vp] * 4 + [vp]),
    'cliora_chart_forward_ragged_train_vl': (i32, [vp, pp] + [vp] * 8 + [vp, sz, i32, vp, u64, vp, vp]),
    'cliora_chart_backward_ragged_vl': (i32, [vp, pp] + [vp] * 12 + [vp, sz, vp, sz, vp, vp, pp, i32, vp, u64] + [vp] * 4 + [vp]),
    'cliora_lstm_forward': (i32, [vp, pp] + [vp] * 7 + [vp, sz, i32, vp]),
    'cliora_lstm_backward': (i32, [vp, pp] + [vp] * 13 + [vp, sz, vp, sz, vp, pp, i32, vp]),
    'cliora_inside_pair_states': (i32, [vp, vp, i32, pvp, pvp, psz, psz]),
    'cliora_outside_pair_states': (i32, [vp, vp, i32, pvp, pvp, psz, psz]),
    'cliora_plan_vl_workspace_bytes': (sz, [vp]),
    'cliora_vl_scores_forward': (i32, [vp] * 6 + [i32, vp, vp, vp, sz, vp]),
    'cliora_vl_scores_backward': (i32, [vp] * 6 + [i32] + [vp] * 6 + [vp, sz, vp]),
    'cliora_vl_scores_max_forward': (i32, [vp] * 4 + [vp, vp, vp, sz, vp]),
    'cliora_vl_scores_max_backward': (i32, [vp] * 4 + [vp, vp, vp, vp, vp, sz, vp]),
    'cliora_contrastive_workspace_bytes': (sz, [i32, i32]),
    'cliora_contrastive_loss': (i32, [i32, i32, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp, sz, vp]),
    'cliora_contrastive_loss_ragged': (i32, [i32, i32, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp, sz, vp]),
    'cliora_proj_workspace_bytes': (sz, [i32, i32, i32]),
    'cliora_proj_forward': (i32, [vp, vp, i32, i32, vp, vp, i32, vp, vp, sz, vp]),
    'cliora_proj_backward': (i32, [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, sz, vp]),
    'cliora_recon_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'cliora_recon_forward': (i32, [vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, sz, vp]),
    'cliora_recon_backward': (i32, [vp, vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    'cliora_rows_scatter_add': (i32, [vp, vp, i32, i32, vp, i64, vp]),
    'cliora_rows_scatter_add_segments': (i32, [pvp, pvp, C.POINTER(i32), i32, i32, vp, i64, vp]),
    'cliora_vg_workspace_bytes': (sz, [i32, i32]),
    'cliora_vg_loss': (i32, [i32, i32, i32, vp, f32, vp, vp, vp, sz, vp]),
    'cliora_vg_loss_ragged': (i32, [i32, i32, i32, vp, vp, f32, vp, vp, vp, sz, vp]),
    'cliora_clip_adam_workspace_bytes': (sz, []),
    'cliora_clip_adam': (i32, [vp, vp, vp, vp, sz, f32, f32, f32, f32, f32, i32, vp, sz, vp]),
    'cliora_cky_decode': (i32, [vp, vp, vp, vp]),
    'cliora_cky_spans': (i32, [vp, vp, vp, vp, vp]),
    'cliora_cky_spans_ragged': (i32, [vp] * 7),
    'cliora_span_posteriors_scratch_bytes': (sz, [vp]),
    'cliora_span_posteriors': (i32, [vp] * 10),
    'cliora_kbest_scratch_bytes': (sz, [vp, i32]),
    'cliora_kbest_spans': (i32, [vp, vp, vp, i32] + [vp] * 6),
    'cliora_sample_trees': (i32, [vp, vp, vp, vp, i32, u64, u64, f32] + [vp] * 5),
    'cliora_constrained_parse': (i32, [vp, vp, vp, vp, i32] + [vp] * 9),
    'cliora_kbest_constrained_scratch_bytes': (sz, [vp, i32, i32]),
    'cliora_kbest_spans_constrained': (i32, [vp, vp, vp, vp, i32, i32] + [vp] * 7),
    'cliora_sample_trees_constrained': (i32, [vp, vp, vp, vp, vp, i32, i32, u64, u64, f32] + [vp] * 7),
    'cliora_plan_split_score_count': (sz, [vp]),
    'cliora_bracket_grad': (i32, [vp, vp, vp, vp, i32] + [vp] * 6),
    'cliora_tree_expectation': (i32, [vp] * 12),
    'cliora_bracket_margin': (i32, [vp, vp, vp, vp, i32, f32, f32] + [vp] * 11),
    'cliora_tree_kl': (i32, [vp] * 16),
    'cliora_ground_eval': (i32, [i32, i32, i32, vp, i64, i64, i64, vp, i32, vp, vp, vp, vp, i32] + [vp] * 8),
    'cliora_ground_eval_ragged': (i32, [i32, i32, i32, vp, vp, i64, i64, i64, vp, i32, vp, vp, vp, vp, i32] + [vp] * 8),
    'cliora_phrase_gather': (i32, [i32, i32, i32, vp, i64, i64, vp, i64, i64, i32, vp, i32, vp, i64, i64, vp, vp]),
    'cliora_knn_ip_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'cliora_knn_ip': (i32, [i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, i64, vp, sz, vp]),
    'cliora_knn_filter': (i32, [i32, i32, vp, i64, vp, i64, vp, vp, i32, i32, vp, vp, vp, vp]),
    'cliora_maxsim_workspace_bytes': (sz, [i32, i32, i32, i32, i32]),
    'cliora_maxsim_scores': (i32, [i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, i64, vp, vp, i64, vp, vp, sz, vp]),
    'cliora_retrieval_ranks': (i32, [i32, i32, vp, i64, vp, vp, vp, vp, vp]),
    'cliora_score_topk': (i32, [i32, i32, i32, vp, i64, i64, vp, vp, vp]),
    'cliora_vocab_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'cliora_vocab_nll_forward': (i32, [i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'cliora_vocab_nll_backward': (i32, [i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, sz, vp]),
    'cliora_token_counts': (i32, [i64, vp, i32, vp, vp, vp]),
    'cliora_neg_sample_workspace_bytes': (sz, [i32, i32, i32]),
    'cliora_neg_sample': (i32, [i32, vp, i32, i32, i32, u64, u64, C.c_uint32, vp, vp, vp, sz, vp]),
    'cliora_prof_enable': (i32, [i32, i32]),
    'cliora_prof_read': (i32, [i32, C.POINTER(C.c_double), C.POINTER(C.c_longlong), vp]),
    'cliora_last_error': (C.c_char_p, []),
    'cliora_version': (C.c_char_p, []),
    'cliora_set_mfma_mode': (i32, [i32]),
    'cliora_set_wavefront': (i32, [i32]),
    'cliora_set_resident': (i32, [i32]),
    'cliora_device_side_stream': (i32, [vp, pvp]),
    'cliora_resident_trace': (i32, [vp, vp, sz, vp]),
    'cliora_launch_record': (i32, [i32]),
    'cliora_launch_record_read': (i32, [C.c_char_p, sz, psz]),
}

_lib = None
_bound = {}      # symbol -> bound function of the loaded library, resolved once (fn)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ChartLibError('HIP extension %s is missing: run `python -m cliora_amd.build` '
                            '(there is no CPU fallback for the chart path)' % LIB_PATH)
    # torch is imported first (above): its bundled HIP runtime must be the one already loaded when our library is dlopen'ed, otherwise
    # the process ends up with two runtimes and ours sees no device ("no ROCm-capable device is detected" at the first hipMalloc)
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():      # a symbol this library lacks (an older build through CLIORA_CHART_LIB): fn() refuses it
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L


def fn(name, L=None):
    """The bound function of the C-ABI symbol `name` (of the library object L when given, for tests): the one place that refuses a
    symbol the loaded library does not have.  The size queries and getters are called through it directly, the status-returning
    entry points through call()."""
    f = _bound.get(name) if L is None else None
    if f is None:
        f = getattr(lib() if L is None else L, name, None)
        if f is None:
            raise ChartLibError('%s has no %s: rebuild it (python -m cliora_amd.build)' % (LIB_PATH, name))
        if L is None:
            _bound[name] = f
    return f


def call(name, *args):
    """Run a status-returning entry point; a non-zero status raises with the library's message (check)."""
    rc = (_bound.get(name) or fn(name))(*args)
    if rc:
        check(rc, name)


def check(rc, what):
    if rc != 0:
        raise ChartLibError('%s failed (%d): %s' % (what, rc, fn('cliora_last_error')().decode()))


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def ptr_or_null(t):
    """ptr() that also gives NULL for a tensor without elements (an empty slice still has an address)."""
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def param_struct(tensors):
    return Params(*[(t.data_ptr() if t is not None else None) for t in map(tensors.get, PARAM_FIELDS)])


class device_guard(object):
    """`with device_guard(t)`: run under the device of the tensor `t`, so that the plan's index tables, the kernels' per-device attributes
    and every allocation land on the tensors' GPU even when it is not the current one.  Nothing to do for None, for a CPU tensor and
    for the device that is current already: `torch.cuda.device` costs ~10 us of host time per use, and a configs[0]-sized step is
    bound by the host (tools/host_bench.py).  Around the body of an autograd forward / backward as around any other block."""
    __slots__ = ('ctx',)

    def __init__(self, t):
        index = t.device.index if t is not None else None
        self.ctx = None if index is None or index == torch.cuda.current_device() else torch.cuda.device(index)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            return self.ctx.__exit__(*a)


_side_streams = {}


def side_stream(device):
    """torch handle of the library's caller lane on `device` (include/cliora_chart.h: cliora_device_side_stream): a stream that runs beside
    the current stream and the chart's own side streams.  One per device, created at the first request."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _side_streams.get(idx)
    if s is None:
        out = C.c_void_p()
        with torch.cuda.device(idx):
            call('cliora_device_side_stream', stream(), C.byref(out))
        s = torch.cuda.ExternalStream(out.value, device=torch.device('cuda', idx))
        _side_streams[idx] = s
    return s


class Plan:
    """Owns one cliora_plan (chart shape + device index tables)."""

    def __init__(self, B, L, D, share=True, normalize='unit', R=0, arch=0, forward_only=False):
        # A plan of 64 < L <= 128 words is forward only (no backward workspace, no use lists: include/cliora_chart.h), so it has to be
        # asked for as such: whoever holds a Plan may otherwise count on bwd_bytes and cliora_chart_backward.  get_plan() asks.
        if L > MAX_L and not forward_only:
            raise ChartLibError('L > %d is not supported by a plan with a backward (one split per lane in its softmax kernels): '
                                'Plan(..., forward_only=True) covers L <= %d for inference' % (MAX_L, MAX_L_FWD))
        self.key = (B, L, D, bool(share), normalize, R, arch)
        self.arch = arch
        self.B, self.L, self.D, self.share, self.normalize, self.R = B, L, D, bool(share), normalize, R
        self.C = L * (L + 1) // 2
        self.Dp = (D + 15) // 16 * 16
        h = C.c_void_p()
        call('cliora_plan_create_ex', B, L, D, int(bool(share)), NORM[normalize], R, arch, C.byref(h))
        self.handle = h
        self.fwd_bytes = fn('cliora_plan_fwd_workspace_bytes')(h)
        self.bwd_bytes = fn('cliora_plan_bwd_workspace_bytes')(h)
        self.pair_bytes = fn('cliora_plan_pair_states_bytes')(h)    # optional workspace tail: per-pair compose outputs for the hooks
        self.table_bytes = fn('cliora_plan_device_bytes')(h)     # index tables: this much host memory, and as much HBM after the first forward

    def table(self, name):
        import numpy as np
        ptr = C.POINTER(C.c_int32)()
        n = C.c_size_t()
        call('cliora_plan_table', self.handle, name.encode(), C.byref(ptr), C.byref(n))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                fn('cliora_plan_destroy')(self.handle)
                self.handle = None
        except Exception:
            pass


# Plan cache: least-recently-used, bounded by the bytes of index tables the cached plans hold on the device AND by their number
# (the host-side use lists of a plan are several times its device tables).  Length-bucketed batches give one (B, L) key per bucket:
# a DioraMLP plan holds 0.1 MB (L 20) to 1 MB (L 40) of device tables, a TreeLSTM plan at B 64 / L 40 about 25 MB (its
# batch-expanded row maps).  A long plan (64 < L <= 128, forward only) uploads its pair tables alone, no use lists: 1.1 MB at L 65,
# 8.4 MB at L 128 -- table_bytes is what cliora_plan_device_bytes reports for it, so the budget below counts it as it is.
PLAN_CACHE_BYTES = int(os.environ.get('CLIORA_PLAN_CACHE_MB', '512')) << 20
PLAN_CACHE_MAX = int(os.environ.get('CLIORA_PLAN_CACHE_MAX', '128'))
_plans = collections.OrderedDict()


def get_plan(B, L, D, share, normalize, R, device_index, arch=0):
    key = (B, L, D, bool(share), normalize, R, device_index, arch)
    pl = _plans.get(key)
    if pl is not None:
        _plans.move_to_end(key)
        return pl
    pl = _plans[key] = Plan(B, L, D, share, normalize, R, arch, forward_only=L > MAX_L)    # long plans: the modules refuse training on them
    total = sum(q.table_bytes for q in _plans.values())
    while (total > PLAN_CACHE_BYTES or len(_plans) > PLAN_CACHE_MAX) and len(_plans) > 1:
        _, old = _plans.popitem(last=False)          # evicted plans free their device tables when the last user drops them
        total -= old.table_bytes
    return pl


def prof_enable(kclass, on=True):
    call('cliora_prof_enable', KCLASS[kclass], int(on))


def prof_read(kclass, stream=0):
    ms, n = C.c_double(), C.c_longlong()
    call('cliora_prof_read', KCLASS[kclass], C.byref(ms), C.byref(n), C.c_void_p(stream))
    return ms.value, n.value


def launch_record_read():
    """The distinct kernel instances noted since the launch record was turned on (include/cliora_chart.h: cliora_launch_record), as a set."""
    read = fn('cliora_launch_record_read')
    n = C.c_size_t()
    call('cliora_launch_record_read', None, 0, C.byref(n))
    while True:         # the record is process-wide: another host thread's launch may lengthen it between the size query and the read
        cap = n.value + 256
        buf = C.create_string_buffer(cap)
        rc = read(buf, cap, C.byref(n))
        if rc == 0:
            return set(buf.value.decode().split('\n')) - {''}
        if n.value <= cap:     # refused, and not for want of room
            check(rc, 'cliora_launch_record_read')


class launch_record(object):
    """`with _lib.launch_record() as rec:` -- `rec` is a set of strings that, when the block ends, holds the kernel instances the library's
    dispatchers launched inside it ('level_compose_bwd<5,0,f32>', 'tn_gemm<2,2,colsum>', ...).  The record is process-wide: launches of
    other host threads during the block are in it too.  Turns the record off again unless it was on already."""

    def __enter__(self):
        self.rec = set()
        self.prev = fn('cliora_launch_record')(1)
        return self.rec

    def __exit__(self, *a):
        self.rec.update(launch_record_read())
        if not self.prev:        # (turning it on again would clear it: a block inside another one restarts the outer one's record)
            fn('cliora_launch_record')(0)


MFMA_MODES = {'f32': 0, 'bf16x3': 1}


WAVEFRONT_MODES = {'auto': -1, 'off': 0, 'on': 1}


def set_wavefront(mode):
    """Scheduling of the inside / outside passes (include/cliora_chart.h: cliora_set_wavefront): 'auto' (default), 'off' (the
    reference's order on the caller's stream alone), 'on' (two streams) or 'merged' (the two passes' launches of a step as one grid on one queue).  Results are bitwise identical.  Returns the previous mode."""
    prev = fn('cliora_set_wavefront')({'merged': 2}.get(mode, WAVEFRONT_MODES.get(mode)))
    return {-1: 'auto', 0: 'off', 1: 'on', 2: 'merged'}[prev]


def set_resident(mode):
    """One workgroup per sentence for the level loops of a small-D DioraMLP plan (include/cliora_chart.h: cliora_set_resident):
    'auto' (default), 'off', 'on'.  Returns the previous mode's name."""
    prev = fn('cliora_set_resident')(WAVEFRONT_MODES[mode])
    return {v: k for k, v in WAVEFRONT_MODES.items()}[prev]


def set_mfma_mode(mode):
    """Arithmetic of the compose-layer GEMMs and their weight gradient: 'bf16x3' (default; three bf16 MFMAs per
    product, fp32 accumulate) or 'f32' (fp32-input MFMA, the reference's arithmetic).  Returns the previous mode."""
    prev = fn('cliora_set_mfma_mode')(MFMA_MODES[mode])
    return 'f32' if prev == 0 else 'bf16x3'
