"""Shared by test_lstm_cases_cpu.py and test_gpu_treelstm_limits.py (not a test module): the cases that take DioraTreeLSTM
(cliora_amd/treelstm.py, csrc/api_lstm.hip, csrc/lstm_kernels.hpp) to the limits of its plan, their seeded inputs, the fp64 oracle
they are held to, and the figures measured for them.

What each case reaches (D -> Dp, the width the kernels run at):
  (16, 2, 64)  L = 64: every lane of pair_scores_fwd / lstm_scores_bwd live; Dp = 16: 4 working threads of a 64-thread cell block, K = 16
  (24, 2, 63)  L = 63; D = 24 -> Dp = 32: the padded copy tables and vload_ext, unshared
  (33, 3, 9)   D = 33 -> Dp = 48 (15 pad columns, K = 48 no multiple of 32), shared and unshared
  (512, 2, 6)  Dp = 512: 128 working threads per cell block, both 16-byte vectors of every lane in the wave-per-row kernels
  (272, 2, 5)  Dp = 272: the lane + 64 range with 4 of its 64 lanes on, a 128-thread cell block with 68 working threads, K = 272
  (400, 1, 3)  the smallest two-stream chart, B * L = 3 rows: below one 16-row tile
  (48, 3, 1)   L = 1: leaves and root only; U and mat unused
  (64, 2, 2)   L = 2: one split, one stream whatever the wavefront mode
  (48, 3, 7) and (33, 2, 6) inside only: run_outside = 0 (the memsets of OH / OC / OS, a backward without the outside chain)
  (100, 2, 17) D = 100 -> Dp = 112 (K = 112), shared
"""
import functools

import numpy as np
import torch

from oracle import diora_ref as R
from oracle import synth

KEYS = synth.TREELSTM_CHARTS          # inside_h, inside_c, inside_s, outside_h, outside_c, outside_s
# (D, B, L, share, outside)
CASES = (
    (16, 2, 64, True, True),
    (24, 2, 63, False, True),
    (33, 3, 9, True, True),
    (33, 3, 9, False, True),
    (512, 2, 6, True, True),
    (272, 2, 5, False, True),
    (400, 1, 3, True, True),
    (48, 3, 1, True, True),
    (64, 2, 2, False, True),
    (48, 3, 7, True, False),
    (33, 2, 6, False, False),
    (100, 2, 17, True, True),
)
# The project's TreeLSTM bounds (tests/test_gpu_treelstm.py): max |x - ref| over a tensor, of max(1, max |ref|).  There are no ReLUs on
# this path, so no kinks: element-wise maxima in both arithmetic modes.  The fp32 oracle alone sits 15 times inside them at every case
# (test_lstm_cases_cpu.py holds it to a tenth).
OUT_TOL = 1e-4
GRAD_TOL = 2e-4
# The process-wide switches (tools/lstm_probe.py): the two shapes of the issue, whose levels all have fewer than 256 rows and so run
# the 16 x 80 gate GEMM whatever CLIORA_GEMM3_SHAPE says (gemm_launch.hpp: launch_rows_direct3), and one whose leaf level (288 rows)
# and first level (256) reach the RT x CT tiles, at K = 112 with a ragged last column block.
PROBE_SHAPES = ((400, 4, 9, True), (100, 2, 17, False), (112, 32, 9, True))


def case(D, B, L, share, outside, dtype=torch.float32):
    """Seeded parameters (R.init_params_treelstm(D, seed=6, share)), x (B, L, D) and the cotangents of the six charts (the three
    inside ones when `outside` is false), drawn in fp32 and cast to `dtype`: the fp32 and fp64 runs see the same numbers.  The draw
    is oracle.synth.treelstm_case, which tools/lstm_probe.py repeats in its own process."""
    return synth.treelstm_case(D, B, L, share=share, outside=outside, dtype=dtype)


def oracle_run(D, B, L, share, outside, dtype):
    """One run of the CPU oracle at `dtype`, differentiated by autograd: dict(out {chart: array}, grad {parameter: array or None},
    x_grad, pair_s_in {level: (B, Lc, N, 1) tensor})."""
    P, x, cot = case(D, B, L, share, outside, dtype)
    for v in P.values():
        v.requires_grad_(True)
    x.requires_grad_(True)
    ref = R.diora_forward(P, x, x, arch='treelstm', share=share, outside=outside, keep_pairs=True)
    sum((ref[k] * cot[k]).sum() for k in cot).backward()
    return dict(out={k: ref[k].detach().numpy() for k in KEYS},
                grad={k: (v.grad.numpy() if v.grad is not None else None) for k, v in P.items()},
                x_grad=x.grad.numpy(), pair_s_in={lv: s.detach() for lv, s in ref['pair_s_in'].items()})


@functools.lru_cache(maxsize=None)
def oracle64(D, B, L, share, outside=True):
    """The yardstick: oracle_run in fp64, once per case and process (both arithmetic modes and the tree test share it; L = 64 takes
    about 10 s of CPU).  Read-only: the arrays refuse writes."""
    ref = oracle_run(D, B, L, share, outside, torch.float64)
    for a in list(ref['out'].values()) + list(ref['grad'].values()) + [ref['x_grad']]:
        if a is not None:
            a.setflags(write=False)
    return ref


def scale(ref):
    return max(1.0, float(np.abs(ref).max())) if ref.size else 1.0


def rel_err(got, ref):
    """max |got - ref| / max(1, max |ref|), in fp64."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    if not ref.size:
        return 0.0
    return float(np.abs(got.astype(np.float64) - ref).max()) / scale(ref)


# Printed by test_gpu_treelstm_limits.py::test_parity_at_the_limits on the MI355X (run with -s): case -> mode -> (worst chart, worst
# gradient), each max |device - fp64| / max(1, max |fp64|).  Beside them the fp32 oracle's own figures (test_lstm_cases_cpu.py).
MEASURED = {
    (16, 2, 64, True, True): {'f32': (1.036e-06, 1.912e-06), 'bf16x3': (2.636e-05, 4.717e-05)},
    (24, 2, 63, False, True): {'f32': (9.513e-07, 3.988e-06), 'bf16x3': (2.575e-05, 4.398e-05)},
    (33, 3, 9, True, True): {'f32': (4.017e-07, 8.012e-07), 'bf16x3': (9.466e-06, 1.712e-05)},
    (33, 3, 9, False, True): {'f32': (6.699e-07, 1.513e-06), 'bf16x3': (1.254e-05, 2.531e-05)},
    (512, 2, 6, True, True): {'f32': (2.464e-06, 9.957e-06), 'bf16x3': (1.900e-05, 1.778e-05)},
    (272, 2, 5, False, True): {'f32': (1.178e-06, 3.626e-06), 'bf16x3': (1.258e-05, 1.661e-05)},
    (400, 1, 3, True, True): {'f32': (1.322e-06, 3.794e-06), 'bf16x3': (3.849e-06, 1.533e-05)},
    (48, 3, 1, True, True): {'f32': (1.940e-07, 5.106e-07), 'bf16x3': (1.940e-07, 5.106e-07)},
    (64, 2, 2, False, True): {'f32': (3.579e-07, 7.944e-07), 'bf16x3': (4.679e-06, 1.406e-05)},
    (48, 3, 7, True, False): {'f32': (3.705e-07, 1.439e-06), 'bf16x3': (6.902e-06, 1.610e-05)},
    (33, 2, 6, False, False): {'f32': (3.366e-07, 3.193e-06), 'bf16x3': (7.236e-06, 3.650e-05)},
    (100, 2, 17, True, True): {'f32': (5.021e-07, 2.445e-06), 'bf16x3': (8.681e-06, 3.155e-05)},
}
# The process-wide switches (test_process_wide_switches), (charts, gradients) against the fp64 oracle: CLIORA_LSTM_PROJ=f32 (1.0e-6, 6.6e-6) /
# (5.3e-7, 3.0e-6) / (1.2e-6, 2.7e-6) at the three PROBE_SHAPES, the default (4.6e-6, 1.7e-5) / (8.7e-6, 3.1e-5) / (1.1e-5, 2.5e-5); the
# CLIORA_GEMM3_SHAPE settings 0, 22 and 11 gave the default's figures to every printed digit at all three shapes (the tile shape does
# not change an element's summation order over k).
#
# The exact-fp32 mode sits at the reference's own fp32 figures at every case (charts 1.9e-7 .. 2.5e-6 beside 2.5e-7 .. 2.4e-6, gradients
# 5.1e-7 .. 1.0e-5 beside 7.4e-7 .. 6.3e-6), so it is held to four times its worst measured figure, the margin of the project's
# pinned-regime tests: charts 4 x 2.464e-6, gradients 4 x 9.957e-6 (both at D 512).
F32_OUT_TOL = 1e-5
F32_GRAD_TOL = 4e-5
