"""Seeded synthetic inputs shared by the golden generator, the tests and bench.py.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  The draw order below is the
one tests/golden/make_golden.py used when it ran the reference, so a case can be
re-created from its seed on any box with the same torch build.
"""
import torch

from . import chart_layout as CL
from .diora_ref import init_params, init_params_treelstm

TREELSTM_CHARTS = ('inside_h', 'inside_c', 'inside_s', 'outside_h', 'outside_c', 'outside_s')


def treelstm_case(D, B, L, share=True, outside=True, dtype=torch.float32):
    """-> (params, x_span, cotangents) of a DioraTreeLSTM case: init_params_treelstm(D, seed=6, share), then x and the cotangents of
    the six charts (the three inside ones without the outside pass) from one generator seeded 7 -- the draw of
    tests/test_gpu_treelstm.py.  Drawn in fp32 and cast to `dtype`, so an fp64 run sees the numbers of the fp32 one."""
    P = {k: v.to(dtype) for k, v in init_params_treelstm(D, seed=6, share=share).items()}
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, L, D, generator=g).to(dtype)
    C = CL.n_cells(L)
    keys = TREELSTM_CHARTS if outside else TREELSTM_CHARTS[:3]
    cot = {k: torch.randn(B, C, 1 if k.endswith('_s') else D, generator=g).to(dtype) for k in keys}
    return P, x, cot


def diora_case(D, B, L, seed, share=True, compress=False):
    """-> (params, x_span, cotangents) exactly as make_golden.diora_case drew them."""
    P = init_params(D, share=share, seed=seed, compress=compress)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, L, D, generator=g)
    C = CL.n_cells(L)
    cot = {}
    for k, w in (('inside_h', D), ('inside_s', 1), ('outside_h', D), ('outside_s', 1)):
        cot[k] = torch.randn((B, C, w), generator=g)
    return P, x, cot
