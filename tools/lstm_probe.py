#!/usr/bin/env python
"""Chart forward + backward of one seeded DioraTreeLSTM case, every chart and gradient saved to an .npz -- run once per setting of a
library switch that is read once per process (tests/test_gpu_treelstm_limits.py compares CLIORA_LSTM_PROJ=f32 with the default and with
the tile shapes of CLIORA_GEMM3_SHAPE).
   python tools/lstm_probe.py D B L share out.npz"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import synth                                     # noqa: E402  (inputs only: the seeded case generator)
from cliora_amd.treelstm import DioraTreeLSTM                # noqa: E402

D, B, L, share = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), bool(int(sys.argv[4]))
P, x, cot = synth.treelstm_case(D, B, L, share=share)
m = DioraTreeLSTM(D, share=share)
sd = m.state_dict()
for k in sd:
    sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
m.load_state_dict(sd)
m = m.cuda().train()
xg = x.clone().cuda().requires_grad_(True)
m(xg, xg)
keys = synth.TREELSTM_CHARTS
torch.autograd.backward([getattr(m, k) for k in keys], [cot[k].cuda() for k in keys])
torch.cuda.synchronize()
out = {'x': xg.grad.cpu().numpy()}
for k, p_ in m.named_parameters():
    if p_.grad is not None:
        out[k] = p_.grad.cpu().numpy()
for k in keys:
    out['out_' + k] = getattr(m, k).detach().cpu().numpy()
np.savez(sys.argv[5], **out)
