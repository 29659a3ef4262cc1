#!/usr/bin/env python
"""The exact word-prediction loss over the whole vocabulary on one GPU; writes one JSON line (profiles/vocab_bench.json).

  * evaluation: cliora_amd.vocab.vocab_nll with ranks at T = 111 826 tokens (the 5 000 captions of tools/retrieval_bench.py), E = 400,
    V in --eval-vocab, per MFMA mode;
  * training: forward + backward at T = 1 280, E = 400, V in --train-vocab, with dK on and off, per MFMA mode;
  * beside each, in the same run, the route a user has without it: torch.mm over chunks of tokens whose logits fit 1 GB +
    torch.logsumexp + gather (evaluation), F.cross_entropy on the full logits with autograd (training); and, for scale, the sampled
    loss at k_neg = 100 (heads.recon_loss, forward + backward);
  * the two routes must agree within the bounds of tests/vocab_cases.py (the score bound on nll, the gradient tolerance on dQ / dK).

Every time is the median of --reps device-event times after a warm-up.

    python tools/vocab_bench.py [--out profiles/vocab_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cliora_amd import _lib                     # noqa: E402
from cliora_amd import heads, vocab             # noqa: E402

PEAK = {'bf16x3': 2.5e15 / 3, 'f32': 157.3e12}       # products per second at the nominal peaks, as FLOP/s of the fp32 product
EPS = {'bf16x3': 2e-5, 'f32': 1e-6}                   # tests/vocab_cases.py: the per-product score bound for unit rows
TORCH_GRAD_ERR = 6.1e-6                               # tests/vocab_cases.py: the largest entry of TORCH_F32_GRAD_ERR


def eps(mode, E):
    return EPS[mode] * (max(1.0, (E / 256.0) ** 0.5) if mode == 'f32' else 1.0)


def median_ms(fn, reps):
    out = fn()                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return dict(ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3)), out


def inputs(T, V, E, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    K = torch.randn(V, E, device='cuda', generator=g)
    tok = torch.randint(0, V, (T,), device='cuda', generator=g)
    Q = torch.randn(T, E, device='cuda', generator=g) + 3.5 * K[tok] / E ** 0.5       # as tests/vocab_cases.py: rows lean towards their word
    return Q, K, tok


def torch_eval(Q, K, tok, budget_bytes=1 << 30):
    chunk = max(1, budget_bytes // (4 * K.shape[0]))
    nll = torch.empty(Q.shape[0], device=Q.device)
    for r in range(0, Q.shape[0], chunk):
        s = torch.mm(Q[r:r + chunk], K.t())
        nll[r:r + chunk] = torch.logsumexp(s, 1) - s.gather(1, tok[r:r + chunk, None])[:, 0]
    return nll


def bound(mode, Q, K):
    return (eps(mode, Q.shape[1]) + eps('f32', Q.shape[1])) * float(Q.norm(dim=1).max()) * float(K.norm(dim=1).max())


def eval_row(T, V, E, reps):
    Q, K, tok = inputs(T, V, E, 0)
    out = dict(T=T, V=V, E=E, logits_avoided_gb=round(4.0 * T * V / 1e9, 1), workspace_mb=round(vocab.workspace_bytes(T, V, E) / 2 ** 20, 1))
    out['torch_mm_logsumexp_gather'], nll_t = median_ms(lambda: torch_eval(Q, K, tok), reps)
    flop = 2.0 * T * V * E
    for mode in ('bf16x3', 'f32'):
        prev = _lib.set_mfma_mode(mode)
        try:
            r, res = median_ms(lambda: vocab.vocab_nll(Q, K, tok, want_rank=True), reps)
        finally:
            _lib.set_mfma_mode(prev)
        diff = float((res[1] - nll_t).abs().max())
        assert diff <= 2 * bound(mode, Q, K), (mode, diff, 2 * bound(mode, Q, K))
        r.update(tflops=round(flop / (r['ms'] * 1e-3) / 1e12, 2), share_of_peak=round(flop / (r['ms'] * 1e-3) / PEAK[mode], 3),
                 speedup_vs_torch=round(out['torch_mm_logsumexp_gather']['ms'] / r['ms'], 2), max_abs_nll_diff_vs_torch=diff,
                 nll_bound=2 * bound(mode, Q, K), mean_nll=float(res[0]), acc_at_1=float((res[4] == 0).float().mean()))
        out[mode] = r
    return out


def train_row(T, V, E, reps, k_neg=100):
    Q, K, tok = inputs(T, V, E, 1)
    out = dict(T=T, V=V, E=E, logits_avoided_gb=round(4.0 * T * V / 1e9, 2), workspace_mb=round(vocab.workspace_bytes(T, V, E, True) / 2 ** 20, 1))

    leaves = {need_k: (Q.clone().requires_grad_(True), K.clone().requires_grad_(need_k)) for need_k in (True, False)}

    def step(fn, need_k):                # the leaves are made once, outside the timed region: a repetition is forward + backward alone
        q, k = leaves[need_k]
        q.grad = k.grad = None
        fn(q, k).backward()
        return q.grad, k.grad

    torch_fn = lambda q, k: F.cross_entropy(torch.mm(q, k.t()), tok)
    ours = lambda q, k: vocab.vocab_nll(q, k, tok)[0]
    ref = {}
    for need_k in (True, False):
        name = 'dQ_dK' if need_k else 'dQ_only'
        out['torch_cross_entropy_' + name], ref[need_k] = median_ms(lambda: step(torch_fn, need_k), reps)
    for mode in ('bf16x3', 'f32'):
        prev = _lib.set_mfma_mode(mode)
        try:
            r = {}
            for need_k in (True, False):
                name = 'dQ_dK' if need_k else 'dQ_only'
                r[name], got = median_ms(lambda: step(ours, need_k), reps)
                # two fp32 routes against each other: the torch route's own error and the kernels' tolerance (twice it; split: plus 2 delta)
                tol = TORCH_GRAD_ERR * 3 + (2 * eps(mode, E) * float(Q.norm(dim=1).max()) * float(K.norm(dim=1).max()) if mode != 'f32' else 0.0)
                for a, b, what in zip(got, ref[need_k], ('dQ', 'dK')):
                    if a is None:
                        continue
                    err = float((a - b).abs().max() / b.abs().max())
                    assert err <= tol, (mode, name, what, err, tol)
                    r[name]['%s_rel_diff_vs_torch' % what] = err
                r[name]['speedup_vs_torch'] = round(out['torch_cross_entropy_' + name]['ms'] / r[name]['ms'], 2)
        finally:
            _lib.set_mfma_mode(prev)
        out[mode] = r
    # for scale: the reference's sampled loss (one positive + k_neg negatives) on the same number of tokens, forward + backward
    B, L, D = T // 20, 20, E
    g = torch.Generator(device='cuda').manual_seed(2)
    oh = torch.randn(B, L * (L + 1) // 2, D, device='cuda', generator=g)
    mat = torch.randn(D, E, device='cuda', generator=g)
    neg = torch.randint(0, V, (k_neg,), device='cuda', generator=g)

    o, m, k = oh.requires_grad_(True), mat.requires_grad_(True), leaves[True][1]

    def sampled():
        o.grad = m.grad = k.grad = None
        heads.recon_loss(k, m, o, tok[:B * L].view(B, L), neg).backward()
        return o.grad

    out['sampled_k_neg_%d' % k_neg], _ = median_ms(sampled, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--eval-tokens', type=int, default=111826)
    ap.add_argument('--eval-vocab', default='20000,400000')
    ap.add_argument('--train-tokens', type=int, default=1280)
    ap.add_argument('--train-vocab', default='8000,20000,400000')
    ap.add_argument('--width', type=int, default=400)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vocab_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vocab_bench needs a GPU: a CPU run measures nothing')
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
               eval=[eval_row(a.eval_tokens, int(V), a.width, a.reps) for V in a.eval_vocab.split(',') if V],
               train=[train_row(a.train_tokens, int(V), a.width, a.reps) for V in a.train_vocab.split(',') if V])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
