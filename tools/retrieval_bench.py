#!/usr/bin/env python
"""Caption-image retrieval scores on one GPU at Flickr30k test size; prints one JSON line.

  * cliora_maxsim_scores (cliora_amd.retrieval.maxsim_scores): N captions of 5..40 words against M images of R regions, width D in
    --widths, per MFMA mode: the median of --reps device-event times after a warm-up, with the default workspace budget (the call is
    split over the captions) and with a budget that takes it in one call; the algorithmic TFLOP/s 2 NT MR D / t on the TRUE rows (the
    padding of captions and images to 16-row tiles is the kernel's own cost) and its share of the mode's MFMA peak;
  * the route a user has without it, in the same run: torch.einsum over chunks of tokens sized so that the (tokens x regions)
    intermediate fits 1 GB, max over each image's regions, times w, index_add_ over each caption's tokens;
  * the agreement of the two score matrices;
  * cliora_retrieval_ranks, and cliora_score_topk (k = 10, both directions) against torch.topk on the score matrix.

    python tools/retrieval_bench.py [--out profiles/retrieval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cliora_amd import _lib                     # noqa: E402
from cliora_amd import retrieval                # noqa: E402

PEAK = {'bf16x3': 2.5e15 / 3, 'f32': 157.3e12}       # products per second at the nominal peaks, as FLOP/s of the fp32 product


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
    return statistics.median(times), min(times), max(times), out


def torch_route(q, cap_of, w, keys, N, M, R, budget_bytes=1 << 30):
    chunk = max(1, budget_bytes // (4 * keys.shape[0]))
    S = torch.zeros((N, M), dtype=torch.float32, device=q.device)
    for r in range(0, q.shape[0], chunk):
        sc = torch.einsum('td,kd->tk', q[r:r + chunk], keys)
        v = sc.view(sc.shape[0], M, R).max(-1).values * w[r:r + chunk, None]
        S.index_add_(0, cap_of[r:r + chunk], v)
    return S


def row(N, M, R, D, reps, seed=0):
    rs = np.random.RandomState(seed)
    lens = rs.randint(5, 41, size=N)
    q_off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    NT, MR = int(q_off[-1]), M * R
    g = torch.Generator(device='cuda').manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(NT, D, device='cuda', generator=g), dim=1)
    keys = torch.nn.functional.normalize(torch.randn(MR, D, device='cuda', generator=g), dim=1)
    w = torch.from_numpy(np.repeat(1.0 / lens, lens).astype(np.float32)).cuda()
    cap_of = torch.from_numpy(np.repeat(np.arange(N), lens)).cuda()
    k_off = [R * m for m in range(M + 1)]
    image_of = torch.from_numpy(rs.randint(0, M, size=N).astype(np.int32)).cuda()
    flop = 2.0 * NT * MR * D
    one_call_mb = _lib.fn('cliora_maxsim_workspace_bytes')(N, NT, M, MR, D) / 2 ** 20
    out = dict(N=N, NT=NT, M=M, R=R, D=D, tflop=round(flop / 1e12, 3), workspace_one_call_mb=round(one_call_mb, 1),
               intermediate_avoided_gb=round(4.0 * NT * MR / 1e9, 2), padded_tile_work=round(
                   sum((n + 15) // 16 * 16 for n in lens) * ((R + 15) // 16 * 16) * M / float(NT * MR), 3))
    ms_t, lo, hi, St = median_ms(lambda: torch_route(q, cap_of, w, keys, N, M, R), reps)
    out['torch_einsum_max_segsum'] = dict(ms=round(ms_t, 3), min_ms=round(lo, 3), max_ms=round(hi, 3))
    for mode in ('bf16x3', 'f32'):
        prev = _lib.set_mfma_mode(mode)
        try:
            ms, lo, hi, S = median_ms(lambda: retrieval.maxsim_scores(q, q_off, w, keys, k_off), reps)
            ms1, lo1, hi1, S1 = median_ms(lambda: retrieval.maxsim_scores(q, q_off, w, keys, k_off, max_workspace_mb=one_call_mb + 1), reps)
        finally:
            _lib.set_mfma_mode(prev)
        assert torch.equal(S.view(torch.int32), S1.view(torch.int32))         # the split over captions changes no bit
        tf = flop / (ms1 * 1e-3)
        out[mode] = dict(ms=round(ms, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), one_call_ms=round(ms1, 3), one_call_min_ms=round(lo1, 3),
                         one_call_max_ms=round(hi1, 3), tflops=round(tf / 1e12, 2), share_of_peak=round(tf / PEAK[mode], 3),
                         floor_ms=round(flop / PEAK[mode] * 1e3, 2), speedup_vs_torch=round(ms_t / ms, 2),
                         max_abs_diff_vs_torch=float((S - St).abs().max()))
        if mode == 'bf16x3':
            Sk = S
    ms_r, _, _, _ = median_ms(lambda: retrieval.retrieval_ranks(Sk, image_of), reps)
    ms_k, _, _, (Dk, Ik) = median_ms(lambda: (retrieval.score_topk(Sk, 10), retrieval.score_topk(Sk, 10, transpose=True))[0], reps)
    ms_tk, _, _, (Dt, It) = median_ms(lambda: (torch.topk(Sk, 10, dim=1), torch.topk(Sk.t(), 10, dim=1))[0], reps)
    out['ranks_ms'] = round(ms_r, 3)
    out['topk10_both_ways'] = dict(ms=round(ms_k, 3), torch_topk_ms=round(ms_tk, 3), same_scores=bool(torch.equal(Dk, Dt)))
    del q, keys, St, S, S1, Sk
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--captions', type=int, default=5000)
    ap.add_argument('--images', type=int, default=1000)
    ap.add_argument('--regions', type=int, default=36)
    ap.add_argument('--widths', default='400,800')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('retrieval_bench needs a GPU: a CPU run measures nothing')
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps,
               rows=[row(a.captions, a.images, a.regions, int(D), a.reps) for D in a.widths.split(',')])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
