"""The kernel instances the CLIORA (vision-language) entries can launch, and one shape per instance and launch edge (not a test module; shared
by test_vl_cases_cpu.py and test_gpu_vl_dispatch.py).  The vision-language counterpart of dispatch_cases.py.

What decides an instance (Dp = D rounded up to 16, NRp = B R rounded up to 16, pick(n) = the widest of 5, 4, 2, 1 dividing n; read off
csrc/gemm_launch.hpp launch_rows / launch_rows3, csrc/api_vl.hip launch_tn_regions / region_segments / launch_scorer and
csrc/api_mlp_launch.hpp with_regions):
  rows_gemm_ws<CT,SC,WAVES>      out = A W^T with W (ncols x Kseg) in LDS: CT = the widest of 5, 4, 2, 1 that divides ncols / 16 and whose
                                 CT 16 Kseg floats fit 150 KiB, SC = pick(Kseg / 16), WAVES 8 above 1536 (row tiles x column blocks), else 4.
                                 Forward scorers: ncols = NRp, Kseg = Dp, rows B C (all_atten, exact mode) or B L (vg_atten, both modes).
                                 Backward (d inside_h + outside_h, d x_word; both modes): ncols = Dp, Kseg = NRp / nseg.
  rows_gemm_ws3<CT,WAVES,K16>    all_atten and the region-max scorer in split-bf16 mode: CT as above with the image stride
                                 roundup32(Dp) + 8 for Kseg; K16 = 25 at Dp 400, else 0.
  tn_gemm(ij)<TI,TJ,nocolsum>    d obj_span / d obj_word: TI = 4 / 2 / 1 by NRp / 16 mod 4, TJ = pick(Dp / 16)
  region_segments(one | several xN)   the backward's split of the region axis: the fewest N segments of NRp / N (a multiple of 16) with
                                 pick(Dp / 16) 16 (NRp / N) floats within 150 KiB; N is geometry, not enumerated ('several x*')
  region_max_bwd_obj(nchunk N)   N = ceil(B / max(4, ceil(B / 8))): 1 .. 8
  cell_attend_fwd / cell_attend_bwd / obj_grad_reduce <NRW>    NRW = 9 regions per wave for R <= 36, 16 for R <= 64

The scorer, region-max and contrastive entries are called directly on drawn tensors (unit-norm chart rows, regions 0.3 randn), one
gradient per call, so that the record of a call names the instance of that one GEMM; only the attention kernels need a chart.
The references are the einsum / max / loss formulas of oracle/diora_ref.py in fp64.

Measured on the MI355X (test_gpu_vl_dispatch.py writes vl_accuracy_<mode>.json), largest error over bound of any tensor of any case:
  f32     0.49  (d obj_span of waves8_4x5; then values of max_k16 0.43, vg_atten_score of k16_ct1 0.42, all_atten_score of k16_ct1 0.37; chart cases up to
                 0.35 (x_span of att_512x64), chart outputs below 0.02).  The forward scores, which nobody had measured against the quantile rule, hold it:
                 their largest error is 1.1e-6 of scale (fp32 oracle on the same case: 2.3e-7), so none is held to 1e-4 instead.
  bf16x3  0.12  (d smax of con_b128: the contrastive kernels, held to the exact mode's rule in both modes; chart outputs up to 0.09 (all_atten_score of
                 att_48x35), every grad_check tensor below 0.01; scores 9.7e-6 of scale at most)
Arg-max regions: none differs from fp64 outside the clearance in either mode (566 312 entries over the region-max cases; at most 0.34 % of a case's
entries are inside the split mode's clearance, 0.008 % inside the exact mode's).  Under the exact mode's clearance split mode names another region
in 2 entries (max_b33, max_w8_5x1), which is why that mode has a clearance of its own (split_bf16_clearance).
Every call's record held the expected entries, and its GEMM entries were exactly the expected ones.
"""
import fnmatch

import dispatch_cases as DC

MODES = DC.MODES
ORACLE_THREADS = DC.ORACLE_THREADS
RELU_MARGIN = DC.RELU_MARGIN
dist = DC.dist
covers = DC.covers

MAX_B, MAX_L, MAX_R, MAX_D = 128, 64, 64, 512          # the ranges the inventory is taken over, per entry
LDS_BUDGET = 150 * 1024
EIGHT_WAVES_ABOVE = 1536

# ------------------------------------------------------------------ the dispatch rules, restated


def pick(n):
    return next(t for t in (5, 4, 2, 1) if n % t == 0)


def pad16(n):
    return (n + 15) // 16 * 16


def n_cells(L):
    return L * (L + 1) // 2


def _ct_waves(ncols, row_floats, nrows):
    nt = ncols // 16
    for ct in (5, 4, 2, 1):
        if nt % ct or ct * 16 * row_floats * 4 > LDS_BUDGET:
            continue
        return ct, 8 if ((nrows + 15) // 16) * (nt // ct) > EIGHT_WAVES_ABOVE else 4
    raise ValueError('weight block does not fit LDS')


def rows_ws(Kseg, ncols, nrows):
    ct, waves = _ct_waves(ncols, Kseg, nrows)
    return 'rows_gemm_ws<%d,%d,%d>' % (ct, pick(Kseg // 16), waves)


def rows_ws3(K, ncols, nrows):
    ct, waves = _ct_waves(ncols, (K + 31) // 32 * 32 + 8, nrows)
    return 'rows_gemm_ws3<%d,%d,%d>' % (ct, waves, 25 if K == 400 else 0)


def tn_regions(NRp, Dp):
    nt = NRp // 16
    return 'tn_gemm(ij)<%d,%d,nocolsum>' % (4 if nt % 4 == 0 else 2 if nt % 2 == 0 else 1, pick(Dp // 16))


def region_segments(NRp, Dp):
    ct = pick(Dp // 16)
    for n in range(1, NRp // 16 + 1):
        if NRp % n or (NRp // n) % 16:
            continue
        if ct * 16 * (NRp // n) * 4 <= LDS_BUDGET:
            return NRp // n, n
    return 16, NRp // 16


def segments_entry(nseg):
    return 'region_segments(one)' if nseg == 1 else 'region_segments(several x%d)' % nseg


def nchunk(B):
    per = max(4, (B + 7) // 8)
    return (B + per - 1) // per


def nrw(R):
    return 9 if R <= 36 else 16


def scorer(mode, Dp, NRp, nrows):
    """launch_scorer: all_atten and the region-max scorer"""
    return rows_ws(Dp, NRp, nrows) if mode == 'f32' else rows_ws3(Dp, NRp, nrows)


def score_expect(B, L, R, D, mode):
    """What each call of a dense-scorer case must leave in the record: the forward, and the backward for one gradient at a time.  The
    same in training and eval mode (eval adds unit_norm_rows / rows_unit_bwd, which have one instance)."""
    Dp, NRp, C = pad16(D), pad16(B * R), n_cells(L)
    Kseg, nseg = region_segments(NRp, Dp)
    seg = segments_entry(nseg)
    return {'forward': {scorer(mode, Dp, NRp, B * C), rows_ws(Dp, NRp, B * L)},
            'sum_h': {seg, rows_ws(Kseg, Dp, B * C)}, 'obj_span': {seg, tn_regions(NRp, Dp)},
            'x_word': {seg, rows_ws(Kseg, Dp, B * L)}, 'obj_word': {seg, tn_regions(NRp, Dp)}}


def max_expect(B, L, R, D, mode):
    return {'forward': {scorer(mode, pad16(D), pad16(B * R), B * n_cells(L))}, 'sum_h': set(),
            'obj_span': {'region_max_bwd_obj(nchunk %d)' % nchunk(B)}}


def chart_expect(R):
    return {'%s<%d>' % (k, nrw(R)) for k in ('cell_attend_fwd', 'cell_attend_bwd', 'obj_grad_reduce')}


# ------------------------------------------------------------------ the inventory
_CT = (5, 4, 2, 1)
NAMEABLE = frozenset(['rows_gemm_ws<%d,%d,%d>' % (ct, sc, w) for ct in _CT for sc in _CT for w in (8, 4)] +
                     ['rows_gemm_ws3<%d,%d,%d>' % (ct, w, k) for ct in _CT for w in (8, 4) for k in (25, 0)] +
                     ['tn_gemm(ij)<%d,%d,nocolsum>' % (ti, tj) for ti in (4, 2, 1) for tj in _CT] +
                     ['%s<%d>' % (k, n) for k in ('cell_attend_fwd', 'cell_attend_bwd', 'obj_grad_reduce') for n in (9, 16)] +
                     ['region_max_bwd_obj(nchunk %d)' % n for n in range(1, 9)] +
                     ['region_segments(one)', 'region_segments(several x*)'])


def _inventory():
    """Every instance some admissible shape takes, by running the rules above over B <= 128, L <= 64, R <= 64, D <= 512.  A launch's row
    count enters through the eight-wave threshold alone, which is monotone in it: the fewest rows (L 1, and the fewest sentences that
    give the NRp) and the most (L 64, the most sentences) decide which of the two a (NRp, Dp) can take."""
    inv = set()
    batches = {}
    for B in range(1, MAX_B + 1):
        inv.add('region_max_bwd_obj(nchunk %d)' % nchunk(B))
        for R in range(1, MAX_R + 1):
            lo, hi = batches.get(pad16(B * R), (B, B))
            batches[pad16(B * R)] = (min(lo, B), max(hi, B))
            inv |= chart_expect(R)
    for NRp, (lo, hi) in batches.items():
        for Dp in range(16, MAX_D + 1, 16):
            Kseg, nseg = region_segments(NRp, Dp)
            inv.add('region_segments(one)' if nseg == 1 else 'region_segments(several x*)')
            inv.add(tn_regions(NRp, Dp))
            for nrows in (lo, hi * n_cells(MAX_L)):                  # B L at L 1 = B C at L 1; B C at L 64 >= B L at L 64
                inv |= {rows_ws(Dp, NRp, nrows), rows_ws3(Dp, NRp, nrows), rows_ws(Kseg, Dp, nrows)}
    return frozenset(inv)


INVENTORY = _inventory()

# What the dispatchers can name or do that no admissible shape takes, and why.  Every nameable INSTANCE is reached (NAMEABLE == INVENTORY:
# test_vl_cases_cpu.py); what is left are three branches of the launchers.  Nothing here is tested.
NOT_REACHED = {
    'launch_scorer: rows_gemm_ws for all_atten in split-bf16 mode (ldo != Dp)': 'every caller passes the region matrix with row stride Dp, in place or as its packed copy',
    'launch_rows / launch_rows3: "weight block does not fit LDS"': 'CT 1 fits whenever 16 Kseg floats are within 150 KiB, Kseg <= 2400: the forward has Kseg = Dp <= 512 '
                                                                   '(image stride <= 520), the backward a Kseg that region_segments sized for the same CT',
    'region_segments: the fall-through to segments of 16 behind the loop': 'the loop\'s last n = NRp / 16 gives segments of 16, which fit (5 x 16 x 16 floats): the split into '
                                                                           'segments of 16 (NRp / 16 prime, case seg31) is taken inside the loop',
}

# ------------------------------------------------------------------ the cases


def _score(B, L, R, D, seed, what):
    return dict(kind='score', B=B, L=L, R=R, D=D, seed=seed, what=what)


def _max(B, L, R, D, seed, what, half=False, skew=False):
    return dict(kind='max', B=B, L=L, R=R, D=D, seed=seed, what=what, half=half, skew=skew)


def _chart(D, R, B, L, seed, what, share=True, training=True):
    return dict(kind='chart', B=B, L=L, R=R, D=D, seed=seed, what=what, share=share, training=training)


def _contr(B, L, seed, what, lengths=None, margin=0.5, alpha=0.7):
    return dict(kind='contrastive', B=B, L=L, seed=seed, what=what, lengths=lengths, margin=margin, alpha=alpha)


# Seeds: the first from the case's starting number onward that holds the seed rules (test_vl_cases_cpu.py).
CASES = {
    # ---- dense scorers: tile shapes.  NRp in {64, 32, 16 or 48, 80} (CT / TI 4, 2, 1 and CT 5) x Dp in {80, 64, 32, 16 or 48} (SC / TJ 5, 4, 2, 1);
    #      'in place': B R and D multiples of 16 (no packed copy of the region matrix); R % 4 == 0: the vector store and one atomic per four regions
    'tile_64x80': _score(2, 3, 32, 80, 100, 'in place, R % 4 == 0'),
    'tile_64x64': _score(4, 3, 15, 64, 110, 'packed copy (B R = 60), R % 4 != 0'),
    'tile_64x32': _score(2, 4, 32, 32, 120, 'in place'),
    'tile_64x16': _score(4, 2, 16, 16, 130, 'in place'),
    'tile_32x80': _score(2, 3, 16, 75, 140, 'padded D 75: every operand through its padded copy'),
    'tile_32x64': _score(3, 3, 9, 64, 150, 'packed copy (B R = 27), R % 4 != 0'),
    'tile_32x32': _score(7, 2, 4, 32, 160, 'packed copy (B R = 28) with R % 4 == 0: the vector paths beside the pad columns'),
    'tile_32x48': _score(2, 4, 16, 48, 170, 'in place'),
    'tile_16x80': _score(3, 3, 5, 80, 180, 'packed copy (B R = 15)'),
    'tile_48x64': _score(3, 2, 16, 64, 190, 'in place, NRp 48'),
    'tile_48x32': _score(2, 3, 22, 32, 200, 'packed copy (B R = 44)'),
    'tile_48x16': _score(8, 2, 6, 16, 205, 'in place with R % 4 != 0 (B R = 48): the scalar stores without a packed copy'),
    'tile_16x33': _score(3, 4, 5, 33, 210, 'padded D 33 (Dp 48)'),
    'tile_80x80': _score(2, 3, 40, 80, 220, 'in place, CT 5 over the regions'),
    'tile_80x64': _score(5, 2, 15, 64, 230, 'packed copy (B R = 75)'),
    'tile_80x32': _score(2, 2, 40, 32, 240, 'in place'),
    'tile_80x16': _score(5, 3, 16, 16, 250, 'in place'),
    'pad260': _score(3, 3, 7, 260, 260, 'padded D 260 (Dp 272, 17 tiles)'),
    # ---- segments of the region axis
    'seg2': _score(8, 2, 64, 80, 300, 'NRp 512: 5 x 16 x 512 floats are above 150 KiB -> two segments of 256'),
    'seg31': _score(8, 2, 61, 80, 310, 'NRp 496 = 31 x 16: no divisor but 31 -> 31 segments of 16'),
    # ---- eight waves (more than 1536 row tiles x column blocks)
    'waves8': _score(24, 12, 36, 16, 400, '117 row tiles x 27 column blocks'),
    'waves8_1x2': _score(3, 24, 6, 432, 410, 'backward: 57 row tiles x 27 column blocks, SC 2'),
    'waves8_2x2': _score(2, 52, 10, 288, 420, 'backward: 173 row tiles x 9 column blocks'),
    'waves8_2x4': _score(24, 45, 1, 64, 430, 'one region per image; 1553 row tiles, forward <2,4,8> and backward <4,2,8>'),
    'waves8_2x5': _score(24, 45, 1, 80, 440, 'forward <2,5,8> and backward <5,2,8>'),
    'waves8_4x5': _score(25, 45, 2, 80, 450, 'forward <4,5,8> and backward <5,4,8>'),
    # ---- the unrolled split-bf16 kernel (K16 25 at D 400)
    'k16': _score(2, 3, 36, 400, 500, 'NRp 80: rows_gemm_ws3<5,4,25>'),
    'k16_ct1': _score(1, 2, 3, 400, 510, 'one sentence (no negatives), NRp 16'),
    'k16_ct2': _score(2, 2, 10, 400, 520, 'NRp 32'),
    'k16_ct4': _score(2, 2, 32, 400, 530, 'NRp 64'),
    # ---- region max: forward values and indices, backward through the arg max
    'max_b5': _max(5, 3, 6, 48, 600, 'nchunk 2'),
    'max_b17': _max(17, 2, 3, 33, 610, 'nchunk 5; the second 16-image round of region_max_bwd_rows; padded D'),
    'max_b33': _max(33, 2, 4, 16, 620, 'nchunk 7 (chunks of 5 sentences); the third round of images'),
    'max_l11': _max(3, 11, 5, 260, 630, 'C 66: the second 64-span block of region_max_bwd_obj; nchunk 1; the second float4 column (Dp 272)'),
    'max_ballot': _max(2, 5, 3, 33, 640, 'one region wins more than four spans of a sentence: the ballot loop', skew=True),
    'max_half': _max(4, 4, 7, 64, 650, 'a cotangent that is zero on the second half of the spans: the live / hit skips', half=True),
    'max_k16': _max(2, 3, 36, 400, 660, 'rows_gemm_ws3<5,4,25> into the key epilogue; R % 4 == 0: one atomic per four regions'),
    'max_seg': _max(8, 2, 64, 80, 670, 'in place, NRp 512'),
    'max_b10': _max(10, 2, 3, 16, 680, 'nchunk 3'),
    'max_b13': _max(13, 2, 3, 16, 690, 'nchunk 4'),
    'max_b21': _max(21, 2, 3, 16, 700, 'nchunk 6'),
    'max_b29': _max(29, 2, 3, 16, 710, 'nchunk 8'),
    # (eight waves into the key epilogue: no dense tensor, so these are the cheap way to the remaining eight-wave instances)
    'max_w8_1x1': _max(29, 4, 48, 16, 720, 'rows_gemm_ws<1,1,8> / rows_gemm_ws3<1,8,0>'),
    'max_w8_4x1': _max(29, 12, 24, 16, 730, 'rows_gemm_ws<4,1,8> / rows_gemm_ws3<4,8,0>'),
    'max_w8_5x1': _max(20, 12, 64, 16, 740, 'rows_gemm_ws<5,1,8> / rows_gemm_ws3<5,8,0>'),
    'max_w8_1x4': _max(25, 6, 30, 64, 750, 'rows_gemm_ws<1,4,8>'),
    'max_w8_1x5': _max(25, 6, 30, 80, 760, 'rows_gemm_ws<1,5,8>'),
    'max_w8_4x4': _max(29, 12, 24, 64, 770, 'rows_gemm_ws<4,4,8>'),
    'max_w8_5x5': _max(29, 12, 30, 80, 780, 'rows_gemm_ws<5,5,8>'),
    'max_w8_k16_ct1': _max(25, 6, 30, 400, 790, 'rows_gemm_ws3<1,8,25>'),
    'max_w8_k16_ct2': _max(22, 14, 16, 400, 800, 'rows_gemm_ws3<2,8,25>: NRp 352 = 11 blocks x 145 row tiles'),
    'max_w8_k16_ct4': _max(24, 18, 16, 400, 810, 'rows_gemm_ws3<4,8,25>: NRp 384 = 6 blocks x 257 row tiles'),
    'max_w8_k16_ct5': _max(25, 20, 16, 400, 820, 'rows_gemm_ws3<5,8,25>: NRp 400 = 5 blocks x 329 row tiles'),
    # ---- contrastive loss
    'con_l64': _contr(3, 64, 900, 'C / 2 = 1040 partial sums: the tail of contrastive_finish behind its 1024 LDS slots'),
    'con_b1': _contr(1, 5, 910, 'one sentence: no negatives, the loss and every gradient are zero'),
    'con_c1': _contr(4, 1, 920, 'C 1: no span enters (nb 0), only the finish kernel runs'),
    'con_b128': _contr(128, 3, 931, 'the largest batch'),
    'con_ragged': _contr(3, 46, 940, 'the ragged entry at C 1081 > 1024, two lengths', lengths=(46, 19, 46)),
    # ---- attention and obj_grad_reduce: chart cases with a fixed dropout mask.  NRW 9 for R <= 36, 16 above
    'att_272x37': _chart(272, 37, 2, 3, 1000, 'R 37: the first R of the 16-register block; the second float4 column live'),
    'att_512x64': _chart(512, 64, 2, 3, 1010, 'the widest row and every region register'),
    'att_400x36': _chart(400, 36, 2, 4, 1020, 'R 36: the last R of the 9-register block'),
    'att_260x63': _chart(260, 63, 3, 3, 1031, 'Dp != D with the second float4 column live: the scalar tail; the last wave one region short'),
    'att_33x3': _chart(33, 3, 3, 4, 1040, 'fewer regions than waves'),
    'att_48x35': _chart(48, 35, 2, 4, 1050, 'R 35: the last wave one region short of 9'),
    'att_16x2': _chart(16, 2, 3, 3, 1060, 'two regions, one float4 per four lanes'),
    'att_l2': _chart(33, 3, 2, 2, 1070, 'C 3: the fourth quarter of obj_grad_reduce is empty'),
    'att_l8': _chart(16, 2, 2, 8, 1080, 'C 36: 9 cells per quarter, a partial block of eight cells in flight'),
    'att_unshared': _chart(48, 35, 2, 3, 1090, 'unshared weights', share=False),
    'att_eval': _chart(272, 37, 2, 3, 1100, 'eval mode: no dropout; vg_atten through all_atten and unit(x_word)', training=False),
}


def expect(name, mode):
    """call -> the entries that call must leave in the record ('forward', or the one input that wants a gradient; a chart case: 'step')"""
    c = CASES[name]
    if c['kind'] == 'score':
        return score_expect(c['B'], c['L'], c['R'], c['D'], mode)
    if c['kind'] == 'max':
        return max_expect(c['B'], c['L'], c['R'], c['D'], mode)
    if c['kind'] == 'chart':
        return {'step': chart_expect(c['R'])}
    return {}


def all_expected():
    out = set()
    for name in CASES:
        for mode in MODES:
            for s in expect(name, mode).values():
                out |= s
    return out


def matches(entry, pattern):
    return entry == pattern or fnmatch.fnmatchcase(entry, pattern)


# ------------------------------------------------------------------ inputs and references (fp64 and, for the error yardstick, fp32)
_ORACLE = {}
SCORE_GRADS = ('sum_h', 'obj_span', 'x_word', 'obj_word')       # sum_h: d inside_h = d outside_h, the gradient of their sum
CHART_OUTS = ('inside_h', 'inside_c', 'inside_s', 'outside_h', 'outside_s', 'all_atten_score', 'vg_atten_score')
CHART_COTS = ('inside_h', 'inside_s', 'outside_h', 'outside_s', 'all_atten_score', 'vg_atten_score')
CHART_INPUTS = ('x_span', 'x_word', 'obj_span', 'obj_word')


def _gen(seed):
    import torch
    return torch.Generator().manual_seed(seed)


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def _precisions(run):
    """run(dtype) -> dict of tensors, in fp64 and in fp32 on ORACLE_THREADS threads (the fp32 run's summation order follows the thread
    count) -> (the fp64 tensors, per tensor the fp32 run's error quantiles against them)"""
    import torch
    threads = torch.get_num_threads()
    torch.set_num_threads(ORACLE_THREADS)
    try:
        r64, r32 = run(torch.float64), run(torch.float32)
    finally:
        torch.set_num_threads(threads)
    return r64, {k: dist(r32[k], r64[k]) for k in r64}


def score_inputs(c):
    """Chart rows of unit norm, like a chart's; words randn; regions 0.3 randn; a dense cotangent for either score tensor."""
    import torch
    B, L, Rn, D, C = c['B'], c['L'], c['R'], c['D'], n_cells(c['L'])
    g = _gen(c['seed'])
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(inside_h=_unit(rn(B, C, D)), outside_h=_unit(rn(B, C, D)), obj_span=0.3 * rn(B, Rn, D), x_word=rn(B, L, D), obj_word=0.3 * rn(B, Rn, D),
                cot_all=rn(B, B, C, Rn), cot_vg=rn(B, B, L, Rn))


def score_oracle(name, training):
    """-> dict(ref64: all_atten_score, vg_atten_score and the four gradients under both cotangents; fp32_dist)"""
    key = (name, bool(training))
    if key not in _ORACLE:
        import torch
        from oracle import diora_ref as R
        c = CASES[name]
        t = score_inputs(c)

        def run(dt):
            v = {k: x.to(dt) for k, x in t.items()}
            leaf = {k: v[k].clone().requires_grad_(True) for k in ('inside_h', 'obj_span', 'x_word', 'obj_word')}
            all_att = torch.einsum('abx,cdx->acbd', leaf['inside_h'] + v['outside_h'], leaf['obj_span'])
            if training:
                vg = torch.einsum('abx,cdx->acbd', leaf['x_word'], leaf['obj_word'])
            else:
                vg = all_att[:, :, :c['L']] + torch.einsum('abx,cdx->acbd', R.unit_norm(leaf['x_word']), leaf['obj_word'])
            ((all_att * v['cot_all']).sum() + (vg * v['cot_vg']).sum()).backward()
            out = dict(all_atten_score=all_att.detach(), vg_atten_score=vg.detach(), sum_h=leaf['inside_h'].grad)
            out.update({k: leaf[k].grad for k in SCORE_GRADS[1:]})
            for k in SCORE_GRADS:       # (training mode, no path from vg to the chart rows: autograd leaves no gradient; the entry writes zeros)
                if out[k] is None:
                    out[k] = torch.zeros_like(leaf['inside_h' if k == 'sum_h' else k])
            return out
        r64, d32 = _precisions(run)
        _ORACLE[key] = dict(ref64=r64, fp32_dist=d32)
    return _ORACLE[key]


def max_inputs(c):
    """skew: every chart row leans towards one direction u and region 0 of every image is 1.5 u, so that region wins most spans.
    half: the cotangent is zero on the spans from C // 2 on, as under the contrastive loss."""
    import torch
    B, L, Rn, D, C = c['B'], c['L'], c['R'], c['D'], n_cells(c['L'])
    g = _gen(c['seed'])
    rn = lambda *s: torch.randn(*s, generator=g)
    ih, oh, obj, w = rn(B, C, D), rn(B, C, D), 0.3 * rn(B, Rn, D), rn(B, B, C)
    if c['skew']:
        u = _unit(rn(D))
        ih, oh = ih + 0.5 * D ** 0.5 * u, oh + 0.5 * D ** 0.5 * u
        obj[:, 0] = 1.5 * u
    if c['half']:
        w[:, :, C // 2:] = 0.0
    return dict(inside_h=_unit(ih), outside_h=_unit(oh), obj_span=obj, cot=w)


def max_oracle(name):
    """-> dict(val64 (B, B, C), arg64, gap: the fp64 distance between the two best regions (inf at R 1), clearance: four times the fp32
    einsum's largest error against fp64, clear: gap > clearance, fp32_dist of the values, row_norm / obj_norm: the largest row norms)"""
    key = (name, 'max')
    if key not in _ORACLE:
        import torch
        c = CASES[name]
        t = max_inputs(c)
        s = {}
        threads = torch.get_num_threads()
        torch.set_num_threads(ORACLE_THREADS)
        try:
            for dt in (torch.float64, torch.float32):
                s[dt] = torch.einsum('abx,cdx->acbd',t['inside_h'].to(dt) + t['outside_h'].to(dt), t['obj_span'].to(dt))
        finally:
            torch.set_num_threads(threads)
        s64, s32 = s[torch.float64], s[torch.float32]
        clearance = 4.0 * float((s32.double() - s64).abs().max())
        val64, arg64 = s64.max(-1)
        top = s64.topk(min(2, c['R']), -1).values
        gap = top[..., 0] - top[..., 1] if c['R'] > 1 else torch.full_like(val64, float('inf'))
        _ORACLE[key] = dict(val64=val64, arg64=arg64, gap=gap, clearance=clearance, clear=gap > clearance,
                            fp32_dist=dist(s32.max(-1).values, val64),
                            row_norm=float((t['inside_h'].double() + t['outside_h'].double()).norm(dim=-1).max()),
                            obj_norm=float(t['obj_span'].double().norm(dim=-1).max()))
    return _ORACLE[key]


def split_bf16_clearance(o):
    """The index clearance in split-bf16 mode.  That mode rounds both operands of every product to 16 significant bits (a bf16 head plus
    a bf16 tail, relative error 2^-17 each) and drops the tail x tail product (2^-18 of the product): each product is off by at most
    1.25 x 2^-16 of its size, a score by at most that of sum |a_k o_k| <= |a| |o| (Cauchy-Schwarz), and the difference of two scores
    of one row by twice that.  Added to the exact mode's clearance, it is the distance inside which that arithmetic can order two
    regions the other way than fp64."""
    return o['clearance'] + 2.0 * 1.25 * 2.0 ** -16 * o['row_norm'] * o['obj_norm']


def max_backward_ref(name, arg):
    """The backward through the arg max `arg` (B, B, C) -- the device's, which the caller has checked against fp64 outside the clearance;
    inside it either region is a subgradient's: d sum_h[a][b] = sum_c w[a][c][b] O[c][arg[a][c][b]], d obj[c][d] = sum over arg == d of
    w S[a][b].  -> (fp64 gradients, the fp32 run's error quantiles)"""
    import torch
    c = CASES[name]
    t = max_inputs(c)

    def run(dt):
        G = torch.zeros(c['B'], c['B'], n_cells(c['L']), c['R'], dtype=dt).scatter_(-1, arg.long().unsqueeze(-1), t['cot'].to(dt).unsqueeze(-1))
        S, O = t['inside_h'].to(dt) + t['outside_h'].to(dt), t['obj_span'].to(dt)
        return dict(sum_h=torch.einsum('acbd,cdx->abx', G, O), obj_span=torch.einsum('acbd,abx->cdx', G, S))
    return _precisions(run)


def contrastive_inputs(c):
    import torch
    B, C = c['B'], n_cells(c['L'])
    g = _gen(c['seed'])
    return dict(smax=torch.randn(B, B, C, generator=g), inside_s=0.3 * torch.randn(B, C, 1, generator=g), outside_s=0.3 * torch.randn(B, C, 1, generator=g))


CONTRASTIVE_COT = 1.7        # the upstream cotangent of the loss
CONTRASTIVE_FLOOR = 1e-8     # trainer.py:86 min_val


def contrastive_oracle(name):
    """oracle.diora_ref.contrastive_loss (mixed lengths: ragged_vl_train_cases.contrastive_loss_ragged) on the
    region maxima -> dict(ref64: loss and the three gradients under CONTRASTIVE_COT, fp32_dist, hinge_gap: the smallest distance of a
    hinge argument of the fp64 run from the floor, clearance: four times the fp32 arguments' largest error against fp64)"""
    key = (name, 'contrastive')
    if key not in _ORACLE:
        import torch
        from oracle import diora_ref as R
        c = CASES[name]
        t = contrastive_inputs(c)
        B, C = c['B'], n_cells(c['L'])

        def run(dt):
            v = {k: x.to(dt).clone().requires_grad_(True) for k, x in t.items()}
            if c['lengths'] is None:
                loss = R.contrastive_loss(v['inside_s'], v['outside_s'], v['smax'].unsqueeze(-1), c['margin'], c['alpha'], CONTRASTIVE_FLOOR)
            else:
                import ragged_vl_train_cases as RC
                loss = RC.contrastive_loss_ragged(v['inside_s'], v['outside_s'], v['smax'], list(c['lengths']), c['margin'], c['alpha'], CONTRASTIVE_FLOOR)
            loss = loss if torch.is_tensor(loss) else torch.zeros((), dtype=dt)
            if loss.requires_grad:
                (loss * CONTRASTIVE_COT).backward()
            out = dict(loss=loss.detach().reshape(()))
            out.update({k: (x.grad if x.grad is not None else torch.zeros_like(x)) for k, x in v.items()})
            return out
        r64, d32 = _precisions(run)
        # the hinge arguments margin + s[a][c] - s[a][a] and margin + s[a][c] - s[c][c], a != c.  (Every span and sentence: a superset of
        # those that enter the loss)
        args = {}
        for dt in (torch.float64, torch.float32):
            s = t['smax'].to(dt)
            diag = torch.diagonal(s, 0, 0, 1).t()                    # (B, C): s[x][x][b]
            off = ~torch.eye(B, dtype=torch.bool)
            args[dt] = torch.cat([(c['margin'] + s - diag[:, None, :])[off], (c['margin'] + s - diag[None, :, :])[off]]).double()
        a64, a32 = args[torch.float64], args[torch.float32]
        _ORACLE[key] = dict(ref64=r64, fp32_dist=d32, hinge_gap=float((a64 - CONTRASTIVE_FLOOR).abs().min()) if a64.numel() else float('inf'),
                            clearance=4.0 * float((a32 - a64).abs().max()) if a64.numel() else 0.0)
    return _ORACLE[key]


def chart_inputs(c):
    """Parameters of oracle.diora_ref.init_params, words randn, regions 0.3 randn, a fixed dropout mask (B, C, R) of zeros and 1 / 0.9
    (rounded to fp32: it casts to fp64 as it is), and a cotangent for every output in CHART_COTS."""
    import torch
    from oracle import diora_ref as R
    B, L, Rn, D, C = c['B'], c['L'], c['R'], c['D'], n_cells(c['L'])
    P = R.init_params(D, share=c['share'], seed=c['seed'])
    g = _gen(c['seed'] + 1)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = dict(x_span=rn(B, L, D), x_word=rn(B, L, D), obj_span=0.3 * rn(B, Rn, D), obj_word=0.3 * rn(B, Rn, D))
    mask = (torch.rand(B, C, Rn, generator=g) >= 0.1).float() / 0.9
    shapes = dict(inside_h=(B, C, D), inside_s=(B, C, 1), outside_h=(B, C, D), outside_s=(B, C, 1), all_atten_score=(B, B, C, Rn), vg_atten_score=(B, B, L, Rn))
    cot = {k: rn(*shapes[k]) for k in CHART_COTS}
    return P, t, mask, cot


def chart_forward(c, dt, P, t, mask, module=None):
    """oracle.diora_ref.diora_forward of the case at precision dt, its dropout replaced by the mask (training mode; level by level, the
    leaves first).  module: the oracle module to run (dispatch_cases.relu_margin hands in the one it has patched)."""
    from oracle import diora_ref as R
    R = module or R
    L, C = c['L'], n_cells(c['L'])
    off = [C - (L - lv) * (L - lv + 1) // 2 for lv in range(L)] + [C]
    calls = [0]
    m = mask.to(dt)

    def replay(x, p, training):
        i = calls[0]
        calls[0] += 1
        return x * m[:, off[i]:off[i + 1]]
    orig = R.F.dropout
    if c['training']:
        R.F.dropout = replay
    try:
        return R.diora_forward(P, t['x_span'], t['x_word'], t['obj_span'], t['obj_word'], share=c['share'], training=c['training'])
    finally:
        R.F.dropout = orig


def chart_oracle(name):
    """-> dict(ref64: the outputs CHART_OUTS as 'out.<name>' and every gradient (parameters, the four inputs) under the cotangents,
    fp32_dist, seconds)"""
    key = (name, 'chart')
    if key not in _ORACLE:
        import time
        c = CASES[name]
        P, t, mask, cot = chart_inputs(c)
        t0 = time.time()

        def run(dt):
            Pd = {k: v.detach().to(dt).requires_grad_(True) for k, v in P.items()}
            td = {k: v.to(dt).clone().requires_grad_(True) for k, v in t.items()}
            o = chart_forward(c, dt, Pd, td, mask)
            sum((o[k] * cot[k].to(dt)).sum() for k in CHART_COTS).backward()
            out = {'out.' + k: o[k].detach() for k in CHART_OUTS}
            out.update({k: v.grad for k, v in Pd.items() if v.grad is not None})
            out.update({k: v.grad for k, v in td.items()})
            return out
        r64, d32 = _precisions(run)
        _ORACLE[key] = dict(ref64=r64, fp32_dist=d32, seconds=time.time() - t0)
    return _ORACLE[key]


def chart_relu_margin(c):
    """dispatch_cases.relu_margin on the vision-language forward: the region inputs and the dropout mask go in with the words."""
    P, t, mask, _ = chart_inputs(c)
    return DC.relu_margin(c, forward=lambda R: chart_forward(c, __import__('torch').float64, {k: v.double() for k, v in P.items()},
                                                            {k: v.double() for k, v in t.items()}, mask, module=R))


# ------------------------------------------------------------------ the accuracy rules (no constant of their own)
F32_FLOORS = (('q50', 2e-7), ('q99', 2e-6), ('max', 2e-5))       # test_c2_full_size_gradients_vs_fp64's floors


def over_bound(hip, o32, ref64, mode):
    """Measured error over its bound.  f32 mode: the quantiles q50 / q99 / max (dist) over three times the fp32 oracle's plus the
    floors; split-bf16 mode: conftest.grad_check(full_size=False) -- median 5e-4, q99 1e-2 (from 1000 elements), max 5e-2 of max(1, scale)."""
    if mode == 'f32':
        return max(hip[q] / (3.0 * o32[q] + fl) for q, fl in F32_FLOORS)
    sc = max(1e-30, float(ref64.abs().max()))
    rel = sc / max(1.0, sc)
    return max(hip['q50'] * rel / 5e-4, hip['q99'] * rel / 1e-2 if ref64.numel() >= 1000 else 0.0, hip['max'] * rel / 5e-2)


def cases_of(entry):
    """The cases (and the call of each) that expect an inventory entry, in either mode."""
    out = []
    for name in sorted(CASES):
        for mode in MODES:
            for call, s in expect(name, mode).items():
                if any(matches(x, entry) for x in s) and (name, call) not in out:
                    out.append((name, call))
    return out


if __name__ == '__main__':          # python tests/vl_cases.py: every inventory entry with the cases that expect it
    for e in sorted(INVENTORY):
        print('%-34s %s' % (e, ', '.join('%s/%s' % nc for nc in cases_of(e))))
    for k, why in NOT_REACHED.items():
        print('not reached: %s -- %s' % (k, why))
