"""Shared by test_ragged_long_cpu.py and test_gpu_ragged_long.py (not a test module): both passes of mixed-length batches whose padded
chart is longer than 64 words (cliora_chart_forward_ragged_wide) -- seeded inputs, the oracle they are checked
against, and the figures measured on the MI355X.

The yardstick of every comparison is the oracle (oracle/diora_ref.py, pinned to the reference's goldens) run in fp64 on ONE sentence
at its exact length (ragged_outside_cases.exact / oracle_atten); for the bitwise claims it is an existing entry of the library.  It is
never the code under test.
"""
import functools

import numpy as np
import torch

import ragged_outside_cases as ROC

FORWARD_BOUND = ROC.FORWARD_BOUND          # 1e-4, the project's: |got - want| <= FORWARD_BOUND * max(1, |want|) on every own cell
REGIONS = 36

# ---- parity with the fp64 oracle at the exact length ------------------------------------------------------------------------------
# name -> (CLIORA plan, D, lengths, seed).  The smallest shapes at which the two-word root-level mask can go wrong:
#   d16:    root levels 64 and 63, the word boundary; the sentence of 66 words is the chart's own root and is not seeded
#   d50:    D 50 is padded to Dp 64 (the un-pad copy); level 126 is the top bit of word 1, 127 the chart's own root
#   d400:   the flagship width
#   cliora: 36 regions, atten_score[b, :n]
PARITY = {
    'd16': (False, 16, [66, 65, 64, 1, 2, 33], 8101),
    'd50': (False, 50, [128, 127, 66, 65, 64, 1], 8102),
    'd400': (False, 400, [70, 65, 9], 8103),
    'cliora': (True, 50, [97, 65, 64, 3, 80], 8104),
}
CHARTS = ('inside_h', 'outside_h', 'outside_s', 'atten_score')
# Largest errors measured on the MI355X, |got - want| / max(1, |want|) over every own cell, per chart of PARITY and arithmetic mode
# (split-bf16 'bf16x3' / exact-product 'f32').  All inside FORWARD_BOUND, which is kept.
MEASURED = {
    ('d16', 'bf16x3'): dict(inside_h=1.54e-5, outside_h=1.32e-5, outside_s=1.44e-5),
    ('d16', 'f32'): dict(inside_h=5.2e-7, outside_h=8.8e-7, outside_s=7.8e-7),
    ('d50', 'bf16x3'): dict(inside_h=4.5e-6, outside_h=3.9e-6, outside_s=1.19e-5),
    ('d50', 'f32'): dict(inside_h=3.5e-7, outside_h=3.8e-7, outside_s=7.2e-7),
    ('d400', 'bf16x3'): dict(inside_h=1.7e-6, outside_h=1.3e-6, outside_s=2.23e-5),
    ('d400', 'f32'): dict(inside_h=6.3e-7, outside_h=1.4e-7, outside_s=2.9e-6),
    ('cliora', 'bf16x3'): dict(inside_h=5.5e-6, outside_h=3.2e-6, outside_s=1.05e-5, atten_score=3.21e-5),
    ('cliora', 'f32'): dict(inside_h=2.7e-7, outside_h=5.7e-7, outside_s=1.0e-6, atten_score=1.7e-6),
}
MEASURED_WORST = 3.21e-5          # atten_score of the CLIORA plan in split-bf16 mode: a third of the bound

# The oracle check of the masking scheme at a padded L of 65 (fp32 masked_outside against fp64 exact): measured on the CPU.
SCHEME_CASE = (16, [65, 64, 1, 2, 33], 8110)
MEASURED_SCHEME_ERR = 2.2e-6


def parity_case(name):
    """-> (vl, D, P, xs, lengths, vl_inputs or None)."""
    vl, D, lengths, seed = PARITY[name]
    P, xs, lengths = ROC.small_case(D, lengths, seed=seed)
    return vl, D, P, xs, lengths, (ROC.vl_inputs(D, lengths, REGIONS, seed=seed) if vl else None)


@functools.lru_cache(maxsize=None)
def parity_oracle(name):
    """Per sentence the fp64 charts of the oracle at the exact length, computed once for both arithmetic modes: a list of dicts of
    double tensors (inside_h, outside_h, outside_s, and atten_score for the CLIORA plan)."""
    vl, D, P, xs, lengths, vli = parity_case(name)
    out = []
    for b in range(len(lengths)):
        o = ROC.exact(P, xs[b], vl=vli[b] if vl else None)
        out.append({k: o[k][0] for k in CHARTS if k in o and (vl or k != 'atten_score')})
    return out


# ---- all lengths equal: bitwise the uniform forward on the sequential schedule -------------------------------------------------------
EQUAL_LENGTHS = (65, 128)
EQUAL_B = 2

# ---- the wide entry on a short plan: bitwise cliora_chart_forward_ragged with the same mask in word 0 ---------------------------------
SHORT_CASE = (50, [14, 1, 2, 3, 5, 8, 9, 11, 13, 14, 6], 211)

# ---- bad lengths at L 65 -------------------------------------------------------------------------------------------------------------
BAD_CASE = (16, [65, 3, 64, 17, 1, 40, 65, 9], 8120)        # sentences 1 and 5 become n = 0 and n = 66
BAD_AT = {1: 0, 5: 66}

# ---- end to end (evaluate_ragged / embed_phrases_ragged with max_len = 128) -----------------------------------------------------------
E2E_LENGTHS = [70, 9, 65, 30, 3, 100, 64, 17, 128, 66]
E2E_SEED = 5
E2E_MAX_BATCH = 4
# A phrase is decided by two rows of the exact-length atten_score: the word maxima over the phrase and the regions of its chosen
# word.  The GPU test excuses no phrase; that is sound iff on the fp64 oracle no such row has its two best entries within
# 2 * FORWARD_BOUND of the scale (an error the parity check allows on each of the two entries).  Measured on the oracle: 28 phrases,
# smallest gap 8.4e-3 of the scale, 42 times that.
E2E_TIE = 2 * FORWARD_BOUND
E2E_PHRASES = 28
MEASURED_E2E_MIN_GAP = 8.4e-3
EMBED_LENGTHS = [70, 9, 65, 3, 2, 1]
EMBED_SEED = 9
MEASURED_EMBED_DIFF = 9.8e-7      # worst relative difference of embed_phrases_ragged's vectors to the exact-length rows, on the MI355X


def e2e_examples(lengths=None, seed=E2E_SEED):
    return ROC.examples(E2E_LENGTHS if lengths is None else lengths, seed=seed)


def phrases_of(ex):
    """(start, end) of an example's phrases, end exclusive, in the order evaluate.Targets reads them."""
    return [(int(a[0]), int(a[1])) for a in ex['VG_GT'][0].values()]


def decisive_gaps(att, phrases):
    """Per phrase the smaller of the two gaps that decide it, as a fraction of the scale max(1, max |atten_score|): between the two
    largest word maxima over the phrase (inf for a phrase of one word) and between the two best regions of its chosen word."""
    att = np.asarray(att, dtype=np.float64)
    scale = max(1.0, float(np.abs(att).max()))
    out = []
    for s, e in phrases:
        m = np.sort(att[s:e].max(1))[::-1]
        r = np.sort(att[s + int(np.argmax(att[s:e].max(1)))])[::-1]
        out.append(min(m[0] - m[1] if len(m) > 1 else np.inf, r[0] - r[1]) / scale)
    return out


# ---- the memory cap of a pack topped by a long sentence ------------------------------------------------------------------------------
CAP_LENGTHS = [128] * 5 + [10] * 5
CAP = 2


def pack_seeded_lengths(seed=3, n=200):
    """Lengths 1..128, about a tenth of them above 64."""
    rs = np.random.RandomState(seed)
    return [int(rs.randint(65, 129)) if rs.rand() < 0.1 else int(rs.randint(1, 65)) for _ in range(n)]


def text_net(D=16, V=97, E=32, seed=11):
    from cliora_amd.harness import build_net
    torch.manual_seed(seed)
    return build_net(D, torch.nn.Embedding(V, E), obj_feats=False)
