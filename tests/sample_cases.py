"""Shared by test_sample_cpu.py and test_gpu_sample.py (not a test module): the yardsticks of the tree sampler (cliora_amd/sample.py,
cliora_sample_trees), its pinned cases and the figures measured for it.

The yardstick chain: enumeration of every binary tree in fp64 (posterior_cases.all_trees) for ``sample_numpy``; ``sample_numpy`` on the
device's own per-split scores, spans bit for bit, for the kernel -- never the code under test against itself.
"""
import math

import numpy as np

import posterior_cases as PC

CATALAN = [1, 1, 2, 5, 14, 42, 132, 429]             # Catalan(n - 1) at index n - 1: the trees of n = 1 .. 8 words
BETAS = (0.0, 0.5, 1.0)

# A sample may differ between two correct fp64 evaluations only where a decision's u c_{N-1} lies within rounding of some c_k.  fp64
# exp / log are within a few ulp; over 127 levels of al <= 176 that moves a probability by about 4e-12 relative, so 1e-9 sits about 250
# times over it, and a decision falls inside it with probability about 2e-9.  Every pinned host case keeps margin >= MARGIN (asserted);
# a device sample below it may be left out of the bitwise comparison, at most MAX_EXCUSED per test.
MARGIN = 1e-9
MAX_EXCUSED = 1

# ---- sample_numpy against enumeration -------------------------------------------------------------------------------------------------
# n = 1 .. 7, seeds 0 .. 2, scores random_scores(1, max(n, 2), 100 n + seed): the product of the conditional split probabilities of
# every tree against exp(beta sum r - log_z) of the enumeration, 1e-12 relative; log_z to 1e-12 of max(1, |log_z|).
ENUM_SEEDS = range(3)
ENUM_RTOL = 1e-12

# ---- frequencies ----------------------------------------------------------------------------------------------------------------------
# n = 5 (14 trees), scores random_scores(1, 5, score seed, scale 0.5), FREQ_S samples: (score seed, beta, draw seed).  The scale keeps
# the rarest tree's probability above 25 / FREQ_S (asserted per case), and each case is one for which every tree's frequency and every
# cell's span frequency lies within FREQ_SIGMAS binomial standard deviations sqrt(p (1 - p) / S) of its enumerated value: a condition
# on pinned inputs, deterministic on the host.  freq_seed_search() found them: the first draw seed from 0 that keeps it, per (score
# seed, beta) -- each was the first one tried.  FREQ_S is a power of two, so the float32 shares of span_frequencies are exact.
FREQ_N, FREQ_S, FREQ_SCALE, FREQ_SIGMAS, FREQ_MIN_COUNT = 5, 4096, 0.5, 5.0, 25
FREQ_CASES = [(3, 1.0, 0), (4, 1.0, 0), (3, 0.5, 0), (5, 0.0, 0)]

# ---- draws ----------------------------------------------------------------------------------------------------------------------------
# Chunking, ids and padding on the host: the padded chart of posterior_cases' mixed lengths with random scores.
DRAW_SCORE_SEED, DRAW_SEED, DRAW_S = 4242, 0x1234567890abcdef, 8

# ---- the device -----------------------------------------------------------------------------------------------------------------------
GPU_LENGTHS = (1, 2, 3, 7, 13)
GPU_S = 64
GPU_LONG = ((65, 16), (128, 8))                      # (L, S): the long instance, two splits per lane
GPU_SEED = 0x5eed5a3b1e5
BOUND = PC.BOUND                                     # |log_prob - fp64| and |log_z - fp64|: the project's bound, 1e-4
# Printed by test_gpu_sample.py on the MI355X (text-only DioraMLP, D 16, B 3, beta 1, S as above): L -> (max |log_prob - log_prob64|,
# max |log_z - log_z64|, samples left out, the restatement's smallest margin).  The errors are the fp32 rounding of the two outputs
# (half an ulp of 53 is 1.9e-6); no sample of any test was left out.
MEASURED = {1: (0.0, 0.0, 0, float('inf')), 2: (0.0, 0.0, 0, 1.006e-2), 3: (1.146e-7, 1.104e-8, 0, 6.847e-5),
            7: (2.310e-7, 9.693e-8, 0, 2.833e-5), 13: (4.638e-7, 1.956e-7, 0, 4.326e-5), 65: (3.753e-6, 1.372e-6, 0, 7.509e-6),
            128: (7.321e-6, 3.696e-6, 0, 1.845e-6)}
# The same at L 13 / beta 0.5: 4.768e-7, 3.503e-7; L 6 / beta 0: 8.806e-8 both; the padded L 14 chart: 4.503e-7, 2.053e-7; the TreeLSTM
# plan at L 5: 1.187e-7, 5.907e-8; max |log_prob - KBest.log_prob| at L 5: 4.768e-7.


def enum_scores(n, seed):
    return PC.random_scores(1, max(n, 2), 100 * n + seed)


def freq_scores(seed):
    return PC.random_scores(1, FREQ_N, seed, scale=FREQ_SCALE)


def enumerate_trees(pair_s, b, n, beta):
    """fp64 by enumeration under beta r: -> (trees, their log-probabilities, log_z, {(level, pos): r row})."""
    r = {}
    for level in range(1, n):
        s = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)
        for pos in range(n - level):
            r[(level, pos)] = s[pos] - s[pos].max()
    trees = PC.all_trees(n)
    w = np.array([sum(beta * r[(lv, p)][k] for lv, p, k in t) for t in trees], dtype=np.float64)
    m = w.max()
    log_z = float(m + np.log(np.exp(w - m).sum()))
    return trees, w - log_z, log_z, r


def span_key(rows):
    """A sample's span rows -> the tuple of its real ones (what posterior_cases.tree_spans gives for a tree)."""
    return tuple((int(s), int(e)) for s, e in rows if s >= 0)


def tree_index(trees):
    return {tuple(PC.tree_spans(t)): i for i, t in enumerate(trees)}


def frequencies_hold(score_seed, beta, draw_seed):
    """-> (every tree and every cell within FREQ_SIGMAS deviations, the rarest tree's expected count, the smallest margin)."""
    from cliora_amd.posterior import cell_id
    from cliora_amd.sample import sample_numpy, span_frequencies
    n, S = FREQ_N, FREQ_S
    pair_s = freq_scores(score_seed)
    trees, logp, _, _ = enumerate_trees(pair_s, 0, n, beta)
    p = np.exp(logp)
    spans, _, _, margin = sample_numpy(pair_s, [n], S, draw_seed, beta=beta)
    index = tree_index(trees)
    got = np.bincount([index[span_key(rows)] for rows in spans[0].tolist()], minlength=len(trees)) / float(S)
    ok = bool((np.abs(got - p) <= FREQ_SIGMAS * np.sqrt(p * (1 - p) / S)).all())
    freq = span_frequencies(spans, n)[0]
    ok = ok and freq[cell_id(n, n - 1, 0)] == 1.0        # the root: in every tree, no deviation to allow
    for level in range(1, n - 1):
        for pos in range(n - level):
            mu = float(sum(pr for t, pr in zip(trees, p) if any(lv == level and q == pos for lv, q, _ in t)))
            ok = ok and abs(freq[cell_id(n, level, pos)] - mu) <= FREQ_SIGMAS * math.sqrt(max(mu * (1 - mu), 0.0) / S)
    return ok, float(p.min() * S), float(margin.min())


def freq_seed_search(pairs=((3, 1.0), (4, 1.0), (3, 0.5), (5, 0.0)), first=20):
    """Per (score seed, beta) the first draw seed of 0 .. first - 1 that keeps the frequency condition and the margin."""
    out = []
    for score_seed, beta in pairs:
        for draw_seed in range(first):
            ok, _, margin = frequencies_hold(score_seed, beta, draw_seed)
            if ok and margin >= MARGIN:
                out.append((score_seed, beta, draw_seed))
                break
    return out
