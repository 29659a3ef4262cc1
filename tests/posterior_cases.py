"""Shared by test_posterior_cpu.py and test_gpu_posterior.py (not a test module): enumeration of every binary tree, seeded inputs, the
bounds of cliora_span_posteriors and the figures measured on the MI355X.

The yardsticks: enumeration of every binary tree (n <= 7) for ``posterior_numpy``; ``posterior_numpy`` in fp64 on the device's own
per-split scores for the kernel's marginals and log_z; ``mbr_numpy`` on the device's own marginals (bitwise) and the fp64 MBR tree
of the oracle's scores (seeded away from near-ties) for the kernel's trees.
"""
import functools

import numpy as np
import torch

from oracle import diora_ref as R

# The project's forward bound on a tensor of scale 1 (DESIGN.md sections 13, 14): max |mu - mu64| <= BOUND; |log_z - log_z64| <=
# BOUND * max(1, |log_z64|); |sum of mu over internal cells - (n - 1)| <= n * BOUND.
BOUND = 1e-4
GPU_LENGTHS = (1, 2, 3, 7, 13, 64, 65, 128)
GPU_B, GPU_D, GPU_SEED = 3, 16, 6203
# L -> (max |mu - mu64|, max |log_z - log_z64| / max(1, |log_z64|)) on the MI355X (text-only DioraMLP, D 16, B 3, random N(0, 1)
# weights), as test_gpu_posterior.py prints them.  Not taken yet: the kernel's tables are fp64, so what is
# expected is the fp32 rounding of the two outputs (6e-8 of mu, 6e-8 of log_z relative).  EMULATED_F32_TABLES: the same recursions
# with fp32 tables in numpy on N(0, 0.5^2) random scores, L -> max |mu - mu64| -- a host figure, the only one behind the choice.
MEASURED = {}
EMULATED_F32_TABLES = {13: 1.6e-7, 64: 3.8e-6, 128: 7.6e-6}

# ---- MBR end to end ---------------------------------------------------------------------------------------------------------------
# L 12, D 50, 4 sentences; a seed is kept only if, in fp64 on the oracle's scores, the two best MBR candidates of every cell with a
# choice differ by at least 2 (n - 1) BOUND: the bound times the number of mu terms a candidate sums.
MBR_L, MBR_D, MBR_PARAM_SEED = 12, 50, 8111
MBR_GAP = 2 * (MBR_L - 1) * BOUND
MBR_SEEDS = [0, 4, 6, 7]           # mbr_seed_search(): the first four of seeds 0 .. 99 that keep the gap
MBR_MEASURED_MIN_GAP = 2.313e-3    # smallest fp64 gap over the seeded sentences (seed 0); MBR_GAP is 2.2e-3

# ---- mixed lengths ----------------------------------------------------------------------------------------------------------------
# One padded chart of L 14 (D 16) against each sentence alone at its exact length.  The trees are compared too, so RAGGED_SEED is the
# first of 0 .. 99 at which every sentence keeps, in fp64 on the oracle's scores, the gap of the end-to-end test for its own length.
RAGGED_L, RAGGED_LENGTHS = 14, [1, 2, 14, 9, 5]
RAGGED_SEED = 1                    # sentences sentence(GPU_D, n, 1000 * RAGGED_SEED + b), parameters of MBR_PARAM_SEED
LONG_RAGGED_L, LONG_RAGGED_LENGTHS = 70, [70, 66, 3]


def params(D, seed):
    return R.init_params(D, share=True, seed=seed)


def sentence(D, L, seed):
    return torch.randn(L, D, generator=torch.Generator().manual_seed(seed))


def batch(D, L, B, seed):
    return torch.stack([sentence(D, L, seed + 1 + b) for b in range(B)])


def text_module(P, D):
    """cliora_amd.diora.DioraMLP with the oracle's parameters, on the CPU (the caller moves it)."""
    from cliora_amd.diora import DioraMLP
    m = DioraMLP(D, outside=True, normalize='unit', compress=False, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P['inside_' + k[len('outside_'):] if k.startswith('outside_') else k].detach().clone()
    m.load_state_dict(sd)
    return m


def random_scores(B, L, seed, scale=2.0):
    """{level: (B, L - level, level)} fp32 N(0, scale^2) per-split scores."""
    rs = np.random.RandomState(seed)
    return {level: (scale * rs.randn(B, L - level, level)).astype(np.float32) for level in range(1, L)}


# ---- enumeration ------------------------------------------------------------------------------------------------------------------
def all_trees(n):
    """Every binary tree over n words as a tuple of its internal nodes (level, pos, split): Catalan(n - 1) of them."""
    @functools.lru_cache(maxsize=None)
    def build(level, pos):
        if level == 0:
            return ((),)
        out = []
        for k in range(level):
            for left in build(k, pos):
                for right in build(level - k - 1, pos + k + 1):
                    out.append(left + right + ((level, pos, k),))
        return tuple(out)
    return build(n - 1, 0)


def enumerate_posteriors(pair_s, b, n):
    """fp64 by enumeration: -> ({(level, pos): mu} over the sentence's triangle, log_z, trees, their probabilities)."""
    r = {}
    for level in range(1, n):
        s = np.asarray(pair_s[level][b], dtype=np.float64).reshape(-1, level)
        for pos in range(n - level):
            r[(level, pos)] = s[pos] - s[pos].max()
    trees = all_trees(n)
    w = np.array([sum(r[(lv, p)][k] for lv, p, k in t) for t in trees], dtype=np.float64)
    m = w.max()
    log_z = m + np.log(np.exp(w - m).sum())
    prob = np.exp(w - log_z)
    mu = {(0, p): 1.0 for p in range(n)}
    for level in range(1, n):
        for pos in range(n - level):
            mu[(level, pos)] = float(sum(pr for t, pr in zip(trees, prob) if any(lv == level and p == pos for lv, p, _ in t)))
    return mu, float(log_z), trees, prob


def tree_spans(tree):
    """Internal nodes (children before parents, as all_trees builds them) -> [(start, end)]."""
    return [(p, p + lv) for lv, p, _ in tree]


# ---- fp64 MBR and its candidate gap ---------------------------------------------------------------------------------------------------
def mbr_fp64(mu_row, n, L):
    """MBR of one sentence in fp64: -> (spans, children before parents; smallest gap between the two best candidates over the cells
    with a choice, inf when there is none)."""
    from cliora_amd.posterior import cell_id
    val = {(0, p): 0.0 for p in range(n)}
    bp, gap = {}, float('inf')
    for level in range(1, n):
        for pos in range(n - level):
            cand = np.array([val[(k, pos)] + val[(level - k - 1, pos + k + 1)] for k in range(level)])
            k = int(np.argmax(cand))
            if level > 1:
                top = np.sort(cand)[::-1]
                gap = min(gap, float(top[0] - top[1]))
            val[(level, pos)] = cand[k] + float(mu_row[cell_id(L, level, pos)])
            bp[(level, pos)] = k
    spans = []

    def walk(level, pos):
        if level == 0:
            return
        k = bp[(level, pos)]
        walk(k, pos)
        walk(level - k - 1, pos + k + 1)
        spans.append((pos, pos + level))
    walk(n - 1, 0)
    return spans, gap


@functools.lru_cache(maxsize=None)
def mbr_oracle(seed, L=MBR_L, D=MBR_D):
    """One sentence of `seed` through the fp64 oracle: -> (fp64 MBR spans, the smallest candidate gap)."""
    from cliora_amd.posterior import posterior_numpy
    P = {k: v.double() for k, v in params(D, MBR_PARAM_SEED).items()}
    x = sentence(D, L, seed)[None].double()
    with torch.no_grad():
        o = R.diora_forward(P, x, outside=False, normalize='unit', share=True, keep_pairs=True)
    pair_s = {lv: s.numpy()[..., 0] for lv, s in o['pair_s_in'].items()}
    mu, _ = posterior_numpy(pair_s, [L], L)
    return mbr_fp64(mu[0], L, L)


def ragged_sentences(seed=None):
    seed = RAGGED_SEED if seed is None else seed
    return [sentence(GPU_D, n, 1000 * seed + b) for b, n in enumerate(RAGGED_LENGTHS)]


def ragged_seed_keeps_the_gap(seed):
    return all(mbr_oracle(1000 * seed + b, n, GPU_D)[1] >= 2 * (n - 1) * BOUND for b, n in enumerate(RAGGED_LENGTHS))


def padded(xs, L, seed=99):
    """(B, L, D): every sentence padded on the right with N(0, 1) rows (no cell of the sentence reads them)."""
    out = torch.randn(len(xs), L, xs[0].shape[1], generator=torch.Generator().manual_seed(seed))
    for b, x in enumerate(xs):
        out[b, :x.shape[0]] = x
    return out


def mbr_seed_search(count=4, first=100):
    """The first `count` of seeds 0 .. first - 1 whose sentence keeps MBR_GAP (fewer if there are fewer)."""
    keep = []
    for seed in range(first):
        if mbr_oracle(seed)[1] >= MBR_GAP:
            keep.append(seed)
            if len(keep) == count:
                break
    return keep
