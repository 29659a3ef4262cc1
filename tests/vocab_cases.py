"""Cases, seeded inputs and bounds of the whole-vocabulary loss tests (tests/test_vocab_cpu.py, tests/test_gpu_vocab.py).

Shapes (T tokens, V words, E columns): the smallest at which the tiling of csrc/vocab_kernels.hpp can go wrong -- T around the MFMA
tile (16) and the workgroup's token tile (64), V around the tile, the 256-word step and its multiples, E around the 32-column chunk,
and one case with several forward key ranges (2048 words each), ten backward ranges (512 words) and three token tile groups."""
import numpy as np

CASES = [
    (1, 1, 1), (15, 16, 1), (15, 2, 31), (16, 15, 32), (17, 16, 33), (63, 17, 50), (64, 255, 100), (65, 256, 300), (130, 257, 32),
    (64, 513, 33), (17, 1000, 50), (130, 1000, 300), (130, 5000, 400), (17, 300, 1324),
]
# the last one: the reference's widest rows (1324), three passes over the output columns in the backward; its own list, since its f32
# tolerance is reasoned separately (grad_tol)
WIDE_GRAD_CASES = [(17, 300, 1324)]
GRAD_CASES = [(15, 2, 31), (17, 16, 33), (63, 17, 50), (65, 256, 300), (130, 257, 32), (64, 513, 33), (130, 5000, 400)] + WIDE_GRAD_CASES

# The project's per-product score bound for unit rows (tests/test_gpu_phrases.py): split-bf16 2e-5, f32 1e-6 growing as sqrt(E / 256).
EPS = {'bf16x3': 2e-5, 'f32': 1e-6}

# Gradients, relative to the largest magnitude of the fp64 gradient of the tensor.  TORCH_F32_GRAD_ERR: per case (T, V, E), the error
# (dQ, dK) of the torch fp32 route (F.cross_entropy(Q @ K.t()) with autograd on the device) against the fp64 analytic gradient, measured
# on an MI355X as tests/test_gpu_vocab.py::test_gradients_against_fp64 prints it.
# Tolerances (grad_tol): the f32 mode gets twice the torch route's error ON THE SAME CASE; the split mode that error plus the score
# bound through p: a logit error delta changes p by the factor exp(+-delta), and the recomputed score and the saved lse each carry
# one, so 2 delta relative on each p, with delta the largest token bound of the case (1.8e-3 ... 5.9e-2 on GRAD_CASES).
# WIDE_GRAD_CASES lie beyond the widths the rule was stated for (E <= 400): a score here is ONE fp32 chain over its E columns (the order
# cliora_knn_ip fixed, which the bitwise target needs), whose error grows as sqrt(E / 256) (EPS above), while torch's GEMM splits
# the sum; their f32 tolerance is the rule times that factor, 2.27 at E = 1324.
# The kernels measured: f32 mode 2.3e-7 ... 6.7e-6, each case within its tolerance (closest: dQ of (17, 16, 33), 2.5e-7 of 3.9e-7);
# split mode 3.5e-6 ... 5.0e-5.
TORCH_F32_GRAD_ERR = {
    (15, 2, 31): (5.157e-7, 5.835e-7), (17, 16, 33): (1.946e-7, 2.496e-7), (63, 17, 50): (7.151e-7, 6.514e-7),
    (65, 256, 300): (5.027e-6, 6.121e-6), (130, 257, 32): (8.860e-7, 1.299e-6), (64, 513, 33): (1.095e-6, 8.817e-7),
    (130, 5000, 400): (5.881e-6, 4.536e-6), (17, 300, 1324): (1.060e-6, 1.069e-6),
}
RANK_CLOSE_CAP = 0.02       # the share of a case's tokens whose target may sit within twice the score bound of another logit


def eps(mode, E):
    return EPS[mode] * (max(1.0, (E / 256.0) ** 0.5) if mode == 'f32' else 1.0)


def make_case(T, V, E, seed=None):
    """-> Q (T, E), K (V, E) float32, tok (T,) int64.  Unit-scale rows: standard normal entries; a token's row leans towards its
    word's (3.5 standard deviations of a logit, 5.5 from 2000 words on), as a trained model's does, which also puts most targets in the thin upper tail of
    their row's logits, where few are within the score bound of a neighbour; a row shorter than 1 is stretched to length 1, so that
    the fp32 spacing of an lse (2.4e-7 below 8, 9.5e-7 below 16) stays under the bound, which is proportional to |Q_t| max |K_v|.
    Targets 0 and V - 1 and a repeated word are always present (T permitting)."""
    rs = np.random.RandomState(1000 * T + 10 * V + E if seed is None else seed)
    K = rs.randn(V, E)
    tok = rs.randint(0, V, size=T).astype(np.int64)
    if T > 0:
        tok[0] = 0
    if T > 1:
        tok[1] = V - 1
    if T > 3:
        tok[3] = tok[2]
    Q = rs.randn(T, E) + (3.5 if V < 2000 else 5.5) * K[tok] / np.sqrt(E)       # more words: a thinner tail for the same share of close logits
    n = np.linalg.norm(Q, axis=1, keepdims=True)
    Q = np.where(n < 1.0, Q / np.maximum(n, 1e-30), Q)
    return Q.astype(np.float32), K.astype(np.float32), tok


def score_bound(mode, Q, K):
    """Per token: the bound on a logit's error, eps x |Q_t| x max_v |K_v|."""
    Q, K = np.asarray(Q, np.float64), np.asarray(K, np.float64)
    return eps(mode, Q.shape[1]) * np.linalg.norm(Q, axis=1) * (np.linalg.norm(K, axis=1).max() if len(K) else 0.0)


def separated(Q, K, tok, mode='bf16x3'):
    """Per token: True when its target's fp64 logit is further than twice the score bound from every other logit of its row."""
    Q64, K64 = np.asarray(Q, np.float64), np.asarray(K, np.float64)
    s = Q64 @ K64.T
    T = len(tok)
    d = np.abs(s - s[np.arange(T), tok][:, None])
    d[np.arange(T), tok] = np.inf
    return d.min(axis=1) > 2.0 * score_bound(mode, Q, K) if K.shape[0] > 1 else np.ones(T, bool)


def grad_tol(mode, Q, K, name, torch_err=None):
    """name: 'dQ' or 'dK'.  torch_err: the torch fp32 route's error on these inputs, for inputs that are no case of the table."""
    T, E = Q.shape
    case = (T, K.shape[0], E)
    if torch_err is None:
        torch_err = TORCH_F32_GRAD_ERR[case][0 if name == 'dQ' else 1]
    if mode == 'f32':
        return 2.0 * torch_err * ((E / 256.0) ** 0.5 if case in WIDE_GRAD_CASES else 1.0)
    return torch_err + 2.0 * float(score_bound(mode, Q, K).max())
