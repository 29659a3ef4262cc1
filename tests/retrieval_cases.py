"""Shared cases of the retrieval tests (tests/test_retrieval_cpu.py, tests/test_gpu_retrieval.py): the reference-made fixture's two
logits as MaxSim problems, hand-made score matrices for the ranks and the top-k, and the grouped random operands of the GPU tests."""
import numpy as np

NAN, INF = float('nan'), float('inf')

# ---- the reference's logits as MaxSim problems -------------------------------------------------------------------------------------
TOKEN_COUNTS = (0, 1, 15, 16, 17, 64, 65, 130)           # per caption, mixed in one call
REGION_COUNTS = (1, 15, 16, 17, 36, 64, 100, 256)        # per image, mixed
WIDTHS = (1, 31, 32, 33, 50, 100, 800)


def unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-8)          # utils.py:12-14


def fixture_problem(g, which):
    """cliora_small.npz as (q, q_off, w, keys, k_off, want (B, B)): which = 'train' (cliora.py:460: Q = x_word, O = obj_word) or 'eval'
    (cliora.py:463-464: Q = [(inside_h + outside_h)[leaves] | unit(x_word)], O = [obj_span | obj_word]); want = the reference's
    vg_atten_score.max(-1).sum(-1) / L (trainer.py:145-152), computed in fp64 from the recorded fp32 scores."""
    x_word, obj_word, obj_span = (g[k].astype(np.float64) for k in ('x_word', 'obj_word', 'obj_span'))
    B, L, D = x_word.shape
    R = obj_word.shape[1]
    if which == 'train':
        q, keys = x_word, obj_word
    else:
        h = g['eval__inside_h'].astype(np.float64)[:, :L] + g['eval__outside_h'].astype(np.float64)[:, :L]
        q, keys = np.concatenate([h, unit(x_word)], -1), np.concatenate([obj_span, obj_word], -1)
    want = g[which + '__vg_atten_score'].astype(np.float64).max(-1).sum(-1) / L
    q_off = [L * b for b in range(B + 1)]
    k_off = [R * b for b in range(B + 1)]
    return q.reshape(B * L, -1), q_off, np.full(B * L, 1.0 / L), keys.reshape(B * R, -1), k_off, want


# ---- hand-made score matrices ------------------------------------------------------------------------------------------------------
def rank_cases():
    """name -> (S (N, M), image_of (N))."""
    rs = np.random.RandomState(5)
    cases = {}
    # exact ties: row 0 ties its own image with an earlier and a later one; column 1 ties captions of both kinds
    cases['ties'] = (np.array([[1.0, 1.0, 1.0, 0.5],
                               [0.5, 2.0, 2.0, 2.0],
                               [2.0, 2.0, 0.0, -0.0],
                               [0.0, 2.0, -0.0, 0.0]]), np.array([1, 1, 3, 2]))
    # five captions per image, as Flickr30k / COCO pair them
    S = rs.randn(15, 3)
    cases['five_per_image'] = (S, np.repeat(np.arange(3), 5))
    # a NaN row (a caption whose token was NaN) and NaN entries elsewhere, with infinities
    S = rs.randn(6, 4)
    S[2, :] = NAN
    S[0, 1], S[4, 3], S[5, 0], S[1, 2] = NAN, -INF, INF, -INF
    cases['nan_row'] = (S, np.array([0, 1, 2, 3, 3, 0]))
    # image 2 has no caption; caption 3 names an image that does not exist
    S = rs.randn(5, 4)
    cases['image_without_captions'] = (S, np.array([0, 1, 3, 7, 0]))
    return cases


def duplicated_columns_case():
    """A random 37 x 23 matrix with duplicated columns (exact ties across images) and duplicated rows."""
    rs = np.random.RandomState(11)
    S = rs.randn(37, 23).astype(np.float32).astype(np.float64)
    S[:, 5], S[:, 17], S[:, 22] = S[:, 2], S[:, 2], S[:, 9]
    S[30], S[8] = S[3], S[3]
    return S, rs.randint(0, 23, size=37)


# ---- grouped random operands ---------------------------------------------------------------------------------------------------------
def grouped_problem(D, token_counts, region_counts, seed, scale=1.0, sign=None):
    """-> (q (NT, D), q_off, w (NT), keys (MR, D), k_off) fp32 / host lists.  Rows are unit vectors times `scale`; w = 1 / len.
    sign = 'negative': Q <= 0 and O >= 0 elementwise, so every true score is negative (or zero)."""
    rs = np.random.RandomState(seed)
    NT, MR = int(sum(token_counts)), int(sum(region_counts))
    q, keys = rs.randn(NT, D), rs.randn(MR, D)
    if sign == 'negative':
        q, keys = -np.abs(q), np.abs(keys)
    q = scale * q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-8)
    keys = scale * keys / np.maximum(np.linalg.norm(keys, axis=1, keepdims=True), 1e-8)
    q_off = np.concatenate([[0], np.cumsum(token_counts)]).astype(np.int64).tolist()
    k_off = np.concatenate([[0], np.cumsum(region_counts)]).astype(np.int64).tolist()
    w = np.concatenate([np.full(n, 1.0 / n) for n in token_counts if n] + [np.zeros(0)])
    return q.astype(np.float32), q_off, w.astype(np.float32), keys.astype(np.float32), k_off


def error_scale(q, q_off, w, keys, k_off):
    """(N, M) fp64: sum_t |w_t| |Q_t| max_r |O_r| per (caption, image) -- what the per-product bound of the kernel's arithmetic is
    scaled by (the error of a maximum is at most the largest error of its candidates, that of the weighted sum their weighted sum)."""
    q, keys, w = (np.asarray(a, dtype=np.float64) for a in (q, keys, w))
    qn, kn = np.linalg.norm(q, axis=1), np.linalg.norm(keys, axis=1)
    N, M = len(q_off) - 1, len(k_off) - 1
    a = np.array([(np.abs(w[q_off[n]:q_off[n + 1]]) * qn[q_off[n]:q_off[n + 1]]).sum() for n in range(N)])
    b = np.array([kn[k_off[m]:k_off[m + 1]].max() if k_off[m + 1] > k_off[m] else 0.0 for m in range(M)])
    return a[:, None] * b[None, :]
