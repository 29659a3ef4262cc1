"""Shared by test_ragged_outside_cpu.py and test_gpu_ragged_outside.py (not a test module): the masked outside pass of a padded chart
restated from the oracle's pieces, and seeded vision-language inputs.

The yardstick of every comparison is the oracle (oracle/diora_ref.py, pinned to the reference's goldens) run on ONE sentence at its
exact length, never the code under test.
"""
import numpy as np
import torch

from oracle import chart_layout as CL
from oracle import diora_ref as R

MASKED = -1e30          # what cliora_chart_forward_ragged writes into inside_s beyond a sentence's triangle
# The project's forward bound (README.md / VERDICT.md; tests/test_gpu_ragged.py applies it to encode_ragged): |got - want| <=
# FORWARD_BOUND * max(1, |want|) on every cell of every sentence's own triangle.
FORWARD_BOUND = 1e-4
# Largest such errors measured on the MI355X (split-bf16 mode; the counterpart of
# ragged_cases.MEASURED_INSIDE_S_DIFF): all inside the bound, which is kept.
MEASURED_OUTSIDE_H_DIFF = 6.2e-6         # D 50; D 400: 1.5e-6
MEASURED_OUTSIDE_S_DIFF = 3.2e-5         # CLIORA plan, D 50; text-only D 50: 2.5e-5, D 400: 1.9e-5
MEASURED_ATTEN_SCORE_DIFF = 2.8e-5       # CLIORA plan, D 50, R 36


def own_cells(L, n):
    """Cell ids, in a chart of length L, of the triangle of a sentence of length n, in the order of a chart of length n."""
    off = CL.level_offsets(L)
    return np.concatenate([np.arange(int(off[lv]), int(off[lv]) + n - lv) for lv in range(n)])


def masked_outside(P, padded, lengths, normalize='unit', share=True):
    """The schedule of cliora_chart_forward_ragged on the oracle's pieces.  padded: diora_forward(..., outside=False) of the
    right-padded batch (its inside charts are read, inside_s is masked in a copy).  -> (outside_h, outside_s) of the padded chart."""
    ih, ins = padded['inside_h'], padded['inside_s'].clone()
    B, C, D = ih.shape
    L = int(round((np.sqrt(8 * C + 1) - 1) / 2))
    nrm = R._normalizer(normalize)
    W = R._side(P, 'outside', share)
    off = CL.level_offsets(L)
    for b, n in enumerate(lengths):                       # 1. the mask
        for level in range(L):
            o = int(off[level])
            for pos in range(L - level):
                if pos + level >= n:
                    ins[b, o + pos] = MASKED
    oh = torch.zeros_like(ih)
    os_ = torch.zeros_like(ins)
    root = nrm(P['root_vector_out_h'].to(ih.dtype).view(1, 1, D).expand(B, 1, D))
    oh[:, -1:] = root
    for level in range(L - 2, -1, -1):
        Lc = L - level
        pidx, sidx = map(R._idx, CL.outside_pairs(L, level))
        par_h, sib_h = oh.index_select(1, pidx).view(-1, D), ih.index_select(1, sidx).view(-1, D)
        par_s, sib_s = os_.index_select(1, pidx).view(-1, 1), ins.index_select(1, sidx).view(-1, 1)
        ph, _ = R.compose_mlp(W, sib_h, par_h)
        s = (R.bilinear(W['M'], sib_h, par_h) + sib_s + par_s).view(B, -1, Lc, 1)
        p = torch.softmax(s, dim=1)
        N = s.shape[1]
        o = int(off[level])
        oh[:, o:o + Lc] = nrm(torch.sum(ph.view(B, N, Lc, -1) * p, 1))
        os_[:, o:o + Lc] = torch.sum(s * p, 1)
        for b, n in enumerate(lengths):                   # 2. the root overwrite, after its level
            if n - 1 == level:
                oh[b, o] = oh[b, C - 1]
                os_[b, o] = os_[b, C - 1]
    return oh, os_


def cast(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def exact(P, x, normalize='unit', share=True, dtype=torch.float64, vl=None):
    """The oracle on one sentence at its exact length.  vl: (x_word (n, D), obj_span (R, D), obj_word (R, D)) for the CLIORA variant."""
    kw = {}
    if vl is not None:
        kw = dict(x_word=vl[0][None].to(dtype), obj_span=vl[1][None].to(dtype), obj_word=vl[2][None].to(dtype))
    with torch.no_grad():
        return R.diora_forward(cast(P, dtype), x[None].to(dtype), outside=True, normalize=normalize, share=share, **kw)


def small_case(D, lengths, seed, share=True, scale=1.0):
    """Seeded parameters (scaled: normalize = 'none' keeps the charts in fp32 range only with small weights) and sentences."""
    P = {k: v * scale for k, v in R.init_params(D, share=share, seed=seed).items()}
    xs = [torch.randn(n, D, generator=torch.Generator().manual_seed(seed + 1 + i)) for i, n in enumerate(lengths)]
    return P, xs, list(lengths)


def vl_inputs(D, lengths, Rn, seed):
    """Per sentence (x_word (n, D), obj_span (R, D), obj_word (R, D)), seeded N(0, 1)."""
    out = []
    for i, n in enumerate(lengths):
        g = torch.Generator().manual_seed(seed + 1000 + i)
        out.append((torch.randn(n, D, generator=g), torch.randn(Rn, D, generator=g), torch.randn(Rn, D, generator=g)))
    return out


def padded(xs, Lmax, seed=99):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(len(xs), Lmax, xs[0].shape[1], generator=g)
    for b, x in enumerate(xs):
        out[b, :x.shape[0]] = x
    return out


# ---- end-to-end inputs (evaluate_ragged / embed_phrases_ragged): a seeded CLIORA net and examples of many lengths -------------
E2E_LENGTHS = [9, 3, 30, 4, 17, 9, 24, 3, 25, 12, 6, 33, 5, 21, 9, 7, 38, 14, 11, 40, 8, 19, 3, 27, 15, 10, 22, 36, 13, 5, 29, 16, 4, 31,
               18, 20, 7, 12, 26, 23]


def vl_net(D=50, V=97, E=32, img=64, seed=11):
    """harness.Net with image regions, on the CPU (the caller moves it)."""
    from cliora_amd.harness import build_net
    torch.manual_seed(seed)
    net = build_net(D, torch.nn.Embedding(V, E), obj_feats=True, img_dim=img)
    for p in net.img_encoder.parameters():          # built as zeros: every region score would tie
        p.data.normal_(0.0, 0.2)
    return net


def examples(lengths, V=97, Rn=36, img=64, seed=5):
    rs = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(lengths):
        xy = torch.randint(0, 300, (Rn, 2), generator=gen).float()
        wh = torch.randint(1, 150, (Rn, 2), generator=gen).float()
        boxes = torch.cat([xy, xy + wh], -1)
        target = {}
        for j in range(rs.randint(1, 5)):
            s = rs.randint(0, n)
            e = rs.randint(s + 1, n + 1)
            bx = boxes[rs.randint(0, Rn)].tolist()
            target[j] = (s, e, [bx[0], bx[1], bx[2] + float(rs.randint(0, 40)), bx[3]])
        gold = []
        for _ in range(rs.randint(0, n)):
            s = rs.randint(0, n - 1)
            gold.append((s, rs.randint(s + 1, n)))
        out.append(dict(sentence=rs.randint(1, V, size=n).tolist(), example_id='ex%d' % i, GT=gold + [(0, n - 1)], VG_GT=(target, None),
                        boxes=boxes, obj_feats=torch.randn(Rn, img, generator=gen)))
    return out


def near_tie_phrases(att, phrases):
    """Indices of the phrases (start, end) whose decisive rows of the exact-length atten_score (n, R) have their two best entries
    within the measured padded-vs-exact difference: the word maxima over the phrase, the regions of its chosen word."""
    att = np.asarray(att, dtype=np.float64)
    tol = MEASURED_ATTEN_SCORE_DIFF * max(1.0, float(np.abs(att).max()))
    out = []
    for k, (s, e) in enumerate(phrases):
        m = np.sort(att[s:e].max(1))[::-1]
        r = np.sort(att[s + int(np.argmax(att[s:e].max(1)))])[::-1]
        if (len(m) > 1 and m[0] - m[1] <= tol) or r[0] - r[1] <= tol:
            out.append(k)
    return out


def oracle_atten(net, ex, dtype=torch.float64):
    """atten_score (n, R) of one example at its exact length on the oracle, from a CPU harness.Net's parameters (eval mode)."""
    sd = {k: v.detach().to(dtype) for k, v in net.state_dict().items()}
    P = {k[len('diora.'):]: v for k, v in sd.items() if k.startswith('diora.')}
    tokens = torch.tensor([ex['sentence']])
    x_span, x_word = R.embed_forward(sd['embed.embeddings.weight'], sd['embed.mat'], sd['embed.mat1'], tokens)
    o_span, o_word = R.image_encoder_forward(sd['img_encoder.fc.weight'], sd['img_encoder.fc.bias'], sd['img_encoder.fc_vis.weight'],
                                             sd['img_encoder.fc_vis.bias'], ex['obj_feats'][None].to(dtype))
    with torch.no_grad():
        out = R.diora_forward(P, x_span, x_word, o_span, o_word, outside=True, normalize=net.diora.normalize, share=net.diora.share)
    return out['atten_score'][0].numpy()
