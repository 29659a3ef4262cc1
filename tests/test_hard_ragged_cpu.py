"""Hard (S-DIORA) charts of mixed lengths in one padded chart, without a GPU: the facts the device code rests on
-- the pair numbering by brute force over the plan's tables, the masked padded hard chart against the per-sentence hard chart in fp64
(charts, selections, gradients) -- the span walk on the host, the margins and ReLU clearances the GPU cases rely on, the refusals
that need no GPU and the new symbols.  Cases and bounds: hard_ragged_cases.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import hard_ragged_cases as RC
import ragged_outside_cases as ROC
import ragged_train_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cells(L):
    """(level, pos) of every cell id of a chart of length L."""
    from cliora_amd.hard import level_offsets
    off = level_offsets(L)
    lvl, pos = np.zeros(L * (L + 1) // 2, dtype=np.int64), np.zeros(L * (L + 1) // 2, dtype=np.int64)
    for lv in range(L):
        lvl[off[lv]:off[lv] + L - lv], pos[off[lv]:off[lv] + L - lv] = lv, np.arange(L - lv)
    return lvl, pos


def _outside_pair_spans(L):
    """{level: (Lc, N, 4) int64}: (sibling start, sibling end, parent start, parent end) of every outside pair, in the plan's order."""
    from cliora_amd.hard import _pair_tables
    lvl, pos = _cells(L)
    out = {}
    for level, (a, b) in _pair_tables(L)[1]['out'].items():
        a, b = a.numpy(), b.numpy()
        out[level] = np.stack([pos[a], pos[a] + lvl[a], pos[b], pos[b] + lvl[b]], -1)
    return out


def test_outside_pair_numbering_does_not_depend_on_the_chart_length():
    """Fact 3, by brute force over the plan's pair tables for L = 2..40: pair n of cell (lv, pos) is the left sibling [n, pos - 1] for
    n < pos, else the right sibling [pos + lv + 1, lv + 1 + n], with the parent their union -- nothing of L in it; for a sentence of
    n_b words the valid pairs of a cell of its triangle are exactly the first n_b - lv - 1, and they are, pair for pair, those of the
    chart of length n_b."""
    spans = {L: _outside_pair_spans(L) for L in range(2, 41)}
    for L in range(2, 41):
        for level, t in spans[L].items():
            Lc, N = t.shape[:2]
            p = np.arange(Lc)[:, None].repeat(N, 1)
            n = np.arange(N)[None, :].repeat(Lc, 0)
            left = n < p
            assert np.array_equal(t[..., 0], np.where(left, n, p + level + 1)), (L, level)
            assert np.array_equal(t[..., 1], np.where(left, p - 1, level + 1 + n)), (L, level)
            assert np.array_equal(t[..., 2], np.where(left, n, p)), (L, level)
            assert np.array_equal(t[..., 3], np.where(left, p + level, level + 1 + n)), (L, level)
            for nb in range(level + 1, L + 1):           # sentences whose triangle holds cells of this level: positions 0 .. nb - level - 1
                own = t[:nb - level]
                valid = (own[..., 1] < nb) & (own[..., 3] < nb)
                assert np.array_equal(valid, n[:nb - level] < nb - level - 1), (L, level, nb)
                if nb - level - 1 > 0:
                    assert np.array_equal(own[:, :nb - level - 1], spans[nb][level]), (L, level, nb)


def _cpu_case(k):
    D, lengths, share, normalize, scale = RC.CPU_CASES[k]
    P, xs, _ = ROC.small_case(D, lengths, seed=700 + k, share=share, scale=scale)
    L = max(lengths)
    return D, lengths, L, share, normalize, P, ROC.padded(xs, L)


@pytest.mark.parametrize('k', range(len(RC.CPU_CASES)))
def test_masked_padded_hard_chart_is_the_per_sentence_hard_chart(k):
    """Facts 1, 2 and 4 in fp64: the hard inside pass of the padded batch, the -1e30 mask, the hard outside pass with the root seeds --
    every cell at the one-hot of its own first maximum -- against hard_forward_torch on each sentence alone: the charts on the own
    triangles, the selections everywhere, and the autograd gradients of a weighted loss, within CPU_BOUND; d x_span beyond a sentence
    is exactly 0."""
    from cliora_amd.hard import hard_forward_ragged_torch
    D, lengths, L, share, normalize, P, xp = _cpu_case(k)
    assert {1, 2, L} <= set(lengths) and len(set(lengths)) < len(lengths)
    own = RC.own(L, lengths)
    W = TC.weights(L, lengths, D, seed=19)
    res = {}
    for which in ('padded', 'exact'):
        Pd = {n: v.detach().double().requires_grad_(True) for n, v in P.items()}
        xd = xp.detach().double().requires_grad_(True)
        o = (RC.masked_hard_padded(Pd, xd, lengths, share, normalize) if which == 'padded'
             else hard_forward_ragged_torch(Pd, xd, lengths, share, normalize))
        RC.weighted_loss([o[c] for c in RC.CHARTS], W, own).backward()
        res[which] = (o, {n: v.grad for n, v in Pd.items()}, xd.grad)
    (got, g_got, dx_got), (want, g_want, dx_want) = res['padded'], res['exact']
    assert torch.equal(got['sel_in'], want['sel_in']) and torch.equal(got['sel_out'], want['sel_out'])
    assert int((want['sel_in'] >= 0).sum()) == sum(n * (n - 1) // 2 for n in lengths)
    for c in RC.CHARTS:
        have, ref = got[c].detach()[own], want[c].detach()[own]
        err = float(((have - ref).abs() / ref.abs().clamp(min=1.0)).max())
        print(c, err)
        assert err <= RC.CPU_BOUND, (c, err)
        assert bool(torch.isnan(want[c].detach()[~own]).all())
    assert sorted(g_got) == sorted(g_want)
    moved = 0
    for n in g_want:
        assert (g_got[n] is None) == (g_want[n] is None), n
        if g_want[n] is None:
            continue
        err = TC.rel_err(g_got[n], g_want[n])
        print(n, err)
        assert err <= RC.CPU_BOUND, (n, err)
        moved += int(float(g_want[n].abs().max()) > 1e-2)
    assert moved >= 3
    assert TC.rel_err(dx_got, dx_want) <= RC.CPU_BOUND
    for b, n in enumerate(lengths):
        assert not dx_got[b, n:].any() and not dx_want[b, n:].any(), (b, n)


def test_teacher_forcing_with_the_padded_selection_re_rows_it():
    """hard_forward_ragged_torch under its own padded selection is itself, and under a perturbed one it follows the perturbation."""
    from cliora_amd.hard import hard_forward_ragged_torch, level_offsets
    D, lengths, L, share, normalize, P, xp = _cpu_case(0)
    with torch.no_grad():
        free = hard_forward_ragged_torch(P, xp, lengths, share, normalize)
        tf = hard_forward_ragged_torch(P, xp, lengths, share, normalize, selection=(free['sel_in'], free['sel_out']))
    own = RC.own(L, lengths)
    for c in RC.CHARTS:
        assert torch.equal(free[c][own], tf[c][own]), c
    assert torch.equal(free['sel_in'], tf['sel_in']) and torch.equal(free['sel_out'], tf['sel_out'])
    b = lengths.index(L)
    forced = free['sel_in'].clone()
    root = level_offsets(L)[L - 1]
    forced[b, root] = (forced[b, root] + 1) % (L - 1)
    with torch.no_grad():
        other = hard_forward_ragged_torch(P, xp, lengths, share, normalize, selection=(forced, free['sel_out']))
    assert int(other['sel_in'][b, root]) == int(forced[b, root]) and not torch.equal(other['inside_h'][b, root], free['inside_h'][b, root])


def test_hard_spans_ragged_numpy():
    """Against trees built directly from the selections, sentence by sentence; the layout of cliora_cky_spans_ragged."""
    from cliora_amd.diora import DioraBase
    from cliora_amd.hard import hard_spans_numpy, hard_spans_ragged_numpy, level_offsets
    for L in (1, 2, 5, 9):
        C = L * (L + 1) // 2
        off = level_offsets(L)
        rng = np.random.RandomState(L)
        lengths = [L, 1] + [int(v) for v in rng.randint(1, L + 1, size=4)]
        sel = np.full((len(lengths), C), -1, dtype=np.int32)
        for level in range(1, L):
            sel[:, off[level]:off[level] + L - level] = rng.randint(0, level, size=(len(lengths), L - level))

        def build(b, level, pos):
            if level == 0:
                return pos
            k = int(sel[b, off[level] + pos])
            return (build(b, k, pos), build(b, level - k - 1, pos + k + 1))
        spans = hard_spans_ragged_numpy(sel, lengths, L)
        assert spans.dtype == np.int32 and spans.shape == (len(lengths), max(L - 1, 0), 2)
        for b, n in enumerate(lengths):
            assert (spans[b, n - 1:] == -1).all()
            assert DioraBase.trees_from_spans(spans[b:b + 1, :n - 1]) == [build(b, n - 1, 0)]
            if n > 1:
                assert spans[b, n - 2].tolist() == [0, n - 1]
        assert np.array_equal(hard_spans_ragged_numpy(sel, [L] * len(lengths), L), hard_spans_numpy(sel, L))
        bad = hard_spans_ragged_numpy(sel[:2], [0, L + 1], L)
        assert (bad == -1).all()


@pytest.mark.parametrize('name', sorted(RC.GPU_CASES))
def test_case_margins_and_relu_clearance(name):
    """What the GPU cases rely on, in the per-sentence fp64 restatement: the ReLU clearance by hard_cases' rule, and on a clear case
    every cell of every own triangle MARGIN_REL * max|inside_s| ahead of its second-best split."""
    c = RC.case(name)
    r = c['ref']
    print('%s: relu margin (selected pairs) %.3g, (every pair) %.3g; smallest selection margin / max|inside_s| %.3g'
          % (name, r['relu_margin'], r['relu_margin_all'], min(r['margin_rel'])))
    assert r['relu_margin'] >= RC.RELU_MARGIN, r['relu_margin']
    if name not in RC.SELECTED_PAIRS_ONLY:
        assert r['relu_margin_all'] >= RC.RELU_MARGIN, r['relu_margin_all']
    if c['clear']:
        assert min(r['margin_rel']) >= RC.MARGIN_REL, r['margin_rel']
    if c['ties']:
        assert int(r['sel_in'].max()) == 0 and int(r['sel_out'].max()) == 0
    own = RC.own(c['L'], c['lengths'])
    assert bool((r['sel_in'][~own] == -1).all()) and bool((r['sel_out'][~own] == -1).all())


def test_refusals_that_need_no_gpu():
    from cliora_amd import harness as H
    from cliora_amd import ragged
    from cliora_amd.diora import DioraMLP
    from cliora_amd.evaluate import evaluate_ragged
    x = torch.zeros(2, 4, 16)
    for slot in ('_ragged', '_ragged_train'):            # the old slots still refuse a hard module
        m = DioraMLP(16, hard=True)
        m.__dict__[slot] = (torch.zeros(2, dtype=torch.int32), 8)
        with pytest.raises(NotImplementedError, match='hard=True.*mixed lengths'):
            m(x, x)
    for slot in ('_ragged_hard', '_ragged_hard_train'):  # ... and the new ones a soft module
        m = DioraMLP(16)
        assert m.__dict__[slot] is None
        m.__dict__[slot] = (torch.zeros(2, dtype=torch.int32), 8)
        with pytest.raises(NotImplementedError, match='_ragged_hard'):
            m(x, x)
    with pytest.raises(ValueError):
        ragged.decode_entry('hard')
    soft = H.build_net(16, torch.nn.Embedding(11, 16), k_neg=3)
    ex = [dict(sentence=[1, 2, 3, 4], example_id='a', GT=[(0, 1), (0, 3)])]
    with pytest.raises(ValueError, match="decode='hard' needs a hard chart module"):
        evaluate_ragged(soft, ex, [str(i) for i in range(11)], decode='hard')
    with pytest.raises(ValueError, match='hard chart module'):
        ragged.parse_ragged_hard(soft, [[1, 2, 3]])
    with pytest.raises(Exception, match='not a hard chart'):
        DioraMLP(16).hard_spans(lengths=torch.ones(2, dtype=torch.int32))


def _refused(plan, flags=1, sel=True, lengths=True, root_levels=(0, 0), status=True, null_plan=False, null_params=False,
             null_mask=False, **params):
    """cliora_chart_forward_ragged_hard on host-only dummies (nothing is dereferenced before the refusals) -> (return code, message)."""
    from cliora_amd import _lib
    buf = np.zeros(16, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    fields = {n: p.value for n in ('leaf_w', 'leaf_b', 'in_w1', 'in_b1', 'in_w2', 'in_b2', 'in_mat', 'root_h')}
    fields.update({k: (p.value if v else None) for k, v in params.items()})
    pst = _lib.Params(*[fields.get(n) for n in _lib.PARAM_FIELDS])
    s = p if sel else None
    mask = (ctypes.c_uint64 * 2)(*root_levels)
    rc = _lib.lib().cliora_chart_forward_ragged_hard(None if null_plan else plan.handle, None if null_params else ctypes.byref(pst), p, p, p,
                                                     p, p, s, s, p, 0, flags, p if lengths else None, None if null_mask else mask,
                                                     p if status else None, None)
    return rc, _lib.fn('cliora_last_error')().decode()


def test_symbols_and_refusals_through_the_c_abi():
    """The new symbols are declared, exported and bound; every refusal of cliora_chart_forward_ragged_hard comes before any launch
    (there is no GPU here), with CLIORA_EINVAL and a message of its own that starts with the entry's name."""
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert 'int cliora_chart_forward_ragged_hard(cliora_plan* plan, const cliora_params* params, const float* x_span,' in header
    assert 'int cliora_hard_spans_ragged(cliora_plan* plan, const int32_t* sel_in, const int32_t* lengths, int32_t* spans, int32_t* status,' in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'cliora_chart_forward_ragged_hard') and hasattr(raw, 'cliora_hard_spans_ragged')
    fwd, spans = _lib.lib().cliora_chart_forward_ragged_hard, _lib.lib().cliora_hard_spans_ragged
    assert len(fwd.argtypes) == 16 and fwd.restype is ctypes.c_int
    assert len(spans.argtypes) == 6 and spans.restype is ctypes.c_int
    text, long_plan = _lib.Plan(2, 5, 16), _lib.Plan(1, 65, 16, forward_only=True)
    seen = set()
    cases = [(text, dict(null_plan=True), 'NULL argument'), (text, dict(null_params=True), 'NULL argument'),
             (text, dict(lengths=False), 'NULL argument'), (text, dict(null_mask=True), 'NULL argument'),
             (text, dict(status=False), 'NULL argument'),
             (_lib.Plan(2, 5, 16, arch=1), {}, 'TreeLSTM'),
             (_lib.Plan(2, 5, 16, R=4), {}, 'R > 0'),
             (text, dict(root_mat=True), 'compress'),
             (text, dict(flags=1 | _lib.FWD_PAIR_STATES), 'CLIORA_FWD_PAIR_STATES'),
             (long_plan, {}, 'CLIORA_FWD_NO_BACKWARD'),
             (text, dict(sel=False), 'selection'),
             (text, dict(flags=1 | 32), 'flag'),
             (text, dict(root_levels=(1 << 5, 0)), 'root_levels'),
             (text, dict(root_levels=(0, 1)), 'root_levels'),
             (long_plan, dict(flags=1 | _lib.FWD_NO_BACKWARD, root_levels=(0, 1 << 1)), 'root_levels')]
    for plan, kw, words in cases:
        rc, msg = _refused(plan, **kw)
        print(rc, msg)
        assert rc == -1 and msg.startswith('cliora_chart_forward_ragged_hard: ') and words in msg, (rc, msg, words)
        seen.add(msg)
    assert len(seen) == 10                               # NULL argument, TreeLSTM, R > 0, compress, pair states, long, selection, flag, root_levels at L 5 and at L 65
    # bit L - 1 is legal; the long plan with the flag and every accepted flag word get past the entry's own refusals: to the workspace check
    for plan, kw in [(text, dict(root_levels=(1 << 4, 0))), (long_plan, dict(flags=1 | _lib.FWD_NO_BACKWARD, root_levels=(1 << 63, 1))),
                     (text, dict(flags=0)), (text, dict(flags=1 | _lib.FWD_HARD_DENSE)), (text, dict(flags=_lib.FWD_NO_BACKWARD | _lib.FWD_HARD_DENSE))]:
        rc, msg = _refused(plan, **kw)
        assert rc == -3 and 'workspace too small' in msg, (rc, msg)
    # cliora_hard_spans_ragged: NULL arguments
    hs = _lib.lib().cliora_hard_spans_ragged
    buf = np.zeros(16, dtype=np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    for args in [(None, p, p, p, p), (text.handle, None, p, p, p), (text.handle, p, None, p, p), (text.handle, p, p, None, p),
                 (text.handle, p, p, p, None)]:
        assert hs(*args, None) == -1 and _lib.fn('cliora_last_error')().decode().startswith('cliora_hard_spans_ragged: ')
