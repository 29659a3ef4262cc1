"""cliora_constrained_parse on the GPU (cliora_amd/constrained.py): the best tree, log_z_c, log_prob and the span posteriors under
required and forbidden brackets.

The yardstick, never the code under test: ``constrained_numpy`` (pinned to enumeration of every binary tree by
test_constrained_cpu.py) on the device's OWN per-split scores, read through cliora_inside_pair_states, so that the comparison isolates
this kernel -- spans and feasibility exact, the sums within the project's bound -- and the project's other decoders on the same chart:
cliora_cky_spans, cliora_span_posteriors, cliora_kbest_spans and cliora_sample_trees.  Cases and measured figures: constrained_cases.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import constrained_cases as CC
import posterior_cases as PC

pytestmark = pytest.mark.gpu

SCALARS = ('score', 'log_z', 'log_z_c', 'log_prob')


def _scores(m):
    """Per-split inside scores of the chart the module just computed, through cliora_inside_pair_states: {level: (B, L - level, level)}."""
    from cliora_amd import _lib
    plan, ws = m._plan, m._wss[0]
    assert len(m._wss) == 1
    wsf = ws.view(torch.float32)
    out = {}
    for level in range(1, plan.L):
        ps, ph, rows, ldh = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.call('cliora_inside_pair_states', plan.handle, C.c_void_p(ws.data_ptr()), level, C.byref(ps), C.byref(ph), C.byref(rows),
                  C.byref(ldh))
        so = (ps.value - ws.data_ptr()) // 4
        out[level] = wsf[so:so + rows.value].view(plan.B, plan.L - level, level).cpu().numpy()
    return out


def _forward(m, x):
    with torch.no_grad():
        m(x, x)


def _parse(m, brackets=None, lengths=None, marginals=True):
    """constrained_parse with host inputs -> dict of numpy arrays (marginals None when not asked for)."""
    from cliora_amd.constrained import constrained_parse
    bt = None if brackets is None else torch.from_numpy(np.ascontiguousarray(brackets, dtype=np.int32))
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    cp = constrained_parse(m, bt, lt, marginals=marginals)
    out = {k: getattr(cp, k).cpu().numpy() for k in ('spans', 'feasible') + SCALARS}
    out['marginals'] = cp.marginals.cpu().numpy() if marginals else None
    out['status'] = cp.status.cpu().tolist()
    return out


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want, what='', rows=None, keys=('spans', 'feasible', 'marginals') + SCALARS):
    for k in keys:
        if got[k] is None or want[k] is None:
            continue
        a, b = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, k)


def _rel(got, want):
    """max |got - want| / max(1, |want|) over the finite entries of want; where want is -inf got is too."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf) and np.isfinite(got[~inf]).all()
    if inf.all():
        return 0.0
    return float((np.abs(got[~inf] - want[~inf]) / np.maximum(1.0, np.abs(want[~inf]))).max())


def _against_numpy(got, scores, lengths, brackets, L, what):
    """The device against constrained_numpy on the device's scores: spans, feasible and status exact; log_z_c, log_prob and log_z
    within BOUND * max(1, |.|); max |mu_c - fp64| <= BOUND with exact 0 on disallowed cells and exact 1 on required ones.
    -> (the three measured maxima, the restatement)."""
    from cliora_amd.constrained import allowed_cells, constrained_numpy
    from cliora_amd.posterior import cell_id
    want = constrained_numpy(scores, lengths, brackets, L=L)
    assert got['status'] == [want.status], what
    assert np.array_equal(got['feasible'], want.feasible), (what, got['feasible'], want.feasible)
    assert got['spans'].dtype == np.int32 and np.array_equal(got['spans'], want.spans), what
    assert np.array_equal(_bits(got['score']), _bits(want.score)), what       # fp32 in the kernel's order: the same bits
    e_lzc, e_lp, e_lz = _rel(got['log_z_c'], want.log_z_c), _rel(got['log_prob'], want.log_prob), _rel(got['log_z'], want.log_z)
    e_mu = float(np.abs(got['marginals'].astype(np.float64) - want.marginals).max())
    print('%s: max |log_z_c - fp64| = %.3e, max |log_prob - fp64| = %.3e (both / max(1, |.|)), max |mu_c - fp64| = %.3e'
          % (what, e_lzc, e_lp, e_mu))
    assert e_lzc <= CC.BOUND and e_lp <= CC.BOUND and e_lz <= CC.BOUND and e_mu <= CC.BOUND, what
    rows = np.zeros((len(lengths), 0, 3), dtype=np.int32) if brackets is None else brackets
    for b, n in enumerate(lengths):
        if not want.feasible[b]:
            assert (got['marginals'][b] == 0).all(), what
            continue
        allowed, required = allowed_cells(n, rows[b])
        for level in range(n):
            for pos in range(n - level):
                mu = got['marginals'][b, cell_id(L, level, pos)]
                if not allowed[level, pos]:
                    assert mu == 0.0, (what, b, level, pos)
                if required[level, pos]:
                    assert mu == 1.0, (what, b, level, pos)
    return (e_lzc, e_lp, e_mu), want


@functools.lru_cache(maxsize=None)
def _uniform(L, B=PC.GPU_B):
    """One eval forward of a text-only DioraMLP (D 16, random weights) at length L and the device's scores -- once per (L, B)."""
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, L, B, PC.GPU_SEED + L).cuda())
    return dict(m=m, scores=_scores(m))


def _rows(sets, M=None):
    return CC.pack_rows(sets, M)


def _nested(n, B, forbidden=()):
    return [[(s, e, 1) for s, e in CC.nested_required(n, b)] + [(s, e, 0) for s, e in forbidden] for b in range(B)]


# ---- 1. no brackets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', CC.GPU_LENGTHS)
def test_no_brackets_is_the_other_decoders_bit_for_bit(L):
    """M = 0 and every row unused: cliora_cky_spans' spans, kbest's rank-0 score, cliora_span_posteriors' log_z and marginals."""
    from cliora_amd.kbest import kbest_spans
    m, B = _uniform(L)['m'], PC.GPU_B
    post = m.span_posteriors()
    log_z, marg = post.log_z.cpu().numpy(), post.marginals.cpu().numpy()
    score = kbest_spans(m, 1).scores.cpu().numpy()[:, 0]
    spans = m.cky_spans_device().cpu().numpy()
    for what, brackets in (('M 0', None), ('unused rows', np.full((B, 4, 3), -1, dtype=np.int32))):
        got = _parse(m, brackets)
        assert got['status'] == [0] and got['feasible'].tolist() == [1] * B, what
        assert got['spans'].shape == (B, L - 1, 2) and np.array_equal(got['spans'], spans), what
        assert np.array_equal(_bits(got['score']), _bits(score)), what
        assert np.array_equal(_bits(got['log_z']), _bits(log_z)) and np.array_equal(_bits(got['log_z_c']), _bits(log_z)), what
        assert np.array_equal(_bits(got['marginals']), _bits(marg)), what
        assert (got['log_prob'] == 0).all() and not np.signbit(got['log_prob']).any(), what


@pytest.mark.parametrize('L', [66, 128])
def test_no_brackets_is_the_other_decoders_bit_for_bit_long(L):
    """The same comparison in a long chart (B 2, D 16): L 66 is the smallest in which a lane carries a second split (level 65) and a
    second use (the leaves' 65), L 128 the plan's limit -- every sentence at L words, then lengths (L, 65)."""
    from cliora_amd.kbest import kbest_spans
    from cliora_amd.ragged import cky_spans_ragged
    B = 2
    m = _uniform(L, B)['m']
    for lengths in (None, [L, 65]):
        what = 'L %d, lengths %r' % (L, lengths)
        lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
        post = m.span_posteriors(lt)
        log_z, marg = post.log_z.cpu().numpy(), post.marginals.cpu().numpy()
        score = kbest_spans(m, 1, lt).scores.cpu().numpy()[:, 0]
        spans = (m.cky_spans_device() if lengths is None else cky_spans_ragged(m, lt)[0]).cpu().numpy()
        got = _parse(m, None, lengths)
        assert got['status'] == [0] and got['feasible'].tolist() == [1] * B, what
        assert got['spans'].shape == (B, L - 1, 2) and np.array_equal(got['spans'], spans), what
        assert np.array_equal(_bits(got['score']), _bits(score)), what
        assert np.array_equal(_bits(got['log_z']), _bits(log_z)) and np.array_equal(_bits(got['log_z_c']), _bits(log_z)), what
        assert np.array_equal(_bits(got['marginals']), _bits(marg)), what
        assert (got['log_prob'] == 0).all() and not np.signbit(got['log_prob']).any(), what


# ---- 2. against constrained_numpy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', CC.NUMPY_LENGTHS)
def test_bracket_sets_are_constrained_numpy(L):
    """Nested required sets, required plus forbidden sets, one crossing pair (infeasible) beside them."""
    r, B = _uniform(L), PC.GPU_B
    cases = {'nested': _nested(L, B),
             'required + forbidden': _nested(L, B, forbidden=[(1, 2), (4, 5), (L - 2, L - 1)]),
             'crossing': [[(0, 3, 1), (2, 5, 1)], [(1, L - 2, 1)], [(0, 1, 0), (0, 2, 0)]]}
    worst = [0.0, 0.0, 0.0]
    for name, sets in cases.items():
        brackets = _rows(sets)
        fig, want = _against_numpy(_parse(r['m'], brackets), r['scores'], [L] * B, brackets, L, 'L %d, %s' % (L, name))
        worst = [max(a, b) for a, b in zip(worst, fig)]
        if name == 'crossing':
            assert want.feasible.tolist() == [0, 1, 1]
        else:
            assert want.feasible.all() and (want.log_prob < 0).all()           # the sets bind
    print('L %d: MEASURED %r' % (L, tuple(float('%.3e' % v) for v in worst)))


# ---- 3. the marginals -------------------------------------------------------------------------------------------------------------
def test_single_bracket_log_prob_is_the_marginal():
    """L 7, every cell of levels 1 .. 5: required, exp(log_prob) is the cell's mu; forbidden, 1 - mu.  Each side carries the bound."""
    from cliora_amd.posterior import cell_id
    L, B = 7, PC.GPU_B
    m = _uniform(L)['m']
    mu = m.span_posteriors().marginals.cpu().numpy().astype(np.float64)
    worst = 0.0
    for level in range(1, L - 1):
        for pos in range(L - level):
            for kind in (1, 0):
                got = _parse(m, _rows([[(pos, pos + level, kind)]] * B), marginals=False)
                assert got['status'] == [0] and got['feasible'].all()
                want = mu[:, cell_id(L, level, pos)] if kind else 1.0 - mu[:, cell_id(L, level, pos)]
                worst = max(worst, float(np.abs(np.exp(got['log_prob'].astype(np.float64)) - want).max()))
    print('L 7: max |exp(log_prob) - mu| over single brackets = %.3e' % worst)
    assert worst <= 2 * CC.BOUND


# ---- 4. the sampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,B', [(13, PC.GPU_B)] + [(L, 2) for L in CC.LONG_LENGTHS])
def test_requiring_a_sampled_tree_returns_it_with_its_log_prob(L, B):
    """One sampled tree per sentence, its n - 1 spans required (127 rows at L 128): the only qualifying tree, so the spans are the
    sample's and log_prob its log-probability.  L 65 and 128: the long instance, above 64 KiB of LDS."""
    from cliora_amd.sample import sample_spans
    m = _uniform(L, B)['m']
    ts = sample_spans(m, 1, CC.GPU_SAMPLE_SEED)
    rows = ts.spans.cpu().numpy()[:, 0]                                       # (B, L-1, 2)
    brackets = np.concatenate([rows, np.ones((B, L - 1, 1), dtype=np.int32)], axis=2)
    if L == 128:                                                              # unused rows up to M = 256: the most LDS a call takes
        brackets = np.concatenate([brackets, np.full((B, 256 - (L - 1), 3), -1, dtype=np.int32)], axis=1)
    got = _parse(m, brackets)
    assert got['status'] == [0] and got['feasible'].tolist() == [1] * B
    assert np.array_equal(got['spans'], rows)
    lp = ts.log_prob.cpu().numpy()[:, 0].astype(np.float64)
    err = float(np.abs(got['log_prob'].astype(np.float64) - lp).max())
    print('L %d: max |log_prob - sample.log_prob| = %.3e' % (L, err))
    assert err <= 2 * CC.BOUND
    assert np.array_equal(_bits(got['log_z']), _bits(ts.log_z.cpu().numpy()))
    tree = np.zeros_like(got['marginals'])                                    # one tree: mu_c is its indicator, leaves included
    from cliora_amd.posterior import cell_id
    for b in range(B):
        tree[b, :L] = 1.0
        for s, e in rows[b]:
            tree[b, cell_id(L, e - s, s)] = 1.0
    assert np.array_equal(got['marginals'], tree)


# ---- 5. k-best ----------------------------------------------------------------------------------------------------------------------
def test_single_brackets_pick_the_first_qualifying_tree_of_the_fourteen():
    """L 5: K = 16 lists all 14 trees by score; under a single bracket of either kind the constrained tree is the first listed tree
    that qualifies, with its listed score bit for bit."""
    from cliora_amd.kbest import kbest_spans
    L, B = 5, PC.GPU_B
    m = _uniform(L)['m']
    kb = kbest_spans(m, 16)
    assert kb.count.cpu().tolist() == [14] * B
    kspans, kscores = kb.spans.cpu().numpy(), kb.scores.cpu().numpy()
    held = [[set(CC.span_key(kspans[b, t].tolist())) | {(p, p) for p in range(L)} for t in range(14)] for b in range(B)]
    for s, e in CC.cells(L):
        for kind in (1, 0):
            got = _parse(m, _rows([[(s, e, kind)]] * B), marginals=False)
            assert got['status'] == [0]
            for b in range(B):
                first = next((t for t in range(14) if ((s, e) in held[b][t]) == bool(kind)), None)
                assert bool(got['feasible'][b]) == (first is not None), (s, e, kind, b)
                if first is None:
                    assert (got['spans'][b] == -1).all() and got['score'][b] == -np.inf
                    continue
                assert np.array_equal(got['spans'][b], kspans[b, first]), (s, e, kind, b)
                assert got['score'][b].view(np.int32) == kscores[b, first].view(np.int32), (s, e, kind, b)


# ---- 6. padded charts -------------------------------------------------------------------------------------------------------------
def _padded(lengths, L, seed0, param_seed):
    xs = [PC.sentence(PC.GPU_D, n, seed0 + b) for b, n in enumerate(lengths)]
    m = PC.text_module(PC.params(PC.GPU_D, param_seed), PC.GPU_D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, L).cuda())
    return m, xs


def _ragged_sets(lengths):
    """Per sentence of three words or more: its nested required set, and the first two words of the innermost bracket forbidden."""
    sets = []
    for b, n in enumerate(lengths):
        req = CC.nested_required(n, b) if n >= 3 else []
        rows = [(s, e, 1) for s, e in req]
        if req and req[-1][1] - req[-1][0] >= 2:
            rows.append((req[-1][0], req[-1][0] + 1, 0))
        sets.append(rows)
    return sets


@pytest.mark.parametrize('L,lengths,seed0', [(PC.RAGGED_L, PC.RAGGED_LENGTHS, 1000 * PC.RAGGED_SEED), (PC.LONG_RAGGED_L, PC.LONG_RAGGED_LENGTHS, 5600)])
def test_padded_chart_is_each_sentence_alone(L, lengths, seed0):
    """Each sentence of the padded chart under its brackets against the sentence alone at its exact length under the same brackets:
    spans exact, scalars within the bound; and against constrained_numpy on the padded chart's scores."""
    m, xs = _padded(lengths, L, seed0, PC.MBR_PARAM_SEED)
    sets = _ragged_sets(lengths)
    M = max(len(s) for s in sets)
    brackets = _rows(sets, M)
    got = _parse(m, brackets, lengths)
    _against_numpy(got, _scores(m), lengths, brackets, L, 'padded L %d' % L)
    alone = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    alone.outside = False
    from cliora_amd.posterior import cell_id
    for b, n in enumerate(lengths):
        _forward(alone, xs[b][None].cuda())
        one = _parse(alone, brackets[b:b + 1])
        assert one['status'] == [0] and one['feasible'][0] == got['feasible'][b] == 1
        assert np.array_equal(got['spans'][b, :n - 1], one['spans'][0]) and (got['spans'][b, n - 1:] == -1).all(), n
        for k in SCALARS:
            assert abs(float(got[k][b]) - float(one[k][0])) <= CC.BOUND * max(1.0, abs(float(one[k][0]))), (n, k)
        beyond = np.ones(got['marginals'].shape[1], dtype=bool)
        for level in range(n):
            for pos in range(n - level):
                beyond[cell_id(L, level, pos)] = False
                assert abs(float(got['marginals'][b, cell_id(L, level, pos)]) - float(one['marginals'][0, cell_id(n, level, pos)])) <= CC.BOUND
        assert (got['marginals'][b, beyond] == 0).all()                       # nothing beyond the triangle


def test_every_length_equal_to_L_is_the_call_without_lengths():
    L, B = 13, PC.GPU_B
    m = _uniform(L)['m']
    brackets = _rows(_nested(L, B, forbidden=[(1, 2)]))
    full = _parse(m, brackets, [L] * B)
    assert full['status'] == [0]
    _same_bits(full, _parse(m, brackets), 'lengths == L')


def test_bad_rows_and_lengths_are_counted_once_and_leave_their_neighbours_alone():
    """The L 14 chart of lengths [1, 2, 14, 9, 5]: a length of 0, a bracket that ends inside the padding (with a second bad row beside
    it) and a kind of 2 -- three sentences, three counts, all -1 rows; the other two as in the clean call, bit for bit."""
    L, lengths = PC.RAGGED_L, list(PC.RAGGED_LENGTHS)
    m, _ = _padded(lengths, L, 1000 * PC.RAGGED_SEED, PC.MBR_PARAM_SEED)
    sets = _ragged_sets(lengths)
    clean = _parse(m, _rows(sets, 6), lengths)
    assert clean['status'] == [0]
    bad_sets = [list(s) for s in sets]
    bad_sets[3] = bad_sets[3] + [(3, 10, 1), (12, 13, 0)]                     # n = 9: end >= n, inside the chart
    bad_sets[4] = bad_sets[4] + [(1, 2, 2)]                                   # kind
    bad_lengths = list(lengths)
    bad_lengths[1] = 0
    got = _parse(m, _rows(bad_sets, 6), bad_lengths)
    assert got['status'] == [3]
    for b in (1, 3, 4):
        assert (got['spans'][b] == -1).all() and got['feasible'][b] == 0 and got['log_z'][b] == 0 and (got['marginals'][b] == 0).all()
        assert got['score'][b] == -np.inf and got['log_z_c'][b] == -np.inf and got['log_prob'][b] == -np.inf
    _same_bits(got, clean, 'neighbours', rows=[0, 2])


# ---- 7. infeasible sentences ------------------------------------------------------------------------------------------------------
def test_infeasible_sentences_are_no_error_and_leave_their_neighbours_alone():
    """L 7: a crossing required pair, a span both required and forbidden, a forbidden leaf, a forbidden root."""
    L, B = 7, PC.GPU_B
    r = _uniform(L)
    m = r['m']
    log_z = m.span_posteriors().log_z.cpu().numpy()
    first = [(s, e, 1) for s, e in CC.nested_required(L, 0)]
    clean = _parse(m, _rows([first, [], []], 2))
    assert clean['feasible'].tolist() == [1, 1, 1]
    for pair in ([[(1, 4, 1), (3, 5, 1)], [(2, 4, 1), (2, 4, 0)]], [[(3, 3, 0)], [(0, L - 1, 0)]]):
        brackets = _rows([first] + pair, 2)
        got = _parse(m, brackets)
        assert got['status'] == [0] and got['feasible'].tolist() == [1, 0, 0]
        for b in (1, 2):
            assert (got['spans'][b] == -1).all() and (got['marginals'][b] == 0).all()
            assert got['score'][b] == -np.inf and got['log_z_c'][b] == -np.inf and got['log_prob'][b] == -np.inf
        assert np.array_equal(_bits(got['log_z']), _bits(log_z))              # still the real value
        _same_bits(got, clean, 'neighbour', rows=[0])
        _against_numpy(got, r['scores'], [L] * B, brackets, L, 'L 7, infeasible')


# ---- 8. plans and paths -----------------------------------------------------------------------------------------------------------
def test_treelstm_plan():
    """A TreeLSTM plan (L 5): the same score rows, the same results."""
    from cliora_amd.treelstm import DioraTreeLSTM
    from oracle import diora_ref as R
    B, L, D = PC.GPU_B, 5, PC.GPU_D
    P = R.init_params_treelstm(D, seed=6, share=True)
    m = DioraTreeLSTM(D, share=True)
    sd = m.state_dict()
    for k in sd:
        sd[k] = P[k if k in P else 'inside_' + k[len('outside_'):]].detach().clone()
    m.load_state_dict(sd)
    m = m.cuda().eval()
    _forward(m, PC.batch(D, L, B, 515).cuda())
    brackets = _rows([[(1, 3, 1)], [(0, 2, 1), (3, 4, 0)], [(2, 3, 0), (0, 1, 0)]])
    _against_numpy(_parse(m, brackets), _scores(m), [L] * B, brackets, L, 'TreeLSTM L 5')


def test_cliora_plan():
    """A CLIORA plan (R 36, L 7): the same score rows, the same results."""
    from cliora_amd.cliora import DioraMLP
    B, L, D, R = PC.GPU_B, 7, PC.GPU_D, 36
    P = PC.params(D, PC.GPU_SEED)
    m = DioraMLP(D, outside=True, normalize='unit', compress=False, share=True)
    sd = m.state_dict()
    for k in sd:
        src = 'inside_' + k[len('outside_'):] if k.startswith('outside_') and k not in P else k
        if src in P:
            sd[k] = P[src].detach().clone()
    m.load_state_dict(sd)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(77)
    x, xw = torch.randn(B, L, D, generator=g).cuda(), torch.randn(B, L, D, generator=g).cuda()
    os_, ow = torch.randn(B, R, D, generator=g).cuda(), torch.randn(B, R, D, generator=g).cuda()
    with torch.no_grad():
        m(x, xw, os_, ow)
    assert m._plan.R == R
    brackets = _rows(_nested(L, B, forbidden=[(2, 3)]))
    _against_numpy(_parse(m, brackets), _scores(m), [L] * B, brackets, L, 'CLIORA L 7')


@pytest.mark.parametrize('L,B', [(13, PC.GPU_B), (65, 2)])
def test_two_calls_give_equal_bits_and_the_outside_pass_is_optional(L, B):
    m = _uniform(L, B)['m']
    brackets = _rows(_nested(L, B, forbidden=[(1, 2), (3, 5)]))
    a, b = _parse(m, brackets), _parse(m, brackets)
    assert a['feasible'].all() and (a['log_prob'] < 0).all()
    _same_bits(a, b, 'two calls')
    _same_bits(_parse(m, brackets, marginals=False), a, 'marginals=None', keys=('spans', 'feasible') + SCALARS)


def test_refusals():
    from cliora_amd import _lib
    from cliora_amd.constrained import constrained_parse
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    # (plan, ws, lengths, brackets, M, spans, score, log_z, log_zc, log_prob, feasible, marginals, status)
    call = lambda *a: lib.cliora_constrained_parse(*(a + (st,)))
    good = lambda h, ws: [h, ws, None, p(0), 2, p(100), p(200), p(300), p(400), p(500), p(600), None, p(700)]
    fresh = _lib.Plan(2, 5, 16)                                               # never ran a forward
    assert call(*good(fresh.handle, p(1000))) != 0
    assert 'before forward' in err()
    m = _uniform(3)['m']
    h, ws = m._plan.handle, C.c_void_p(m._wss[0].data_ptr())
    for M in (-1, 257):
        a = good(h, ws)
        a[4] = M
        assert call(*a) != 0
        assert 'M outside 0..256' in err()
    for i in (0, 1, 6, 7, 8, 9, 10, 12):                                      # plan, workspace, the four scalars, feasible, status
        a = good(h, ws)
        a[i] = None
        assert call(*a) != 0
        assert 'NULL argument' in err(), i
    a = good(h, ws)
    a[5] = None
    assert call(*a) != 0
    assert 'NULL spans_out' in err()
    a = good(h, ws)
    a[3] = None
    assert call(*a) != 0
    assert 'NULL brackets' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                      # nothing was launched
    a = good(h, ws)                                                           # M = 0 with NULL brackets is a call
    a[3], a[4] = None, 0
    assert call(*a) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.ChartLibError, match='M outside 0..256'):         # through the Python entry: the library's reason
        constrained_parse(m, torch.full((PC.GPU_B, 257, 3), -1, dtype=torch.int32))
    with pytest.raises(ValueError):
        constrained_parse(m, torch.full((PC.GPU_B, 2, 3), -1, dtype=torch.int64))
    with pytest.raises(ValueError):
        constrained_parse(m, torch.full((PC.GPU_B + 1, 2, 3), -1, dtype=torch.int32))
    with pytest.raises(ValueError):
        constrained_parse(m, None, torch.zeros(PC.GPU_B, dtype=torch.int64))


def test_module_entries_return_trees_and_log_probs():
    """DioraBase.cky_constrained and bracket_log_prob at L 7: the C entry's rows as trees, None where infeasible, and its log_prob."""
    from cliora_amd import _lib
    L = 7
    m = _uniform(L)['m']
    required, forbidden = [[(1, 3), (1, 2)], [(0, 3), (2, 5)], []], [[(4, 5)], [], [(0, 5), (1, 6)]]
    sets = [[(s, e, 1) for s, e in req] + [(s, e, 0) for s, e in forb] for req, forb in zip(required, forbidden)]
    got = _parse(m, _rows(sets))
    assert got['feasible'].tolist() == [1, 0, 1]
    trees = m.cky_constrained(required, forbidden)
    assert trees[1] is None
    for b in (0, 2):
        assert str(trees[b]) == str(m.trees_from_spans(got['spans'][b:b + 1])[0])
    assert str(trees[0]) != str(m.cky()[0]) or got['log_prob'][0] == 0
    assert m.bracket_log_prob(required, forbidden) == got['log_prob'].tolist()
    assert [str(t) for t in m.cky_constrained([[], [], []])] == [str(t) for t in m.cky()]
    assert m.bracket_log_prob([[], [], []]) == [0.0] * 3
    with pytest.raises(_lib.ChartLibError, match='rejected 1 sentence'):
        m.cky_constrained([[(0, L)], [], []])
    with pytest.raises(_lib.ChartLibError, match='rejected 2 sentence'):
        m.bracket_log_prob([[(0, L)], [], [(3, 2)]])


def test_parse_ragged_constrained_returns_the_callers_order():
    """Sentences of 9, 70, 3, 1, 3, 12 and 9 words, one of them infeasible, max_batch 3: what constrained_parse gives on each pack's
    padded chart, back in the caller's order; and the same trees from other packs (max_batch 2), log_prob within the bound."""
    from cliora_amd import _lib, ragged
    from cliora_amd.constrained import constrained_parse, host_results, pack_brackets
    from cliora_amd.harness import build_net
    torch.manual_seed(11)
    net = build_net(50, torch.nn.Embedding(97, 32), obj_feats=False).cuda()
    rs = np.random.RandomState(5)
    lens = [9, 70, 3, 1, 3, 12, 9]
    sents = [rs.randint(1, 97, size=n).tolist() for n in lens]
    required = [CC.nested_required(n, i) if n >= 3 else [] for i, n in enumerate(lens)]
    required[5] = [(0, 5), (3, 8)]                                            # crossing
    forbidden = [[(n - 2, n - 1)] if n >= 5 else [] for n in lens]
    got = ragged.parse_ragged_constrained(net, sents, required, forbidden, max_batch=3)
    want = [None] * len(sents)

    def per_pack(idx, lengths):
        cp = constrained_parse(net.diora, pack_brackets([required[i] for i in idx], [forbidden[i] for i in idx]), lengths)
        spans, feasible, log_prob, rejected = host_results(cp)
        assert rejected == 0
        for b, i in enumerate(idx):
            tree = net.diora.trees_from_spans(spans[b:b + 1, :lens[i] - 1])[0] if feasible[b] else None
            want[i] = (tree, float(log_prob[b]))

    ragged._run_packs(net, sents, 3, ragged.DEFAULT_MAX_WASTE, 0, per_pack, max_len=128)
    assert [(str(t), p) for t, p in got] == [(str(t), p) for t, p in want]
    assert got[3] == (0, 0.0) and got[5] == (None, float('-inf'))
    assert all(t is not None and p < 0 for i, (t, p) in enumerate(got) if i not in (3, 5))
    other = ragged.parse_ragged_constrained(net, sents, required, forbidden, max_batch=2)
    assert [str(t) for t, _ in other] == [str(t) for t, _ in got]
    for (_, p), (_, q) in zip(other, got):
        assert p == q or abs(p - q) <= CC.BOUND * max(1.0, abs(q))
    with pytest.raises(_lib.ChartLibError, match='rejected 1 sentence'):
        ragged.parse_ragged_constrained(net, sents, [[(0, 9)]] + [[]] * 6)
    with pytest.raises(_lib.ChartLibError):
        ragged.parse_ragged_constrained(net, sents, required, max_len=64)
