"""Every after-forward chart query on an object that carries TWO forward workspaces (cliora_amd/query.py: the loop over workspaces).

No module produces more than one workspace per forward, so nothing else runs a query's second workspace on the device: its slice of
every per-sentence tensor, its offset into the d_split buffer, its own status word, and the samplers' default sentence ids.  The
yardstick is the same query on each forward's own module with the matching half of the inputs, bit for bit.
"""
import types

import pytest
import torch

import posterior_cases as PC

pytestmark = pytest.mark.gpu

B, L, D, S, K = 2, 5, 16, 4, 4
LENGTHS = [5, 3, 4, 1]                     # the full-length sentence and the one-word one: the two edges of the sentence view
BAD_LENGTHS = [9, 3, 4, 1]                 # one length outside the chart, in the first workspace
REQUIRED = [[(1, 3)], [(0, 1), (1, 2)], [(0, 1)], []]          # row 1: two crossing brackets, so no tree qualifies
FORBIDDEN = [[(0, 1)], [], [], []]
SEED = 77


def _charts():
    """Two eval forwards (outside pass on) of one set of weights over different inputs -> (module 1, module 2, an object that presents
    the two workspaces under the one plan, as a module holding both would)."""
    from cliora_amd.diora import ChartWorkspaces
    mods = []
    for i in range(2):
        m = PC.text_module(PC.params(D, PC.GPU_SEED), D).cuda().eval()
        x = PC.batch(D, L, B, PC.GPU_SEED + 50 * i).cuda()
        with torch.no_grad():
            m(x, x)
        mods.append(m)
    assert mods[0]._plan is mods[1]._plan
    holder = ChartWorkspaces()
    holder.extend([mods[0]._wss[0], mods[1]._wss[0]])
    return mods[0], mods[1], types.SimpleNamespace(_plan=mods[0]._plan, _wss=holder)


def _inputs():
    from cliora_amd.constrained import pack_brackets
    g = torch.Generator().manual_seed(SEED)
    return dict(brackets=pack_brackets(REQUIRED, FORBIDDEN), cost=torch.randn(2 * B, L * (L + 1) // 2, generator=g),
                w=torch.rand(2 * B, generator=g) + 0.5, w2=torch.randn(2 * B, generator=g))


def _fields(obj, names):
    return {n: getattr(obj, n) for n in names}


def _queries(inp):
    """name -> f(chart, rows, lengths, ids) -> {field: device tensor}: the ten queries, each over the sentences `rows` of the inputs."""
    from cliora_amd import constrained, kbest, posterior, ragged, sample, structured
    br, cost, w, w2 = inp['brackets'], inp['cost'], inp['w'], inp['w2']

    def cky(m, rows, lens, ids):
        spans, status, split = ragged.cky_spans_ragged(m, lens, split_out=True)
        return dict(spans=spans, status=status, split=split)

    return {
        'cky_spans_ragged': cky,
        'span_posteriors': lambda m, rows, lens, ids: _fields(posterior.span_posteriors(m, lens, mbr=True),
                                                              ('marginals', 'log_z', 'spans', 'split', 'status')),
        'kbest_spans': lambda m, rows, lens, ids: _fields(kbest.kbest_spans(m, K, lens), ('spans', 'scores', 'count', 'status')),
        'sample_spans': lambda m, rows, lens, ids: sample.sample_spans(m, S, SEED, lens, ids=ids)._asdict(),
        'constrained_parse': lambda m, rows, lens, ids: constrained.constrained_parse(m, br[rows], lens, marginals=True)._asdict(),
        'constrained_kbest': lambda m, rows, lens, ids: _fields(constrained.constrained_kbest(m, br[rows], K, lens),
                                                                ('spans', 'scores', 'count', 'status', 'feasible')),
        'constrained_samples': lambda m, rows, lens, ids: constrained.constrained_samples(m, br[rows], S, SEED, lens, ids=ids)._asdict(),
        'bracket_grad': lambda m, rows, lens, ids: structured.bracket_grad(m, br[rows], weights=w[rows], lengths=lens)._asdict(),
        'tree_expectation': lambda m, rows, lens, ids: structured.tree_expectation(m, cost[rows], w[rows], w2[rows], lens)._asdict(),
        'bracket_margin': lambda m, rows, lens, ids: structured.bracket_margin(m, br[rows], 1.0, float('inf'), weights=w[rows], lengths=lens,
                                                                               spans=True)._asdict(),
    }


def _same(a, b):
    """Bitwise: floats are compared as their 32-bit words."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def test_two_workspaces_give_each_forwards_own_results():
    from cliora_amd.diora import DioraBase
    from cliora_amd.structured import split_score_count
    m1, m2, both = _charts()
    count = split_score_count(both._plan)
    lens = lambda v, rows=slice(None): torch.tensor(v[rows], dtype=torch.int32)
    halves = [(m1, slice(0, B), torch.tensor([0, 1], dtype=torch.int32)), (m2, slice(B, 2 * B), torch.tensor([2, 3], dtype=torch.int32))]
    feasible = None
    for name, query in _queries(_inputs()).items():
        whole = query(both, slice(None), lens(LENGTHS), None)
        for i, (m, rows, ids) in enumerate(halves):
            part = query(m, rows, lens(LENGTHS, rows), ids)
            assert part['status'].shape == (1,), name
            for field, t in part.items():
                w = whole[field]
                w = w[i:i + 1] if field == 'status' else w[i * count:(i + 1) * count] if field == 'd_split' else w[rows]
                assert _same(w, t), (name, field, i)
        assert whole['status'].shape == (2,) and whole['status'].tolist() == [0, 0], name
        if 'd_split' in whole:
            assert whole['d_split'].shape == (2 * count,), name
        if 'feasible' in whole and name != 'bracket_margin':
            feasible = whole['feasible'].tolist()
            assert feasible == [1, 0, 1, 1], name
        bad = query(both, slice(None), lens(BAD_LENGTHS), None)
        assert bad['status'].shape == (2,) and bad['status'].tolist() == [1, 0], name
    assert feasible is not None
    # the decode that takes no lengths and no status word
    whole = DioraBase.cky_spans_device(both)
    assert whole.shape == (2 * B, L - 1, 2)
    for m, rows, _ in halves:
        assert _same(whole[rows], m.cky_spans_device())
    # the samplers' default ids over two workspaces are the rows of the whole chart, not of each workspace
    from cliora_amd import sample
    again = sample.sample_spans(both, S, SEED, lens(LENGTHS), ids=torch.arange(2 * B, dtype=torch.int32))
    assert _same(again.spans, sample.sample_spans(both, S, SEED, lens(LENGTHS)).spans)
