"""cliora_span_posteriors on the GPU (cliora_amd/posterior.py): span posteriors, log-partition and MBR trees.

Yardsticks, never the code under test: ``posterior_numpy`` in fp64 (pinned to enumeration of every binary tree by
test_posterior_cpu.py) on the device's OWN per-split scores, so that the comparison isolates this kernel; ``mbr_numpy`` on the device's
own marginals, bitwise; the fp64 MBR tree of the oracle's scores on sentences seeded away from near-ties.  Bounds and measured
figures: posterior_cases.py.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import posterior_cases as PC

pytestmark = pytest.mark.gpu


def _scores(m):
    """Per-split inside scores of the chart the module just computed, through cliora_inside_pair_states: {level: (B, L - level, level)}."""
    from cliora_amd import _lib
    plan, ws = m._plan, m._wss[0]
    assert len(m._wss) == 1
    wsf = ws.view(torch.float32)
    out = {}
    for level in range(1, plan.L):
        ps, ph, rows, ldh = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.check(_lib.lib().cliora_inside_pair_states(plan.handle, C.c_void_p(ws.data_ptr()), level, C.byref(ps), C.byref(ph), C.byref(rows),
                                                        C.byref(ldh)), 'cliora_inside_pair_states')
        so = (ps.value - ws.data_ptr()) // 4
        out[level] = wsf[so:so + rows.value].view(plan.B, plan.L - level, level).cpu().numpy()
    return out


def _forward(m, x):
    with torch.no_grad():
        m(x, x)


def _host(post):
    return dict(marg=post.marginals.cpu().numpy(), log_z=post.log_z.cpu().numpy(), spans=post.spans.cpu().numpy(),
                split=post.split.cpu().numpy(), status=post.status.cpu().tolist())


@functools.lru_cache(maxsize=None)
def _uniform(L):
    """One eval forward of a text-only DioraMLP (D 16, B 3, random weights) at length L, the kernel's outputs with MBR on, the device's
    scores and the fp64 restatement on them -- computed once per length and shared by the tests below."""
    from cliora_amd.posterior import posterior_numpy, span_posteriors
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.batch(PC.GPU_D, L, PC.GPU_B, PC.GPU_SEED + L).cuda())
    got = _host(span_posteriors(m, mbr=True))
    scores = _scores(m)
    mu64, lz64 = posterior_numpy(scores, [L] * PC.GPU_B, L)
    return dict(m=m, scores=scores, mu64=mu64, lz64=lz64, **got)


def _check_accuracy(got, mu64, lz64, lengths, L, what):
    """The issue's bounds; prints each figure before it asserts.  -> (max |mu - mu64|, max relative log_z error)."""
    from cliora_amd.posterior import cell_id
    emu = float(np.abs(got['marg'].astype(np.float64) - mu64).max())
    elz = float((np.abs(got['log_z'].astype(np.float64) - lz64) / np.maximum(1.0, np.abs(lz64))).max())
    print('%s: max |mu - mu64| = %.3e, max |log_z - log_z64| / max(1, |log_z64|) = %.3e (log_z64 up to %.3f)'
          % (what, emu, elz, float(np.abs(lz64).max())))
    assert emu <= PC.BOUND
    assert elz <= PC.BOUND
    for b, n in enumerate(lengths):
        own = np.zeros(got['marg'].shape[1], dtype=bool)
        internal = 0.0
        for level in range(n):
            c0 = cell_id(L, level, 0)
            own[c0:c0 + n - level] = True
            if level:
                internal += float(got['marg'][b, c0:c0 + n - level].astype(np.float64).sum())
        assert (got['marg'][b, ~own] == 0).all()                              # exactly 0 outside the triangle
        if n < 1:
            continue
        assert abs(internal - (n - 1)) <= n * PC.BOUND, (b, n, internal)
        assert np.abs(got['marg'][b, :n] - 1).max() <= PC.BOUND               # the leaves
        assert abs(got['marg'][b, cell_id(L, n - 1, 0)] - 1) <= PC.BOUND      # the root
    return emu, elz


def _check_mbr_bitwise(got, lengths, L):
    from cliora_amd.posterior import mbr_numpy
    spans, split = mbr_numpy(got['marg'], lengths, L)
    assert np.array_equal(got['split'], split)
    for b, n in enumerate(lengths):
        assert got['spans'][b, :max(n - 1, 0)].tolist() == [list(s) for s in spans[b]], b
        assert (got['spans'][b, max(n - 1, 0):] == -1).all()
        if n > 1:
            assert got['spans'][b, n - 2].tolist() == [0, n - 1]              # the sentence's own root, last


@pytest.mark.parametrize('L', PC.GPU_LENGTHS)
def test_marginals_and_log_z_against_fp64_on_the_device_scores(L):
    """max |mu - mu64| <= 1e-4 and |log_z - log_z64| <= 1e-4 max(1, |log_z64|), sum of mu over internal cells within n 1e-4 of n - 1,
    leaves and root 1 -- at every length of the issue's table.  Measured per L: posterior_cases.MEASURED."""
    r = _uniform(L)
    assert r['status'] == [0]
    _check_accuracy(r, r['mu64'], r['lz64'], [L] * PC.GPU_B, L, 'L %d' % L)


def test_device_against_the_enumeration_directly():
    """L 7: every one of the 132 trees, weighed in fp64 on the device's scores."""
    from cliora_amd.posterior import cell_id
    r = _uniform(7)
    for b in range(PC.GPU_B):
        mu, log_z, _, _ = PC.enumerate_posteriors(r['scores'], b, 7)
        for (level, pos), w in mu.items():
            assert abs(float(r['marg'][b, cell_id(7, level, pos)]) - w) <= PC.BOUND
        assert abs(float(r['log_z'][b]) - log_z) <= PC.BOUND * max(1.0, abs(log_z))


@pytest.mark.parametrize('L', PC.GPU_LENGTHS)
def test_mbr_is_bitwise_mbr_numpy_on_the_device_marginals(L):
    r = _uniform(L)
    _check_mbr_bitwise(r, [L] * PC.GPU_B, L)


@pytest.mark.parametrize('L', [13, 65, 128])
def test_two_calls_give_equal_bits(L):
    from cliora_amd.posterior import span_posteriors
    r = _uniform(L)
    again = _host(span_posteriors(r['m'], mbr=True))
    for k in ('marg', 'log_z', 'spans', 'split'):
        assert np.array_equal(r[k].view(np.int32), again[k].view(np.int32)), k
    full = _host(span_posteriors(r['m'], torch.full((PC.GPU_B,), L, dtype=torch.int32).cuda(), mbr=True))
    for k in ('marg', 'log_z', 'spans', 'split'):                            # lengths all L: bitwise the lengths = None call
        assert np.array_equal(r[k].view(np.int32), full[k].view(np.int32)), k
    assert full['status'] == [0]


def test_mbr_trees_are_the_fp64_trees_of_the_oracle():
    """L 12, D 50, the four seeded sentences (posterior_cases.MBR_SEEDS; every cell's two best fp64 candidates at least
    2 (n - 1) 1e-4 apart on the oracle's scores): every device tree is the fp64 MBR tree.  None is excused."""
    from cliora_amd.posterior import span_posteriors
    m = PC.text_module(PC.params(PC.MBR_D, PC.MBR_PARAM_SEED), PC.MBR_D).cuda().eval()
    _forward(m, torch.stack([PC.sentence(PC.MBR_D, PC.MBR_L, s) for s in PC.MBR_SEEDS]).cuda())
    spans = span_posteriors(m, mbr=True).spans.cpu().numpy()
    for b, seed in enumerate(PC.MBR_SEEDS):
        assert spans[b].tolist() == [list(s) for s in PC.mbr_oracle(seed)[0]], seed
    assert [str(t) for t in m.mbr()] == [str(t) for t in m.trees_from_spans(spans)]       # DioraBase.mbr(): the same trees, nested
    assert torch.equal(m.mbr_spans_device(), torch.from_numpy(spans).cuda())


def _triangle(L, n):
    from cliora_amd.posterior import cell_id
    return np.concatenate([np.arange(cell_id(L, lv, 0), cell_id(L, lv, 0) + n - lv) for lv in range(n)])


def test_mixed_lengths_in_one_padded_chart():
    """L 14, lengths [1, 2, 14, 9, 5]: each sentence against fp64 on the padded chart's scores and against the same sentence run alone
    at its exact length; the trees identical (the seed keeps the fp64 gap, test_posterior_cpu.py)."""
    from cliora_amd.posterior import posterior_numpy, span_posteriors
    L, lengths = PC.RAGGED_L, PC.RAGGED_LENGTHS
    xs = PC.ragged_sentences()
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    alone = []
    for x in xs:
        _forward(m, x[None].cuda())
        alone.append(_host(span_posteriors(m, mbr=True)))
    _forward(m, PC.padded(xs, L).cuda())
    got = _host(span_posteriors(m, torch.tensor(lengths, dtype=torch.int32).cuda(), mbr=True))
    assert got['status'] == [0]
    mu64, lz64 = posterior_numpy(_scores(m), lengths, L)
    _check_accuracy(got, mu64, lz64, lengths, L, 'L 14 padded')
    _check_mbr_bitwise(got, lengths, L)
    for b, n in enumerate(lengths):
        one = alone[b]
        dmu = float(np.abs(got['marg'][b, _triangle(L, n)] - one['marg'][0]).max())
        dlz = abs(float(got['log_z'][b]) - float(one['log_z'][0]))
        print('n %d: |mu(padded) - mu(alone)| = %.3e, |log_z(padded) - log_z(alone)| = %.3e' % (n, dmu, dlz))
        assert dmu <= PC.BOUND and dlz <= PC.BOUND * max(1.0, abs(float(one['log_z'][0])))
        assert got['spans'][b, :n - 1].tolist() == one['spans'][0].tolist(), n


def test_bad_lengths_are_counted_and_harm_no_other_sentence():
    from cliora_amd.posterior import span_posteriors
    L = PC.RAGGED_L
    m = PC.text_module(PC.params(PC.GPU_D, PC.MBR_PARAM_SEED), PC.GPU_D).cuda().eval()
    _forward(m, PC.padded(PC.ragged_sentences(), L).cuda())
    good = torch.tensor(PC.RAGGED_LENGTHS, dtype=torch.int32).cuda()
    want = _host(span_posteriors(m, good, mbr=True))
    bad = good.clone()
    bad[1], bad[3] = 0, L + 1
    got = _host(span_posteriors(m, bad, mbr=True))
    assert got['status'] == [2]
    for b in range(len(PC.RAGGED_LENGTHS)):
        if b in (1, 3):
            assert (got['marg'][b] == 0).all() and got['log_z'][b] == 0 and (got['spans'][b] == -1).all() and (got['split'][b] == -1).all()
        else:
            for k in ('marg', 'log_z', 'spans', 'split'):
                assert np.array_equal(got[k][b], want[k][b]), (b, k)


def test_long_padded_chart():
    """L 70 (a long plan: two splits / uses per lane), lengths [70, 66, 3], through the inside-only padded forward."""
    from cliora_amd.posterior import posterior_numpy, span_posteriors
    L, lengths = PC.LONG_RAGGED_L, PC.LONG_RAGGED_LENGTHS
    xs = [PC.sentence(PC.GPU_D, n, 4400 + b) for b, n in enumerate(lengths)]
    m = PC.text_module(PC.params(PC.GPU_D, PC.GPU_SEED), PC.GPU_D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, L).cuda())
    got = _host(span_posteriors(m, torch.tensor(lengths, dtype=torch.int32).cuda(), mbr=True))
    assert got['status'] == [0]
    mu64, lz64 = posterior_numpy(_scores(m), lengths, L)
    _check_accuracy(got, mu64, lz64, lengths, L, 'L 70 padded')
    _check_mbr_bitwise(got, lengths, L)


def test_boundary_lengths_share_one_long_chart():
    """L 65 (a long plan), D 50, lengths [65, 64, 2, 1] in one padded chart: the two callers of the shared walk and the shared
    first-maximum reduction, at 65 and 64 words (two splits per lane, and the most one lane each holds) and at two words and one.
    cky_spans_ragged's splits and spans == decode_ragged_numpy on the device's own per-split scores, and the MBR tree of
    span_posteriors == mbr_numpy on the device's own marginals: integers, row for row, no tolerance."""
    from cliora_amd import ragged
    from cliora_amd.posterior import span_posteriors
    L, D, lengths = 65, 50, [65, 64, 2, 1]
    xs = [PC.sentence(D, n, 5500 + b) for b, n in enumerate(lengths)]
    m = PC.text_module(PC.params(D, PC.GPU_SEED), D).cuda().eval()
    m.outside = False
    _forward(m, PC.padded(xs, L).cuda())
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    spans, status, split = ragged.cky_spans_ragged(m, lens, split_out=True)
    assert status.cpu().tolist() == [0]
    want_spans, want_split = ragged.decode_ragged_numpy(_scores(m), lengths, L)
    assert np.array_equal(split.cpu().numpy(), want_split)
    spans = spans.cpu().numpy()
    for b, n in enumerate(lengths):
        assert spans[b, :n - 1].tolist() == [list(s) for s in want_spans[b]], n
        assert (spans[b, n - 1:] == -1).all()
    got = _host(span_posteriors(m, lens, mbr=True))
    assert got['status'] == [0]
    _check_mbr_bitwise(got, lengths, L)


def test_cliora_plan():
    """A CLIORA plan (R 36, L 9): the same score rows, the same bounds."""
    from cliora_amd.cliora import DioraMLP
    from cliora_amd.posterior import posterior_numpy, span_posteriors
    B, L, D, R = PC.GPU_B, 9, PC.GPU_D, 36
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
    got = _host(span_posteriors(m, mbr=True))
    mu64, lz64 = posterior_numpy(_scores(m), [L] * B, L)
    _check_accuracy(got, mu64, lz64, [L] * B, L, 'CLIORA L 9')
    _check_mbr_bitwise(got, [L] * B, L)


def test_marginal_table_and_module_entry():
    from cliora_amd.posterior import cell_id, marginal_table
    r = _uniform(13)
    post = r['m'].span_posteriors()
    assert post.spans is None and post.split is None
    assert np.array_equal(post.marginals.cpu().numpy(), r['marg'])            # without MBR: the same marginals
    table = marginal_table(post.marginals, 13)
    assert table.is_cuda and table.shape == (PC.GPU_B, 13, 13)
    assert float(table[1, 2, 7]) == float(r['marg'][1, cell_id(13, 5, 2)]) and float(table[0, 5, 3]) == 0.0


def test_parse_ragged_mbr_returns_the_callers_order():
    from cliora_amd import ragged
    from cliora_amd.harness import build_net
    torch.manual_seed(11)
    net = build_net(50, torch.nn.Embedding(97, 32), obj_feats=False).cuda()
    rs = np.random.RandomState(5)
    sents = [rs.randint(1, 97, size=n).tolist() for n in [9, 1, 20, 2, 17, 9, 3, 12]]
    got = ragged.parse_ragged(net, sents, max_batch=3, decode='mbr')
    net.eval()
    want = []
    with torch.no_grad():
        for s in sents:
            net(torch.tensor([s]).cuda(), compute_loss=False)
            want.append(net.diora.mbr()[0])
    assert [str(t) for t in got] == [str(t) for t in want]
    assert got[1] == 0 and got[3] == (0, 1)
    with pytest.raises(ValueError):
        ragged.parse_ragged(net, sents, decode='best')


def test_evaluate_counts_f1_against_the_mbr_spans(tmp_path):
    """evaluate(decode='mbr') on the fixture batches of eval_parse.npz: its parse.jsonl holds the MBR spans and its F1 is the F1 of
    those spans; decode='viterbi' returns what evaluate() returns, to the last digit."""
    from conftest import load_golden
    from test_gpu_eval import _batches, _net
    from cliora_amd.evaluate import evaluate
    from cliora_amd.interchange import SpanF1
    g = load_golden('eval_parse.npz')
    meta = g['meta']
    words = {i: 'w%d' % i for i in range(meta['V'])}
    net, batches = _net(g), _batches(g)
    base = evaluate(net, batches, words)
    assert evaluate(net, batches, words, decode='viterbi') == base
    path = os.path.join(str(tmp_path), 'parse.jsonl')
    got = evaluate(net, batches, words, out_path=path, decode='mbr')
    lines = [json.loads(x) for x in open(path).read().splitlines()]
    f1, k = SpanF1(), 0
    dev = next(net.parameters()).device
    with torch.no_grad():
        for bm in batches:
            if bm['sentences'].shape[1] <= 2:
                continue
            net(bm['sentences'].to(dev), bm['obj_feats'].to(dev), bm['neg_samples'].to(dev), compute_loss=True)
            spans = net.diora.mbr_spans_device().cpu().numpy()
            for b in range(spans.shape[0]):
                pred = set(tuple(s) for s in spans[b, :-1].tolist())
                gold = set(tuple(s) for s in bm['GT'][b][:-1])
                f1.add_counts(len(pred & gold), len(pred), len(gold))
                assert set(tuple(s) for s in lines[k]['pred_spans']) == pred
                k += 1
    assert k == len(lines)
    tp, fp, fn = f1.tp, f1.fp, f1.fn
    prec, rec = tp / (tp + fp) if tp + fp else 0., tp / (tp + fn) if tp + fn else 0.
    assert got['corpus_f1'] == (2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.)
    assert got['sent_f1'] == float(np.mean(np.array(f1.sentence)))


def test_refusals():
    from cliora_amd import _lib
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(4096, dtype=torch.float32, device='cuda')
    p = lambda off: C.c_void_p(buf.data_ptr() + 4 * off)
    err = lambda: lib.cliora_last_error().decode()
    fresh = _lib.Plan(2, 5, 16)                                               # never ran a forward
    assert lib.cliora_span_posteriors(fresh.handle, p(0), None, p(100), p(200), None, None, None, None, st) != 0
    assert 'before forward' in err()
    m = _uniform(3)['m']
    ws = C.c_void_p(m._wss[0].data_ptr())
    assert lib.cliora_span_posteriors(m._plan.handle, ws, None, None, p(200), None, None, None, None, st) != 0
    assert 'NULL argument' in err()
    assert lib.cliora_span_posteriors(m._plan.handle, ws, p(300), p(100), p(200), None, None, None, None, st) != 0
    assert 'without status' in err()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0                                      # nothing was launched
