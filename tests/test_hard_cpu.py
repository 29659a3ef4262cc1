"""Hard (single-tree) charts without a GPU: the torch restatement against the oracle with the softmax put back, the symbols' declaration,
export and binding, every refusal of cliora_chart_forward_hard through the C ABI, the span walk on the host, the selection margins and
ReLU clearances the GPU cases rely on, and the compose grid.  Cases and bounds: hard_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hard_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('D,B,L,share,seed', [(16, 3, 3, True, 11), (24, 2, 6, False, 12), (48, 2, 5, True, 13)])
def test_restatement_with_the_softmax_put_back_is_the_oracle(D, B, L, share, seed):
    """hard_forward_torch(soft=True) walks the library's split order; the oracle the reference's: the same chart to 1e-12 in fp64."""
    from cliora_amd.hard import hard_forward_torch
    from oracle import diora_ref as R
    from oracle import synth
    P, x, _ = synth.diora_case(D, B, L, seed, share=share)
    P64, x64 = {k: v.double() for k, v in P.items()}, x.double()
    with torch.no_grad():
        want = R.diora_forward(P64, x64, x64, share=share)
        got = hard_forward_torch(P64, x64, share, 'unit', soft=True)
    for k in HC.CHARTS:
        w = want[k].squeeze(-1) if want[k].shape[-1] == 1 else want[k]
        err = float((got[k] - w).abs().max())
        print(k, err)
        assert err <= 1e-12, (k, err)


def test_symbols_declared_exported_and_bound():
    from cliora_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'cliora_chart.h')).read()
    assert '#define CLIORA_FWD_HARD_DENSE 16' in header
    assert 'int cliora_chart_forward_hard(cliora_plan* plan, const cliora_params* params, const float* x_span,' in header
    assert 'int cliora_hard_spans(cliora_plan* plan, const int32_t* sel_in, int32_t* spans, void* stream);' in header
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'cliora_chart_forward_hard') and hasattr(raw, 'cliora_hard_spans')
    fwd, spans = _lib.lib().cliora_chart_forward_hard, _lib.lib().cliora_hard_spans
    assert len(fwd.argtypes) == 13 and fwd.restype is ctypes.c_int
    assert len(spans.argtypes) == 4 and spans.restype is ctypes.c_int
    assert _lib.FWD_HARD_DENSE == 16


def _refused(plan, flags=1, sel=True, **params):
    """cliora_chart_forward_hard on host-only dummies (nothing is dereferenced before the refusals) -> (return code, message)."""
    from cliora_amd import _lib
    buf = np.zeros(16, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    fields = {n: p.value for n in ('leaf_w', 'leaf_b', 'in_w1', 'in_b1', 'in_w2', 'in_b2', 'in_mat', 'root_h')}
    fields.update({k: (p.value if v else None) for k, v in params.items()})
    pst = _lib.Params(*[fields.get(n) for n in _lib.PARAM_FIELDS])
    s = p if sel else None
    rc = _lib.lib().cliora_chart_forward_hard(plan.handle, ctypes.byref(pst), p, p, p, p, p, s, s, p, 0, flags, None)
    return rc, _lib.fn('cliora_last_error')().decode()


def test_refusals_through_the_c_abi():
    """Every refusal comes before any launch (there is no GPU here), with CLIORA_EINVAL and a message that says why."""
    from cliora_amd import _lib
    text = _lib.Plan(2, 5, 16)
    for plan, kw, words in [
            (_lib.Plan(2, 5, 16, arch=1), {}, 'TreeLSTM'),
            (_lib.Plan(2, 5, 16, R=4), {}, 'R > 0'),
            (text, dict(root_mat=True), 'compress'),
            (text, dict(flags=1 | _lib.FWD_PAIR_STATES), 'CLIORA_FWD_PAIR_STATES'),
            (_lib.Plan(1, 65, 16, forward_only=True), {}, 'CLIORA_FWD_NO_BACKWARD'),
            (text, dict(sel=False), 'selection'),
            (text, dict(flags=1 | 32), 'flag')]:
        rc, msg = _refused(plan, **kw)
        print(rc, msg)
        assert rc == -1 and 'cliora_chart_forward_hard' in msg and words in msg, (rc, msg, words)
    # the long plan with the flag, and every accepted flag word, get past the hard entry's own refusals: to the workspace check
    for plan, flags in [(_lib.Plan(1, 65, 16, forward_only=True), 1 | _lib.FWD_NO_BACKWARD), (text, 0), (text, 1 | _lib.FWD_HARD_DENSE),
                        (text, _lib.FWD_NO_BACKWARD | _lib.FWD_HARD_DENSE)]:
        rc, msg = _refused(plan, flags=flags)
        assert rc == -3 and 'workspace too small' in msg, (rc, msg)
    # cliora_hard_spans: NULL arguments; nothing to do (and nothing read) for one word
    spans = _lib.lib().cliora_hard_spans
    assert spans(text.handle, None, None, None) == -1 and 'cliora_hard_spans' in _lib.fn('cliora_last_error')().decode()
    assert spans(_lib.Plan(2, 1, 16).handle, None, None, None) == 0


def _tree_from_cells(cells, L):
    """A nested-tuple tree from the (level, pos) cells of its internal nodes, by the rule the reference's tree reader applies to
    inside_tree: spans as (pos, size), the words added, sorted by size then position; a span adopts the finished nodes that start inside
    it and have no parent yet."""
    spans = sorted([(pos, level + 1) for level, pos in cells] + [(w, 1) for w in range(L)], key=lambda s: (s[1], s[0]))
    top = {}                                   # word -> the largest finished node covering it: (pos, size, tree)
    for pos, size in spans:
        if size == 1:
            top[pos] = (pos, 1, pos)
            continue
        kids, w = [], pos
        while w < pos + size:
            kids.append(top[w])
            w += top[w][1]
        node = (pos, size, tuple(k[2] for k in kids))
        for w in range(pos, pos + size):
            top[w] = node
    return top[0][2]


def test_hard_spans_numpy():
    from cliora_amd.diora import DioraBase
    from cliora_amd.hard import hard_spans_numpy, inside_tree_from_spans, level_offsets
    for L in (2, 3, 5, 9):
        C = L * (L + 1) // 2
        # an all-zero selection: every cell splits off its first word -- the right-branching tree
        spans = hard_spans_numpy(np.zeros((2, C), dtype=np.int32), L)
        assert spans.dtype == np.int32 and spans.shape == (2, L - 1, 2)
        assert spans[0].tolist() == [[s, L - 1] for s in range(L - 2, -1, -1)]
        tree = L - 1
        for w in range(L - 2, -1, -1):
            tree = (w, tree)
        assert DioraBase.trees_from_spans(spans) == [tree, tree]
        # random selections: the walk, the span-list reader and the reference-shaped reader of inside_tree agree on the tree
        rng = np.random.RandomState(L)
        off = level_offsets(L)
        sel = np.full((4, C), -1, dtype=np.int32)
        for level in range(1, L):
            sel[:, off[level]:off[level] + L - level] = rng.randint(0, level, size=(4, L - level))

        def build(b, level, pos):
            if level == 0:
                return pos
            k = int(sel[b, off[level] + pos])
            return (build(b, k, pos), build(b, level - k - 1, pos + k + 1))
        spans = hard_spans_numpy(sel, L)
        want = [build(b, L - 1, 0) for b in range(4)]
        assert DioraBase.trees_from_spans(spans) == want
        assert (spans[:, -1] == [0, L - 1]).all()
        it = inside_tree_from_spans(spans)
        assert [_tree_from_cells(it[(b, 0)][(L - 1, 0)], L) for b in range(4)] == want
    assert hard_spans_numpy(np.zeros((3, 1), dtype=np.int32), 1).shape == (3, 0, 2)


@pytest.mark.parametrize('name', sorted(HC.CASES))
def test_case_margins_and_relu_clearance(name):
    """What the GPU cases rely on, in the fp64 restatement: every ReLU pre-activation, of every pair of both passes, stays RELU_MARGIN
    off zero (tests/dispatch_cases.py's clearance: an fp32 run then agrees with fp64 on every ReLU) -- at L 128 those of the pairs the
    hard chart composes (hard_cases.SELECTED_PAIRS_ONLY: over all 44 M the case measures 1.96e-7, and no seed reaches 5e-7); a clear
    case keeps every cell of both passes MARGIN_REL * max|inside_s| ahead of its second-best split -- no cell is exempt from the
    selection comparison there."""
    c = HC.CASES[name]
    r = HC.reference(name)
    print('%s: relu margin (selected pairs) %.3g, (every pair) %.3g; smallest selection margin / max|inside_s| %.3g'
          % (name, r['relu_margin'], r['relu_margin_all'], HC.min_margin_rel(r)))
    assert r['relu_margin'] >= HC.RELU_MARGIN, r['relu_margin']
    if name not in HC.SELECTED_PAIRS_ONLY:
        assert r['relu_margin_all'] >= HC.RELU_MARGIN, r['relu_margin_all']
    if c['clear']:
        assert HC.min_margin_rel(r) >= HC.MARGIN_REL
    if c['ties']:          # every split of a cell scores the same: the first wins everywhere
        assert int(r['sel_in'].max()) == 0 and int(r['sel_out'].max()) == 0


def test_fp32_restatement_is_close_to_fp64_on_the_clear_cases():
    """The margins above are far above what fp32 arithmetic moves a score by: the fp32 run of the same code under its own selection."""
    from cliora_amd.hard import hard_forward_torch
    for name in HC.CLEAR:
        c = HC.CASES[name]
        P, x, _ = HC.case_inputs(c)
        with torch.no_grad():
            r32 = hard_forward_torch(P, x, c['share'], c['normalize'], dtype=torch.float32)
        r64 = HC.reference(name)
        assert torch.equal(r32['sel_in'], r64['sel_in']) and torch.equal(r32['sel_out'], r64['sel_out']), name
        err = max(float((r32[k].double() - r64[k]).abs().max()) for k in ('inside_s', 'outside_s'))
        scale = float(r64['inside_s'].abs().max())
        print('%s: fp32 scores off fp64 by %.3g at scale %.3g; smallest margin %.3g' % (name, err, scale, HC.min_margin_rel(r64) * scale))
        assert err <= 0.1 * HC.min_margin_rel(r64) * scale, (name, err)


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_hard_compose_geometry(tmp_path):
    exe = str(tmp_path / 'hard_geometry')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
           os.path.join(ROOT, 'tests', 'native', 'hard_geometry_driver.cpp')]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'hard geometry ok' in r.stdout


def test_python_refusals_need_no_gpu():
    """hard=True on what a hard chart does not take is refused in forward, before any tensor reaches the library."""
    from cliora_amd.cliora import DioraMLP as VL
    from cliora_amd.diora import DioraMLP
    from cliora_amd.treelstm import DioraTreeLSTM
    x = torch.zeros(2, 4, 16)
    m = DioraMLP(16, hard=True)
    assert m.hard is True and DioraMLP(16).hard is False
    for mod, words in [(VL(16), 'cliora_amd.cliora.DioraMLP'), (DioraTreeLSTM(16), 'DioraTreeLSTM'), (DioraMLP(16, compress=True), 'compress')]:
        mod.hard = True
        with pytest.raises(NotImplementedError, match='hard=True.*' + words):
            mod(x, x, *((torch.zeros(2, 3, 16), torch.zeros(2, 3, 16)) if mod.vision_language else ()))
    hooked = DioraMLP(16, hard=True)
    hooked.inside_hook = lambda level, h, c, s: None
    with pytest.raises(NotImplementedError, match='hard=True.*hook'):
        hooked(x, x)
    for slot in ('_ragged', '_ragged_train'):
        r = DioraMLP(16, hard=True)
        r.__dict__[slot] = (torch.zeros(2, dtype=torch.int32), 8)
        with pytest.raises(NotImplementedError, match='hard=True.*mixed lengths'):
            r(x, x)
    with pytest.raises(Exception, match='not a hard chart'):
        DioraMLP(16).hard_spans()
