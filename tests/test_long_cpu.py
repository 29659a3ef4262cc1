"""CPU tests of forward-only plans for sentences of 65 .. 128 words (include/cliora_chart.h): their index tables against the closed
forms of oracle/chart_layout.py (the comparison test_plan_tables.py makes for L <= 40) and against the reference's own tables at
L = 65, what such a plan sizes, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest
import torch

import long_cases as LC
from cliora_amd import _lib, ragged
from cliora_amd.index import Index
from oracle import chart_layout as CL


@pytest.mark.parametrize('L', LC.LENGTHS)
def test_long_plan_tables_match_the_closed_forms(L):
    ix = Index()
    off = ix.get_offset(L)
    assert [off[i] for i in range(L)] == CL.level_offsets(L).tolist()
    for lv in range(1, L):
        a, b = ix.get_inside_index(L, lv)
        l, r = CL.inside_pairs(L, lv)
        assert np.array_equal(a.numpy(), l) and np.array_equal(b.numpy(), r), lv
    for lv in (L - 2, L - 3, L // 2, 1, 0):          # (the reordering to the reference's enumeration is a Python loop: a few levels)
        p, s = ix.get_outside_index(L, lv)
        wp, ws = CL.outside_pairs(L, lv)
        assert np.array_equal(p.numpy(), wp) and np.array_equal(s.numpy(), ws), lv
    pl = _lib.Plan(3, L, 48, forward_only=True)
    assert len(pl.table('pair_a_in')) == CL.n_inside_pairs(L) and len(pl.table('pair_a_out')) == CL.n_outside_pairs(L)
    bin_, bout = pl.table('pair_lvl_base_in'), pl.table('pair_lvl_base_out')
    assert [int(bin_[lv]) for lv in range(1, L)] == np.cumsum([0] + [(L - lv) * lv for lv in range(1, L - 1)]).tolist()
    assert [int(bout[lv]) for lv in range(L - 1)] == np.cumsum([0] + [(L - lv) * (L - lv - 1) for lv in range(L - 2)]).tolist()
    # every outside pair, in the plan's own order: sibling + target = parent
    offs = CL.level_offsets(L)
    sib, par = pl.table('pair_a_out').astype(np.int64), pl.table('pair_b_out').astype(np.int64)
    lvl_of = np.searchsorted(offs, np.arange(L * (L + 1) // 2), side='right') - 1
    tgt = np.concatenate([np.repeat(offs[lv] + np.arange(L - lv), L - lv - 1) for lv in range(L - 1)])
    span = lambda c: (c - offs[lvl_of[c]], c - offs[lvl_of[c]] + lvl_of[c])
    (ss, se), (ps, pe), (ts, te) = span(sib), span(par), span(tgt)
    assert ((ps == np.minimum(ss, ts)) & (pe == np.maximum(se, te)) & ((se + 1 == ts) | (te + 1 == ss))).all()
    geom = pl.table('level_geom').reshape(2 * L, 8)
    for pass_ in range(2):
        for lv in range(L):
            Lc, N, _, _, _, TG, SP, ntask = geom[pass_ * L + lv][[0, 1, 2, 3, 4, 5, 6, 7]]
            assert Lc == L - lv and N == (L - lv - 1 if pass_ else lv)
            assert TG in (1, 2, 4, 8) and SP in (1, 2, 4) and ntask == -(-(-(-3 * Lc // 16)) // TG) * SP, (pass_, lv)


def test_closed_forms_match_the_reference_at_65(golden):
    """oracle/chart_layout.py is pinned to the reference's tables for L <= 40 (test_oracle_golden.py); this pins it, and the plan, at
    one length above 64 (tests/golden/make_golden_index65.py)."""
    g = golden('index_tables_65.npz')
    L = 65
    assert np.array_equal(CL.level_offsets(L), g['off_65'])
    li = np.concatenate([CL.inside_pairs(L, lv)[0] for lv in range(1, L)])
    ri = np.concatenate([CL.inside_pairs(L, lv)[1] for lv in range(1, L)])
    pi = np.concatenate([CL.outside_pairs(L, lv)[0] for lv in range(L - 2, -1, -1)])
    si = np.concatenate([CL.outside_pairs(L, lv)[1] for lv in range(L - 2, -1, -1)])
    assert np.array_equal(li, g['lidx_65']) and np.array_equal(ri, g['ridx_65'])
    assert np.array_equal(pi, g['pidx_65']) and np.array_equal(si, g['sidx_65'])
    pl = _lib.Plan(1, L, 16, forward_only=True)
    assert np.array_equal(pl.table('pair_a_in'), g['lidx_65']) and np.array_equal(pl.table('pair_b_in'), g['ridx_65'])


def test_long_plan_sizes_the_forward_only():
    """No backward workspace, no pair-state tail, no use lists, no ReLU bits; the figure DESIGN.md section 14 quotes."""
    pl = _lib.Plan(8, 128, 400, forward_only=True)
    assert pl.bwd_bytes == 0 and pl.pair_bytes == 0
    assert pl.fwd_bytes == 1363988992                   # 1300.8 MiB
    for role in ('ina', 'inb', 'outa', 'outb'):
        assert len(pl.table('use_row_' + role)) == 0
    lib = _lib.lib()
    ym, pp, hp = (lib.cliora_plan_fwd_offset(pl.handle, n) for n in (b'ymask', b'pp', b'hp'))
    assert ym == lib.cliora_plan_fwd_offset(pl.handle, b'nrmi')        # an empty region
    short = _lib.Plan(8, 64, 400)
    assert short.bwd_bytes > 0 and short.pair_bytes > 0 and len(short.table('use_row_ina')) > 0
    # the plan cache's budget counts what the plan uploads: the pair tables and level tables, nothing else
    n_in, n_out = CL.n_inside_pairs(128), CL.n_outside_pairs(128)
    assert 4 * 2 * (n_in + n_out) <= pl.table_bytes <= 4 * 2 * (n_in + n_out) + 4 * (4 * (8256 + 1) + 18 * 128)


def test_long_plan_bounds_and_plan_level_refusals():
    with pytest.raises(_lib.ChartLibError, match='L > 128'):
        _lib.Plan(2, 129, 16, forward_only=True)
    with pytest.raises(_lib.ChartLibError, match='L > 64'):
        _lib.Plan(2, 65, 16)                            # a plan with a backward
    with pytest.raises(_lib.ChartLibError, match='TreeLSTM'):
        _lib.Plan(2, 65, 16, arch=1, forward_only=True)
    assert _lib.get_plan(2, 65, 16, True, 'unit', 0, -1).bwd_bytes == 0
    assert _lib.get_plan(2, 64, 16, True, 'unit', 0, -1).bwd_bytes > 0


def test_c_abi_refuses_what_a_long_plan_does_not_cover():
    """Argument checks come before any HIP call: each returns CLIORA_EINVAL and says why."""
    L = _lib.lib()
    p = _lib.Plan(2, 65, 16, forward_only=True)
    one = C.c_void_p(16)
    prm = _lib.Params()
    prm.root_h = 16

    def fwd(flags, params=prm):
        return L.cliora_chart_forward(p.handle, C.byref(params), one, None, None, one, one, one, one, None, one, C.c_size_t(p.fwd_bytes),
                                      flags, None)
    assert fwd(1) == -1 and b'CLIORA_FWD_NO_BACKWARD' in L.cliora_last_error()
    assert fwd(1 | _lib.FWD_NO_BACKWARD | _lib.FWD_PAIR_STATES) == -1 and b'PAIR_STATES' in L.cliora_last_error()
    cmp_ = _lib.Params()
    cmp_.root_mat = 16
    assert fwd(1 | _lib.FWD_NO_BACKWARD, cmp_) == -1 and b'compress' in L.cliora_last_error()
    prev = L.cliora_set_resident(1)
    try:
        assert fwd(1 | _lib.FWD_NO_BACKWARD) == -1 and b'resident' in L.cliora_last_error()
    finally:
        L.cliora_set_resident(prev)
    L.cliora_chart_backward.restype = C.c_int
    rc = L.cliora_chart_backward(p.handle, C.byref(prm), one, None, None, one, one, one, one, None, None, None, None, one,
                                 C.c_size_t(p.fwd_bytes), one, C.c_size_t(0), None, None, C.byref(prm), 1, None)
    assert rc == -1 and b'forward only' in L.cliora_last_error()
    rc = L.cliora_chart_forward_ragged(p.handle, C.byref(prm), one, None, None, one, one, one, one, None, one, C.c_size_t(p.fwd_bytes),
                                       1 | _lib.FWD_NO_BACKWARD, one, C.c_uint64(1), one, None)
    assert rc == -1 and b'root-level mask' in L.cliora_last_error()


def _net(D=50, V=97, E=32):
    from cliora_amd.harness import build_net
    torch.manual_seed(11)
    return build_net(D, torch.nn.Embedding(V, E), obj_feats=False)


def test_python_refusals_come_before_any_launch():
    """On CPU tensors: the long-chart refusals are raised before the chart path would complain about the device."""
    from cliora_amd.diora import DioraMLP
    m = DioraMLP(16)
    x = torch.randn(2, 65, 16)
    with pytest.raises(_lib.ChartLibError, match='inference only'):
        m(x, x)                                         # training mode at L 65
    m.eval()
    with pytest.raises(_lib.ChartLibError, match='inference only'):
        m(x, x)                                         # a parameter that needs a gradient
    with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='GPU only'):
        m(x, x)                                         # nothing else is refused: the call reaches the device check
    net = _net()
    sents = [[1, 2, 3, 4, 5], list(range(1, 66))]
    with pytest.raises(_lib.ChartLibError, match='L > 64'):
        ragged.parse_ragged(net, sents)                 # the default max_len
    with pytest.raises(_lib.ChartLibError, match='L > 64'):
        ragged.encode_ragged(net, sents)
    with pytest.raises(_lib.ChartLibError, match='L > 64.*both-pass'):
        ragged.forward_ragged(net, sents)
    with pytest.raises(_lib.ChartLibError, match='L > 128'):
        ragged.parse_ragged(net, [list(range(1, 97)) + list(range(1, 34))], max_len=128)
    with pytest.raises(ValueError):
        ragged.parse_ragged(net, sents, max_len=129)


def test_root_level_mask_is_unchanged():
    assert ragged.MAX_L == 64
    assert ragged.root_level_mask([0, 65]) == 0
    assert ragged.root_level_mask([1, 64, 65, 128]) == (1 << 0) | (1 << 63)


def test_pack_treats_long_sentences_like_any_other():
    lengths = LC.RAGGED_LENGTHS
    packs = ragged.pack(lengths, max_batch=4)
    assert sorted(i for p in packs for i in p) == list(range(len(lengths)))
    assert all(len(p) <= 4 for p in packs)
    assert packs[0][:2] == [4, 10]                      # the two sentences of 128 words first


@pytest.mark.parametrize('L', LC.LENGTHS)
def test_seeded_tree_sentences_have_no_near_tie_in_fp64(L):
    """The premise of test_gpu_long.py's tree test: no CKY cell of a seeded sentence has its two best candidates within NEAR_TIE[L]
    (four times the |inside_s| error measured on the device) in the fp64 oracle, so the reference alone excuses no sentence."""
    assert LC.TREE_SEEDS[L] and LC.NEAR_TIE[L] is not None
    gaps = LC.tree_oracle(L)['gaps']
    assert min(gaps) >= LC.NEAR_TIE[L], (L, gaps)
    assert abs(min(gaps) - LC.MEASURED_MIN_GAP[L]) <= 0.01 * LC.MEASURED_MIN_GAP[L]
