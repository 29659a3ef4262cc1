"""tests/vl_cases.py on the CPU: the cases cover the inventory, the inventory is what the dispatchers can name, a plan accepts every shape,
every case reaches the edge it is there for, and the seeds hold the rules that keep the fp64 reference comparable with an fp32 run
(ReLU margin, arg-max clearance, hinge clearance).  The counterpart of test_dispatch_cases_cpu.py; no launch happens here."""
import os

import pytest
import torch

import vl_cases as V
from cliora_amd import _lib

KINDS = {k: sorted(n for n, c in V.CASES.items() if c['kind'] == k) for k in ('score', 'max', 'contrastive', 'chart')}


def test_cases_cover_the_inventory_exactly():
    exp = V.all_expected()
    stray = sorted(x for x in exp if not any(V.matches(x, e) for e in V.INVENTORY))
    assert not stray, stray                                   # no case expects an instance the inventory does not list
    bare = sorted(e for e in V.INVENTORY if not any(V.matches(x, e) for x in exp))
    assert not bare, bare                                     # every instance has a case
    # every instance the dispatchers can name is reached by an admissible shape, or stands in NOT_REACHED with its reason
    assert V.INVENTORY | (set(V.NOT_REACHED) & V.NAMEABLE) == V.NAMEABLE, sorted(V.NAMEABLE ^ V.INVENTORY)
    assert not set(V.NOT_REACHED) & V.INVENTORY
    assert all(V.NOT_REACHED.values())


def test_every_scorer_entry_sees_every_tile_count():
    """Per scorer entry and arithmetic mode: every CT over NRp / 16 and every SC over Dp / 16 of the forward, every CT over Dp / 16 and SC
    over the segment of the backward, every TI x TJ of the region gradients; both wave counts; one segment, two and 31."""
    for mode in V.MODES:
        calls = {}
        for n in KINDS['score']:
            for call, s in V.expect(n, mode).items():
                calls.setdefault(call, set()).update(s)
        fwd = {e for e in calls['forward'] if e.startswith('rows_gemm_ws<')}
        assert {e[13] for e in fwd} == set('5421') and {e[15] for e in fwd} == set('5421')
        if mode == 'f32':               # (split mode: all_atten takes rows_gemm_ws3, and the B L rows of vg_atten stay below eight waves)
            assert {e[17] for e in fwd} == set('84')
        for call in ('sum_h', 'x_word'):
            ws = {e for e in calls[call] if e.startswith('rows_gemm_ws<')}
            assert {e[13] for e in ws} == set('5421') and {e[15] for e in ws} == set('5421'), (call, sorted(ws))
        for call in ('obj_span', 'obj_word'):
            assert {e for e in calls[call] if e.startswith('tn_gemm')} == {e for e in V.NAMEABLE if e.startswith('tn_gemm')}
            assert {'region_segments(one)', 'region_segments(several x2)', 'region_segments(several x31)'} <= calls[call]
    ws3 = set().union(*(s for n in V.CASES for s in V.expect(n, 'bf16x3').values()))
    assert {e for e in V.NAMEABLE if e.startswith('rows_gemm_ws3')} <= ws3
    assert {V.nchunk(V.CASES[n]['B']) for n in KINDS['max']} == set(range(1, 9))
    assert V.region_segments(512, 80) == (256, 2) and V.region_segments(496, 80) == (16, 31) and V.region_segments(2304, 400) == (384, 6)


def test_copy_and_store_paths_of_the_scorers():
    """In place (B R and D multiples of 16: the region matrix is read where it is) and through the packed copy, each with R % 4 == 0 (the
    vector store, one atomic per four regions) and without; padded D."""
    seen = set()
    for n in KINDS['score']:
        c = V.CASES[n]
        inplace = c['D'] % 16 == 0 and (c['B'] * c['R']) % 16 == 0
        seen.add(('in place' if inplace else 'padded' if c['D'] % 16 else 'packed', c['R'] % 4 == 0))
    assert seen >= {(how, r4) for how in ('in place', 'packed', 'padded') for r4 in (True, False)}, seen


def test_inventory_entries_are_what_the_dispatchers_write():
    """Every inventory name is noted where its kernel is launched (the string stands in the source)."""
    csrc = os.path.join(os.path.dirname(_lib.HERE), 'cliora_amd', 'csrc')
    src = {f: open(os.path.join(csrc, f)).read() for f in ('gemm_launch.hpp', 'api_vl.hip', 'api_mlp.hip', 'api_mlp_launch.hpp')}
    for k in ('rows_gemm_ws', 'rows_gemm_ws3'):
        assert 'inst("%s"' % k in src['gemm_launch.hpp']
    assert '"tn_gemm(ij)"' in src['api_vl.hip'] and 'inst(rule.name' in src['gemm_launch.hpp']
    for k in ('cell_attend_fwd', 'cell_attend_bwd', 'obj_grad_reduce'):
        assert 'NOTE_LAUNCH(inst("%s"' % k in src['api_mlp.hip'], k
    for s in ('"region_segments(one)"', '"region_segments(several x"', '"region_max_bwd_obj(nchunk "'):
        assert s in src['api_vl.hip'], s
    for e in V.INVENTORY:
        assert e.split('<')[0].split('(')[0] in ('rows_gemm_ws', 'rows_gemm_ws3', 'tn_gemm', 'cell_attend_fwd', 'cell_attend_bwd', 'obj_grad_reduce',
                                                  'region_segments', 'region_max_bwd_obj'), e
    # the thresholds the rules of vl_cases.py restate
    assert 'R <= 36 ? f(Int<9>{}) : f(Int<16>{})' in src['api_mlp_launch.hpp']
    assert '> 1536 ? 8 : 4' in src['gemm_launch.hpp'] and 'budget = 150 * 1024' in src['gemm_launch.hpp'] and '<= 150 * 1024' in src['api_vl.hip']
    assert 'std::max(4, (B + 7) / 8)' in src['api_vl.hip']


@pytest.mark.parametrize('name', KINDS['score'] + KINDS['max'] + KINDS['chart'])
def test_a_plan_accepts_the_shape(name):
    c = V.CASES[name]
    assert c['B'] <= V.MAX_B and c['L'] <= V.MAX_L and c['R'] <= V.MAX_R and c['D'] <= V.MAX_D
    p = _lib.Plan(c['B'], c['L'], c['D'], c.get('share', True), R=c['R'])         # host only
    assert p.Dp == V.pad16(c['D']) and p.C == V.n_cells(c['L']) and p.R == c['R']
    assert _lib.fn('cliora_plan_vl_workspace_bytes')(p.handle) > 0
    if c['kind'] == 'chart':
        assert c['L'] <= 4 or c['D'] <= 16          # the attention cases stay small: L <= 4 but for the one with 36 cells
        assert p.fwd_bytes > 0 and p.bwd_bytes > 0


@pytest.mark.parametrize('name', KINDS['chart'])
def test_chart_seed_keeps_off_the_relu_kinks_and_the_oracle_is_quick(name):
    c = V.CASES[name]
    margin = V.chart_relu_margin(c)
    print('%s: smallest |pre-activation| / std %.2g' % (name, margin))
    assert margin >= V.RELU_MARGIN, margin
    r = V.chart_oracle(name)
    worst = max((d['max'] / max(d['q99'], 1e-300), k) for k, d in r['fp32_dist'].items())
    print('%s: both oracle runs %.1f s; largest max / q99 of the fp32 oracle against fp64: %.1f (%s)' % ((name, r['seconds']) + worst))
    assert r['seconds'] <= 10.0
    mask = V.chart_inputs(c)[2]
    assert set(mask.unique().tolist()) <= {0.0, float(torch.tensor(1.0) / 0.9)} and float(mask.min()) == 0.0      # some region of some cell is dropped
    V._ORACLE.pop((name, 'chart'), None)


@pytest.mark.parametrize('name', KINDS['max'])
def test_arg_max_clearance(name):
    """At most 1 % of the (sentence, image, span) entries of the fp64 reference have their two best regions closer than the clearance
    (four times the fp32 einsum's largest error), in either mode's clearance: those are left out of the index comparison on the device."""
    c = V.CASES[name]
    o = V.max_oracle(name)
    for what, cl in (('exact', o['clearance']), ('split-bf16', V.split_bf16_clearance(o))):
        out = float((o['gap'] <= cl).double().mean())
        print('%s: %s clearance %.3g leaves out %.4f of %d entries' % (name, what, cl, out, o['gap'].numel()))
        assert out <= 0.01, (what, out)
    assert 0 < o['clearance'] < 1e-4 * float(o['val64'].abs().max())
    t = V.max_inputs(c)
    C = V.n_cells(c['L'])
    if c['skew'] or C > 64:
        # some (sentence, image) has one region winning more than four spans inside one block of 64 spans: the ballot loop goes round twice
        wins = torch.zeros(c['B'], c['B'], c['R']).scatter_add_(-1, o['arg64'][:, :, :64], torch.ones(c['B'], c['B'], min(C, 64)))
        assert float(wins.max()) > 4
    if c['half']:
        assert float(t['cot'][:, :, C // 2:].abs().max()) == 0.0 and float(t['cot'][:, :, :C // 2].abs().min()) > 0.0
    V._ORACLE.pop((name, 'max'), None)


@pytest.mark.parametrize('name', KINDS['contrastive'])
def test_hinge_clearance(name):
    """Every hinge argument margin + s - diag of the fp64 reference stays the clearance away from the floor, so an fp32 run clamps the
    same ones."""
    c = V.CASES[name]
    o = V.contrastive_oracle(name)
    print('%s: smallest hinge distance %.3g, clearance %.3g; loss %.6g' % (name, o['hinge_gap'], o['clearance'], float(o['ref64']['loss'])))
    assert o['hinge_gap'] >= o['clearance'], (o['hinge_gap'], o['clearance'])
    C = V.n_cells(c['L'])
    if c['B'] == 1 or C == 1:
        assert float(o['ref64']['loss']) == 0.0
    else:
        assert float(o['ref64']['loss']) > 0.0
    if c['lengths'] is not None:
        assert len(set(c['lengths'])) == 2 and max(c['lengths']) == c['L'] and C > 1024
    V._ORACLE.pop((name, 'contrastive'), None)


def test_the_edges_the_cases_are_there_for():
    con = {n: V.CASES[n] for n in KINDS['contrastive']}
    assert {(c['B'], c['L']) for c in con.values() if c['lengths'] is None} == {(3, 64), (1, 5), (4, 1), (128, 3)}
    assert V.n_cells(64) // 2 > 1024
    att = {(c['D'], c['R']) for c in (V.CASES[n] for n in KINDS['chart'])}
    assert att >= {(272, 37), (512, 64), (400, 36), (260, 63), (33, 3), (48, 35), (16, 2)}
    charts = [V.CASES[n] for n in KINDS['chart']]
    assert any(c['L'] == 2 for c in charts) and any(c['L'] == 8 and c['D'] == 16 for c in charts)
    assert any(not c['share'] for c in charts) and any(not c['training'] for c in charts)
    assert all(2 <= c['B'] <= 3 for c in charts)
    mx = [V.CASES[n] for n in KINDS['max']]
    assert {5, 17, 33} <= {c['B'] for c in mx} and any(V.n_cells(c['L']) > 64 for c in mx)
    assert any(c['skew'] for c in mx) and any(c['half'] for c in mx)
    w8 = V.CASES['waves8']
    assert (w8['B'], w8['L'], w8['R'], w8['D']) == (24, 12, 36, 16) and V.score_expect(24, 12, 36, 16, 'f32')['forward'] >= {'rows_gemm_ws<2,1,8>'}
