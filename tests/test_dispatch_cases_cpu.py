"""tests/dispatch_cases.py on the CPU: the cases cover the inventory, a plan accepts every shape, the oracle of every case is quick enough
for a GPU test and its seed keeps the reference itself free of ReLU flips; and the launch record's host side (no launch happens here)."""
import threading

import pytest

import dispatch_cases as DC
from cliora_amd import _lib


def test_cases_cover_the_inventory_exactly():
    exp = DC.all_expected()
    assert exp - DC.INVENTORY == set(), sorted(exp - DC.INVENTORY)        # no case expects an instance the inventory does not list
    assert DC.INVENTORY - exp == set(), sorted(DC.INVENTORY - exp)        # every instance has a case
    assert not ((set(DC.NOT_REACHED) | set(DC.OUT_OF_SCOPE)) & DC.INVENTORY)
    for name in DC.PLACEMENT_CASES:
        assert name in DC.CASES and DC.CASES[name]['dma3x']


def test_inventory_entries_are_what_the_dispatchers_write():
    """Every inventory name is noted by a dispatcher (the string stands in its source), so a renamed entry cannot leave the inventory
    pointing at nothing."""
    import os
    src = ''
    for f in ('gemm_launch.hpp', 'api_mlp_launch.hpp'):
        src += open(os.path.join(os.path.dirname(_lib.HERE), 'cliora_amd', 'csrc', f)).read()
    for e in DC.INVENTORY:
        kernel = e.split('<')[0]
        assert 'inst("%s"' % kernel in src or (kernel == 'tn_gemm' and 'inst(rule.name' in src), e
    for variant in ('(two ranges)', '(level rows)'):
        assert 'tn_gemm_dma3x' + variant in src
    assert '"(level rows x" + std::to_string(ny)' in src           # the level rows carry their problem count: x3, x5


@pytest.mark.parametrize('name', sorted(DC.CASES) + ['forward'])
def test_a_plan_accepts_the_shape(name):
    c = DC.FORWARD_CASE if name == 'forward' else DC.CASES[name]
    p = _lib.Plan(c['B'], c['L'], c['D'], c['share'])         # host only: the tables are uploaded at the first forward
    assert p.Dp == (c['D'] + 15) // 16 * 16 and p.fwd_bytes > 0 and p.bwd_bytes > 0
    # the launch path: a plan of Dp <= 64 stays off the sentence-resident kernels only above 1000 span pairs per sentence and below 128 sentences
    if p.Dp <= 64:
        L = c['L']
        assert (L - 1) * L * (L + 1) // 2 > 1000 and c['B'] < 128


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_oracle_is_quick_and_its_seed_keeps_off_the_relu_kinks(name):
    """Both oracle runs within the time a GPU test may take (printed); the seed keeps every ReLU pre-activation of the fp64 reference
    RELU_MARGIN away from zero (dispatch_cases.relu_margin: what makes an fp32 run, the oracle's or the device's, agree with fp64 on
    every ReLU).  The fp32 oracle's own max / q99 -- the rule the margin stands for -- is printed, not asserted: it follows the host."""
    c = DC.CASES[name]
    margin = DC.relu_margin(c)
    print('%s: smallest |pre-activation| / std %.2g' % (name, margin))
    assert margin >= DC.RELU_MARGIN, margin
    r = DC.oracle(name)
    print('%s: fp64 %.1f s, fp32 %.1f s' % ((name,) + r['seconds']))
    worst = max((d['max'] / max(d['q99'], 1e-300), k) for k, d in r['fp32_dist'].items())
    print('%s: largest max / q99 of the fp32 oracle against fp64: %.1f (%s)%s' % ((name,) + worst + ('' if DC.kink_free(r['fp32_dist']) else ' -- a ReLU flipped on this host',)))
    assert sum(r['seconds']) <= 10.0, r['seconds']          # the limit a GPU test's reference is given, both runs together (measured: under 2 s)
    DC._ORACLE.pop(name, None)                              # (nothing else in this process needs it)


def test_forward_sentences():
    s = DC.forward_sentences()
    assert len(s) == 8 == len(set(s)) and s[0] == 0 and s[-1] == 231
    for b in s[1:-1]:
        assert (14 * b) // 16 != (14 * b + 13) // 16
    assert 232 * 14 >= 3200                                 # level 1 of both passes: 203 row groups x 5 column blocks >= 1000


def test_launch_record_host_side():
    """On / off / read without a launch: the previous state comes back, turning it on clears, the read is empty; and two host threads
    toggling and reading at once leave it consistent."""
    rec = _lib.fn('cliora_launch_record')
    prev = rec(0)
    try:
        assert rec(1) == 0 and rec(1) == 1 and rec(0) == 1 and rec(0) == 0
        with _lib.launch_record() as got:
            assert rec(1) == 1
        assert got == set() and rec(0) == 0
        errs = []

        def worker():
            try:
                for _ in range(200):
                    rec(1)
                    assert _lib.launch_record_read() == set()
                    rec(0)
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=worker) for _ in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
    finally:
        rec(prev)
