"""CPU tests of the both-pass padded chart beyond 64 words (cliora_chart_forward_ragged_wide): the root-level
mask and its two-word split, the memory cap of ``pack``, the refusals that need no device, the masking scheme on the oracle at a
padded L of 65, and the premise of the end-to-end GPU test."""
import ctypes as C

import numpy as np
import pytest
import torch

import ragged_long_cases as RL
import ragged_outside_cases as ROC
from cliora_amd import _lib, diora, ragged
from oracle import diora_ref as R


# ---- the mask ---------------------------------------------------------------------------------------------------------------------
def test_root_level_mask_default_ignores_long_sentences_and_128_takes_them():
    assert ragged.root_level_mask([65, 128, 1]) == 1                        # the default: as before
    assert ragged.root_level_mask([0, 64, 65, 129]) == 1 << 63
    m = ragged.root_level_mask([65, 128, 1], max_len=128)
    assert m == (1 << 64) | (1 << 127) | 1
    assert ragged.root_level_mask([0, 129, 200], max_len=128) == 0
    assert ragged.root_level_mask(iter([64, 65]), max_len=128) == (1 << 63) | (1 << 64)      # the packs hand over a generator
    with pytest.raises(ValueError):
        ragged.root_level_mask([3], max_len=129)


def test_two_word_split_at_the_word_boundary():
    w = diora.split_root_levels(ragged.root_level_mask([64], max_len=128))
    assert (w[0], w[1]) == (1 << 63, 0)
    w = diora.split_root_levels(ragged.root_level_mask([65], max_len=128))
    assert (w[0], w[1]) == (0, 1)
    w = diora.split_root_levels(ragged.root_level_mask([1, 64, 65, 127, 128], max_len=128))
    assert (w[0], w[1]) == ((1 << 63) | 1, (1 << 63) | (1 << 62) | 1)
    assert C.sizeof(w) == 16 and isinstance(w[0], int)
    for t in (0, 1, 62, 63, 64, 65, 126, 127):                              # bit t & 63 of word t >> 6
        w = diora.split_root_levels(1 << t)
        assert [w[0], w[1]][t >> 6] == 1 << (t & 63) and [w[0], w[1]][1 - (t >> 6)] == 0


# ---- pack(max_long_batch=) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_batch,cap', [(64, 8), (16, 3), (4, 8), (64, 1)])
def test_pack_caps_the_packs_topped_by_a_long_sentence(max_batch, cap):
    lengths = RL.pack_seeded_lengths()
    assert sum(n > 64 for n in lengths) >= 10
    packs = ragged.pack(lengths, max_batch=max_batch, max_long_batch=cap)
    assert sorted(i for p in packs for i in p) == list(range(len(lengths)))         # every index exactly once
    longs = [p for p in packs if max(lengths[i] for i in p) > 64]
    assert longs and all(len(p) <= min(cap, max_batch) for p in longs)
    assert all(len(p) <= max_batch for p in packs)
    assert any(len(p) > cap for p in packs) or cap >= max_batch                     # the cap binds the long packs only
    for p in packs:                                                                 # longest first, as pack sorts them
        assert [lengths[i] for i in p] == sorted((lengths[i] for i in p), reverse=True)


def test_pack_without_long_sentences_or_without_the_cap_is_unchanged():
    rs = np.random.RandomState(4)
    short = [int(n) for n in rs.randint(1, 65, size=150)]
    assert ragged.pack(short, 16, 2.0, max_long_batch=2) == ragged.pack(short, 16, 2.0)
    lengths = RL.pack_seeded_lengths()
    assert ragged.pack(lengths, 16, 2.0, max_long_batch=None) == ragged.pack(lengths, 16, 2.0)
    # today's result, restated: greedy over (-length, index) with the waste rule and max_batch alone
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    want, cur, exact, top = [], [], 0, 0
    for i in order:
        w = ragged.work(lengths[i])
        if cur and (len(cur) >= 16 or (len(cur) + 1) * top > 3.0 * (exact + w)):
            want.append(cur)
            cur, exact = [], 0
        if not cur:
            top = w
        cur.append(i)
        exact += w
    want.append(cur)
    assert ragged.pack(lengths, 16, 2.0) == want
    with pytest.raises(ValueError):
        ragged.pack(lengths, 16, 2.0, max_long_batch=0)


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------
def test_wide_entry_refuses_before_any_hip_call():
    """Dummy pointers throughout: nothing may be dereferenced or launched.  Each refusal is CLIORA_EINVAL with a message of its own that
    starts with the entry's name."""
    L = _lib.lib()
    f = _lib.fn('cliora_chart_forward_ragged_wide')
    NAME = b'cliora_chart_forward_ragged_wide: '
    long_plan = _lib.Plan(2, 65, 16, forward_only=True)
    short_plan = _lib.Plan(2, 5, 16)
    full_plan = _lib.Plan(1, 128, 16, forward_only=True)
    lstm_plan = _lib.Plan(2, 5, 16, arch=1)
    one = C.c_void_p(16)
    prm = _lib.Params()
    prm.root_h = 16
    cmp_ = _lib.Params()
    cmp_.root_mat = 16
    ok = 1 | _lib.FWD_NO_BACKWARD
    kinds = {}

    def call(word, plan=long_plan, params=prm, flags=ok, words=(1, 0), lengths=one, status=one, drop=None, null_mask=False):
        mask = None if null_mask else (C.c_uint64 * 2)(*words)
        rc = f(plan.handle if plan is not None else None, C.byref(params) if params is not None else None, one, None, drop, one, one, one,
               one, None, one, C.c_size_t(plan.fwd_bytes if plan is not None else 0), flags, lengths, mask, status, None)
        msg = L.cliora_last_error()
        assert rc == -1 and msg.startswith(NAME) and word in msg, (rc, msg)          # CLIORA_EINVAL
        kinds[word] = msg

    for kw in (dict(plan=None), dict(params=None), dict(lengths=None), dict(status=None), dict(null_mask=True)):
        call(b'NULL argument', **kw)
    call(b'TreeLSTM', plan=lstm_plan)
    call(b'CLIORA_FWD_NO_BACKWARD', flags=1)
    call(b'PAIR_STATES', flags=ok | _lib.FWD_PAIR_STATES)
    call(b'root_mat', params=cmp_)
    call(b'drop_mask', drop=one)
    # a bit at or above L; bit L - 1, the chart's own root, is legal
    for plan, words in ((long_plan, (0, 2)), (long_plan, (0, 1 << 63)), (short_plan, (1 << 5, 0)), (short_plan, (0, 1)),
                        (short_plan, (1 << 63, 0))):
        call(b'at or above L', plan=plan, words=words)
    prev = L.cliora_set_resident(1)
    try:
        call(b'resident')
        # ... and with the legal top bits set the call gets as far as this last refusal: the mask itself was accepted
        call(b'resident', words=((1 << 64) - 1, 1))
        call(b'resident', plan=full_plan, words=((1 << 64) - 1, (1 << 64) - 1))
    finally:
        L.cliora_set_resident(prev)
    assert len(kinds) == 8 and len(set(kinds.values())) == 8             # eight refusals, each with a message of its own
    # the entry of L <= 64 and the training entries keep their refusal of a long plan
    rc = _lib.fn('cliora_chart_forward_ragged')(long_plan.handle, C.byref(prm), one, None, None, one, one, one, one, None, one,
                                                C.c_size_t(long_plan.fwd_bytes), ok, one, C.c_uint64(1), one, None)
    assert rc == -1 and b'root-level mask' in L.cliora_last_error()


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
def test_python_takes_long_sentences_up_to_the_device_check():
    net = RL.text_net()
    sents = [[1, 2, 3, 4, 5], list(range(1, 66))]
    with pytest.raises(_lib.ChartLibError, match='GPU only'):
        ragged.forward_ragged(net, sents, max_len=128)                   # nothing else refuses it: the call reaches the device check
    assert net.training                                                 # ... and the mode is restored
    with pytest.raises(_lib.ChartLibError, match='L > 64.*both-pass'):
        ragged.forward_ragged(net, sents)                               # the default, and its message, as before
    with pytest.raises(ValueError, match='max_len'):
        ragged.forward_ragged(net, sents, max_len=129)
    ran = []
    with pytest.raises(_lib.ChartLibError, match='L > 128'):
        ragged.forward_ragged(net, sents + [[1] * 129], max_len=128, per_pack=lambda *a: ran.append(a))
    assert not ran
    with pytest.raises(_lib.ChartLibError, match='L > 100.*max_len=128'):
        ragged.forward_ragged(net, [[1] * 101], max_len=100)
    # the module: a _ragged call at 64 < L <= 128 is taken; every other long-chart refusal stays
    from cliora_amd.diora import DioraMLP
    m = DioraMLP(16)
    x = torch.randn(2, 65, 16)
    m._ragged = (torch.tensor([65, 3], dtype=torch.int32), ragged.root_level_mask([65, 3], max_len=128))
    try:
        with pytest.raises(_lib.ChartLibError, match='inference only'):
            m(x, x)                                                     # training mode
        m.eval()
        with pytest.raises(_lib.ChartLibError, match='inference only'):
            m(x, x)                                                     # a parameter that needs a gradient
        with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='GPU only'):
            m(x, x)
        mc = DioraMLP(16, compress=True).eval()
        mc._ragged = m._ragged
        with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='compress'):
            mc(x, x)
        m.inside_hook = lambda *a: None
        with torch.no_grad(), pytest.raises(_lib.ChartLibError, match='hook'):
            m(x, x)
    finally:
        m._ragged = None


def test_entry_points_pass_max_len_through():
    import inspect
    from cliora_amd import evaluate, phrases
    for fn_ in (ragged.forward_ragged, evaluate.evaluate_ragged, phrases.embed_phrases_ragged):
        p = inspect.signature(fn_).parameters
        assert p['max_len'].default == 64 and p['max_long_batch'].default == 8, fn_.__name__
    for fn_ in (ragged.parse_ragged, ragged.encode_ragged):
        assert inspect.signature(fn_).parameters['max_long_batch'].default is None, fn_.__name__
    assert inspect.signature(ragged.pack).parameters['max_long_batch'].default is None
    assert 'cliora_chart_forward_ragged_wide' in _lib.ABI


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_masking_scheme_holds_on_the_oracle_at_a_padded_length_of_65():
    """fp32 masked_outside of the padded chart against the fp64 oracle at each exact length: the argument of DESIGN.md section 13 past
    the 64th level.  It pins the argument, not the code (it passes without the wide entry)."""
    D, lengths, seed = RL.SCHEME_CASE
    P, xs, lengths = ROC.small_case(D, lengths, seed=seed)
    Lmax = max(lengths)
    with torch.no_grad():
        pad = R.diora_forward(ROC.cast(P, torch.float32), ROC.padded(xs, Lmax), outside=False, normalize='unit', share=True)
        oh, os_ = ROC.masked_outside(ROC.cast(P, torch.float32), pad, lengths)
    assert bool(torch.isfinite(oh).all()) and bool(torch.isfinite(os_).all())
    worst = 0.0
    for b, n in enumerate(lengths):
        want = ROC.exact(P, xs[b])
        own = torch.from_numpy(ROC.own_cells(Lmax, n))
        for got, w in ((oh[b, own].double(), want['outside_h'][0]), (os_[b, own].double(), want['outside_s'][0])):
            worst = max(worst, float(((got - w).abs() / w.abs().clamp(min=1.0)).max()))
    print('masked outside pass at padded L %d: worst error %.3e (most negative outside_s %.3e)' % (Lmax, worst, float(os_.min())))
    assert worst <= RL.FORWARD_BOUND


def test_end_to_end_inputs_have_no_decisive_near_tie_in_fp64():
    """The premise of test_gpu_ragged_long.py's end-to-end test, which excuses no phrase."""
    net = ROC.vl_net().eval()
    gaps = []
    for ex in RL.e2e_examples():
        gaps += RL.decisive_gaps(ROC.oracle_atten(net, ex), RL.phrases_of(ex))
    print('%d phrases, smallest decisive gap %.3e of the scale' % (len(gaps), min(gaps)))
    assert len(gaps) == RL.E2E_PHRASES
    assert min(gaps) > RL.E2E_TIE
    assert abs(min(gaps) - RL.MEASURED_E2E_MIN_GAP) <= 0.02 * RL.MEASURED_E2E_MIN_GAP
