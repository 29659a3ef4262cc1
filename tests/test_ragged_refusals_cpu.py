"""Every refusal of the six padded-chart entries of csrc/api_ragged.hip, word for word: return code and full message of each entry
under each of its conditions, one at a time, against tests/golden/ragged_refusals.json.  Then the ORDER of the refusals: with a
condition and every later one of its entry set together, the entry answers with that condition's message.  Dummy pointers
throughout, so nothing is dereferenced or launched: every call here must be refused.

``python tests/test_ragged_refusals_cpu.py --record`` rewrites the golden file from the library as built; it was recorded on the
commit before the entries were folded into one description each and is not to be re-recorded for a change that means to keep them."""
import ctypes as C
import json
import os
import sys

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cliora_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ragged_refusals.json')
EINVAL = -1
ONE = C.c_void_p(16)              # "some pointer": never dereferenced, every call is refused first
FORWARDS = ('cliora_chart_forward_ragged', 'cliora_chart_forward_ragged_wide', 'cliora_chart_forward_ragged_train',
            'cliora_chart_forward_ragged_train_vl')

_plans = {}


def plan(kind):
    if kind not in _plans:
        _plans[kind] = {'short': lambda: _lib.Plan(2, 5, 16), 'long': lambda: _lib.Plan(2, 65, 16, forward_only=True),
                        'full': lambda: _lib.Plan(1, 128, 16, forward_only=True), 'lstm': lambda: _lib.Plan(2, 5, 16, arch=1),
                        'vl': lambda: _lib.Plan(2, 5, 16, R=4), 'vl_long': lambda: _lib.Plan(2, 65, 16, R=4, forward_only=True)}[kind]()
    return _plans[kind]


# A call every entry would take (were its pointers real), by entry; a case changes some of these.
#   plan: a key of plan() or None (NULL); params: 'root_h', 'root_mat' (compress) or None (NULL); nb / pair: the two flag bits;
#   obj, drop, lengths, status, d_obj: the pointer is given; words: the root-level mask (word 1 only reaches the wide entry);
#   null_mask: the wide entry's mask pointer is NULL; cots / masked: which of the four cotangents and of their buffers are given;
#   resident: cliora_set_resident(1) around the call.
COMMON = dict(params='root_h', pair=False, lengths=True, status=True, words=(1, 0), null_mask=False, resident=False)
BASE = {
    'cliora_chart_forward_ragged': dict(COMMON, plan='short', nb=True, obj=False, drop=False),
    'cliora_chart_forward_ragged_wide': dict(COMMON, plan='long', nb=True, obj=False, drop=False),
    'cliora_chart_forward_ragged_train': dict(COMMON, plan='short', nb=False, obj=False, drop=False),
    'cliora_chart_backward_ragged': dict(COMMON, plan='short', nb=False, obj=False, drop=False, d_obj=False, cots=(1, 1, 1, 1),
                                         masked=(1, 1, 1, 1)),
    'cliora_chart_forward_ragged_train_vl': dict(COMMON, plan='vl', nb=False, obj=True, drop=True),
    'cliora_chart_backward_ragged_vl': dict(COMMON, plan='vl', nb=False, obj=True, drop=True, d_obj=True, cots=(1, 1, 1, 1),
                                            masked=(1, 1, 1, 1)),
}

NULLS_FWD = [('NULL plan', dict(plan=None)), ('NULL params', dict(params=None)), ('NULL lengths', dict(lengths=False)),
             ('NULL status', dict(status=False))]
NULLS_BWD = [('NULL plan', dict(plan=None)), ('NULL lengths', dict(lengths=False))]
LSTM, PAIR, COMPRESS, DROP = ('TreeLSTM plan', dict(plan='lstm')), ('PAIR_STATES', dict(pair=True)), \
    ('compress', dict(params='root_mat')), ('drop_mask', dict(drop=True))
NO_MASKED = [('cotangent %d without its buffer' % k, dict(masked=tuple(int(j != k) for j in range(4)))) for k in range(4)]

# Per entry: its refusals IN THE ENTRY'S ORDER (the NULL checks are one refusal: only the last of them stands in the order), then
# further inputs of refusals already listed.
ORDER = {
    'cliora_chart_forward_ragged': NULLS_FWD + [LSTM, ('long plan', dict(plan='long')), ('without NO_BACKWARD', dict(nb=False)), PAIR,
                                                COMPRESS, DROP],
    'cliora_chart_forward_ragged_wide': NULLS_FWD + [('NULL mask', dict(null_mask=True)), LSTM, ('without NO_BACKWARD', dict(nb=False)),
                                                     PAIR, COMPRESS, DROP, ('bit 65 of L 65', dict(words=(0, 2))),
                                                     ('resident forced on', dict(resident=True))],
    'cliora_chart_forward_ragged_train': NULLS_FWD + [LSTM, ('CLIORA plan', dict(plan='vl')), ('obj_span on a text-only plan', dict(obj=True)),
                                                      ('long plan', dict(plan='long')), PAIR, COMPRESS, DROP,
                                                      ('with NO_BACKWARD', dict(nb=True))],
    'cliora_chart_backward_ragged': NULLS_BWD + [LSTM, ('CLIORA plan', dict(plan='vl')), ('obj_span on a text-only plan', dict(obj=True)),
                                                 ('long plan', dict(plan='long')), PAIR, COMPRESS, DROP, ('d_obj_span', dict(d_obj=True)),
                                                 NO_MASKED[0]],
    'cliora_chart_forward_ragged_train_vl': NULLS_FWD + [LSTM, ('text-only plan', dict(plan='short')), ('without obj_span', dict(obj=False)),
                                                         ('long plan', dict(plan='vl_long')), PAIR, COMPRESS,
                                                         ('with NO_BACKWARD', dict(nb=True))],
    'cliora_chart_backward_ragged_vl': NULLS_BWD + [LSTM, ('text-only plan', dict(plan='short')), ('without obj_span', dict(obj=False)),
                                                    ('long plan', dict(plan='vl_long')), PAIR, COMPRESS, NO_MASKED[0]],
}
MORE = {
    'cliora_chart_forward_ragged_wide': [
        ('top bit of word 1 at L 65', dict(words=(0, 1 << 63))), ('bit 5 of L 5', dict(plan='short', words=(1 << 5, 0))),
        ('word 1 at L 5', dict(plan='short', words=(0, 1))), ('bit 63 of L 5', dict(plan='short', words=(1 << 63, 0))),
        ('resident forced on, every legal bit of L 65', dict(resident=True, words=((1 << 64) - 1, 1))),
        ('resident forced on, every bit of L 128', dict(resident=True, plan='full', words=((1 << 64) - 1, (1 << 64) - 1)))],
    'cliora_chart_backward_ragged': NO_MASKED[1:] + [('one cotangent, no buffer', dict(cots=(0, 0, 1, 0), masked=(1, 1, 0, 1)))],
    'cliora_chart_backward_ragged_vl': NO_MASKED[1:] + [('one cotangent, no buffer', dict(cots=(0, 0, 1, 0), masked=(1, 1, 0, 1)))],
}
# The refusals of csrc/api_ragged.hip on the commit the golden file was recorded on, entry by entry (those of the two shared helpers
# counted under each entry that runs them): the table above must name at least as many.
REFUSALS = {'cliora_chart_forward_ragged': 7, 'cliora_chart_forward_ragged_wide': 8, 'cliora_chart_forward_ragged_train': 8,
            'cliora_chart_backward_ragged': 9, 'cliora_chart_forward_ragged_train_vl': 8, 'cliora_chart_backward_ragged_vl': 8}


def refusal(entry, **changes):
    """-> (return code, message) of `entry` called with its BASE arguments changed by `changes`."""
    a = dict(BASE[entry], **changes)
    L = _lib.lib()
    pl = plan(a['plan']) if a['plan'] is not None else None
    handle = pl.handle if pl is not None else None
    prm = None
    if a['params'] is not None:
        prm = _lib.Params()
        setattr(prm, a['params'], 16)
    pref = C.byref(prm) if prm is not None else None
    some = lambda given: ONE if given else None
    flags = 1 | (_lib.FWD_NO_BACKWARD if a['nb'] else 0) | (_lib.FWD_PAIR_STATES if a['pair'] else 0)
    fwd_bytes = C.c_size_t(pl.fwd_bytes if pl is not None else 0)
    if entry in FORWARDS:
        if entry.endswith('_wide'):
            mask = None if a['null_mask'] else (C.c_uint64 * 2)(*a['words'])
        else:
            mask = C.c_uint64(a['words'][0])
        args = (handle, pref, ONE, some(a['obj']), some(a['drop']), ONE, ONE, ONE, ONE, some(a['obj']), ONE, fwd_bytes, flags,
                some(a['lengths']), mask, some(a['status']), None)
    else:
        grads = _lib.Params()
        grads.root_h = 16
        args = (handle, pref, ONE, some(a['obj']), some(a['drop']), ONE, ONE, ONE, ONE, *map(some, a['cots']), None, ONE, fwd_bytes, ONE,
                C.c_size_t(pl.bwd_bytes if pl is not None else 0), ONE, some(a['d_obj']), C.byref(grads), flags, some(a['lengths']),
                C.c_uint64(a['words'][0]), *map(some, a['masked']), None)
    prev = L.cliora_set_resident(1) if a['resident'] else None
    try:
        rc = _lib.fn(entry)(*args)
        return rc, L.cliora_last_error().decode()
    finally:
        if prev is not None:
            L.cliora_set_resident(prev)


def cases():
    """-> [(entry, case name, changes)]: each refusal alone, then each with every later refusal of its entry set too (where two change
    the same argument, the earlier one's value stands)."""
    out = []
    for entry, order in ORDER.items():
        alone = order + MORE.get(entry, [])
        out += [(entry, name, ch) for name, ch in alone]
        for i, (name, _) in enumerate(order[:-1]):
            both = {}
            for _, ch in reversed(order[i:]):
                both.update(ch)
            out.append((entry, name + ' and every later refusal', both))
    return out


def run_cases():
    return [dict(entry=e, case=name, **dict(zip(('rc', 'message'), refusal(e, **ch)))) for e, name, ch in cases()]


def test_the_table_names_every_refusal_of_the_six_entries():
    assert set(ORDER) == set(BASE) == set(REFUSALS) and len(ORDER) == 6
    for entry, order in ORDER.items():
        nulls = sum(name.startswith('NULL') for name, _ in order)
        assert len(order) - nulls + 1 >= REFUSALS[entry], entry
    assert sum(REFUSALS.values()) == 48


def test_every_refusal_is_the_recorded_one_word_for_word():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = run_cases()
    assert [(w['entry'], w['case']) for w in want] == [(g['entry'], g['case']) for g in got]      # the table the file was recorded from
    for w, g in zip(want, got):
        assert g == w, (g, w)


def test_each_refusal_has_its_own_message_under_its_entrys_name_and_wins_over_the_later_ones():
    for entry, order in ORDER.items():
        alone = {name: refusal(entry, **ch) for name, ch in order + MORE.get(entry, [])}
        for name, (rc, msg) in alone.items():
            assert rc == EINVAL and msg.startswith(entry + ': '), (entry, name, rc, msg)
        kinds = {alone[name][1] for name, _ in order}            # MORE's inputs repeat refusals (with another L in the message)
        assert len(kinds) == REFUSALS[entry], (entry, sorted(kinds))
    for entry, name, ch in cases():
        if name.endswith(' and every later refusal'):
            first = name[:-len(' and every later refusal')]
            assert refusal(entry, **ch) == refusal(entry, **dict(ORDER[entry])[first]), (entry, name)


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: python tests/test_ragged_refusals_cpu.py --record')
    rows = run_cases()
    with open(GOLDEN, 'w') as f:
        json.dump(rows, f, indent=1)
        f.write('\n')
    print('recorded %d cases of %d entries in %s' % (len(rows), len(ORDER), GOLDEN))
