"""cliora_amd.retrieval without a GPU: the fp64 restatements against the reference-made fixture and hand-made matrices, and the
refusals of the three C entries (dummy pointers: nothing launches)."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden

import retrieval_cases as RC

EINVAL, ENOMEM = -1, -3
ONE = C.c_void_p(16)              # "some pointer": never dereferenced, every call is refused first
NULL = C.c_void_p(0)


# ---- the reference's logits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['train', 'eval'])
def test_maxsim_numpy_is_the_reference_logit(which):
    """One weighted MaxSim form reproduces both logits of the reference (cliora.py:460 and 463-464 with trainer.py:145-152) on
    tests/golden/cliora_small.npz: fp64 arithmetic on the recorded fp32 data, within 1e-6."""
    from cliora_amd.retrieval import maxsim_numpy
    q, q_off, w, keys, k_off, want = RC.fixture_problem(load_golden('cliora_small.npz'), which)
    got = maxsim_numpy(q, q_off, w, keys, k_off)
    err = float(np.abs(got - want).max())
    print('%s: max |maxsim_numpy - reference logit| = %.3e' % (which, err))
    assert err <= 1e-6, err


@pytest.mark.parametrize('which', ['train', 'eval'])
def test_fixture_ranks_are_pinned(which):
    """The fixture's 4 x 4 logits have gaps of 4.4e-3 and more between neighbours, so its ranks (diagonal image_of) are the same from
    maxsim_numpy and from the recorded scores."""
    from cliora_amd.retrieval import maxsim_numpy, retrieval_ranks_numpy
    q, q_off, w, keys, k_off, want = RC.fixture_problem(load_golden('cliora_small.npz'), which)
    got = maxsim_numpy(q, q_off, w, keys, k_off)
    B = want.shape[0]
    a, b = retrieval_ranks_numpy(got, np.arange(B)), retrieval_ranks_numpy(want, np.arange(B))
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2] == 0
    order = np.argsort(-want, axis=1, kind='stable')                      # no ties in the fixture: a plain sort gives the ranks
    assert a[0].tolist() == [int(np.where(order[n] == n)[0][0]) for n in range(B)]
    order = np.argsort(-want, axis=0, kind='stable')
    assert a[1].tolist() == [int(np.where(order[:, m] == m)[0][0]) for m in range(B)]


def test_maxsim_numpy_edge_cases():
    from cliora_amd.retrieval import maxsim_numpy
    q = np.array([[1.0, 0.0], [0.0, -2.0], [NAN_, 1.0]])
    keys = np.array([[-1.0, 0.0], [0.0, 1.0], [2.0, 2.0], [NAN_, 0.0]])
    #          captions: {0,1}, {} , {2}         images: {0,1}, {}, {2}, {3}
    S = maxsim_numpy(q, [0, 2, 2, 3], np.array([0.5, 0.5, 1.0]), keys, [0, 2, 2, 3, 4])
    assert S[0, 0] == 0.5 * 0.0 + 0.5 * 0.0 and S[0, 2] == 0.5 * 2.0 + 0.5 * -4.0       # all-negative rows keep their maxima
    assert S[1].tolist() == [0.0, 0.0, 0.0, 0.0]                                      # an empty caption: zeros, against anything
    assert S[0, 1] == -np.inf                                                         # an empty image
    assert np.isnan(S[2, 0]) and np.isnan(S[2, 2]) and np.isnan(S[0, 3])              # NaN token -> its row, NaN region -> its column
    S = maxsim_numpy(q, [0, 2, 1, 3], np.ones(3), keys, [0, 5, 4])
    assert np.isnan(S[1]).all() and np.isnan(S[:, 0]).all() and np.isnan(S[:, 1]).all()   # decreasing / out-of-range offsets
    S = maxsim_numpy(np.ones((1, 1)), [0, 1], np.ones(1), np.ones((257, 1)), [0, 257])
    assert np.isnan(S[0, 0])                                                          # more than 256 regions


NAN_ = float('nan')


# ---- ranks and top-k on hand-made matrices ---------------------------------------------------------------------------------------------
def test_ranks_with_exact_ties():
    from cliora_amd.retrieval import retrieval_ranks_numpy
    S, io = RC.rank_cases()['ties']
    t2i, i2t, skipped = retrieval_ranks_numpy(S, io)
    # row 0: own image 1 ties images 0 and 2 -> only the earlier index orders before it; row 1: own image 1 leads its tie;
    # row 2: own image 3 holds -0.0 == 0.0 of image 2 (earlier index) under 2.0, 2.0; row 3: own image 2 ties images 0 and 3 under 2.0
    assert t2i.tolist() == [1, 0, 3, 2] and skipped == 0
    # column 1: captions 0 and 1 own it with 1.0 and 2.0; captions 2 and 3 tie caption 1 at 2.0 with later indices -> nobody before it
    # column 2: caption 3 owns it with -0.0; 1.0 and 2.0 are above, and caption 2's 0.0 ties with an earlier index -> three before it;
    # column 3: caption 2 owns it with -0.0; 0.5 and 2.0 are above, caption 3's 0.0 ties with a later index -> two
    assert i2t.tolist() == [-1, 0, 3, 2]


def test_ranks_five_captions_per_image():
    from cliora_amd.retrieval import retrieval_ranks_numpy
    S, io = RC.rank_cases()['five_per_image']
    t2i, i2t, _ = retrieval_ranks_numpy(S, io)
    for n in range(15):
        assert t2i[n] == sum(1 for m in range(3) if m != io[n] and S[n, m] > S[n, io[n]])
    for m in range(3):
        others = S[io != m, m]
        assert i2t[m] == min(int((others > S[n, m]).sum()) for n in np.where(io == m)[0])


def test_ranks_put_nan_below_every_number():
    from cliora_amd.retrieval import retrieval_ranks_numpy
    S, io = RC.rank_cases()['nan_row']
    t2i, i2t, _ = retrieval_ranks_numpy(S, io)
    assert t2i[2] == 2                       # a NaN row: everything ties as NaN, the two earlier indices order before image 2
    assert t2i[4] == 3                       # -inf: every number is above it
    assert t2i[5] == 0                       # +inf
    assert t2i[0] == sum(1 for m in (2, 3) if S[0, m] > S[0, 0])          # the NaN of image 1 orders below the own score
    assert i2t[2] == 5                       # column 2: its only caption holds a NaN, every other caption a number (or -inf)


def test_ranks_image_without_captions_and_bad_image():
    from cliora_amd.retrieval import retrieval_ranks_numpy
    S, io = RC.rank_cases()['image_without_captions']
    t2i, i2t, skipped = retrieval_ranks_numpy(S, io)
    assert skipped == 1 and t2i[3] == -1 and i2t[2] == -1 and (t2i[[0, 1, 2, 4]] >= 0).all()
    # the caption of no image still competes in the columns
    assert i2t[1] == int((np.delete(S[:, 1], 1) > S[1, 1]).sum())


def test_topk_numpy_order_and_padding():
    from cliora_amd.retrieval import score_topk_numpy
    S, _ = RC.rank_cases()['ties']
    D, I = score_topk_numpy(S, 6)
    assert I.tolist() == [[0, 1, 2, 3, -1, -1], [1, 2, 3, 0, -1, -1], [0, 1, 2, 3, -1, -1], [1, 0, 2, 3, -1, -1]]
    assert (D[:, 4:] == -np.inf).all() and D[1, :4].tolist() == [2.0, 2.0, 2.0, 0.5]
    S, _ = RC.rank_cases()['nan_row']
    D, I = score_topk_numpy(S, 3)
    assert I[2].tolist() == [0, 1, 2] and np.isnan(D[2]).all()
    assert I[5, 0] == 0 and D[5, 0] == np.inf
    D1, I1 = score_topk_numpy(S.T, 2)                                     # the captions per image
    assert I1[0, 0] == 5 and I1.shape == (4, 2)


# ---- refusals of the C entries -------------------------------------------------------------------------------------------------------
def _refused(name, code, *args):
    from cliora_amd import _lib
    rc = _lib.fn(name)(*args)
    msg = _lib.fn('cliora_last_error')().decode()
    assert rc == code, (rc, msg)
    assert msg.startswith(name + ':'), msg
    return msg


def _maxsim_args(**kw):
    a = dict(N=3, NT=40, M=2, MR=50, D=20, Q=ONE, ldq=20, q_off=ONE, w=ONE, O=ONE, ldo=20, o_off=ONE, S=ONE, lds=2, status=ONE, ws=ONE,
             ws_bytes=1 << 40, stream=NULL)
    a.update(kw)
    return [a[k] for k in ('N', 'NT', 'M', 'MR', 'D', 'Q', 'ldq', 'q_off', 'w', 'O', 'ldo', 'o_off', 'S', 'lds', 'status', 'ws', 'ws_bytes',
                           'stream')]


@pytest.mark.parametrize('change', [dict(D=0), dict(N=-1), dict(NT=-1), dict(M=-1), dict(MR=-1), dict(ldq=19), dict(ldo=19), dict(lds=1),
                                    dict(Q=NULL), dict(q_off=NULL), dict(w=NULL), dict(O=NULL), dict(o_off=NULL), dict(S=NULL),
                                    dict(status=NULL), dict(ws=NULL)])
def test_maxsim_refusals(change):
    _refused('cliora_maxsim_scores', EINVAL, *_maxsim_args(**change))


def test_maxsim_workspace_refusal_and_size():
    from cliora_amd import _lib
    size = _lib.fn('cliora_maxsim_workspace_bytes')
    need = size(3, 40, 2, 50, 20)
    assert need > 0
    msg = _refused('cliora_maxsim_scores', ENOMEM, *_maxsim_args(ws_bytes=need - 1))
    assert 'cliora_maxsim_workspace_bytes' in msg
    assert size(3, 40, 2, 50, 0) == 0 and size(-1, 40, 2, 50, 20) == 0
    # no buffer of NT x MR or NT x M elements: at Flickr30k test size the workspace is the packed operands, the layout tables and one
    # fp32 per (16-row query tile, image)
    N, NT, M, MR, D = 5000, 110000, 1000, 36000, 400
    qt, chunks = (NT + 15) // 16 + N + 3, (D + 31) // 32
    kt = 16 * min(M, 2 * (((MR + 15) // 16 + M) // 16) + 1)
    packed = (qt + kt) * chunks * 2048                   # the two operands in 16 x 32 fragment blocks, padding bounds included
    rest = (qt + kt + N + M) * 16 + qt * M * 4 + 16 * 256
    assert 0 < size(N, NT, M, MR, D) <= packed + rest
    assert rest < 4 * NT * M // 4                        # everything but the operands: under a quarter of an NT x M fp32 buffer
    assert packed + rest < 4 * NT * MR // 16             # and the whole far below the 16 GB (tokens x regions) intermediate


def test_ranks_and_topk_refusals():
    _refused('cliora_retrieval_ranks', EINVAL, -1, 2, ONE, 2, ONE, ONE, ONE, ONE, NULL)
    _refused('cliora_retrieval_ranks', EINVAL, 3, 2, ONE, 1, ONE, ONE, ONE, ONE, NULL)
    for k in range(2, 8):
        args = [3, 2, ONE, 2, ONE, ONE, ONE, ONE, NULL]
        args[k] = NULL if k != 3 else 2
        if k != 3:
            _refused('cliora_retrieval_ranks', EINVAL, *args)
    for k in (0, 129):
        _refused('cliora_score_topk', EINVAL, 3, 4, k, ONE, 4, 1, ONE, ONE, NULL)
    _refused('cliora_score_topk', EINVAL, -1, 4, 2, ONE, 4, 1, ONE, ONE, NULL)
    _refused('cliora_score_topk', EINVAL, 3, -1, 2, ONE, 4, 1, ONE, ONE, NULL)
    for k in (3, 6, 7):
        args = [3, 4, 2, ONE, 4, 1, ONE, ONE, NULL]
        args[k] = NULL
        _refused('cliora_score_topk', EINVAL, *args)


def test_wrapper_checks_before_any_launch():
    import torch
    from cliora_amd import retrieval
    with pytest.raises(ValueError, match='fp32 CUDA'):
        retrieval.maxsim_scores(torch.zeros(3, 4), [0, 3], torch.zeros(3), torch.zeros(2, 4), [0, 2])
    with pytest.raises(ValueError, match='one width'):
        retrieval._maxsim(torch.zeros(3, 4), [0, 3], torch.zeros(3), torch.zeros(2, 5), [0, 2], 256)
    with pytest.raises(ValueError, match='supports 1 <= k'):
        retrieval.score_topk(torch.zeros(3, 4), 129)
