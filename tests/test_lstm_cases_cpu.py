"""The yardstick of test_gpu_treelstm_limits.py, checked on the CPU: at every case of lstm_cases.CASES the oracle's own fp32 run stays
within a tenth of the device's bounds of its fp64 run, so those bounds are never met by the reference only narrowly; and the
structural facts the device test relies on (which gradients do not exist at L = 1 and without the outside pass) hold in fp64."""
import numpy as np
import pytest
import torch

import lstm_cases as LC


@pytest.mark.parametrize('D,B,L,share,outside', LC.CASES)
def test_fp32_oracle_is_a_tenth_of_the_bounds_from_fp64(D, B, L, share, outside):
    ref = LC.oracle64(D, B, L, share, outside)
    got = LC.oracle_run(D, B, L, share, outside, torch.float32)
    out = max(LC.rel_err(got['out'][k], ref['out'][k]) for k in LC.KEYS)
    grads = [LC.rel_err(got['x_grad'], ref['x_grad'])]
    for k, g in ref['grad'].items():
        assert (g is None) == (got['grad'][k] is None), k
        if g is not None:
            grads.append(LC.rel_err(got['grad'][k], g))
    print('D %d B %d L %d share %d outside %d: fp32 oracle against fp64: outputs %.2e gradients %.2e' % (D, B, L, share, outside, out, max(grads)))
    assert out <= 0.1 * LC.OUT_TOL
    assert max(grads) <= 0.1 * LC.GRAD_TOL


def test_one_word_has_no_gradient_on_u_and_mat():
    """L = 1: leaves and root only.  The compose weight U and the score matrix are not used, and of the gate bias only the three
    leaf blocks B[:3D]."""
    for D, B, L, share, outside in LC.CASES:
        if L != 1:
            continue
        g = LC.oracle64(D, B, L, share, outside)['grad']
        assert g['inside_compose_func.U'] is None and g['inside_score_func.mat'] is None
        assert g['inside_compose_func.W'] is not None and g['root_vector_out_h'] is not None and g['root_vector_out_c'] is not None
        b = g['inside_compose_func.B']
        assert np.abs(b[:3 * D]).max() > 0 and not b[3 * D:].any()
        break
    else:
        raise AssertionError('no L = 1 case')


def test_inside_only_has_no_gradient_on_the_outside_parameters():
    seen = 0
    for D, B, L, share, outside in LC.CASES:
        if outside:
            continue
        seen += 1
        ref = LC.oracle64(D, B, L, share, outside)
        g = ref['grad']
        assert g['root_vector_out_h'] is None and g['root_vector_out_c'] is None
        if not share:
            assert all(g[k] is None for k in ('outside_compose_func.U', 'outside_compose_func.B', 'outside_score_func.mat'))
        assert all(g[k] is not None for k in ('inside_compose_func.W', 'inside_compose_func.U', 'inside_compose_func.B', 'inside_score_func.mat'))
        for k in LC.KEYS[3:]:
            assert not ref['out'][k].any(), k
    assert seen == 2
