"""The mid-chain weight-gradient pieces (the projections' part from level ksplit, the pair rows' early dW2 after step J) are taken only
when the lane probe finds the weight-gradient stream concurrent with the chains (api_mlp.hip: wgrad_placement, sw_beside); with too few hardware queues
every weight gradient runs in the tail.  Whichever the default on this device, both placements must give the reference's gradients:
the existing oracle checks run once more in a fresh process with the pieces forced on through their switches (read once per process)."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('placement', [
    {'CLIORA_WGRAD_EARLY_STEP': '9', 'CLIORA_WGRAD_SPLIT_LEVEL': '6'},     # the pieces beside the chains, forced
    {'CLIORA_WGRAD_EARLY_STEP': '-1', 'CLIORA_WGRAD_SPLIT_LEVEL': '0'},    # everything in the tail, forced
])
def test_weight_gradient_placements_against_oracle(placement):
    env = dict(os.environ, **placement)
    sel = 'tests/test_gpu_parity.py::test_early_weight_gradient_ranges'
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-p', 'no:cacheprovider', '-m', 'gpu', sel],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
