"""SURVEY.md section 8(b) "Selection": with cliora_amd/shim ahead of the reference on sys.path, the reference's own
build_net (cliora/net/trainer.py:518-526, 552) constructs the MI355X-native chart modules without any edit to the
reference.  build_net picks its chart class by importing `DioraMLP` from `cliora.net.diora` (--obj_feats off) or
`cliora.net.cliora` (on) and calls it as `Diora(size, outside=True, normalize=..., compress=False, share=...)`.
tests/golden/shim_selection.npz records, from the reference's own build_net, which module that is and the state_dict keys
of what it builds; here the same imports and the same call go through the shim alone (the reference is not on the path)
and must land on the native modules with exactly those keys.  Construction is CPU-side, no chart call is made."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import importlib, json, sys
import torch
want = json.loads(sys.argv[1])
for tag, native in (('text', 'cliora_amd.diora'), ('vl', 'cliora_amd.cliora')):
    mod = importlib.import_module(want['module__' + tag])             # build_net's `from cliora.net.<x> import DioraMLP as Diora`
    assert mod.__file__.startswith(ROOT), mod.__file__
    diora = mod.DioraMLP(16, outside=True, normalize='unit', compress=False, share=True)
    assert type(diora).__module__ == native, type(diora).__module__
    assert sorted(diora.state_dict()) == want['keys__' + tag], (sorted(diora.state_dict()), want['keys__' + tag])
print('shim ok')
'''


def test_reference_build_net_selects_the_native_modules(golden, tmp_path):
    g = golden('shim_selection.npz')
    want = {k: (str(v) if v.ndim == 0 else [str(s) for s in v]) for k, v in g.items() if k != 'meta'}
    assert set(want) == {'module__text', 'keys__text', 'module__vl', 'keys__vl'}
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'cliora_amd', 'shim'), ROOT]))
    code = 'ROOT = %r\n' % ROOT + SCRIPT
    r = subprocess.run([sys.executable, '-c', code, json.dumps(want)], env=env, cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and 'shim ok' in r.stdout, r.stdout + r.stderr
