#!/usr/bin/env python
"""Generate index_tables_65.npz by RUNNING THE REFERENCE: its chart index tables for one length above 64.

Runs only where the reference is on disk (/root/reference), like make_golden.py; the test machines need only the .npz.  index_tables.npz
pins the closed forms of oracle/chart_layout.py (and through them the plan's tables) to the reference for L <= 40; this file does the
same at L = 65, the shortest length of a forward-only plan, stored as int32:
  off_65                 offset_cache.py            level offsets
  lidx_65 / ridx_65      inside_index.py            levels 1 .. 64 concatenated
  pidx_65 / sidx_65      outside_index.py           levels 63 .. 0 concatenated
Lengths 96 and 128 rest on the closed form alone (their tables would not fit the size limit of a committed file).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, '/root/reference')

from cliora.net.inside_index import get_inside_index      # noqa: E402
from cliora.net.outside_index import get_outside_index    # noqa: E402
from cliora.net.offset_cache import get_offset_cache      # noqa: E402

L = 65


def main():
    off = get_offset_cache(L)
    out = {'off_%d' % L: np.array([off[i] for i in range(L)], dtype=np.int32)}
    li, ri, pi, si = [], [], [], []
    for level in range(1, L):
        a, b = get_inside_index(L, level, off)
        li.append(a.numpy()); ri.append(b.numpy())
    for level in range(L - 2, -1, -1):
        a, b = get_outside_index(L, level, off)
        pi.append(a.numpy()); si.append(b.numpy())
    for name, parts in (('lidx', li), ('ridx', ri), ('pidx', pi), ('sidx', si)):
        out['%s_%d' % (name, L)] = np.concatenate(parts).astype(np.int32)
    path = os.path.join(HERE, 'index_tables_%d.npz' % L)
    np.savez_compressed(path, **out)
    print('wrote', os.path.basename(path), os.path.getsize(path) // 1024, 'KiB')


if __name__ == '__main__':
    main()
