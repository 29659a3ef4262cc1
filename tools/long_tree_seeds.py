#!/usr/bin/env python
"""Chooses the seeded sentences of the long-chart tree tests (tests/long_cases.py: TREE_SEEDS) on the CPU.

A sentence is kept when the fp64 oracle's smallest gap between a CKY cell's two best candidates is at least `--margin`, which the
caller sets to four times the largest |inside_s| error measured on the device at that length (DESIGN.md section 13's rule).
    python tools/long_tree_seeds.py --length 128 --margin 4e-4 --count 4
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))

import long_cases as LC      # noqa: E402
import ragged_cases as RC    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--length', type=int, required=True)
    ap.add_argument('--margin', type=float, required=True)
    ap.add_argument('--count', type=int, default=4)
    ap.add_argument('--first', type=int, default=1000)
    ap.add_argument('--tries', type=int, default=200)
    a = ap.parse_args()
    kept = []
    for seed in range(a.first, a.first + a.tries):
        P, x = LC.tree_case(a.length, [seed])
        o = LC.oracle(P, x, outside=False, keep_pairs=True)
        gap = RC.cky_margin(o['pair_s_in'], a.length)
        print('seed %d gap %.3e %s' % (seed, gap, 'kept' if gap >= a.margin else ''), flush=True)
        if gap >= a.margin:
            kept.append((seed, gap))
            if len(kept) == a.count:
                break
    print('TREE_SEEDS[%d] = %s   # smallest gap %.3e' % (a.length, [s for s, _ in kept], min(g for _, g in kept) if kept else float('nan')))


if __name__ == '__main__':
    main()
