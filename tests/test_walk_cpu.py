"""The one host walk of the restatements (cliora_amd/query.py: walk) against its definition, over every binary tree of 1 .. 6 words."""
import numpy as np

import posterior_cases as PC


def _post_order(bp, level, pos, out):
    """The definition: the left subtree, the right subtree, then the node."""
    if level == 0:
        return
    k = bp[(level, pos)]
    _post_order(bp, k, pos, out)
    _post_order(bp, level - k - 1, pos + k + 1, out)
    out.append((pos, pos + level))


def _pre_order(bp, level, pos, out):
    if level == 0:
        return
    k = bp[(level, pos)]
    out.append((level, pos))
    _pre_order(bp, k, pos, out)
    _pre_order(bp, level - k - 1, pos + k + 1, out)


def test_walk_is_the_post_order_chooses_in_pre_order_and_carries_the_kbest_ranks():
    from cliora_amd.query import walk, walk_spans
    count = 0
    for n in range(1, 7):
        for tree in PC.all_trees(n):
            bp = {(level, pos): k for level, pos, k in tree}
            want, order, calls = [], [], []
            _post_order(bp, n - 1, 0, want)
            _pre_order(bp, n - 1, 0, order)

            def choose(level, pos, state):
                calls.append((level, pos))
                return bp[(level, pos)], (state, 'l'), (state, 'r')
            rows = walk(n, choose, 'root')
            assert [r[:2] for r in rows] == want and len(want) == n - 1
            assert [r[2] for r in rows] == [bp[(e - s, s)] for s, e in want]
            assert calls == order                          # once per internal cell, the node before its subtrees, left first
            assert rows[-1][3] == 'root' if n > 1 else rows == []
            states = {(e - s, s): st for s, e, _, st in rows}
            for (level, pos), k in bp.items():             # every cell got the state its parent chose for its side
                for child, side in (((k, pos), 'l'), ((level - k - 1, pos + k + 1), 'r')):
                    if child[0] > 0:
                        assert states[child] == (states[(level, pos)], side)
            assert walk_spans(n, lambda level, pos: bp[(level, pos)]) == want
            count += 1
    assert count == 1 + 1 + 2 + 5 + 14 + 42
    # the rank as the walk's state: key[level][pos, rank] = (split, left rank, right rank).  The rows are those of the explicit-stack
    # walk of cliora_amd.kbest that this one replaced, computed with it before it went
    from cliora_amd.kbest import _walk
    key = {1: np.array([[[0, 0, 0]], [[0, 0, 0]], [[0, 0, 0]], [[0, 0, 0]]]),
           2: np.array([[[0, 0, 0], [1, 0, 0]], [[1, 0, 0], [0, 0, 0]], [[0, 0, 0], [1, 0, 0]]]),
           3: np.array([[[0, 0, 1], [1, 0, 0], [2, 1, 0]], [[2, 0, 0], [0, 0, 1], [1, 0, 0]]]),
           4: np.array([[[0, 0, 2], [3, 1, 0], [1, 0, 1], [2, 1, 0]]])}
    want = [[(1, 2), (3, 4), (1, 4), (0, 4)],
            [(0, 1), (2, 3), (0, 3), (0, 4)],
            [(0, 1), (2, 3), (2, 4), (0, 4)],
            [(0, 1), (0, 2), (3, 4), (0, 4)]]
    assert [_walk(key, 5, t) for t in range(4)] == want
    assert _walk(key, 1, 0) == []
