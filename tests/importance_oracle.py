"""NumPy restatement of the importance-neighborhood table of graphsage_amd/csrc/gs_importance.hip (the rule: include/graphsage_amd.h,
section IMPORTANCE): table and stats, bit for bit.

TEST INFRASTRUCTURE ONLY.  The reference has no such table (its neighborhoods are adjacency rows, minibatch.py:227-245); this
file is what the kernel is held to.  Plain Python integers per row, one rule after the other, no sort network and no packed keys:
nothing here shares a construction with the kernel.
"""
import numpy as np


def importance_row(walks, n_nodes, top, slots, pad_id):
    """walks: int array [num_walks, walk_len] of ONE start -> (row: list of `slots` ints, (m, nodes with a slot))."""
    u = int(walks[0][0])
    if not 0 <= u < n_nodes:                                         # rule 1
        return [pad_id] * slots, (0, 0)
    counts = {}
    for x in np.asarray(walks)[:, 1:].reshape(-1).tolist():          # rules 2 and 3
        if 0 <= x < n_nodes and x != u:
            counts[x] = counts.get(x, 0) + 1
    m = len(counts)
    if m == 0:
        return [pad_id] * slots, (0, 0)
    selected = sorted(counts, key=lambda x: (-counts[x], x))[:min(m, top)]            # rule 4
    C = sum(counts[x] for x in selected)                             # rule 5
    q = {x: counts[x] * slots // C for x in selected}
    r = {x: counts[x] * slots - q[x] * C for x in selected}
    rest = slots - sum(q.values())
    assert 0 <= rest <= sum(1 for x in selected if r[x] > 0) and (rest == 0 or rest < len(selected))
    n = dict(q)
    for x in sorted(selected, key=lambda x: (-r[x], x))[:rest]:
        n[x] += 1
    row = [x for x in sorted(selected) for _ in range(n[x])]         # rule 6
    assert len(row) == slots
    return row, (m, sum(1 for x in selected if n[x] > 0))


def importance_rows(paths, num_walks, walk_len, n_nodes, top, slots, pad_id):
    """paths int32 [n_starts * num_walks, >= walk_len] (gs_walk_paths: the walks of start i in rows i * num_walks ..) ->
    (table int32 [n_starts, slots], stats int32 [n_starts, 2])."""
    paths = np.asarray(paths)
    assert paths.ndim == 2 and paths.shape[0] % num_walks == 0 and paths.shape[1] >= walk_len >= 2 and num_walks >= 1
    n_starts = paths.shape[0] // num_walks
    table = np.empty((n_starts, slots), dtype=np.int32)
    stats = np.empty((n_starts, 2), dtype=np.int32)
    for i in range(n_starts):
        row, st = importance_row(paths[i * num_walks:(i + 1) * num_walks, :walk_len], n_nodes, top, slots, pad_id)
        table[i] = row
        stats[i] = st
    return table, stats
