"""Exact, layer-wise, full-neighborhood inference.

Training draws `num_samples` neighbors per node and recomputes a node's 2-hop tree in every batch it appears in.  Using a
trained model asks for something else: layer 1 for ALL nodes from their WHOLE neighbor lists, then layer 2 from layer 1 --
every node visited once per layer, no sampling noise.

    graph = FullGraph.from_csr(rowptr, col, n_nodes)            # or FullGraph.from_padded(adj)
    emb = model.embed_full(graph)                               # [N, d] l2-normalised (models.py:368-370)
    emb, preds = sup_model.predict_full(graph)                  # + softmax / sigmoid head (supervised_models.py:86-93)

`FullGraph` is a CSR adjacency over N + 1 rows (row N = the pad node) whose column ids have been checked ONCE, plus the
work-item plan of the reduce kernel (gs_csr_reduce_fwd, csrc/gs_csr_reduce.hip).

The pad-row rule.  The reference pads every adjacency row with the id N, and row N itself is [N, N, ...]
(minibatch.py:227-245); the pad node's FEATURES are zero but its hidden states are not once a bias is trained
(relu(0 . W + b) != 0).  So the pad row is computed like any other row, in every layer: `from_padded` keeps row N of the
table as it is, `from_csr` gives the pad node -- and every node without neighbors, whose reference row is all pad -- the
single neighbor N (a mean or max of identical entries is that entry).

The split rule.  One wave reduces one work item; a row longer than `split_len` (512) edges is cut into items of at most that
many, reduced by separate waves into a workspace and combined in segment order by a second small launch: a hub of thousands
of neighbors does not outlive the launch, no float atomics, one fixed summation order.  (CSR_SOFTMAX, the attention pooling
over the whole list: a partial carries its maximum and weight sum, and the combine rescales the partials to their common maximum.)

A node subset.  The same exact pass over only the rows a request depends on:

    emb, stats = model.embed_nodes(graph, nodes)                # rows in request order; stats: rows [|S_K| .. |S_0|], edges
    emb, preds, stats = sup_model.predict_nodes(graph, nodes)

S_K = the distinct requested ids, S_{l-1} = S_l U N(S_l), found on the device (gs_frontier_expand, csrc/gs_frontier.hip);
layer l is computed for the rows of S_l into a compact table, read and written through position maps (gs_csr_reduce_rows:
the window kernel's own item loop, so every row comes out with the same bits).  When |S_0| reaches about half of the graph
the whole-graph pass is the faster one (profiles/embed_nodes.md).

Link ranking.  What the exact embeddings are for: where does the true partner of a held-out edge (u, v) stand among ALL nodes?

    res = model.rank_full(graph, edges)                         # ranks, ranks_optimistic, n_gt, n_eq, scores, mrr, hits
    res = rank_full(engine, Z, edges, n_cand=N, filt=RankFilter.from_full_graph(graph))

One fused launch scores every (query, candidate) pair on the matrix cores and counts the candidates above / level with the
true partner in its epilogue (gs_rank_count, csrc/gs_rank.hip): no score matrix exists.  rank = 1 + n_gt + n_eq: a tie loses.

Retrieval.  The answer itself: which k nodes should u be linked to?

    res = model.topk_full(graph, nodes, k=10)                   # ids [n, k], scores [n, k], count [n]
    res = topk_full(engine, Z, nodes, 10, n_cand=N, filt=RankFilter.from_full_graph(graph))

The same sweep with a select epilogue (gs_topk_select, csrc/gs_topk.hip): order (score descending, id ascending), the scores
bit-equal to those rank_full reports for the same pair.
"""
import numpy as np

from . import ops
from ._lib import CSR_MAX, CSR_MEAN, CSR_MEAN_SELF, CSR_SOFTMAX, GraphsageAmdError  # noqa: F401

SPLIT_LEN = 512          # longest run of edges one wave reduces (rows beyond it are cut)


def plan_work_items(rowptr, split_len=SPLIT_LEN):
    """The work items of gs_csr_reduce_fwd for a CSR row pointer (NumPy, no device needed).

    Returns (items, item_ptr, splits):
      items    int64 [n_items, 4] = (row, first edge, count, partial slot or -1), rows ascending; a row of degree <= split_len
               is one item (count 0 for an empty row); a longer row is cut into ceil(deg / split_len) items of at most split_len
               edges with consecutive partial slots
      item_ptr int64 [n_rows + 1]: the items of row r are items[item_ptr[r]: item_ptr[r + 1]]
      splits   int64 [n_split, 3] = (row, first partial slot, partials) of the rows that were cut, rows ascending
    """
    rowptr = np.asarray(rowptr, dtype=np.int64)
    L = int(split_len)
    if L <= 0:
        raise GraphsageAmdError("split_len must be positive")
    n_rows = rowptr.shape[0] - 1
    deg = np.diff(rowptr)
    parts = np.where(deg > L, (deg + L - 1) // L, 1)
    item_ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(parts, out=item_ptr[1:])
    row = np.repeat(np.arange(n_rows, dtype=np.int64), parts)
    k = np.arange(item_ptr[-1], dtype=np.int64) - item_ptr[row]
    cut = np.flatnonzero(parts > 1)
    first = np.zeros(cut.shape[0] + 1, np.int64)
    np.cumsum(parts[cut], out=first[1:])
    slot0 = np.full(n_rows, -1, np.int64)
    slot0[cut] = first[:-1]
    items = np.empty((row.shape[0], 4), np.int64)
    items[:, 0] = row
    items[:, 1] = rowptr[row] + k * L
    items[:, 2] = np.minimum(L, deg[row] - k * L)
    items[:, 3] = np.where(slot0[row] >= 0, slot0[row] + k, -1)
    splits = np.stack([cut.astype(np.int64), first[:-1], parts[cut]], axis=1).reshape(-1, 3)
    return items, item_ptr, splits


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _partial_width(op, d):
    """Width of a cut row's partial: CSR_SOFTMAX carries its (max, sum) pair behind the accumulator."""
    return d + 4 if op == CSR_SOFTMAX else d


class FullGraph(object):
    """CSR adjacency over n_nodes + 1 rows (row n_nodes = the pad node), checked once, with its reduce plan."""

    def __init__(self, rowptr, col, n_nodes, split_len=SPLIT_LEN):
        self.n_nodes = int(n_nodes)
        self.n_rows = self.n_nodes + 1
        self.split_len = int(split_len)
        self._on_device = _is_torch(rowptr)
        if self._on_device != _is_torch(col):
            raise GraphsageAmdError("FullGraph: rowptr and col must both be NumPy arrays or both device tensors")
        if self._on_device:
            import torch
            if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or rowptr.dim() != 1 or col.dim() != 1:
                raise GraphsageAmdError("FullGraph: device CSR must be int64 rowptr / int32 col vectors")
            self.rowptr, self.col = rowptr.contiguous(), col.contiguous()
            rowptr_host = self.rowptr.cpu().numpy()
        else:
            self.rowptr = rowptr_host = np.ascontiguousarray(rowptr, dtype=np.int64)
            col = np.asarray(col)
            if col.size and (col.min() < np.iinfo(np.int32).min or col.max() > np.iinfo(np.int32).max):
                raise GraphsageAmdError("FullGraph: column ids do not fit int32")
            self.col = np.ascontiguousarray(col, dtype=np.int32)
        self._check(rowptr_host)
        self.nnz = int(rowptr_host[-1])
        self.rowptr_host = rowptr_host
        self.items, self.item_ptr, self.splits = plan_work_items(rowptr_host, self.split_len)
        self._dev = {}
        self._rank_filter = None

    def rank_filter(self):
        """Every edge of this graph as a RankFilter (built and uploaded once)."""
        if self._rank_filter is None:
            self._rank_filter = RankFilter.from_full_graph(self)
        return self._rank_filter

    def _check(self, rowptr_host):
        """rowptr non-decreasing from 0, rowptr[-1] == len(col), 0 <= col < n_rows: an id outside the table must never reach
        the kernel."""
        if rowptr_host.ndim != 1 or rowptr_host.shape[0] != self.n_rows + 1:
            raise GraphsageAmdError("FullGraph: rowptr must have n_nodes + 2 = %d entries (got %s)"
                                    % (self.n_rows + 1, rowptr_host.shape,))
        if rowptr_host[0] != 0 or (np.diff(rowptr_host) < 0).any():
            raise GraphsageAmdError("FullGraph: rowptr must start at 0 and be non-decreasing")
        n_col = int(self.col.numel() if self._on_device else self.col.shape[0])
        if int(rowptr_host[-1]) != n_col:
            raise GraphsageAmdError("FullGraph: rowptr[-1] = %d but col has %d entries" % (int(rowptr_host[-1]), n_col))
        if n_col:
            lo, hi = int(self.col.min()), int(self.col.max())
            if lo < 0 or hi >= self.n_rows:
                raise GraphsageAmdError("FullGraph: column ids must lie in [0, %d] (found %d .. %d)" % (self.n_nodes, lo, hi))

    # ------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def from_padded(cls, adj, split_len=SPLIT_LEN):
        """The reference's own multigraph: row v is adj[v] verbatim ([N + 1, max_degree] table of minibatch.py:227-259), the pad
        row included.  With num_samples == max_degree the reference's forward pass is the full pass over this graph."""
        adj = np.asarray(adj.cpu().numpy() if _is_torch(adj) else adj)
        if adj.ndim != 2 or adj.shape[0] < 1:
            raise GraphsageAmdError("FullGraph.from_padded: adj must be an [N + 1, max_degree] table")
        rowptr = np.arange(adj.shape[0] + 1, dtype=np.int64) * adj.shape[1]
        return cls(rowptr, adj.reshape(-1), adj.shape[0] - 1, split_len)

    @classmethod
    def from_csr(cls, rowptr, col, n_nodes, split_len=SPLIT_LEN):
        """The true graph: rows 0 .. n_nodes - 1 are the CSR's neighbor lists; every node without neighbors and the pad node
        n_nodes get the single neighbor n_nodes (the reference's all-pad row, minibatch.py:227-245).  NumPy arrays or
        device-resident tensors (int64 rowptr [n_nodes + 1], int32 col)."""
        n = int(n_nodes)
        if _is_torch(rowptr):
            import torch
            if rowptr.numel() != n + 1:
                raise GraphsageAmdError("FullGraph.from_csr: rowptr must have n_nodes + 1 entries")
            rp = rowptr.to(torch.int64)
            if int(rp[-1]) != col.numel() or int(rp[0]) != 0 or bool((rp[1:] < rp[:-1]).any()):
                raise GraphsageAmdError("FullGraph.from_csr: rowptr must run from 0 to len(col) without decreasing")
            deg = rp[1:] - rp[:-1]
            new_deg = torch.cat([torch.where(deg == 0, torch.ones_like(deg), deg), torch.ones_like(deg[:1])])
            new_rp = torch.zeros(n + 2, dtype=torch.int64, device=rp.device)
            new_rp[1:] = torch.cumsum(new_deg, 0)
            new_col = torch.full((int(new_rp[-1]),), n, dtype=torch.int32, device=rp.device)
            if col.numel():
                shift = torch.cumsum((deg == 0).to(torch.int64), 0) - (deg == 0).to(torch.int64)     # empty rows before each row
                src_row = torch.repeat_interleave(torch.arange(n, device=rp.device), deg)
                new_col[torch.arange(col.numel(), device=rp.device) + shift[src_row]] = col.to(torch.int32)
            return cls(new_rp, new_col, n, split_len)
        rp = np.asarray(rowptr, dtype=np.int64)
        col = np.asarray(col)
        if rp.ndim != 1 or rp.shape[0] != n + 1:
            raise GraphsageAmdError("FullGraph.from_csr: rowptr must have n_nodes + 1 entries")
        if rp[0] != 0 or (np.diff(rp) < 0).any() or int(rp[-1]) != col.shape[0]:
            raise GraphsageAmdError("FullGraph.from_csr: rowptr must run from 0 to len(col) without decreasing")
        deg = np.diff(rp)
        new_deg = np.concatenate([np.where(deg == 0, 1, deg), [1]])
        new_rp = np.zeros(n + 2, np.int64)
        np.cumsum(new_deg, out=new_rp[1:])
        new_col = np.full(int(new_rp[-1]), n, dtype=np.int64)
        if col.shape[0]:
            empty = (deg == 0).astype(np.int64)
            shift = np.cumsum(empty) - empty
            new_col[np.arange(col.shape[0]) + shift[np.repeat(np.arange(n), deg)]] = col
        return cls(new_rp, new_col, n, split_len)

    # ------------------------------------------------------------------------------------------------ host views
    def lists(self):
        """Neighbor list of every row (host copies; tests and oracles)."""
        rp = self.rowptr.cpu().numpy() if self._on_device else self.rowptr
        col = self.col.cpu().numpy() if self._on_device else self.col
        return [col[rp[r]:rp[r + 1]] for r in range(self.n_rows)]

    def window(self, row0, n):
        """(item range, split range, slot range) of the rows [row0, row0 + n)."""
        i0, i1 = int(self.item_ptr[row0]), int(self.item_ptr[row0 + n])
        s0, s1 = (int(x) for x in np.searchsorted(self.splits[:, 0], [row0, row0 + n]))
        t0 = int(self.splits[s0, 1]) if s0 < s1 else 0
        t1 = int(self.splits[s1 - 1, 1] + self.splits[s1 - 1, 2]) if s0 < s1 else 0
        return (i0, i1), (s0, s1), (t0, t1)

    def windows(self, max_rows):
        for r0 in range(0, self.n_rows, int(max_rows)):
            yield r0, min(int(max_rows), self.n_rows - r0)

    # ------------------------------------------------------------------------------------------------ device side
    def on(self, device):
        """(rowptr, col, items, splits) as tensors on `device` (uploaded once)."""
        key = str(device)
        if key not in self._dev:
            import torch
            up = (lambda a: a.to(device)) if self._on_device else (lambda a: torch.from_numpy(a).to(device))
            col = up(self.col)
            if col.numel() == 0:
                col = torch.zeros(1, dtype=torch.int32, device=device)[:0]
            splits = torch.from_numpy(self.splits).to(device) if self.splits.shape[0] else None
            self._dev[key] = (up(self.rowptr), col, torch.from_numpy(self.items).to(device), splits)
            torch.cuda.synchronize()
        return self._dev[key]

    def reduce(self, engine, op, X, out, row0, n, act=ops.ACT_IDENTITY):
        """out[0:n] = op over the whole neighbor lists of rows [row0, row0 + n) of the rows of X ([>= n_rows, d] Mat)."""
        if X.rows < self.n_rows:
            raise GraphsageAmdError("FullGraph.reduce: the table has %d rows, the graph %d" % (X.rows, self.n_rows))
        if out.rows < n or row0 < 0 or row0 + n > self.n_rows:
            raise GraphsageAmdError("FullGraph.reduce: bad row window [%d, +%d)" % (row0, n))
        rowptr, col, items, splits = self.on(engine.device)
        item_r, split_r, slot_r = self.window(row0, n)
        ws = None
        if slot_r[1] > slot_r[0]:
            words = ops.csr_reduce_ws_bytes(slot_r[1] - slot_r[0], _partial_width(op, X.d)) // 4
            ws = engine.ws_f32(("csr_reduce_ws",), max(1 << 16, 1 << (words - 1).bit_length()))     # few sizes, few buffers
        ops.csr_reduce_fwd(rowptr, col, items, splits, self.n_rows, self.split_len, op, X, out, row0, n, item_r, split_r,
                           slot_r, ws=ws, act=act, stream=engine.stream)
        return out

    # ------------------------------------------------------------------------------------------------ row subsets
    def plan_rows(self, rows):
        """(items, splits) of the row subset `rows` (ascending, duplicate-free, in [0, n_rows)), cut from the graph's own plan
        (NumPy, no device needed): the items of those rows in the plan's order, with the partial slots re-based to
        0 .. sum(splits[:, 2]) -- what gs_csr_reduce_rows takes."""
        rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int64)
        if rows.size and (rows[0] < 0 or rows[-1] >= self.n_rows or (np.diff(rows) <= 0).any()):
            raise GraphsageAmdError("FullGraph.plan_rows: rows must be ascending, duplicate-free ids in [0, %d)" % self.n_rows)
        first = self.item_ptr[rows]
        cnt = self.item_ptr[rows + 1] - first
        start = np.zeros(rows.shape[0] + 1, np.int64)
        np.cumsum(cnt, out=start[1:])
        items = self.items[np.repeat(first - start[:-1], cnt) + np.arange(start[-1], dtype=np.int64)]
        cut = items[:, 3] >= 0
        items[cut, 3] = np.arange(int(cut.sum()), dtype=np.int64)          # consecutive within a row, rows ascending
        splits = self.splits[np.isin(self.splits[:, 0], rows)] if self.splits.shape[0] else self.splits.copy()
        splits[:, 1] = np.cumsum(splits[:, 2]) - splits[:, 2]
        return items, splits

    def reduce_rows(self, engine, op, X, out, rows, out_pos, x_pos=None, act=ops.ACT_IDENTITY, plan=None):
        """out[out_pos[r]] = op over the whole neighbor list of every row r of `rows` (host ids: ascending, duplicate-free) of
        the rows X[x_pos[col]] (x_pos None: X is indexed by node id, [>= n_rows, d]).  out_pos / x_pos: int32 device maps
        [n_rows] (receptive_field makes them).  plan: the (items, splits) device tensors and slot count of plan_rows(rows), as
        upload_plan returns them, when the caller reduces the same rows more than once."""
        if x_pos is None and X.rows < self.n_rows:
            raise GraphsageAmdError("FullGraph.reduce_rows: the table has %d rows, the graph %d" % (X.rows, self.n_rows))
        rowptr, col, _, _ = self.on(engine.device)
        items, splits, n_slots = plan if plan is not None else self.upload_plan(engine, rows)
        ws = None
        if n_slots:
            words = ops.csr_reduce_ws_bytes(n_slots, _partial_width(op, X.d)) // 4
            ws = engine.ws_f32(("csr_reduce_ws",), max(1 << 16, 1 << (words - 1).bit_length()))
        ops.csr_reduce_rows(rowptr, col, items, splits, self.n_rows, self.split_len, op, X, out, out_pos, x_pos=x_pos,
                            n_slots=n_slots, ws=ws, act=act, stream=engine.stream)
        return out

    def upload_plan(self, engine, rows):
        """plan_rows(rows) on the engine's device: (items, splits or None, slot count)."""
        import torch
        items, splits = self.plan_rows(rows)
        n_slots = int(splits[:, 2].sum())
        items_dev = torch.from_numpy(items).to(engine.device) if items.shape[0] else \
            torch.zeros((1, 4), dtype=torch.int64, device=engine.device)[:0]
        splits_dev = torch.from_numpy(splits).to(engine.device) if splits.shape[0] else None
        torch.cuda.synchronize()          # the uploads ran on torch's stream; order them before the engine's
        return items_dev, splits_dev, n_slots


# ---------------------------------------------------------------------------------------------------- model passes
WINDOW_ROWS = 32768      # rows per launch group: the per-window workspaces (means, pooled rows, partials) do not grow with N


def _table(engine, rows, d, ld_multiple=4):
    import torch
    m = ops.Mat.zeros(rows, d, engine.device, ld_multiple)
    torch.cuda.synchronize()          # the zero-fill ran on torch's stream; order it before the engine's
    return m


def check_graph(model, graph):
    if not isinstance(graph, FullGraph):
        raise GraphsageAmdError("full-neighborhood inference needs a FullGraph (FullGraph.from_csr / from_padded)")
    if graph.n_rows != model.features.rows:
        raise GraphsageAmdError("the graph has %d rows (N + 1), the feature table %d" % (graph.n_rows, model.features.rows))


def layers_full(model, graph):
    """hidden[K] of models.py:321-330 for EVERY row of the graph: [N + 1, dim_mult * dims[-1]] Mat (before l2_normalize)."""
    check_graph(model, graph)
    e = model.engine
    e.sync()
    H = model.features
    for agg in model.aggregators:
        H = agg.infer_full(graph, H)
    return H


# ---------------------------------------------------------------------------------------------------- node subsets
def receptive_field(engine, graph, nodes, n_layers):
    """The rows a K-layer exact pass needs to answer `nodes`: S_K = the distinct requested ids, sorted, and
    S_{l-1} = S_l U N(S_l), found on the device (gs_frontier_expand; the graph's CSR may only exist there).

    Returns (sets, pos, edges), all ordered from the request down: sets[j] = S_{K-j} as an ascending int32 NumPy array
    (|S| int32s and one count word come back per layer), pos[j] = its int32 device map [n_rows] (index in the set, -1 for a
    non-member), edges[j] = the number of edges of the rows of S_{K-j}, j < K: what layer K - j visits."""
    import torch
    e = engine
    ids = np.asarray(nodes).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= graph.n_rows):
        raise GraphsageAmdError("node ids must lie in [0, %d]" % (graph.n_rows - 1))
    S = np.unique(ids).astype(np.int32)
    rowptr, col, _, _ = graph.on(e.device)
    S_dev = torch.from_numpy(S).to(e.device)
    pos = torch.full((graph.n_rows,), -1, dtype=torch.int32, device=e.device)
    pos[S_dev.long()] = torch.arange(S.shape[0], dtype=torch.int32, device=e.device)
    ws = e.ws_i32(("frontier_ws",), ops.frontier_ws_bytes(graph.n_rows) // 4)
    count = torch.zeros(1, dtype=torch.int32, device=e.device)
    sets, maps, edges = [S], [pos], []
    deg = np.diff(graph.rowptr_host)
    for _ in range(int(n_layers)):
        n_edges = int(deg[S].sum())
        cap = max(1, min(graph.n_rows, S.shape[0] + n_edges))
        rows_out = torch.empty(cap, dtype=torch.int32, device=e.device)
        pos = torch.empty(graph.n_rows, dtype=torch.int32, device=e.device)
        torch.cuda.synchronize()          # uploads and fills ran on torch's stream; order them before the engine's
        ops.frontier_expand(rowptr, col, graph.n_rows, S_dev if S.shape[0] else None, S.shape[0], rows_out, pos, count, ws,
                            stream=e.stream)
        e.sync()
        S_dev = rows_out[:int(count.item())]
        S = S_dev.cpu().numpy()
        sets.append(S)
        maps.append(pos)
        edges.append(n_edges)
    return sets, maps, edges


def _sage(e, H, self_ids, reduced, n, W_self, W_neigh, o, concat, act, bias, out):
    """The SAGE matmuls over [rows self_ids of H | reduced] (H None: the one-matrix GCN call, no self operand)."""
    ops.sage_dense_fwd(H, self_ids if H is not None else None, reduced, None, n, W_self, W_neigh, o, concat, act, bias, out,
                       stream=e.stream)


class GraphLayer(object):
    """The scope of a layer computed for EVERY row of `graph` in row windows of WINDOW_ROWS (read at call time): it computes
    and may read all n_rows rows, and every table is indexed by node id.  An aggregator's infer(scope, H) is written on the
    output-table allocator `table` and the four primitives below it; RowsLayer offers the same five for a row subset.  `agg`
    names the engine and the workspaces.  `of_src` (is X the layer's source table, or a `dense` table over the readable rows?)
    only matters where the two are indexed differently, in RowsLayer's compact tables: here both are indexed by node id."""

    def __init__(self, graph):
        self.graph = graph

    def _windows(self):
        return self.graph.windows(WINDOW_ROWS)

    def table(self, agg, d):
        """A zeroed [computed rows, d] output table."""
        return _table(agg.engine, self.graph.n_rows, d)

    def dense(self, agg, H, stack, spare=0):
        """The Dense stack [(W, bias, width, act), ...] over every row the layer may read: a table indexed like those rows.
        The intermediate of a two-layer stack lives in a per-window workspace.  spare: zeroed columns kept behind the table's
        own (the logit column of CSR_SOFTMAX), inside its leading dimension."""
        e = agg.engine
        T = self.table(agg, stack[-1][2] + spare).cols_slice(0, stack[-1][2])
        mid = e.ws_mat((agg.name, "full_h1"), min(WINDOW_ROWS, self.graph.n_rows), stack[0][2]) if len(stack) > 1 else None
        for r0, n in self._windows():
            X, k = H.rows_slice(r0, r0 + n), H.d
            for i, (W, bias, width, act) in enumerate(stack):
                Y = T.rows_slice(r0, r0 + n) if i + 1 == len(stack) else mid.rows_slice(0, n)
                ops.gemm(False, False, n, width, k, X, W, Y, bias=bias, act=act, stream=e.stream)
                X, k = Y, width
        return T

    def self_gemm(self, agg, H, W, width, dst, act):
        """dst = act(computed rows of H . W): the self term into the output table or a column slice of it."""
        for r0, n in self._windows():
            ops.gemm(False, False, n, width, H.d, H.rows_slice(r0, r0 + n), W, dst.rows_slice(r0, r0 + n), act=act,
                     stream=agg.engine.stream)

    def reduce(self, agg, op, X, of_src, dst, act=ops.ACT_IDENTITY):
        """dst = act(op over every computed row's whole neighbor list of the rows of X).  X is the layer's source table
        (of_src) or a table over the readable rows (dense); dst the output table or a column slice of it."""
        for r0, n in self._windows():
            self.graph.reduce(agg.engine, op, X, dst.rows_slice(r0, r0 + n), r0, n, act=act)
        return dst

    def reduce_sage(self, agg, op, X, of_src, H, W_self, W_neigh, o, concat, act, bias):
        """reduce X into a workspace of whole 128-byte lines per row, then the SAGE matmuls over [computed rows of H | reduced]
        (H None: one matrix, no self operand).  Returns the output table."""
        e = agg.engine
        out = self.table(agg, o * (2 if concat else 1))
        # ld_multiple=32 for every aggregator: the mean forms always had it; the pooling forms' hidden widths (256, 512, 1024:
        # _PoolBase._WIDTHS) are multiples of 32, so their workspace keeps the leading dimension the default of 4 gave it
        reduced = e.ws_mat((agg.name, "full_reduced"), min(WINDOW_ROWS, self.graph.n_rows), X.d, ld_multiple=32)
        for r0, n in self._windows():
            self.graph.reduce(e, op, X, reduced, r0, n)
            _sage(e, H.rows_slice(r0, r0 + n) if H is not None else None, None, reduced, n, W_self, W_neigh, o, concat, act, bias,
                  out.rows_slice(r0, r0 + n))
        return out


class RowsLayer(object):
    """The scope of a layer of layers_nodes: compute the layer for the rows `rows` (S_l, n of them) into a compact [n, d_out]
    table, from the table `src` of the layer below.  The same `table` and four primitives as GraphLayer.

      rows / rows_dev   S_l: ascending host ids / the same on the device (int32)
      out_pos           device map id -> row of the output table (pos of S_l)
      prev_n            |S_{l-1}|: the rows of the layer below that this layer may read
      prev_ids          device ids that pick S_{l-1} out of `src`, in set order; None when src IS the compact table over S_{l-1}
      prev_pos          device map id -> index in S_{l-1}: the x_pos of a compact table over S_{l-1}
      src_pos           the x_pos of `src` itself (None: src is indexed by node id, the feature table)
      self_ids          device ids that pick the rows of S_l out of `src`, in set order
      plan              upload_plan(rows): shared by every reduce of the layer"""

    def __init__(self, graph, engine, rows, rows_dev, out_pos, prev_rows_dev, prev_pos, by_id):
        self.graph, self.rows, self.rows_dev, self.n, self.out_pos = graph, rows, rows_dev, int(rows.shape[0]), out_pos
        self.prev_n, self.prev_pos = int(prev_rows_dev.numel()), prev_pos
        self.prev_ids = prev_rows_dev if by_id else None
        self.src_pos = None if by_id else prev_pos
        self.self_ids = rows_dev if by_id else prev_pos[rows_dev.long()]
        self.plan = graph.upload_plan(engine, rows)

    def table(self, agg, d):
        return _table(agg.engine, self.n, d)

    def dense(self, agg, H, stack, spare=0):
        e = agg.engine
        tables = [_table(e, self.prev_n, width) for _, _, width, _ in stack[:-1]]
        tables.append(_table(e, self.prev_n, stack[-1][2] + spare).cols_slice(0, stack[-1][2]))
        X, idx, k = H, self.prev_ids, H.d
        for (W, bias, width, act), Y in zip(stack, tables):
            ops.gemm(False, False, self.prev_n, width, k, X, W, Y, a_row_idx=idx, bias=bias, act=act, stream=e.stream)
            X, idx, k = Y, None, width
        return X

    def self_gemm(self, agg, H, W, width, dst, act):
        ops.gemm(False, False, self.n, width, H.d, H, W, dst, a_row_idx=self.self_ids, act=act, stream=agg.engine.stream)

    def reduce(self, agg, op, X, of_src, dst, act=ops.ACT_IDENTITY):
        return self.graph.reduce_rows(agg.engine, op, X, dst, self.rows, self.out_pos,
                                      x_pos=self.src_pos if of_src else self.prev_pos, act=act, plan=self.plan)

    def reduce_sage(self, agg, op, X, of_src, H, W_self, W_neigh, o, concat, act, bias):
        out = self.table(agg, o * (2 if concat else 1))
        reduced = _table(agg.engine, self.n, X.d, ld_multiple=32)
        self.reduce(agg, op, X, of_src, reduced)
        _sage(agg.engine, H, self.self_ids, reduced, self.n, W_self, W_neigh, o, concat, act, bias, out)
        return out


def layers_nodes(model, graph, nodes):
    """hidden[K] for the rows `nodes` depend on only: layer l is computed for the rows of S_l (receptive_field) into a compact
    [|S_l|, d] table, layer 0 reading model.features by node id.  Returns (table over S_K Mat, S_K ids, pos of S_K, stats)
    with stats = {"rows": [|S_K|, ..., |S_0|], "edges": [...], "n_rows": N + 1}."""
    import torch
    check_graph(model, graph)
    e = model.engine
    e.sync()
    K = len(model.aggregators)
    if np.asarray(nodes).size == 0:
        raise GraphsageAmdError("receptive-field inference needs at least one node")
    sets, maps, edges = receptive_field(e, graph, nodes, K)
    devs = [torch.from_numpy(np.ascontiguousarray(S)).to(e.device) for S in sets]
    torch.cuda.synchronize()
    H = model.features
    for l, agg in enumerate(model.aggregators):
        j = K - 1 - l                          # sets[j] = S_{l+1}: the rows this layer computes; sets[j + 1] the rows it reads
        H = agg.infer_rows(RowsLayer(graph, e, sets[j], devs[j], maps[j], devs[j + 1], maps[j + 1], by_id=(l == 0)), H)
    e.sync()
    return H, sets[0], maps[0], {"rows": [int(S.shape[0]) for S in sets], "edges": edges, "n_rows": graph.n_rows}


def _gather(model, table, idx):
    """(rows Mat [n, d], n): rows `idx` (host indices) of `table` on the device, at least one row allocated."""
    import torch
    e = model.engine
    idx_dev = torch.from_numpy(idx.astype(np.int32)).to(e.device)
    torch.cuda.synchronize()
    out = _table(e, max(idx.size, 1), table.d)
    if idx.size:
        ops.gather_rows(table, idx_dev, out=out, stream=e.stream)
    e.sync()
    return out, int(idx.size)


def request_rows(model, table, S, nodes):
    """(rows Mat [n, d], n): the rows of the compact table over the sorted distinct ids S in REQUEST order (a duplicate request
    is answered twice)."""
    return _gather(model, table, np.searchsorted(S, np.asarray(nodes).reshape(-1)))


def select_rows(model, table, nodes):
    """(rows Mat [n, d], n): the rows `nodes` of a layer table (default: the N real nodes, in id order)."""
    if nodes is None:
        return table.rows_slice(0, table.rows - 1), table.rows - 1
    ids = np.ascontiguousarray(np.asarray(nodes).reshape(-1), dtype=np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= table.rows):
        raise GraphsageAmdError("node ids must lie in [0, %d]" % (table.rows - 1))
    return _gather(model, table, ids)


def l2_rows(engine, rows, n):
    """The first n rows of `rows` l2-normalised (models.py:368-370) into a new table of at least one row; the launch is left on
    the engine's stream."""
    y = _table(engine, max(n, 1), rows.d)
    ops.l2norm_fwd(rows, n, y, None, stream=engine.stream)
    return y


# ---------------------------------------------------------------------------------------------------- link ranking
class RankFilter(object):
    """Known edges to leave out of a ranking: a CSR over the candidate table's rows (row u = the ids that are no candidates for
    a query from u), rows sorted and de-duplicated, ids checked ONCE on the host (an id outside the table must never reach the
    kernel), uploaded once per device."""

    def __init__(self, rowptr, col, n_nodes):
        self.n_nodes = int(n_nodes)
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self._dev = {}

    @classmethod
    def from_csr(cls, rowptr, col, n_nodes):
        """rowptr [n_nodes + 1], col with entries in [0, n_nodes); rows in any order, duplicates allowed."""
        n = int(n_nodes)
        rp = np.asarray(rowptr.cpu().numpy() if _is_torch(rowptr) else rowptr).astype(np.int64)
        col = np.asarray(col.cpu().numpy() if _is_torch(col) else col).reshape(-1)
        if n < 0 or rp.ndim != 1 or rp.shape[0] != n + 1:
            raise GraphsageAmdError("RankFilter: rowptr must have n_nodes + 1 = %d entries" % (n + 1))
        if rp[0] != 0 or (np.diff(rp) < 0).any() or int(rp[-1]) != col.shape[0]:
            raise GraphsageAmdError("RankFilter: rowptr must run from 0 to len(col) without decreasing")
        if col.size and (col.min() < 0 or col.max() >= n):
            raise GraphsageAmdError("RankFilter: ids must lie in [0, %d) (found %d .. %d)" % (n, col.min(), col.max()))
        # rows that already are strictly ascending (a CSR built by sorting edges usually is) are taken as they are: one pass
        # over neighboring entries, no sort and no 64-bit key per edge
        rising = col[1:] > col[:-1]
        starts = rp[1:-1]
        rising[starts[(starts > 0) & (starts < col.shape[0])] - 1] = True          # the step from one row into the next
        if rising.all():
            return cls(rp, col, n)
        key = np.unique(np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * max(n, 1) + col)      # sorts and de-duplicates
        new_rp = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(key // max(n, 1), minlength=n), out=new_rp[1:])
        return cls(new_rp, key % max(n, 1), n)

    @classmethod
    def from_full_graph(cls, graph):
        """Every edge of a FullGraph (its pad row and pad entries included: the pad node is no candidate anyway)."""
        rp = graph.rowptr.cpu().numpy() if graph._on_device else graph.rowptr
        col = graph.col.cpu().numpy() if graph._on_device else graph.col
        return cls.from_csr(rp, col, graph.n_rows)

    def lists(self):
        return [self.col[self.rowptr[r]:self.rowptr[r + 1]] for r in range(self.n_nodes)]

    def on(self, device, n_rows):
        """(rowptr int64 [n_rows + 1], col int32) on `device` for a table of n_rows >= n_nodes rows (the rows beyond the filter's
        are empty)."""
        if n_rows < self.n_nodes:
            raise GraphsageAmdError("RankFilter: the filter covers %d rows, the table has %d" % (self.n_nodes, n_rows))
        key = (str(device), int(n_rows))
        if key not in self._dev:
            import torch
            rp = np.concatenate([self.rowptr, np.full(n_rows - self.n_nodes, self.rowptr[-1], np.int64)])
            col = torch.from_numpy(self.col).to(device) if self.col.size else torch.zeros(1, dtype=torch.int32, device=device)
            self._dev[key] = (torch.from_numpy(rp).to(device), col)
            torch.cuda.synchronize()
        return self._dev[key]


def rank_metrics(n_gt, n_eq, hits=(1, 10, 50, 100)):
    """ranks = 1 + n_gt + n_eq (the reference's convention, models.py:392-404: the true score stands last in aff_all and top_k is
    stable, so a tie loses), ranks_optimistic = 1 + n_gt, mrr = mean(1 / ranks), hits[k] = share of ranks <= k."""
    n_gt = np.asarray(n_gt, dtype=np.int64)
    n_eq = np.asarray(n_eq, dtype=np.int64)
    ranks = 1 + n_gt + n_eq
    return {"ranks": ranks, "ranks_optimistic": 1 + n_gt, "n_gt": n_gt, "n_eq": n_eq,
            "mrr": float(np.mean(1.0 / ranks)) if ranks.size else 0.0,
            "hits": {int(k): (float(np.mean(ranks <= k)) if ranks.size else 0.0) for k in hits}}


def _queries(engine, Z, ids, filt, weights, who):
    """What rank_full and topk_full do before their launch: (src, Xq, f_rowptr, f_col) = the query ids on the device, their rows
    of Z (times the bilinear weights, if any) and the filter's device CSR.  Ends with everything torch's stream did in order."""
    import torch
    e = engine
    if weights is not None and (weights.rows != Z.d or weights.d != Z.d):
        raise GraphsageAmdError("%s: bilinear weights must be [%d, %d]" % (who, Z.d, Z.d))
    src = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(e.device)
    f_rowptr, f_col = filt.on(e.device, Z.rows) if filt is not None else (None, None)
    Xq = _table(e, src.numel(), Z.d)
    U = _table(e, src.numel(), Z.d) if weights is not None else None
    torch.cuda.synchronize()              # uploads and zero-fills ran on torch's stream; order them before the engine's
    ops.gather_rows(Z, src, out=Xq, stream=e.stream)
    if weights is not None:
        ops.gemm(False, False, src.numel(), Z.d, Z.d, Xq, weights, U, stream=e.stream)
        Xq = U
    return src, Xq, f_rowptr, f_col


def rank_full(engine, Z, edges, *, n_cand=None, filt=None, exclude_self=True, weights=None, hits=(1, 10, 50, 100)):
    """Rank the true partner of every edge (src, dst) among the rows 0 .. n_cand - 1 of the device table Z ([n_rows, d] Mat): the
    score of a candidate w is <Z[src], Z[w]>, or <Z[src] . A, Z[w]> with the bilinear weights A ([d, d] Mat, prediction.py:68-92,
    applied on the query side as in neg_cost).  dst itself, src (exclude_self) and the filter row of src (filt: RankFilter;
    independent of exclude_self: with exclude_self=False the query node only names its filter row and stays a candidate)
    are no candidates.  One fused score-and-count launch per 65,536 queries (gs_rank_count); no score matrix exists."""
    import torch
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    Q = edges.shape[0]
    n_cand = Z.rows if n_cand is None else int(n_cand)
    if not 0 <= n_cand <= Z.rows:
        raise GraphsageAmdError("rank_full: n_cand = %d, the table has %d rows" % (n_cand, Z.rows))
    if Q and (edges.min() < 0 or edges.max() >= Z.rows):
        raise GraphsageAmdError("rank_full: edge ends must lie in [0, %d)" % Z.rows)
    if Q == 0:
        res = rank_metrics(np.zeros(0, np.int64), np.zeros(0, np.int64), hits)
        res["scores"] = np.zeros(0, np.float32)
        return res
    e = engine
    dst = torch.from_numpy(np.ascontiguousarray(edges[:, 1], dtype=np.int32)).to(e.device)
    out = (torch.zeros(Q, dtype=torch.float32, device=e.device), torch.zeros(Q, dtype=torch.int32, device=e.device),
           torch.zeros(Q, dtype=torch.int32, device=e.device))
    ws = torch.zeros(max(2, max(ops.rank_ws_bytes(n, n_cand) for n in {min(Q, ops.RANK_CHUNK), Q % ops.RANK_CHUNK}) // 4),
                     dtype=torch.int32, device=e.device)
    src, Xq, f_rowptr, f_col = _queries(e, Z, edges[:, 0], filt, weights, "rank_full")
    ops.rank_count(Xq, Z, dst, n_cand=n_cand, src=src if (exclude_self or filt is not None) else None,
                   keep_src=not exclude_self, f_rowptr=f_rowptr,
                   f_col=f_col, t=out[0], n_gt=out[1], n_eq=out[2], ws=ws, stream=e.stream)
    e.sync()
    res = rank_metrics(out[1].cpu().numpy(), out[2].cpu().numpy(), hits)
    res["scores"] = out[0].cpu().numpy()
    return res


# ---------------------------------------------------------------------------------------------------- retrieval
def topk_full(engine, Z, nodes, k, *, n_cand=None, filt=None, exclude_self=True, weights=None):
    """The k best-scoring partners of every node in `nodes` among the rows 0 .. n_cand - 1 of the device table Z ([n_rows, d]
    Mat): the score of a candidate w for the query node u is <Z[u], Z[w]>, or <Z[u] . A, Z[w]> with the bilinear weights A (as
    rank_full).  u itself (exclude_self) and the filter row of u (filt: RankFilter; independent of exclude_self: with
    exclude_self=False the query node only names its filter row and stays a candidate) are no candidates.  Returns
    {"ids": int32 [n, k], "scores": float32 [n, k], "count": int32 [n]} as NumPy arrays, every row in the order (score
    descending, id ascending); entries at and beyond count = min(k, candidates) are -1 / -inf.  One fused score-and-select
    launch per 65,536 queries (gs_topk_select); no score matrix exists."""
    import torch
    nodes = np.ascontiguousarray(np.asarray(nodes).reshape(-1), dtype=np.int64)
    Q, k = nodes.shape[0], int(k)
    n_cand = Z.rows if n_cand is None else int(n_cand)
    if not 1 <= k <= ops.TOPK_MAX:
        raise GraphsageAmdError("topk_full: k = %d must lie in [1, %d]" % (k, ops.TOPK_MAX))
    if not 0 <= n_cand <= Z.rows:
        raise GraphsageAmdError("topk_full: n_cand = %d, the table has %d rows" % (n_cand, Z.rows))
    if Q and (nodes.min() < 0 or nodes.max() >= Z.rows):
        raise GraphsageAmdError("topk_full: node ids must lie in [0, %d)" % Z.rows)
    if Q == 0:
        return {"ids": np.zeros((0, k), np.int32), "scores": np.zeros((0, k), np.float32), "count": np.zeros(0, np.int32)}
    e = engine
    out = (torch.zeros((Q, k), dtype=torch.int32, device=e.device), torch.zeros((Q, k), dtype=torch.float32, device=e.device),
           torch.zeros(Q, dtype=torch.int32, device=e.device))
    need = max(ops.topk_ws_bytes(n, n_cand, k) for n in {min(Q, ops.RANK_CHUNK), Q % ops.RANK_CHUNK})
    ws = torch.zeros(max(1, (need + 7) // 8), dtype=torch.int64, device=e.device)
    src, Xq, f_rowptr, f_col = _queries(e, Z, nodes, filt, weights, "topk_full")
    ops.topk_select(Xq, Z, k, n_cand=n_cand, src=src if (exclude_self or filt is not None) else None,
                    keep_src=not exclude_self, f_rowptr=f_rowptr, f_col=f_col, ids=out[0], scores=out[1], count=out[2], ws=ws,
                    stream=e.stream)
    e.sync()
    return {"ids": out[0].cpu().numpy(), "scores": out[1].cpu().numpy(), "count": out[2].cpu().numpy()}
