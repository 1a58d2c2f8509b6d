"""Typed Python wrappers over the C ABI (one function per entry point of include/graphsage_amd.h).

`Mat` is a row-major fp32 device matrix with a padded leading dimension (what every kernel expects:
16-byte aligned base, ld % 4 == 0).  torch only owns the memory.
"""
import ctypes

import torch

from . import _lib
from ._lib import ACT_IDENTITY, ACT_RELU, call, ptr  # noqa: F401


def round_up(x, m):
    return (x + m - 1) // m * m


class Mat(object):
    """fp32 [rows, d] matrix stored in a [rows, ld] buffer, ld % 4 == 0 (pad columns are zero)."""

    __slots__ = ("buf", "d")

    def __init__(self, buf, d):
        assert buf.dim() == 2 and buf.dtype == torch.float32 and buf.stride(1) == 1
        assert buf.stride(0) % 4 == 0 and buf.data_ptr() % 16 == 0 and d <= buf.shape[1]
        self.buf = buf
        self.d = d

    @staticmethod
    def zeros(rows, d, device, ld_multiple=4):
        ld = round_up(max(d, 1), ld_multiple)
        return Mat(torch.zeros((rows, ld), dtype=torch.float32, device=device), d)

    @staticmethod
    def from_numpy(a, device, ld_multiple=4):
        import numpy as np
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim == 1:
            a = a[None, :]
        m = Mat.zeros(a.shape[0], a.shape[1], device, ld_multiple)
        m.buf[:, : a.shape[1]].copy_(torch.from_numpy(a))
        return m

    @property
    def rows(self):
        return self.buf.shape[0]

    @property
    def ld(self):
        return self.buf.stride(0)

    @property
    def ptr(self):
        return ptr(self.buf)

    def view(self):
        """Logical [rows, d] view (torch tensor)."""
        return self.buf[:, : self.d]

    def numpy(self):
        return self.view().detach().cpu().numpy()

    def rows_slice(self, r0, r1):
        return Mat(self.buf[r0:r1], self.d)

    def cols_slice(self, c0, c1):
        """Columns [c0, c1) as a matrix with the same leading dimension (c0 % 4 == 0)."""
        assert c0 % 4 == 0 and c1 <= self.buf.shape[1]
        return Mat(self.buf[:, c0:c1], c1 - c0)


def current_stream():
    return torch.cuda.current_stream().cuda_stream


def _s(stream):
    return current_stream() if stream is None else stream


# ------------------------------------------------------------------------------------------ K1
def sample_padded(adj, ids, col_perm, num_samples, out=None, stream=None):
    n = ids.numel()
    if out is None:
        out = torch.empty((n * num_samples,), dtype=torch.int32, device=ids.device)
    call("gs_sample_padded", ptr(adj), adj.shape[0], adj.shape[1], ptr(ids), n, ptr(col_perm), num_samples,
         ptr(out), _s(stream))
    return out


def sample_uniform_csr(rowptr, col, n_nodes, pad_id, ids, num_samples, seed, step=0, step_dev=None, hop=0,
                       global_row_offset=0, out=None, stream=None, law=0, max_degree=0):
    n = ids.numel()
    if out is None:
        out = torch.empty((n * num_samples,), dtype=torch.int32, device=ids.device)
    call("gs_sample_uniform_csr", ptr(rowptr), ptr(col), n_nodes, pad_id, ptr(ids), n, num_samples,
         seed & 0xFFFFFFFFFFFFFFFF, step, ptr(step_dev), hop, global_row_offset, law, max_degree, ptr(out), _s(stream))
    return out


def sample_fanout_csr(rowptr, col, n_nodes, pad_id, fans, offsets, ids_all, B, seed, step_dev=None, hop0=0,
                      root_offset=0, order=None, cursor_dev=None, label_table=None, labels_out=None, stream=None,
                      law=0, max_degree=0):
    """Fused multi-hop sampler (+ optional batch/label staging); see gs_sample_fanout_csr."""
    import ctypes
    fan = (ctypes.c_int32 * len(fans))(*fans)
    off = (ctypes.c_int64 * len(offsets))(*offsets)
    call("gs_sample_fanout_csr", ptr(rowptr), ptr(col), n_nodes, pad_id, len(fans), ctypes.addressof(fan),
         ctypes.addressof(off), ptr(ids_all), B, seed & 0xFFFFFFFFFFFFFFFF, 0, ptr(step_dev), hop0, root_offset,
         ptr(order), order.numel() if order is not None else 0, ptr(cursor_dev),
         label_table.ptr if label_table is not None else None, label_table.ld if label_table is not None else 0,
         label_table.d if label_table is not None else 0, labels_out.ptr if labels_out is not None else None,
         labels_out.ld if labels_out is not None else 0, law, max_degree, _s(stream))


def fanout_desc(rowptr, col, n_nodes, pad_id, fans, offsets, ids_all, B, seed, step_dev=None, hop0=0, root_offset=0,
                order=None, cursor_dev=None, label_table=None, labels_out=None, law=0, max_degree=0, unsup=None,
                padded_table=None, segments=None):
    """unsup = (pairs [n_pairs, 2] int32, n_pair_roots, cdf (uint32 bits), guide or None, guide_bits, n_neg, neg_seed): the
    roots are staged by the launch itself as [pairs[:, 0] | pairs[:, 1] | negatives] (see gs_fanout_desc).
    The arguments of sample_fanout_csr as a struct gs_fanout_desc (for gs_flat_reduce_adam_sample).  The tensors are
    kept alive on the descriptor object."""
    q = _lib.FanoutDesc()
    q.rowptr, q.col, q.n_nodes, q.pad_id = ptr(rowptr), ptr(col), n_nodes, pad_id
    q.n_hops = len(fans)
    for k, f in enumerate(fans):
        q.fan[k] = f
    for k, o in enumerate(offsets[: len(fans) + 1]):
        q.offsets[k] = o
    q.ids_all, q.B, q.seed, q.step, q.step_dev = ptr(ids_all), B, seed & 0xFFFFFFFFFFFFFFFF, 0, ptr(step_dev)
    q.hop0, q.root_offset = hop0, root_offset
    q.law, q.max_degree = law, max_degree
    q.order, q.n_order, q.cursor_dev = ptr(order), (order.numel() if order is not None else 0), ptr(cursor_dev)
    if label_table is not None:
        q.label_table, q.ld_table, q.C = label_table.ptr, label_table.ld, label_table.d
    if labels_out is not None:
        q.labels_out, q.ld_out = labels_out.ptr, labels_out.ld
    q.padded_table = ptr(padded_table)
    if segments is not None:       # root boundaries of the reference's three sample() calls (gs_fanout_desc.seg_begin)
        q.seg_begin[0], q.seg_begin[1] = int(segments[0]), int(segments[1])
    q._keep = (rowptr, col, ids_all, step_dev, order, cursor_dev, label_table, labels_out, unsup, padded_table)
    if unsup is not None:
        pairs, n_pair_roots, cdf, guide, guide_bits, n_neg, neg_seed = unsup
        q.pairs, q.n_pairs, q.n_pair_roots = ptr(pairs), pairs.shape[0], n_pair_roots
        q.cdf, q.guide, q.n_cdf = ptr(cdf), ptr(guide), cdf.numel()
        q.n_neg, q.guide_bits, q.neg_seed = n_neg, guide_bits, neg_seed & 0xFFFFFFFFFFFFFFFF
    return q


def build_padded_table(rowptr, col, n_nodes, pad_id, max_degree, seed, stream=None):
    """The reference law's padded table [n_nodes + 1, max_degree] (int32, device) from the CSR (gs_build_padded_table)."""
    table = torch.empty((n_nodes + 1) * max_degree, dtype=torch.int32, device=rowptr.device)
    call("gs_build_padded_table", ptr(rowptr), ptr(col), n_nodes, pad_id, max_degree, seed & 0xFFFFFFFFFFFFFFFF, ptr(table),
         _s(stream))
    return table


def sample_fanout_desc(desc, stream=None):
    """Launch the fused fan-out sampler from a descriptor built by fanout_desc()."""
    call("gs_sample_fanout_desc", ctypes.addressof(desc), _s(stream))


def select_batch(order, cursor_dev, n, out, stream=None):
    call("gs_select_batch", ptr(order), order.numel(), ptr(cursor_dev), n, ptr(out), _s(stream))
    return out


def advance_counter(counter_dev, delta, stream=None):
    call("gs_advance_counter", ptr(counter_dev), delta, _s(stream))


# ------------------------------------------------------------------------------------------ K2
def gather_rows(X, ids, out=None, stream=None):
    n = ids.numel()
    if out is None:
        out = Mat.zeros(n, X.d, ids.device)
    call("gs_gather_rows", X.ptr, X.ld, ptr(ids), n, X.d, out.ptr, out.ld, _s(stream))
    return out


def input_grad_pull(out, rows, d, d_self=None, n_self=0, segments=(), mask_y=None, stream=None):
    """One-launch input gradient of a layer (gs_input_grad_pull).  segments: (src Mat, row0, n, s, scale) tuples:
    out[row0 + i*s + j] += scale * src[i]."""
    q = _lib.PullDesc()
    q.d_self, q.ld_self, q.n_self = (d_self.ptr, d_self.ld, n_self) if d_self is not None else (None, 0, 0)
    assert len(segments) <= _lib.GS_PULL_MAX
    q.n_seg, q.d = len(segments), d
    for k, (src, row0, n, s, scale) in enumerate(segments):
        q.src[k], q.ld_src[k], q.row0[k], q.n[k], q.s[k], q.scale[k] = src.ptr, src.ld, row0, n, s, scale
    q.mask_y, q.ldy = (mask_y.ptr, mask_y.ld) if mask_y is not None else (None, 0)
    q.out, q.ldo, q.rows = out.ptr, out.ld, rows
    call("gs_input_grad_pull", ctypes.addressof(q), _s(stream))
    return out


def dropout_desc(seed, clock_dev, site, rate, row0=0, keep=None):
    """struct gs_dropout; None when rate == 0 (dropout off).  keep: uint8 device tensor [rows, ld] of injected keep bits
    (parity tests: the masks the reference run drew), addressed by the call's global row index."""
    if not rate:
        return None
    d = _lib.Dropout(int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(clock_dev), int(site), float(rate), int(row0), None, 0)
    if keep is not None:
        assert keep.dtype == torch.uint8 and keep.dim() == 2 and keep.stride(1) == 1 and keep.stride(0) % 4 == 0
        d.keep_bits, d.keep_ld = keep.data_ptr(), keep.stride(0)
        d._keep = keep
    return d


def dropout_rows(X, ids, n, drop, out, stream=None):
    """out[i] = mask * X[ids[i] or i] / keep_prob (tf.nn.dropout); also its own backward.  In place when ids is None."""
    call("gs_dropout_rows", X.ptr, X.ld, ptr(ids), n, X.d, ctypes.addressof(drop) if drop is not None else None,
         out.ptr, out.ld, _s(stream))
    return out


def gather_mean_fwd(X, idx, n, s, out=None, self_src=None, self_idx=None, drop=None, stream=None):
    """idx: int32 [n*s] or None (contiguous groups).  self_src (Mat) switches to the GCN mean.  `drop`: dropout of
    every gathered neighbor row before the mean."""
    if out is None:
        out = Mat.zeros(n, X.d, X.buf.device)
    if drop is not None:
        call("gs_gather_mean_dropout_fwd", X.ptr, X.ld, ptr(idx), n, s, X.d,
             self_src.ptr if self_src is not None else None, self_src.ld if self_src is not None else 0,
             ptr(self_idx), out.ptr, out.ld, ctypes.addressof(drop), _s(stream))
        return out
    call("gs_gather_mean_fwd", X.ptr, X.ld, ptr(idx), n, s, X.d,
         self_src.ptr if self_src is not None else None, self_src.ld if self_src is not None else 0,
         ptr(self_idx), out.ptr, out.ld, _s(stream))
    return out


def mean_bwd(d_mean, n, s, scale, d_neigh, mask_y=None, accumulate=False, stream=None):
    call("gs_mean_bwd", d_mean.ptr, d_mean.ld, n, s, d_mean.d, scale,
         mask_y.ptr if mask_y is not None else None, mask_y.ld if mask_y is not None else 0,
         d_neigh.ptr, d_neigh.ld, 1 if accumulate else 0, _s(stream))
    return d_neigh


# ------------------------------------------------------------------------------------------ INF
def csr_reduce_ws_bytes(n_slots, d):
    """Bytes of the partials workspace gs_csr_reduce_fwd needs for n_slots segments of long rows at width d (CSR_SOFTMAX: the
    table's d + 4, its partial carries the (max, sum) pair)."""
    out = ctypes.c_int64(0)
    call("gs_csr_reduce_ws_bytes", n_slots, d, ctypes.byref(out))
    return out.value


def _csr_desc(q, rowptr, col, items, splits, n_rows, split_len, op, X, out, ws, act):
    """The fields CsrReduceDesc and CsrRowsDesc have in common."""
    q.rowptr, q.col, q.items, q.splits = ptr(rowptr), ptr(col), ptr(items), ptr(splits)
    q.X, q.out, q.ws = X.ptr, out.ptr, ptr(ws)
    q.n_rows, q.nnz, q.n_items, q.n_split = n_rows, col.numel(), items.shape[0], (splits.shape[0] if splits is not None else 0)
    q.ldx, q.x_rows, q.ldo, q.ws_bytes = X.ld, X.rows, out.ld, (4 * ws.numel() if ws is not None else 0)
    q.d, q.op, q.act, q.split_len = X.d, op, act, split_len
    return q


def csr_reduce_fwd(rowptr, col, items, splits, n_rows, split_len, op, X, out, row0, n, item_range, split_range, slot_range,
                   ws=None, act=ACT_IDENTITY, stream=None):
    """gs_csr_reduce_fwd: out[r - row0] = mean | mean-with-self | max | softmax-weighted sum (CSR_SOFTMAX: the logit of a row is
    column X.d of X, ws sized for width X.d + 4) over the whole neighbor list of row r of X's rows, for the window
    [row0, row0 + n) of a planned CSR graph (inference.FullGraph owns the plan and has checked the column ids)."""
    q = _csr_desc(_lib.CsrReduceDesc(), rowptr, col, items, splits, n_rows, split_len, op, X, out, ws, act)
    q.row0, q.n = row0, n
    (q.item0, q.item1), (q.split0, q.split1), (q.slot0, q.slot1) = item_range, split_range, slot_range
    call("gs_csr_reduce_fwd", ctypes.addressof(q), _s(stream))
    return out


def csr_reduce_rows(rowptr, col, items, splits, n_rows, split_len, op, X, out, out_pos, x_pos=None, n_slots=0, ws=None,
                    act=ACT_IDENTITY, stream=None):
    """gs_csr_reduce_rows: out[out_pos[r]] = mean | mean-with-self | max over the whole neighbor list of row r of the rows
    X[x_pos[col[e]]], for the rows of a subset plan (inference.FullGraph.plan_rows: items / splits with slots 0 .. n_slots).
    x_pos None: X is indexed by node id.  out_pos, x_pos: int32 device vectors [n_rows]."""
    for name, m in (("out_pos", out_pos), ("x_pos", x_pos)):
        if m is not None and (m.dtype != torch.int32 or m.numel() != n_rows):
            raise _lib.GraphsageAmdError("csr_reduce_rows: %s must be an int32 vector of n_rows = %d entries" % (name, n_rows))
    q = _csr_desc(_lib.CsrRowsDesc(), rowptr, col, items, splits, n_rows, split_len, op, X, out, ws, act)
    q.x_pos, q.out_pos, q.n_slots, q.out_rows = ptr(x_pos), ptr(out_pos), n_slots, out.rows
    call("gs_csr_reduce_rows", ctypes.addressof(q), _s(stream))
    return out


def frontier_ws_bytes(n_rows):
    """Bytes of the int32 workspace gs_frontier_expand needs for a graph of n_rows rows (flags, zero on first use, + block sums)."""
    out = ctypes.c_int64(0)
    call("gs_frontier_ws_bytes", n_rows, ctypes.byref(out))
    return out.value


def frontier_expand(rowptr, col, n_rows, rows_in, m, rows_out, pos, count, ws, stream=None):
    """gs_frontier_expand: rows_out = rows_in[:m] U their column ids (ascending, duplicate-free), pos[id] = index in rows_out or
    -1, count[0] = members.  rows_in: ascending duplicate-free int32 device vector (None when m == 0); ws: int32 device vector
    of frontier_ws_bytes(n_rows) bytes whose flag half is zero (every call leaves it zero)."""
    q = _lib.FrontierDesc()
    q.rowptr, q.col, q.rows_in, q.rows_out, q.pos, q.count, q.ws = (ptr(rowptr), ptr(col), ptr(rows_in), ptr(rows_out), ptr(pos),
                                                                    ptr(count), ptr(ws))
    q.n_rows, q.nnz, q.m, q.rows_out_cap, q.ws_bytes = n_rows, col.numel(), m, rows_out.numel(), 4 * ws.numel()
    call("gs_frontier_expand", ctypes.addressof(q), _s(stream))
    return rows_out, pos, count


# ------------------------------------------------------------------------------------------ RANK
RANK_CHUNK = 65536       # query rows per gs_rank_count call: the slab workspace does not grow with Q


def rank_ws_bytes(Q, n_cand):
    """Bytes of the int32 slab workspace gs_rank_count needs for Q queries against n_cand candidates."""
    out = ctypes.c_int64(0)
    call("gs_rank_ws_bytes", Q, n_cand, ctypes.byref(out))
    return out.value


def _query_desc(q, who, Xq, Zc, Q, n_cand, f_rowptr, f_col, keep_src):
    """The width and filter checks of rank_count and topk_select (`who`: the message prefix and what follows the shapes), made
    before anything is allocated or asked of the library, and the fields RankDesc and TopkDesc have in common but for the
    workspace."""
    if Xq.d != Zc.d or Xq.rows < Q:
        raise _lib.GraphsageAmdError("%s: Xq is [%d, %d], Zc [%d, %d]%s" % (who[0], Xq.rows, Xq.d, Zc.rows, Zc.d, who[1]))
    if (f_rowptr is None) != (f_col is None) or (f_rowptr is not None and (
            f_rowptr.dtype != torch.int64 or f_col.dtype != torch.int32 or f_rowptr.numel() != Zc.rows + 1)):
        raise _lib.GraphsageAmdError("%s: the filter is an int64 rowptr [n_rows + 1] with an int32 col" % who[0])
    q.Zc, q.f_rowptr, q.f_col = Zc.ptr, ptr(f_rowptr), ptr(f_col)
    q.n_rows, q.n_cand, q.ldz, q.ldq = Zc.rows, n_cand, Zc.ld, Xq.ld
    q.f_nnz, q.d, q.flags = (f_col.numel() if f_col is not None else 0), Xq.d, (_lib.RANK_KEEP_SRC if keep_src else 0)
    return q


def _query_chunks(Q):
    """(q0, n) of every RANK_CHUNK of Q queries (one empty chunk when Q == 0)."""
    for q0 in range(0, max(Q, 1), RANK_CHUNK):
        yield q0, min(RANK_CHUNK, Q - q0)


def rank_count(Xq, Zc, dst, n_cand=None, src=None, f_rowptr=None, f_col=None, t=None, n_gt=None, n_eq=None, ws=None,
               keep_src=False, stream=None):
    """gs_rank_count: t[q] = <Xq[q], Zc[dst[q]]> and the numbers of candidates w < n_cand (dst[q], src[q] and the filter row
    of src[q] left out) that score above / exactly t[q].  Xq, Zc: Mats of the same width; dst, src: int32 device vectors with
    entries in [0, Zc.rows) (checked by the caller); f_rowptr int64 [Zc.rows + 1], f_col int32 (a filter needs src).
    keep_src: src[q] stays a candidate and only names the filter row (GS_RANK_KEEP_SRC).  Returns (t, n_gt, n_eq)."""
    Q = dst.numel()
    n_cand = Zc.rows if n_cand is None else int(n_cand)
    q = _query_desc(_lib.RankDesc(), ("rank_count", ", %d queries" % Q), Xq, Zc, Q, n_cand, f_rowptr, f_col, keep_src)
    if dst.dtype != torch.int32 or (src is not None and (src.dtype != torch.int32 or src.numel() != Q)):
        raise _lib.GraphsageAmdError("rank_count: dst and src must be int32 vectors of the same length")
    dev = dst.device
    t = torch.empty(Q, dtype=torch.float32, device=dev) if t is None else t
    n_gt = torch.empty(Q, dtype=torch.int32, device=dev) if n_gt is None else n_gt
    n_eq = torch.empty(Q, dtype=torch.int32, device=dev) if n_eq is None else n_eq
    need = max(rank_ws_bytes(n, n_cand) for n in {min(Q, RANK_CHUNK), Q % RANK_CHUNK})      # the two chunk sizes that occur
    if ws is None:
        ws = torch.empty(max(need // 4, 2), dtype=torch.int32, device=dev)
    q.ws, q.ws_bytes = ptr(ws), 4 * ws.numel()
    for q0, n in _query_chunks(Q):
        q.Q, q.Xq = n, Xq.ptr + 4 * q0 * Xq.ld
        q.dst, q.src = ptr(dst[q0:q0 + n]), (ptr(src[q0:q0 + n]) if src is not None else None)
        q.t, q.n_gt, q.n_eq = ptr(t[q0:q0 + n]), ptr(n_gt[q0:q0 + n]), ptr(n_eq[q0:q0 + n])
        call("gs_rank_count", ctypes.addressof(q), _s(stream))
    return t, n_gt, n_eq


# ------------------------------------------------------------------------------------------ TOPK
TOPK_MAX = _lib.TOPK_MAX  # largest k of gs_topk_select


def topk_ws_bytes(Q, n_cand, k):
    """Bytes of the workspace gs_topk_select needs for Q queries against n_cand candidates at this k."""
    out = ctypes.c_int64(0)
    call("gs_topk_ws_bytes", Q, n_cand, k, ctypes.byref(out))
    return out.value


def topk_select(Xq, Zc, k, n_cand=None, src=None, f_rowptr=None, f_col=None, keep_src=False, ids=None, scores=None, count=None,
                ws=None, stream=None):
    """gs_topk_select: for every row q of Xq the k candidates w < n_cand (src[q] and the filter row of src[q] left out) that come
    first by (<Xq[q], Zc[w]> descending, w ascending).  Xq, Zc: Mats of the same width; src: int32 device vector [Xq.rows] with
    entries in [0, Zc.rows) (checked by the caller); f_rowptr int64 [Zc.rows + 1], f_col int32 (a filter needs src).
    keep_src: src[q] stays a candidate and only names the filter row (GS_RANK_KEEP_SRC).  Returns (ids int32 [Q, k], scores
    float32 [Q, k], count int32 [Q]); entries at and beyond count[q] = min(k, candidates of q) are -1 / -inf."""
    Q, k = Xq.rows, int(k)
    n_cand = Zc.rows if n_cand is None else int(n_cand)
    q = _query_desc(_lib.TopkDesc(), ("topk_select", ""), Xq, Zc, Q, n_cand, f_rowptr, f_col, keep_src)
    if not 1 <= k <= TOPK_MAX:
        raise _lib.GraphsageAmdError("topk_select: k=%d must lie in [1, %d]" % (k, TOPK_MAX))
    if src is not None and (src.dtype != torch.int32 or src.numel() != Q):
        raise _lib.GraphsageAmdError("topk_select: src must be an int32 vector with one entry per query")
    dev = Xq.buf.device
    ids = torch.empty((Q, k), dtype=torch.int32, device=dev) if ids is None else ids
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev) if scores is None else scores
    count = torch.empty(Q, dtype=torch.int32, device=dev) if count is None else count
    if tuple(ids.shape) != (Q, k) or tuple(scores.shape) != (Q, k) or count.numel() != Q or not (
            ids.is_contiguous() and scores.is_contiguous() and count.is_contiguous()) or (
            ids.dtype, scores.dtype, count.dtype) != (torch.int32, torch.float32, torch.int32):
        raise _lib.GraphsageAmdError("topk_select: ids int32 [Q, k], scores float32 [Q, k] and count int32 [Q] must be dense")
    need = max(topk_ws_bytes(n, n_cand, k) for n in {min(Q, RANK_CHUNK), Q % RANK_CHUNK})     # the two chunk sizes that occur
    if ws is None:
        ws = torch.empty(max((need + 7) // 8, 1), dtype=torch.int64, device=dev)
    q.ws, q.ws_bytes, q.k = ptr(ws), ws.element_size() * ws.numel(), k
    for q0, n in _query_chunks(Q):
        q.Q, q.Xq = n, Xq.ptr + 4 * q0 * Xq.ld
        q.src = ptr(src[q0:q0 + n]) if src is not None else None
        q.ids, q.scores, q.count = ptr(ids[q0:q0 + n]), ptr(scores[q0:q0 + n]), ptr(count[q0:q0 + n])
        call("gs_topk_select", ctypes.addressof(q), _s(stream))
    return ids, scores, count


# ------------------------------------------------------------------------------------------ WALK
WALK_MIN_RATIO = 16  # min(1/p, 1, 1/q) / max(1/p, 1, 1/q) >= 1 / 16: what the attempt cap's bound rests on


def walk_thresholds(p, q):
    """(p, q) of node2vec -> (thr_return, thr_common, thr_far), the integer acceptance thresholds of gs_walk_paths:
    floor(w / wmax * 2^32) for w = (1/p, 1, 1/q), in exact rational arithmetic (the largest is exactly 2^32).  Refuses p, q
    whose smallest weight is below 1/16 of the largest."""
    from fractions import Fraction
    try:
        fp, fq = Fraction(float(p)), Fraction(float(q))
    except (TypeError, ValueError, OverflowError):
        raise ValueError("walk parameters p=%r q=%r must be finite positive numbers" % (p, q))
    if fp <= 0 or fq <= 0:
        raise ValueError("walk parameters p=%r q=%r must be positive" % (p, q))
    w = (1 / fp, Fraction(1), 1 / fq)
    wmax = max(w)
    if min(w) * WALK_MIN_RATIO < wmax:
        raise ValueError("walk parameters p=%g q=%g are out of range: min(1/p, 1, 1/q) / max(1/p, 1, 1/q) = %.4g must be at "
                         "least 1/%d (rejection sampling with a bounded number of attempts; p and q within [0.25, 4] with "
                         "max(p, q, 1) / min(p, q, 1) <= %d qualify)"
                         % (p, q, float(min(w) / wmax), WALK_MIN_RATIO, WALK_MIN_RATIO))
    return tuple(int(x / wmax * (1 << 32)) for x in w)


def _walk_desc(rowptr, col, starts, num_walks, walk_len, walk0, n_walks, paths):
    n_starts = starts.numel()
    total = n_starts * int(num_walks)
    n_walks = total - walk0 if n_walks is None else int(n_walks)
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or starts.dtype != torch.int32 or not (
            rowptr.is_contiguous() and col.is_contiguous() and starts.is_contiguous()) or rowptr.numel() < 1:
        raise _lib.GraphsageAmdError("walks: rowptr int64 [n_nodes + 1], col int32 and starts int32 must be dense vectors")
    if num_walks < 1 or walk0 < 0 or n_walks < 0 or walk0 + n_walks > total:
        raise _lib.GraphsageAmdError("walks: walks %d .. %d lie outside the job of %d starts x %d walks"
                                     % (walk0, walk0 + n_walks, n_starts, num_walks))
    if paths is not None and (paths.dtype != torch.int32 or paths.dim() != 2 or paths.shape[0] != n_walks
                              or paths.shape[1] != walk_len or paths.stride(1) != 1):
        raise _lib.GraphsageAmdError("walks: paths must be int32 [n_walks, walk_len] with unit column stride")
    d = _lib.WalkDesc()
    d.rowptr, d.col, d.starts = ptr(rowptr), (ptr(col) if col.numel() else None), (ptr(starts) if n_starts else None)
    d.n_nodes, d.nnz, d.n_starts, d.walk0, d.n_walks = rowptr.numel() - 1, col.numel(), n_starts, walk0, n_walks
    d.num_walks, d.walk_len = int(num_walks), int(walk_len)
    return d


def walk_paths(rowptr, col, starts, num_walks, walk_len, thresholds, seed, walk0=0, n_walks=None, paths=None, counts=None,
               stream=None):
    """gs_walk_paths: walks walk0 .. walk0 + n_walks - 1 of the job `num_walks walks of walk_len nodes from every entry of
    starts` under the (p, q) law given by `thresholds` (walk_thresholds).  rowptr int64 [n_nodes + 1], col int32 with ascending
    rows, starts int32: device vectors.  Returns (paths int32 [n_walks, walk_len], counts int32 [n_walks])."""
    d = _walk_desc(rowptr, col, starts, num_walks, walk_len, int(walk0), n_walks, paths)
    dev = rowptr.device
    paths = torch.empty((d.n_walks, max(int(walk_len), 0)), dtype=torch.int32, device=dev) if paths is None else paths
    counts = torch.empty(d.n_walks, dtype=torch.int32, device=dev) if counts is None else counts
    if counts.dtype != torch.int32 or counts.numel() != d.n_walks or not counts.is_contiguous():
        raise _lib.GraphsageAmdError("walk_paths: counts must be a dense int32 [n_walks]")
    d.paths, d.counts = (ptr(paths) if paths.numel() else None), (ptr(counts) if d.n_walks else None)
    d.ld_paths = paths.stride(0) if d.n_walks > 1 else max(int(walk_len), 1)
    d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    d.thr_return, d.thr_common, d.thr_far = (int(t) for t in thresholds)
    call("gs_walk_paths", ctypes.addressof(d), _s(stream))
    return paths, counts


def walk_pairs(paths, offsets, total, pairs=None, stream=None):
    """gs_walk_pairs: the (start, current) pairs of `paths` (walk_paths) written at `offsets` = the exclusive prefix sum of its
    counts (int64 [n_walks]); total = the sum of the counts.  Returns pairs int32 [total, 2], by walk and then by position."""
    n_walks, walk_len = paths.shape
    if offsets.dtype != torch.int64 or offsets.numel() != n_walks or not offsets.is_contiguous() or paths.dtype != torch.int32 \
            or paths.stride(1) != 1:
        raise _lib.GraphsageAmdError("walk_pairs: paths int32 [n_walks, walk_len], offsets a dense int64 [n_walks]")
    pairs = torch.empty((int(total), 2), dtype=torch.int32, device=paths.device) if pairs is None else pairs
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous() \
            or pairs.shape[0] < total:
        raise _lib.GraphsageAmdError("walk_pairs: pairs must be a dense int32 [>= total, 2]")
    d = _lib.WalkDesc()
    d.paths, d.offsets, d.pairs = (ptr(paths) if paths.numel() else None), (ptr(offsets) if n_walks else None), \
        (ptr(pairs) if pairs.numel() else None)
    d.n_walks, d.walk_len, d.pairs_cap = n_walks, walk_len, int(total)
    d.ld_paths = paths.stride(0) if n_walks > 1 else max(int(walk_len), 1)
    call("gs_walk_pairs", ctypes.addressof(d), _s(stream))
    return pairs[:int(total)]


def importance_table(paths, num_walks, walk_len, n_nodes, top, slots, pad_id, table=None, stats=None, stream=None):
    """gs_importance_table: the importance neighborhoods of the starts whose walks `paths` holds (walk_paths: int32
    [n_starts * num_walks, >= walk_len], unit column stride; the walks of start i in rows i * num_walks ..).  The `top` most
    visited nodes of each start share `slots` table entries by largest remainder (include/graphsage_amd.h, section
    IMPORTANCE).  Returns (table int32 [n_starts, slots], stats int32 [n_starts, 2] = (distinct visited, nodes with a slot))."""
    num_walks, walk_len, top, slots = int(num_walks), int(walk_len), int(top), int(slots)
    if paths.dtype != torch.int32 or paths.dim() != 2 or (paths.shape[0] and paths.stride(1) != 1) or num_walks < 1 \
            or paths.shape[0] % num_walks:
        raise _lib.GraphsageAmdError("importance_table: paths must be int32 [n_starts * num_walks, >= walk_len] with unit column "
                                     "stride")
    n_starts = paths.shape[0] // num_walks
    dev = paths.device
    table = torch.empty((n_starts, max(slots, 0)), dtype=torch.int32, device=dev) if table is None else table
    stats = torch.empty((n_starts, 2), dtype=torch.int32, device=dev) if stats is None else stats
    if table.dtype != torch.int32 or tuple(table.shape) != (n_starts, slots) or not table.is_contiguous() \
            or stats.dtype != torch.int32 or tuple(stats.shape) != (n_starts, 2) or not stats.is_contiguous() \
            or table.device != dev or stats.device != dev:
        raise _lib.GraphsageAmdError("importance_table: table must be a dense int32 [n_starts, slots] and stats a dense int32 "
                                     "[n_starts, 2], both on the device of paths")
    d = _lib.ImportanceDesc()
    d.paths, d.table, d.stats = (ptr(paths) if paths.numel() else None), (ptr(table) if table.numel() else None), \
        (ptr(stats) if stats.numel() else None)
    d.n_starts, d.n_nodes = n_starts, int(n_nodes)
    # (a view narrower than walk_len is refused by the library whatever its row stride)
    d.ld_paths = paths.stride(0) if paths.shape[0] > 1 and paths.shape[1] >= walk_len else max(paths.shape[1], 1)
    d.num_walks, d.walk_len, d.top, d.slots, d.pad_id = num_walks, walk_len, top, slots, int(pad_id)
    call("gs_importance_table", ctypes.addressof(d), _s(stream))
    return table, stats


# ------------------------------------------------------------------------------------------ K3
def sage_dense_fwd(self_m, self_idx, agg, agg_idx, n, W_self, W_neigh, out_dim, concat, act, bias, out,
                   stream=None):
    call("gs_sage_dense_fwd",
         self_m.ptr if self_m is not None else None, self_m.ld if self_m is not None else 0, ptr(self_idx),
         self_m.d if self_m is not None else 0,
         agg.ptr, agg.ld, ptr(agg_idx), agg.d, n,
         W_self.ptr if W_self is not None else None, W_self.ld if W_self is not None else 0,
         W_neigh.ptr, W_neigh.ld, out_dim, 1 if concat else 0, act, ptr(bias), out.ptr, out.ld, _s(stream))
    return out


def gather_job(X, idx, n, s, out, self_src=None, self_idx=None):
    """Descriptor of one gather+mean job for sage_dense_fwd_cogather (same arguments as gather_mean_fwd)."""
    j = _lib.GatherDesc()
    j.X, j.idx, j.out = X.ptr, ptr(idx), out.ptr
    j.self_src = self_src.ptr if self_src is not None else None
    j.self_idx = ptr(self_idx)
    j.ldx, j.ld_self, j.ldo, j.n, j.s, j.d = X.ld, (self_src.ld if self_src is not None else 0), out.ld, n, s, X.d
    return j


def split_gather_jobs(jobs, frac):
    """Split a gather job list into (head, tail): `tail` gets the last (1 - frac) of the ROWS of the largest job (its
    idx / out / self pointers advanced accordingly), `head` everything else.  Used to spread one step's gather over
    two horizontally fused launches."""
    if not jobs or frac >= 1.0:
        return list(jobs or ()), []
    big = max(range(len(jobs)), key=lambda i: jobs[i].n * jobs[i].s)
    j = jobs[big]
    n_head = int(j.n * max(frac, 0.0))
    if n_head >= j.n:
        return list(jobs), []
    tail = _lib.GatherDesc()
    for name, _ in _lib.GatherDesc._fields_:
        setattr(tail, name, getattr(j, name))
    tail.n = j.n - n_head
    tail.idx = (j.idx + 4 * n_head * j.s) if j.idx else None
    tail.out = j.out + 4 * n_head * j.ldo
    if j.self_src:
        if j.self_idx:
            tail.self_idx = j.self_idx + 4 * n_head
        else:
            tail.self_src = j.self_src + 4 * n_head * j.ld_self
    head = list(jobs)
    if n_head == 0:
        del head[big]
    else:
        h = _lib.GatherDesc()
        for name, _ in _lib.GatherDesc._fields_:
            setattr(h, name, getattr(j, name))
        h.n = n_head
        head[big] = h
    return head, [tail]


def sage_dense_fwd_cogather(self_m, self_idx, agg, agg_idx, n, W_self, W_neigh, out_dim, concat, act, bias, out,
                            jobs, stream=None):
    """gs_sage_dense_fwd + the gather jobs in ONE horizontally fused launch."""
    import ctypes
    arr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_dense_fwd_cogather", self_m.ptr if self_m is not None else None, self_m.ld if self_m is not None else 0,
         ptr(self_idx), self_m.d if self_m is not None else 0, agg.ptr, agg.ld, ptr(agg_idx),
         agg.d, n, W_self.ptr if W_self is not None else None, W_self.ld if W_self is not None else 0,
         W_neigh.ptr, W_neigh.ld, out_dim, 1 if concat else 0, act, ptr(bias),
         out.ptr, out.ld, ctypes.addressof(arr), len(jobs), _s(stream))
    return out


def sage_dense_fwd_stream(self_m, self_idx, agg, n, W_self, W_neigh, out_dim, act, bias, out, jobs, stream=None):
    """gs_sage_dense_fwd_stream: split-K stream contraction workgroups + the gather jobs in ONE launch (self rows
    optionally gathered through self_idx; agg dense)."""
    import ctypes
    jobs = list(jobs or ())
    arr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_dense_fwd_stream", self_m.ptr if self_m is not None else None, self_m.ld if self_m is not None else 0,
         ptr(self_idx), agg.ptr, agg.ld, agg.d, n, W_self.ptr if W_self is not None else None,
         W_self.ld if W_self is not None else 0, W_neigh.ptr, W_neigh.ld, out_dim, act, ptr(bias), out.ptr, out.ld,
         ctypes.addressof(arr), len(jobs), _s(stream))
    return out


def sage_dense_fwd_stream2(self_m, self_idx, agg, n, W_self, W_neigh, out_dim, act, bias, out, jobs=(), stream=None):
    """gs_sage_dense_fwd_stream2: the stream contraction with different reduction lengths of the two terms (pooling aggregators:
    self rows of self_m.d features gathered through self_idx | pooled rows of agg.d = hidden_dim), concat output."""
    import ctypes
    jobs = list(jobs or ())
    arr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_dense_fwd_stream2", self_m.ptr, self_m.ld, ptr(self_idx), self_m.d, agg.ptr, agg.ld, agg.d, n, W_self.ptr, W_self.ld,
         W_neigh.ptr, W_neigh.ld, out_dim, act, ptr(bias), out.ptr, out.ld, ctypes.addressof(arr), len(jobs), _s(stream))
    return out


def sage_dense_fwd_tiled3(self_m, self_idx, agg, n, W_self, W_neigh, out_dim, act, bias, out, jobs=(), stream=None):
    """gs_sage_dense_fwd_tiled3: the layer-0 contraction LDS-tiled on the bf16 matrix pipe (fp32 operands cut into three bf16 pieces
    INSIDE the kernel: same arguments as sage_dense_fwd_stream2), concat output; self_m None = one term (GCN)."""
    import ctypes
    jobs = list(jobs or ())
    arr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_dense_fwd_tiled3", self_m.ptr if self_m is not None else None, self_m.ld if self_m is not None else 0,
         ptr(self_idx), self_m.d if self_m is not None else 0, agg.ptr, agg.ld, agg.d, n,
         W_self.ptr if W_self is not None else None, W_self.ld if W_self is not None else 0, W_neigh.ptr, W_neigh.ld, out_dim, act,
         ptr(bias), out.ptr, out.ld, ctypes.addressof(arr), len(jobs), _s(stream))
    return out


def sage_dense_fwd_tiled3_means(self_m, self_idx, agg, n, W_self, W_neigh, out_dim, act, bias, out, n_roots, s, l1_means, jobs=(),
                                stream=None):
    """gs_sage_dense_fwd_tiled3_means: sage_dense_fwd_tiled3 (concat form) over the rows [roots | hop 1], n = n_roots (1 + s), that
    also writes the NEXT layer's neighbor means l1_means [n_roots, 2 out_dim] from its finished tiles; `out` is bit-identical."""
    import ctypes
    jobs = list(jobs or ())
    arr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_dense_fwd_tiled3_means", self_m.ptr, self_m.ld, ptr(self_idx), self_m.d, agg.ptr, agg.ld, agg.d, n, W_self.ptr,
         W_self.ld, W_neigh.ptr, W_neigh.ld, out_dim, act, ptr(bias), out.ptr, out.ld, ctypes.addressof(arr), len(jobs), n_roots, s,
         l1_means.ptr, l1_means.ld, _s(stream))
    return out


def split_rows_words(K, N):
    """int32 words of gs_split_rows' output (gs_split_rows_bytes / 4): groups of 8 k up to an even count of 32-k stages."""
    import ctypes
    n = ctypes.c_int64()
    call("gs_split_rows_bytes", int(K), int(N), ctypes.byref(n))
    return int(n.value) // 4


_SPLIT_WS_WORDS = None


def split_tiled_ws_words():
    """fp32 words of the workspace gs_dense_fwd_rows_split_ws wants (one 128 x 256 partial tile per CU)."""
    global _SPLIT_WS_WORDS
    if _SPLIT_WS_WORDS is None:
        import ctypes
        n = ctypes.c_int64()
        call("gs_dense_fwd_rows_split_ws_bytes", ctypes.byref(n))
        _SPLIT_WS_WORDS = int(n.value) // 4
    return _SPLIT_WS_WORDS


def split_rows(W, out=None, stream=None):
    """gs_split_rows: the three bf16 pieces of W^T ([groups of 8 k][3][N][8] bf16, as an int32 tensor) for the split-MFMA
    contractions; W is a Mat [K, N]."""
    K, N = W.rows, W.d
    if out is None:
        out = torch.empty(split_rows_words(K, N), dtype=torch.int32, device=W.buf.device)
    call("gs_split_rows", W.ptr, W.ld, K, N, ptr(out), _s(stream))
    return out


def split_rows_f16_words(K, N):
    """int32 words of gs_split_rows_f16's output: the two fp16 pieces of the scaled weights + the column exponents."""
    import ctypes
    n = ctypes.c_int64()
    call("gs_split_rows_f16_bytes", int(K), int(N), ctypes.byref(n))
    return int(n.value) // 4


def split_rows_f16(W, out=None, stream=None):
    """gs_split_rows_f16: W [K, N] as two fp16 pieces per element under a power-of-two scale per COLUMN ([groups of 8 k][2][N][8]
    fp16 + N int32 exponents, as an int32 tensor) for gs_dense_fwd_rows_split16."""
    K, N = W.rows, W.d
    if out is None:
        out = torch.empty(split_rows_f16_words(K, N), dtype=torch.int32, device=W.buf.device)
    call("gs_split_rows_f16", W.ptr, W.ld, K, N, ptr(out), _s(stream))
    return out


def split_table_f16(X, stream=None):
    """gs_split_table_f16: a (constant) feature table as two fp16 pieces per element under a power-of-two scale per ROW.
    Returns (X2 int32 tensor: [rows][2][KP] fp16, row exponents int32 [rows])."""
    import ctypes
    tb, eb = ctypes.c_int64(), ctypes.c_int64()
    call("gs_split_table_f16_bytes", X.rows, X.d, ctypes.byref(tb), ctypes.byref(eb))
    X2 = torch.empty(int(tb.value) // 4, dtype=torch.int32, device=X.buf.device)
    rexp = torch.empty(int(eb.value) // 4, dtype=torch.int32, device=X.buf.device)
    call("gs_split_table_f16", X.ptr, X.ld, X.rows, X.d, ptr(X2), ptr(rexp), _s(stream))
    return X2, rexp


def dense_wgrad(A, a_idx, dZ, col0, out_dim, n, n_slabs, slabs, ld_slab, stream=None):
    """slabs: flat fp32 tensor with room for n_slabs * A.d * ld_slab floats."""
    call("gs_dense_wgrad", A.ptr, A.ld, ptr(a_idx), A.d, dZ.ptr, dZ.ld, col0, out_dim, n, n_slabs, ptr(slabs),
         ld_slab, _s(stream))


def sage_dense_dgrad(dZ, n, out_dim, fwd_concat, W_self, W_neigh, d_in, dX2, stream=None):
    call("gs_sage_dense_dgrad", dZ.ptr, dZ.ld, n, out_dim, 1 if fwd_concat else 0, W_self.ptr, W_self.ld,
         W_neigh.ptr, W_neigh.ld, d_in, dX2.ptr, dX2.ld, _s(stream))
    return dX2


def stage_batch(order, cursor_dev, n, batch, label_table, labels_out, stream=None):
    call("gs_stage_batch", ptr(order), order.numel(), ptr(cursor_dev), n, ptr(batch), label_table.ptr, label_table.ld,
         label_table.d, labels_out.ptr, labels_out.ld, _s(stream))


def dense_dgrad(dZ, col0, out_dim, n, W, dX, accumulate=False, stream=None):
    call("gs_dense_dgrad", dZ.ptr, dZ.ld, col0, out_dim, n, W.ptr, W.ld, W.rows, dX.ptr, dX.ld,
         1 if accumulate else 0, _s(stream))
    return dX


def act_bwd(dY, Y, n, n_cols, act, dZ, stream=None):
    call("gs_act_bwd", dY.ptr, dY.ld, Y.ptr if Y is not None else None, Y.ld if Y is not None else 0, n, n_cols,
         act, dZ.ptr, dZ.ld, _s(stream))
    return dZ


def colsum_slabs(Z, n, n_cols, n_slabs, slabs, ld_slab, stream=None):
    call("gs_colsum_slabs", Z.ptr, Z.ld, n, n_cols, n_slabs, ptr(slabs), ld_slab, _s(stream))


def gemm(transA, transB, M, N, K, A, B, C, a_row_idx=None, bias=None, act=ACT_IDENTITY, stream=None):
    call("gs_gemm_f32", 1 if transA else 0, 1 if transB else 0, M, N, K, A.ptr, A.ld, ptr(a_row_idx), B.ptr, B.ld,
         ptr(bias), act, C.ptr, C.ld, _s(stream))
    return C


# ------------------------------------------------------------------------------------------ K4
def dense_pool_max_fwd(X, idx, n, s, W, bias, pooled, argmax, stream=None):
    """gs_dense_pool_max_fwd: pooled = max over each group's s rows of relu(X[idx] . W + bias), + arg-max."""
    call("gs_dense_pool_max_fwd", X.ptr, X.ld, ptr(idx), X.d, n, s, W.ptr, W.ld, W.d, ptr(bias), pooled.ptr, pooled.ld,
         ptr(argmax), argmax.stride(0), _s(stream))


def segment_max_fwd(H, n, s, pooled, argmax, stream=None):
    call("gs_segment_max_fwd", H.ptr, H.ld, n, s, H.d, pooled.ptr, pooled.ld, ptr(argmax), argmax.stride(0),
         _s(stream))


def segment_max_bwd(d_pooled, pooled, argmax, n, s, dH, stream=None):
    call("gs_segment_max_bwd", d_pooled.ptr, d_pooled.ld, pooled.ptr, pooled.ld, ptr(argmax), argmax.stride(0), n, s,
         pooled.d, dH.ptr, dH.ld, _s(stream))


ATTN_MAX_S, ATTN_MAX_HIDDEN = 128, 1024      # GS_ATTN_MAX_S / GS_ATTN_MAX_HIDDEN (csrc/gs_attn.hip)


def segment_attn_supported(s, hidden):
    """The range of gs_segment_attn_fwd / _bwd (GS_ENOTSUP outside it)."""
    return 1 <= s <= ATTN_MAX_S and 4 <= hidden <= ATTN_MAX_HIDDEN and hidden % 4 == 0


def segment_attn_fwd(H, inv, a, n, s, pooled, alpha, stream=None):
    """gs_segment_attn_fwd: alpha[i] = softmax_j <V_j, a>, pooled[i] = sum_j alpha[i, j] V_j over each group's s rows V_j =
    H[inv[i*s + j]] (inv None: H[i*s + j]).  a: fp32 device vector [H.d]; alpha: fp32 device vector [n * s]."""
    call("gs_segment_attn_fwd", H.ptr, H.ld, ptr(inv), ptr(a), n, s, H.d, pooled.ptr, pooled.ld, ptr(alpha), _s(stream))
    return pooled


def segment_attn_bwd(dP, H, inv, a, alpha, n, s, dV, n_slabs, slabs_ptr, stream=None):
    """gs_segment_attn_bwd: dV [n*s, H.d] per sampled row (relu mask of V applied) and n_slabs partial sums of da
    ([n_slabs, H.d] at slabs_ptr, each fully written)."""
    call("gs_segment_attn_bwd", dP.ptr, dP.ld, H.ptr, H.ld, ptr(inv), ptr(a), ptr(alpha), n, s, H.d, dV.ptr, dV.ld, slabs_ptr,
         n_slabs, _s(stream))
    return dV


def attn_scores(H, a, stream=None):
    """gs_attn_scores: column H.d of every row of H = <H[r, :H.d], a> (H.ld >= H.d + 4): the logit column of CSR_SOFTMAX."""
    call("gs_attn_scores", H.ptr, H.ld, H.rows, H.d, ptr(a), _s(stream))
    return H


def maxpool_sparse_wgrad(X, ids, n, s, argmax, dpm, hidden, n_slabs, slabs_ptr, ld_slab, stream=None):
    """dW slabs [n_slabs, X.d, ld_slab] of the max-pool MLP from the arg-max rows only (dH never materialised)."""
    call("gs_maxpool_sparse_wgrad", X.ptr, X.ld, ptr(ids), n, s, X.d, ptr(argmax), argmax.stride(0), dpm.ptr, dpm.ld,
         hidden, n_slabs, slabs_ptr, ld_slab, _s(stream))


def pool2_transpose(W, out, stream=None):
    """gs_pool2_transpose: out [W.d, W.rows] = W^T."""
    call("gs_pool2_transpose", W.ptr, W.ld, W.rows, W.d, out.ptr, out.ld, _s(stream))
    return out


def pool2_iota(out, n, stream=None):
    """gs_pool2_iota: out[i] = i for i < n (int32 device tensor)."""
    call("gs_pool2_iota", ptr(out), n, _s(stream))
    return out


def pool2_dgrad_supported(s, hid1, hid2):
    """The range of gs_pool2_dgrad (GS_ENOTSUP outside it: compose segment_max_bwd + dense_dgrad + act_bwd)."""
    return 1 <= s <= 64 and hid1 >= 4 and hid2 >= 4 and hid1 % 4 == 0 and hid2 % 4 == 0 and hid2 <= 1024


def pool2_dgrad(dpm, argmax, H1, h_idx, n, s, dH1, W2=None, W2T=None, stream=None):
    """gs_pool2_dgrad: dH1 [n*s, hid1] of the two-layer max-pool from dpm [n, hid2] and the arg-max, through W2 [hid1, hid2] and
    the relu mask of H1 (rows through h_idx when given).  With W2T (= W2^T, pool2_transpose) the kernel is launched directly
    (gs_pool2_dgrad_t); with W2 the library makes the copy for the call.  A shape outside pool2_dgrad_supported raises."""
    hid1, hid2 = H1.d, dpm.d
    if (W2 is None) == (W2T is None):
        raise _lib.GraphsageAmdError("pool2_dgrad: give W2 or W2T (one of them)")
    if W2T is not None:
        call("gs_pool2_dgrad_t", dpm.ptr, dpm.ld, ptr(argmax), argmax.stride(0), W2T.ptr, W2T.ld, H1.ptr, H1.ld, ptr(h_idx), n, s,
             hid1, hid2, dH1.ptr, dH1.ld, _s(stream))
    else:
        call("gs_pool2_dgrad", dpm.ptr, dpm.ld, ptr(argmax), argmax.stride(0), W2.ptr, W2.ld, H1.ptr, H1.ld, ptr(h_idx), n, s,
             hid1, hid2, dH1.ptr, dH1.ld, _s(stream))
    return dH1


def scatter_add_rows(d, n, s, cols, scale, ids, table, stream=None):
    """table[ids[i*s + j], :cols] += scale * d[i, :cols]  (gradient of a row gather w.r.t. the gathered table)."""
    call("gs_scatter_add_rows", d.ptr, d.ld, n, s, cols, scale, ptr(ids), table.ptr, table.ld, _s(stream))


def copy_cols(src, dst, rows, cols, stream=None):
    call("gs_copy_cols", src.ptr, src.ld, dst.ptr, dst.ld, rows, cols, _s(stream))


# ------------------------------------------------------------------------------------------ K5
def l2norm_fwd(x, n, y, inv_norm, stream=None):
    call("gs_l2norm_fwd", x.ptr, x.ld, n, x.d, y.ptr, y.ld, ptr(inv_norm), _s(stream))


def l2norm_bwd(dy, y, inv_norm, n, dx, stream=None):
    call("gs_l2norm_bwd", dy.ptr, dy.ld, y.ptr, y.ld, ptr(inv_norm), n, y.d, dx.ptr, dx.ld, _s(stream))


def class_loss(logits, labels, n, C, sigmoid_loss, loss_rows, preds=None, dlogits=None, stream=None):
    call("gs_class_loss", logits.ptr, logits.ld, labels.ptr, labels.ld, n, C, 1 if sigmoid_loss else 0,
         ptr(loss_rows), preds.ptr if preds is not None else None, preds.ld if preds is not None else 0,
         dlogits.ptr if dlogits is not None else None, dlogits.ld if dlogits is not None else 0, _s(stream))


def head_fwd_bwd(x, n, W, bias, labels, C, sigmoid_loss, y, logits, preds, dlogits, loss_rows, dx, stream=None):
    call("gs_head_fwd_bwd", x.ptr, x.ld, n, x.d, W.ptr, W.ld, ptr(bias), labels.ptr, labels.ld, C,
         1 if sigmoid_loss else 0, y.ptr, y.ld, logits.ptr if logits is not None else None,
         logits.ld if logits is not None else 0, preds.ptr if preds is not None else None,
         preds.ld if preds is not None else 0, dlogits.ptr, dlogits.ld, ptr(loss_rows),
         dx.ptr if dx is not None else None, dx.ld if dx is not None else 0, _s(stream))


def sage_tail_supported(d_in, out_dim, C):
    return bool(_lib.load().gs_sage_tail_supported(int(d_in), int(out_dim), int(C)))


def tail_sync_words(n, out_dim=128):
    """Size (uint32 words) of the hand-over buffer gs_sage_tail_fwd_bwd needs for n batch rows: epochs, the error word and
    16 x 2*out_dim eight-byte granules per 16-row group (gs_tail_desc.sync).  A buffer serves ONE n."""
    G = (n + 15) // 16
    return 2 * G + 2 + 64 * G * out_dim


def tail_sync_error(sync, n):
    """The error word of a tail hand-over buffer (0 = fine); synchronises."""
    return int(sync[2 * ((n + 15) // 16)].item())


def sage_tail_fwd_bwd(h0, n, s, W_self, W_neigh, out_dim, W_head, b_head, labels, C, sigmoid_loss, means, z, y, logits,
                      preds, dlogits, loss_rows, dz=None, d_h0=None, counters=(), jobs=(), stream=None, sync=None,
                      split=False, jobs_z=(), gcn=False, ids_copy=None, means_ready=False):
    """gs_sage_tail_fwd_bwd: layer 1 + head (+ their input gradients when dz / d_h0 are given) in ONE launch.
    counters: up to three (device int64 tensor, delta) pairs advanced at the end of the launch.
    sync: int32 device tensor of tail_sync_words(n) words, zero-initialised once and owned by ONE caller / stream
    (kernel-internal hand-over state + an error word, see tail_sync_error); a fresh one is allocated if not given.
    split: two launches instead -- gs_sage_tail_z (lean z-helper kernel carrying the gather jobs `jobs_z`) and then this
    entry with z_ready (no helpers, no hand-over state) carrying `jobs`; same results bit for bit.
    ids_copy: (src int32 tensor, dst int32 tensor, count) -- the launch's helper workgroups copy the step's node ids into the
    private buffer the weight gradients gather through (gs_tail_desc.ids_copy_*).
    means_ready: `means` is an input, written by sage_dense_fwd_tiled3_means earlier on the stream (the *_means entry points)."""
    if sync is None and not split:
        import torch
        sync = torch.zeros(tail_sync_words(n, out_dim), dtype=torch.int32, device=h0.buf.device)
        torch.cuda.synchronize()
    assert split or sync.numel() >= tail_sync_words(n, out_dim)
    q = _lib.TailDesc()
    q._keep = sync
    q.sync = ptr(sync) if not split else None
    q.z_ready = 1 if split else 0
    q.h0, q.ldh, q.n = h0.ptr, h0.ld, n
    q.W_self, q.ldws, q.W_neigh, q.ldwn = W_self.ptr, W_self.ld, W_neigh.ptr, W_neigh.ld
    q.W_head, q.ldwh, q.b_head = W_head.ptr, W_head.ld, ptr(b_head)
    q.labels, q.ldlab = labels.ptr, labels.ld
    q.means, q.ldm, q.z, q.ldz, q.y, q.ldy = means.ptr, means.ld, z.ptr, z.ld, y.ptr, y.ld
    q.logits, q.ldlo = (logits.ptr, logits.ld) if logits is not None else (None, 0)
    q.preds, q.ldp = (preds.ptr, preds.ld) if preds is not None else (None, 0)
    q.dlogits, q.lddl, q.loss_rows = dlogits.ptr, dlogits.ld, ptr(loss_rows)
    train = dz is not None and d_h0 is not None
    q.dz, q.lddz = (dz.ptr, dz.ld) if train else (None, 0)
    q.d_h0, q.lddh = (d_h0.ptr, d_h0.ld) if train else (None, 0)
    cs = [(ptr(c), int(d)) for c, d in counters if c is not None and d]
    cs += [(None, 0)] * (3 - len(cs))
    (q.c0, q.d0), (q.c1, q.d1), (q.c2, q.d2) = cs[:3]
    q.s, q.d_in, q.out_dim, q.C, q.sigmoid, q.train = s, h0.d, out_dim, C, 1 if sigmoid_loss else 0, 1 if train else 0
    q.gcn = 1 if gcn else 0          # GCNAggregator layer 1: W_self / W_neigh are the two column halves of ONE weight matrix
    if ids_copy is not None:
        q.ids_copy_src, q.ids_copy_dst, q.ids_copy_n = ptr(ids_copy[0]), ptr(ids_copy[1]), int(ids_copy[2])
    if split:
        jz = list(jobs_z or ())
        jzarr = (_lib.GatherDesc * max(len(jz), 1))(*jz)
        call("gs_sage_tail_z_means" if means_ready else "gs_sage_tail_z", ctypes.addressof(q), ctypes.addressof(jzarr), len(jz),
             _s(stream))
    jobs = list(jobs or ())
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_tail_fwd_bwd_means" if means_ready else "gs_sage_tail_fwd_bwd", ctypes.addressof(q), ctypes.addressof(jarr),
         len(jobs), _s(stream))


def sage_tail_z(h0, n, s, W_self, W_neigh, out_dim, means, z, jobs=(), stream=None, means_ready=False, gcn=False):
    """gs_sage_tail_z: z = [h0[:n] . W_self | mean_j(h0[n + i s + j]) . W_neigh] and the neighbor means of a LAST
    mean-aggregator layer (concat, identity act, no bias) in one lean launch (+ gather jobs riding at the full HBM rate).
    means_ready: gs_sage_tail_z_means (`means` is an input)."""
    q = _lib.TailDesc()
    q.gcn = 1 if gcn else 0
    q.h0, q.ldh, q.n = h0.ptr, h0.ld, n
    q.W_self, q.ldws, q.W_neigh, q.ldwn = W_self.ptr, W_self.ld, W_neigh.ptr, W_neigh.ld
    q.means, q.ldm, q.z, q.ldz = means.ptr, means.ld, z.ptr, z.ld
    q.s, q.d_in, q.out_dim, q.C = s, h0.d, out_dim, 1
    q.z_ready = 1
    jobs = list(jobs or ())
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_tail_z_means" if means_ready else "gs_sage_tail_z", ctypes.addressof(q), ctypes.addressof(jarr), len(jobs), _s(stream))
    return z


def sage_tail_dh0(h0, n, s, W_self, W_neigh, out_dim, dz, d_h0, jobs=(), stream=None):
    """gs_sage_tail_dh0: d_h0 = relu'(h0) * ([dz[:, :O] . W_self^T on the self rows | dz[:, O:] . W_neigh^T / s on the
    neighbor rows]) of a last mean layer, one launch (+ gather jobs)."""
    q = _lib.TailDesc()
    q.h0, q.ldh, q.n = h0.ptr, h0.ld, n
    q.W_self, q.ldws, q.W_neigh, q.ldwn = W_self.ptr, W_self.ld, W_neigh.ptr, W_neigh.ld
    q.dz, q.lddz, q.d_h0, q.lddh = dz.ptr, dz.ld, d_h0.ptr, d_h0.ld
    q.s, q.d_in, q.out_dim, q.C = s, h0.d, out_dim, 1
    q.z_ready = 1
    jobs = list(jobs or ())
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_sage_tail_dh0", ctypes.addressof(q), ctypes.addressof(jarr), len(jobs), _s(stream))
    return d_h0


def linkpred_tail_supported(d_in, out_dim, n_neg):
    return bool(_lib.load().gs_linkpred_tail_supported(int(d_in), int(out_dim), int(n_neg)))


def lp_tail_sync_words(B, n_neg):
    """Size (uint32 words) of the hand-over buffer of linkpred_tail for B pairs and n_neg negatives."""
    return 2 * ((B + 7) // 8 + (n_neg + 15) // 16) + 2


def lp_tail_sync_error(sync, B, n_neg):
    return int(sync[2 * ((B + 7) // 8 + (n_neg + 15) // 16)].item())


def linkpred_tail_desc(h0, B, n_neg, s, W_self, W_neigh, out_dim, means, z, y, loss_rows, rr_rows, aff_all, neg_weight, scale,
                       sync, dz=None, d_h0=None, neg_slabs=None):
    """struct gs_lp_tail_desc of the unsupervised fused tail (see include/graphsage_amd.h); dz / d_h0 / neg_slabs given =
    training (forward + backward), else forward only."""
    assert sync.numel() >= lp_tail_sync_words(B, n_neg)
    q = _lib.LpTailDesc()
    q._keep = (sync, neg_slabs)
    q.h0, q.ldh, q.B, q.n_neg, q.s, q.d_in, q.out_dim = h0.ptr, h0.ld, B, n_neg, s, h0.d, out_dim
    q.W_self, q.ldws, q.W_neigh, q.ldwn = W_self.ptr, W_self.ld, W_neigh.ptr, W_neigh.ld
    q.means, q.ldm, q.z, q.ldz, q.y, q.ldy = means.ptr, means.ld, z.ptr, z.ld, y.ptr, y.ld
    train = dz is not None and d_h0 is not None and neg_slabs is not None
    q.train = 1 if train else 0
    if train:
        q.dz, q.lddz, q.d_h0, q.lddh, q.neg_slabs = dz.ptr, dz.ld, d_h0.ptr, d_h0.ld, ptr(neg_slabs)
    q.loss_rows, q.rr_rows = ptr(loss_rows), ptr(rr_rows)
    q.aff_all, q.ld_aff = (aff_all.ptr, aff_all.ld) if aff_all is not None else (None, 0)
    q.neg_weight, q.scale, q.sync = float(neg_weight), float(scale), ptr(sync)
    return q


def linkpred_tail(desc, jobs=(), stream=None, means_ready=False):
    """gs_linkpred_tail: launch 1 of the unsupervised fused tail (+ gather jobs riding).  means_ready: gs_linkpred_tail_means
    (desc.means is an input, written by sage_dense_fwd_tiled3_means earlier on the stream)."""
    jobs = list(jobs or ())
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_linkpred_tail_means" if means_ready else "gs_linkpred_tail", ctypes.addressof(desc), ctypes.addressof(jarr), len(jobs), _s(stream))


def linkpred_tail_neg(desc, loss_out=None, accumulate=False, mrr_out=None, counters=(), jobs=(), stream=None):
    """gs_linkpred_tail_neg: launch 2 (the negatives' rows, the step epilogue, the commit of the hand-over state) + gather jobs."""
    cs = [(ptr(c), int(d)) for c, d in counters if c is not None and d]
    cs += [(None, 0)] * (3 - len(cs))
    jobs = list(jobs or ())
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_linkpred_tail_neg", ctypes.addressof(desc), ptr(loss_out), 1 if accumulate else 0, ptr(mrr_out),
         cs[0][0], cs[0][1], cs[1][0], cs[1][1], cs[2][0], cs[2][1], ctypes.addressof(jarr), len(jobs), _s(stream))


# ------------------------------------------------------------------------------------------ loss kinds (gs_linkpred_loss.hip)
LP_LOSS_KINDS = {"xent": 0, "skipgram": 1, "hinge": 2}      # GS_LP_LOSS_* of include/graphsage_amd.h
LP_WIDTHS = (64, 128, 256, 512)


def linkpred_loss_fwd_bwd(kind, X, B, n_neg, neg_weight, margin, scale, loss_rows, rr_rows, aff_all, dX, neg_slabs, Y=None,
                          U=None, dU=None, epilogue=None, stream=None):
    """gs_linkpred_loss_fwd_bwd[_step].  U is None: X [2B + n_neg, d] raw aggregator outputs -> Y normalised, dX = dLoss/dX.
    U given ([B, d], the bilinear left operand): X normalised -> dU and rows [B, 2B + n_neg) of dX.
    epilogue: (loss_out, accumulate, mrr_out, [(counter, delta)] * 3) rides in the second launch."""
    if isinstance(kind, str):
        kind = LP_LOSS_KINDS[kind]
    m = lambda a: (a.ptr, a.ld) if a is not None else (None, 0)
    args = (int(kind), X.ptr, X.ld) + m(U) + (B, X.d, n_neg, float(neg_weight), float(margin), float(scale)) + m(Y) + \
           (ptr(loss_rows), ptr(rr_rows)) + m(aff_all) + m(dX) + m(dU) + (ptr(neg_slabs),)
    if epilogue is None:
        call("gs_linkpred_loss_fwd_bwd", *args, _s(stream))
        return
    loss_out, accumulate, mrr_out, counters = epilogue
    cargs = []
    for c, dlt in counters:
        cargs += [ptr(c) if (c is not None and dlt) else None, int(dlt) if c is not None else 0]
    call("gs_linkpred_loss_fwd_bwd_step", *args, ptr(loss_out), 1 if accumulate else 0, ptr(mrr_out), *cargs, _s(stream))


# ------------------------------------------------------------------------------------------ in-batch softmax (gs_infonce.hip)
INFONCE_TAU_RANGE = (0.01, 10.0)


def linkpred_infonce_ws_floats(B, d, n_neg, train=True):
    """gs_linkpred_infonce_ws_floats: fp32 elements of the head's workspace (row statistics, per-tile partial statistics and,
    when training, the partial gradients of the cut sweeps)."""
    n = ctypes.c_int64()
    call("gs_linkpred_infonce_ws_floats", int(B), int(d), int(n_neg), 1 if train else 0, ctypes.byref(n))
    return int(n.value)


def linkpred_infonce_fwd_bwd(X, U, B, n_neg, tau, scale, loss_rows, rr_rows, aff_all, ws, dX=None, dU=None, ids=None,
                             epilogue=None, stream=None):
    """gs_linkpred_infonce_fwd_bwd[_step].  X [2B + n_neg, d] normalised rows, U [B, d] the left operand; ws: fp32 workspace of
    linkpred_infonce_ws_floats(B, d, n_neg, train) elements (its first 2B hold the rows' (maximum, log sum) afterwards).
    dX and dU both given: dU and rows [B, 2B + n_neg) of dX are written; both None: forward only.
    ids: (ids1, ids2) int32 device tensors of the pairs' node ids (the false-negative mask) or None.
    epilogue: (loss_out, accumulate, mrr_out, [(counter, delta)] * 3), as linkpred_loss_fwd_bwd."""
    m = lambda a: (a.ptr, a.ld) if a is not None else (None, 0)
    ids1, ids2 = ids if ids is not None else (None, None)
    for t in (ids1, ids2):
        if t is not None and (t.dtype != torch.int32 or t.numel() < B or not t.is_contiguous()):
            raise _lib.GraphsageAmdError("linkpred_infonce_fwd_bwd: ids must be contiguous int32 tensors of B elements")
    if ws.dtype != torch.float32 or not ws.is_contiguous():
        raise _lib.GraphsageAmdError("linkpred_infonce_fwd_bwd: ws must be a contiguous float32 tensor")
    for name, a in (("U", U), ("dX", dX), ("dU", dU)):
        if a is not None and a.d != X.d:
            raise _lib.GraphsageAmdError("linkpred_infonce_fwd_bwd: %s has width %d, X has %d" % (name, a.d, X.d))
    args = (X.ptr, X.ld, U.ptr, U.ld, B, X.d, n_neg, float(tau), float(scale), ptr(ids1), ptr(ids2), ptr(loss_rows),
            ptr(rr_rows)) + m(aff_all) + (ptr(ws), ws.numel()) + m(dX) + m(dU)
    if epilogue is None:
        call("gs_linkpred_infonce_fwd_bwd", *args, _s(stream))
        return
    loss_out, accumulate, mrr_out, counters = epilogue
    cargs = []
    for c, dlt in counters:
        cargs += [ptr(c) if (c is not None and dlt) else None, int(dlt) if c is not None else 0]
    call("gs_linkpred_infonce_fwd_bwd_step", *args, ptr(loss_out), 1 if accumulate else 0, ptr(mrr_out), *cargs, _s(stream))


# ------------------------------------------------------------------------------------------ LSTM aggregator (gs_lstm.hip)
def lstm_segments(segs):
    """segs: [(X Mat | None, ids int32 tensor | None, n sequences, T steps, row0)] -> (struct gs_lstm_seg array, number of
    sequences, number of step rows).  Sequence rows (lengths, h_last, dh_last) follow the segments' order."""
    assert 1 <= len(segs) <= _lib.GS_LSTM_MAX_SEG, len(segs)
    arr = (_lib.LstmSeg * len(segs))()
    seq0 = rows = 0
    for k, (X, ids, n, T, row0) in enumerate(segs):
        assert n >= 0 and T >= 1 and row0 >= 0
        if ids is not None:
            assert ids.dtype == torch.int32 and ids.is_contiguous() and ids.numel() >= n * T
        elif X is not None:
            assert X.rows >= n * T
        arr[k].X, arr[k].ids = (X.ptr, X.ld) if X is not None else (None, 0)
        arr[k].ids = ptr(ids)
        arr[k].ldx = X.ld if X is not None else 0
        arr[k].n, arr[k].row0, arr[k].seq0, arr[k].T = n, row0, seq0, T
        seq0 += n
        rows = max(rows, row0 + n * T)
    return arr, seq0, rows


def lstm_lengths(segs, d, lengths, stream=None):
    """lengths[r] = max(1, #{t : row t of sequence r is not all zeros}) (aggregators.py:411-414)."""
    arr, n_total, _ = lstm_segments(segs)
    assert lengths.dtype == torch.int32 and lengths.numel() >= n_total
    assert all(X is not None and X.d >= d for X, _, n, _, _ in segs if n > 0)
    call("gs_lstm_lengths", ctypes.addressof(arr), len(segs), d, ptr(lengths), _s(stream))
    return lengths


def lstm_fwd(segs, H, W_h, lengths, G, A, C, H_prev, h_last, stream=None):
    """Forward recurrence of BasicLSTMCell under dynamic_rnn (gs_lstm_fwd); A may be G (in place)."""
    arr, n_total, rows = lstm_segments(segs)
    assert W_h.rows == H and W_h.d == 4 * H and lengths.numel() >= n_total
    assert min(G.rows, A.rows, C.rows, H_prev.rows) >= rows and h_last.rows >= n_total
    assert G.d >= 4 * H and A.d >= 4 * H and C.d >= H and H_prev.d >= H and h_last.d >= H
    call("gs_lstm_fwd", ctypes.addressof(arr), len(segs), H, W_h.ptr, W_h.ld, ptr(lengths), G.ptr, G.ld, A.ptr, A.ld,
         C.ptr, C.ld, H_prev.ptr, H_prev.ld, h_last.ptr, h_last.ld, _s(stream))
    return h_last


def lstm_bwd(segs, H, W_h, wt_ws, lengths, A, C, dh_last, dG, stream=None):
    """Backward recurrence (gs_lstm_bwd): dG = d loss / d(gate pre-activations), zero past each length; dG may be A."""
    arr, n_total, rows = lstm_segments(segs)
    assert W_h.rows == H and W_h.d == 4 * H and lengths.numel() >= n_total and wt_ws.numel() >= 4 * H * H
    assert min(A.rows, C.rows, dG.rows) >= rows and dh_last.rows >= n_total
    assert A.d >= 4 * H and C.d >= H and dh_last.d >= H and dG.d >= 4 * H
    call("gs_lstm_bwd", ctypes.addressof(arr), len(segs), H, W_h.ptr, W_h.ld, ptr(wt_ws), ptr(lengths), A.ptr, A.ld,
         C.ptr, C.ld, dh_last.ptr, dh_last.ld, dG.ptr, dG.ld, _s(stream))
    return dG


# ------------------------------------------------------------------------------------------ K6
def reduce_slabs(slabs, n_slabs, slab_stride, rows, cols, ld_slab, weight_decay, w_ptr, ldw, grad_ptr, ldg,
                 accumulate=False, stream=None):
    call("gs_reduce_slabs", ptr(slabs) if hasattr(slabs, "is_cuda") else slabs, n_slabs, slab_stride, rows, cols,
         ld_slab, weight_decay, w_ptr, ldw, grad_ptr, ldg, 1 if accumulate else 0, _s(stream))


def adam_step(p, grad, m, v, count, lr, step_dev, beta1=0.9, beta2=0.999, eps=1e-8, clip=5.0, grad_scale=1.0,
              step_offset=1, stream=None):
    """TF Adam with t = *step_dev + step_offset (0 when the step counter was already advanced this step)."""
    call("gs_adam_step", ptr(p), ptr(grad), ptr(m), ptr(v), count, lr, beta1, beta2, eps, clip, grad_scale,
         ptr(step_dev), int(step_offset), _s(stream))


def flat_reduce_adam_sample(var_descs, params, grads, m, v, total, weight_decay, fuse_adam, lr, step_dev, beta1=0.9, beta2=0.999,
                            eps=1e-8, clip=5.0, grad_scale=1.0, step_offset=1, loss=None, sampler=None, jobs=(), stream=None):
    """gs_flat_reduce_adam_sample: the slab reduce (+ weight decay, + clip and Adam when fuse_adam) over the ctypes array
    `var_descs` of VarDesc, with its riders -- loss = (loss_rows, n, scale, loss_out, accumulate) or None, sampler = a fanout_desc()
    or None, jobs = gather_job() descriptors of the next mini-batch."""
    lr_, ln, lscale, lout, lacc = loss if loss is not None else (None, 0, 0.0, None, False)
    jobs = list(jobs or ())
    jarr = (_lib.GatherDesc * max(len(jobs), 1))(*jobs)
    call("gs_flat_reduce_adam_sample", ctypes.addressof(var_descs), len(var_descs), ptr(params), ptr(grads), ptr(m), ptr(v), total,
         float(weight_decay), 1 if fuse_adam else 0, lr, beta1, beta2, eps, clip, grad_scale, ptr(step_dev), int(step_offset),
         ptr(lr_), ln, float(lscale), ptr(lout), 1 if lacc else 0, ctypes.addressof(sampler) if sampler is not None else None,
         ctypes.addressof(jarr), len(jobs), _s(stream))


def sum_scaled(x, count, scale, out, accumulate=False, stream=None):
    call("gs_sum_scaled", ptr(x), count, scale, ptr(out), 1 if accumulate else 0, _s(stream))


def sumsq_scaled(x, count, scale, out, accumulate=False, stream=None):
    call("gs_sumsq_scaled", ptr(x), count, scale, ptr(out), 1 if accumulate else 0, _s(stream))


# ------------------------------------------------------------------------------------------ LOGREG (gs_logreg.hip)
LOGREG_FIT, LOGREG_PREDICT = _lib.LOGREG_FIT, _lib.LOGREG_PREDICT
LOGREG_MAX_D, LOGREG_MAX_C = _lib.LOGREG_MAX_D, _lib.LOGREG_MAX_C


def logreg_ws_bytes(n, d, c):
    """Bytes of the fp32 workspace gs_logreg_eval needs for n rows of width d and c classes."""
    out = ctypes.c_int64(0)
    call("gs_logreg_ws_bytes", n, d, c, ctypes.byref(out))
    return out.value


def logreg_eval(X, W, b, n=None, rows=None, y_class=None, y_multi=None, mode=LOGREG_FIT, loss=None, gW=None, gb=None,
                pred_class=None, pred_multi=None, ws=None, stream=None):
    """gs_logreg_eval: one evaluation of the one-vs-rest logistic regression z = X[rows] W + b on the device.
    X: Mat [n_rows, d]; W: Mat [d, c]; b: float32 [c]; rows: int32 [n] with entries in [0, X.rows) (checked by the caller) or
    None (rows 0 .. n-1); y_class: int32 [n] in [0, c) or y_multi: uint8 [n, >= c].
    LOGREG_FIT returns (loss [c], gW [d, c], gb [c]) as float64 SUMS over the rows (no mean, no regulariser).
    LOGREG_PREDICT writes the given pred_class (int32 [n]) / pred_multi (uint8 [n, >= c]) and, with labels and `loss`, loss."""
    d, c = X.d, W.d
    n = (rows.numel() if rows is not None else X.rows) if n is None else int(n)
    if W.rows != d or b.numel() != c or b.dtype != torch.float32:
        raise _lib.GraphsageAmdError("logreg_eval: X is [%d, %d], W [%d, %d], b has %d entries" % (X.rows, d, W.rows, c, b.numel()))
    if rows is not None and (rows.dtype != torch.int32 or rows.numel() != n):
        raise _lib.GraphsageAmdError("logreg_eval: rows must be an int32 vector of n=%d entries" % n)
    if y_class is not None and (y_class.dtype != torch.int32 or y_class.numel() != n):
        raise _lib.GraphsageAmdError("logreg_eval: y_class must be an int32 vector of n=%d entries" % n)
    for name, m in (("y_multi", y_multi), ("pred_multi", pred_multi)):
        if m is not None and (m.dtype != torch.uint8 or m.dim() != 2 or m.shape[0] != n or m.shape[1] < c or m.stride(1) != 1):
            raise _lib.GraphsageAmdError("logreg_eval: %s must be a uint8 matrix [n=%d, >= c=%d]" % (name, n, c))
    if pred_class is not None and (pred_class.dtype != torch.int32 or pred_class.numel() != n):
        raise _lib.GraphsageAmdError("logreg_eval: pred_class must be an int32 vector of n=%d entries" % n)
    dev = X.buf.device
    fit = mode == LOGREG_FIT
    if fit:
        loss = torch.empty(c, dtype=torch.float64, device=dev) if loss is None else loss
        gW = torch.empty((d, c), dtype=torch.float64, device=dev) if gW is None else gW
        gb = torch.empty(c, dtype=torch.float64, device=dev) if gb is None else gb
    for name, t, numel in (("loss", loss, c), ("gW", gW, d * c), ("gb", gb, c)):
        if t is not None and (t.dtype != torch.float64 or t.numel() != numel or not t.is_contiguous()):
            raise _lib.GraphsageAmdError("logreg_eval: %s must be a dense float64 array of %d entries" % (name, numel))
    if loss is not None and ws is None:
        ws = torch.empty(max(logreg_ws_bytes(n, d, c) // 4, 2), dtype=torch.float32, device=dev)
    q = _lib.LogregDesc()
    q.X, q.rows, q.W, q.b, q.y_class, q.y_multi = X.ptr, ptr(rows), W.ptr, ptr(b), ptr(y_class), ptr(y_multi)
    q.loss, q.gW, q.gb, q.pred_class, q.pred_multi, q.ws = ptr(loss), ptr(gW), ptr(gb), ptr(pred_class), ptr(pred_multi), ptr(ws)
    q.n, q.n_rows, q.ldx, q.ldw = n, X.rows, X.ld, W.ld
    q.ldy = y_multi.stride(0) if y_multi is not None else 0
    q.ldp = pred_multi.stride(0) if pred_multi is not None else 0
    q.ws_bytes = 4 * ws.numel() if ws is not None else 0
    q.d, q.c, q.mode, q.flags = d, c, mode, 0
    call("gs_logreg_eval", ctypes.addressof(q), _s(stream))
    return (loss, gW, gb) if fit else (pred_class, pred_multi, loss)


LOGREG_JOINED_MAX_D = _lib.LOGREG_JOINED_MAX_D


def logreg_joined_ws_bytes(n, d, c):
    """Bytes of the fp32 workspace gs_logreg_eval_joined needs for n rows of joined width d and c classes."""
    out = ctypes.c_int64(0)
    call("gs_logreg_joined_ws_bytes", n, d, c, ctypes.byref(out))
    return out.value


def _joined_sources(who, Xa, rows_a, Xb, rows_b, n):
    """(n, da, db) of a joined problem after the checks a pointer cannot carry."""
    n = (rows_a.numel() if rows_a is not None else (rows_b.numel() if rows_b is not None else Xa.rows)) if n is None else int(n)
    if Xb is None and rows_b is not None:
        raise _lib.GraphsageAmdError("%s: rows_b without Xb" % who)
    for name, r in (("rows_a", rows_a), ("rows_b", rows_b)):
        if r is not None and (r.dtype != torch.int32 or r.numel() != n):
            raise _lib.GraphsageAmdError("%s: %s must be an int32 vector of n=%d entries" % (who, name, n))
    return n, Xa.d, (Xb.d if Xb is not None else 0)


def logreg_eval_joined(Xa, W, b, Xb=None, n=None, rows_a=None, rows_b=None, mu=None, inv=None, y_class=None, y_multi=None,
                       mode=LOGREG_FIT, loss=None, gW=None, gb=None, pred_class=None, pred_multi=None, ws=None, stream=None):
    """gs_logreg_eval_joined: logreg_eval on rows joined from two tables and standardised while they are staged,
    x[i] = ([Xa[rows_a[i]] | Xb[rows_b[i]]] - mu) * inv.  Xa: Mat [*, da]; Xb: Mat [*, db] or None; W: Mat [da + db, c];
    mu, inv: float32 [da + db], both or neither; the rest as logreg_eval.  da + db <= LOGREG_JOINED_MAX_D."""
    n, da, db = _joined_sources("logreg_eval_joined", Xa, rows_a, Xb, rows_b, n)
    d, c = da + db, W.d
    if W.rows != d or b.numel() != c or b.dtype != torch.float32:
        raise _lib.GraphsageAmdError("logreg_eval_joined: the joined width is %d + %d, W [%d, %d], b has %d entries" % (
            da, db, W.rows, c, b.numel()))
    for name, t in (("mu", mu), ("inv", inv)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != d or not t.is_contiguous()):
            raise _lib.GraphsageAmdError("logreg_eval_joined: %s must be a dense float32 vector of d=%d entries" % (name, d))
    if y_class is not None and (y_class.dtype != torch.int32 or y_class.numel() != n):
        raise _lib.GraphsageAmdError("logreg_eval_joined: y_class must be an int32 vector of n=%d entries" % n)
    for name, m in (("y_multi", y_multi), ("pred_multi", pred_multi)):
        if m is not None and (m.dtype != torch.uint8 or m.dim() != 2 or m.shape[0] != n or m.shape[1] < c or m.stride(1) != 1):
            raise _lib.GraphsageAmdError("logreg_eval_joined: %s must be a uint8 matrix [n=%d, >= c=%d]" % (name, n, c))
    if pred_class is not None and (pred_class.dtype != torch.int32 or pred_class.numel() != n):
        raise _lib.GraphsageAmdError("logreg_eval_joined: pred_class must be an int32 vector of n=%d entries" % n)
    dev = Xa.buf.device
    fit = mode == LOGREG_FIT
    if fit:
        loss = torch.empty(c, dtype=torch.float64, device=dev) if loss is None else loss
        gW = torch.empty((d, c), dtype=torch.float64, device=dev) if gW is None else gW
        gb = torch.empty(c, dtype=torch.float64, device=dev) if gb is None else gb
    for name, t, numel in (("loss", loss, c), ("gW", gW, d * c), ("gb", gb, c)):
        if t is not None and (t.dtype != torch.float64 or t.numel() != numel or not t.is_contiguous()):
            raise _lib.GraphsageAmdError("logreg_eval_joined: %s must be a dense float64 array of %d entries" % (name, numel))
    if loss is not None and ws is None:
        ws = torch.empty(max(logreg_joined_ws_bytes(n, d, c) // 4, 2), dtype=torch.float32, device=dev)
    q = _lib.LogregJoinedDesc()
    q.Xa, q.rows_a, q.lda, q.n_rows_a, q.da = Xa.ptr, ptr(rows_a), Xa.ld, Xa.rows, da
    if Xb is not None:
        q.Xb, q.rows_b, q.ldb, q.n_rows_b, q.db = Xb.ptr, ptr(rows_b), Xb.ld, Xb.rows, db
    q.mu, q.inv, q.W, q.b, q.y_class, q.y_multi = ptr(mu), ptr(inv), W.ptr, ptr(b), ptr(y_class), ptr(y_multi)
    q.loss, q.gW, q.gb, q.pred_class, q.pred_multi, q.ws = ptr(loss), ptr(gW), ptr(gb), ptr(pred_class), ptr(pred_multi), ptr(ws)
    q.n, q.ldw = n, W.ld
    q.ldy = y_multi.stride(0) if y_multi is not None else 0
    q.ldp = pred_multi.stride(0) if pred_multi is not None else 0
    q.ws_bytes = 4 * ws.numel() if ws is not None else 0
    q.c, q.mode, q.flags = c, mode, 0
    call("gs_logreg_eval_joined", ctypes.addressof(q), _s(stream))
    return (loss, gW, gb) if fit else (pred_class, pred_multi, loss)


def col_moments(Xa, Xb=None, n=None, rows_a=None, rows_b=None, mean=None, var=None, ws=None, stream=None):
    """gs_col_moments: (mean, var) float64 [da + db] of the joined rows [Xa[rows_a[i]] | Xb[rows_b[i]]], i < n: the column
    means and the POPULATION variances, centred, in a fixed order (bitwise repeatable; a constant column has var == 0.0)."""
    n, da, db = _joined_sources("col_moments", Xa, rows_a, Xb, rows_b, n)
    d = da + db
    dev = Xa.buf.device
    mean = torch.empty(d, dtype=torch.float64, device=dev) if mean is None else mean
    var = torch.empty(d, dtype=torch.float64, device=dev) if var is None else var
    for name, t in (("mean", mean), ("var", var)):
        if t.dtype != torch.float64 or t.numel() != d or not t.is_contiguous():
            raise _lib.GraphsageAmdError("col_moments: %s must be a dense float64 vector of d=%d entries" % (name, d))
    if ws is None:
        ws = torch.empty(_lib.COL_MOMENTS_MAX_CHUNKS * d, dtype=torch.float64, device=dev)
    call("gs_col_moments", Xa.ptr, ptr(rows_a), Xa.ld, da, Xa.rows, Xb.ptr if Xb is not None else None, ptr(rows_b),
         Xb.ld if Xb is not None else 0, db, Xb.rows if Xb is not None else 0, n, ptr(mean), ptr(var), ptr(ws),
         ws.numel() * ws.element_size(), _s(stream))
    return mean, var


# ------------------------------------------------------------------------------------------ KMEANS (gs_kmeans.hip)
KMEANS_MAX_K = _lib.KMEANS_MAX_K  # largest k of gs_kmeans_assign / gs_kmeans_members


def _kmeans_rows(who, X, rows, n):
    """n of a (table, rows) pair; rows: int32 device vector with entries in [0, X.rows) (checked by the caller) or None."""
    n = (rows.numel() if rows is not None else X.rows) if n is None else int(n)
    if rows is not None and (rows.dtype != torch.int32 or rows.numel() != n or not rows.is_contiguous()):
        raise _lib.GraphsageAmdError("%s: rows must be a dense int32 vector of n=%d entries" % (who, n))
    if n < 1 or (rows is None and n > X.rows):
        raise _lib.GraphsageAmdError("%s: n=%d rows asked of a table of %d" % (who, n, X.rows))
    return n


def _kmeans_vec(who, name, t, dtype, n):
    if t is not None and (t.dtype != dtype or t.numel() != n or not t.is_contiguous()):
        raise _lib.GraphsageAmdError("%s: %s must be a dense %s vector of %d entries" % (who, name, str(dtype).split(".")[-1], n))


def kmeans_sqnorm(X, rows=None, n=None, out=None, stream=None):
    """gs_kmeans_sqnorm: out[i] = |X[rows[i]]|^2 (rows None: row i), float32 [n], in a fixed order of additions."""
    n = _kmeans_rows("kmeans_sqnorm", X, rows, n)
    out = torch.empty(n, dtype=torch.float32, device=X.buf.device) if out is None else out
    _kmeans_vec("kmeans_sqnorm", "out", out, torch.float32, n)
    call("gs_kmeans_sqnorm", X.ptr, X.ld, X.rows, ptr(rows), n, X.d, ptr(out), _s(stream))
    return out


def kmeans_assign_ws_bytes(n):
    """Bytes of the workspace gs_kmeans_assign needs for n rows (one 16-byte slot per workgroup of 128 rows)."""
    out = ctypes.c_int64(0)
    call("gs_kmeans_assign_ws_bytes", n, ctypes.byref(out))
    return out.value


def kmeans_assign(X, C, csq, rows=None, n=None, xsq=None, prev=None, assign=None, dist=None, stats=None, ws=None, stream=None):
    """gs_kmeans_assign: assign[i] = argmax_j <X[rows[i]], C[j]> - csq[j] / 2 (an exact tie to the lowest j), dist[i] =
    max(0, xsq[i] - 2 * that score) where `dist` is given, and stats = one 16-byte device buffer (torch.int64 [2]): the bits
    of the float64 sum of dist, then the number of rows with assign[i] != prev[i] (0 without prev); read it with
    kmeans_stats.  X: Mat [n_rows, d]; C: Mat [k, d]; csq float32 [k] (kmeans_sqnorm(C)); rows: int32 [n] with entries in
    [0, X.rows) (checked by the caller) or None; xsq float32 [n] by position; prev, assign int32 [n].
    Returns (assign, dist, stats)."""
    who = "kmeans_assign"
    k, d = C.rows, C.d
    n = _kmeans_rows(who, X, rows, n)
    if X.d != d:
        raise _lib.GraphsageAmdError("%s: X is [%d, %d], C [%d, %d]" % (who, X.rows, X.d, k, d))
    if not 1 <= k <= KMEANS_MAX_K:
        raise _lib.GraphsageAmdError("%s: k=%d must lie in [1, %d]" % (who, k, KMEANS_MAX_K))
    dev = X.buf.device
    assign = torch.empty(n, dtype=torch.int32, device=dev) if assign is None else assign
    stats = torch.zeros(2, dtype=torch.int64, device=dev) if stats is None else stats
    if ws is None:
        ws = torch.empty(max(kmeans_assign_ws_bytes(n) // 8, 2), dtype=torch.int64, device=dev)
    for name, t, dtype, m in (("csq", csq, torch.float32, k), ("xsq", xsq, torch.float32, n), ("prev", prev, torch.int32, n),
                              ("assign", assign, torch.int32, n), ("dist", dist, torch.float32, n),
                              ("stats", stats, torch.int64, 2)):
        _kmeans_vec(who, name, t, dtype, m)
    if csq is None:
        raise _lib.GraphsageAmdError("%s: csq is needed (kmeans_sqnorm of the centroids)" % who)
    q = _lib.KmeansDesc()
    q.X, q.rows, q.C, q.csq, q.xsq, q.prev = X.ptr, ptr(rows), C.ptr, ptr(csq), ptr(xsq), ptr(prev)
    q.assign, q.dist, q.stats, q.ws = ptr(assign), ptr(dist), ptr(stats), ptr(ws)
    q.n, q.n_rows, q.ld, q.ldc, q.ws_bytes = n, X.rows, X.ld, C.ld, ws.numel() * ws.element_size()
    q.k, q.d = k, d
    call("gs_kmeans_assign", ctypes.addressof(q), _s(stream))
    return assign, dist, stats


def kmeans_stats(stats):
    """(inertia, changed) of kmeans_assign's stats buffer: one 16-byte copy to the host."""
    h = stats.cpu().numpy()
    return float(h.view("float64")[0]), int(h[1])


def kmeans_members_ws_bytes(n, k, chunk=0):
    """Bytes of the int32 workspace gs_kmeans_members needs (one histogram of k counters per chunk of the n entries)."""
    out = ctypes.c_int64(0)
    call("gs_kmeans_members_ws_bytes", n, k, chunk, ctypes.byref(out))
    return out.value


def kmeans_members(assign, k, rows=None, rowptr=None, members=None, ws=None, chunk=0, stream=None):
    """gs_kmeans_members: the stable grouping of assign int32 [n] (entries in [0, k)): rowptr int64 [k + 1] and members int32
    [n], cluster j's run holding rows[i] (i without rows) of its members in ascending i.  chunk: the entries one wave walks
    (0: the library's default; a multiple of 64) -- the result does not depend on it.  Returns (rowptr, members)."""
    who = "kmeans_members"
    n, k, chunk = assign.numel(), int(k), int(chunk)
    if not 1 <= k <= KMEANS_MAX_K or n < 1:
        raise _lib.GraphsageAmdError("%s: k=%d must lie in [1, %d] and n=%d be positive" % (who, k, KMEANS_MAX_K, n))
    dev = assign.device
    rowptr = torch.empty(k + 1, dtype=torch.int64, device=dev) if rowptr is None else rowptr
    members = torch.empty(n, dtype=torch.int32, device=dev) if members is None else members
    for name, t, dtype, m in (("assign", assign, torch.int32, n), ("rows", rows, torch.int32, n),
                              ("rowptr", rowptr, torch.int64, k + 1), ("members", members, torch.int32, n)):
        _kmeans_vec(who, name, t, dtype, m)
    if ws is None:
        ws = torch.empty(max(kmeans_members_ws_bytes(n, k, chunk) // 4, 1), dtype=torch.int32, device=dev)
    q = _lib.KmeansMembersDesc()
    q.assign, q.rows, q.rowptr, q.members, q.ws = ptr(assign), ptr(rows), ptr(rowptr), ptr(members), ptr(ws)
    q.n, q.ws_bytes, q.k, q.chunk, q.reserved_ = n, ws.numel() * ws.element_size(), k, chunk, 0
    call("gs_kmeans_members", ctypes.addressof(q), _s(stream))
    return rowptr, members


# ------------------------------------------------------------------------------------------ IVF (gs_ivf.hip)
IVF_MAX_PROBE = _lib.IVF_MAX_PROBE  # largest nprobe of gs_ivf_search


def ivf_ws_bytes(Q, n_clusters, k, nprobe):
    """Bytes of the workspace gs_ivf_search needs for Q queries probing nprobe of n_clusters lists at this k."""
    out = ctypes.c_int64(0)
    call("gs_ivf_ws_bytes", Q, n_clusters, k, nprobe, ctypes.byref(out))
    return out.value


def ivf_search(Xq, Zc, centers, list_ptr, list_ids, k, nprobe, n_cand=None, src=None, f_rowptr=None, f_col=None, keep_src=False,
               ids=None, scores=None, count=None, scanned=None, ws=None, chunk=RANK_CHUNK, stop_after=0, stream=None):
    """gs_ivf_search: for every row q of Xq the k first candidates of gs_topk_select (same src, filter and keep_src) among the
    members of the nprobe lists whose centres come first by (<Xq[q], centers[j]> descending, j ascending).  centers: Mat [C, d];
    list_ptr int64 [C + 1] and list_ids int32 (ops.kmeans_members; entries in [0, n_cand), checked by the caller).  chunk:
    the queries of one library call (the result does not depend on it); stop_after: 1 .. 5 ends every call after that step
    (measurement only).  Returns (ids int32 [Q, k], scores float32 [Q, k], count int32 [Q], scanned int64 [Q])."""
    who = "ivf_search"
    Q, k, nprobe, chunk = Xq.rows, int(k), int(nprobe), int(chunk)
    n_cand = Zc.rows if n_cand is None else int(n_cand)
    q = _query_desc(_lib.IvfDesc(), (who, ""), Xq, Zc, Q, n_cand, f_rowptr, f_col, keep_src)
    C = centers.rows
    if centers.d != Zc.d or not 1 <= C <= KMEANS_MAX_K:
        raise _lib.GraphsageAmdError("%s: centers is [%d, %d], Zc [%d, %d]; 1 to %d clusters" % (who, C, centers.d, Zc.rows, Zc.d,
                                                                                            KMEANS_MAX_K))
    if not 1 <= k <= TOPK_MAX:
        raise _lib.GraphsageAmdError("%s: k=%d must lie in [1, %d]" % (who, k, TOPK_MAX))
    if not 1 <= nprobe <= min(IVF_MAX_PROBE, C):
        raise _lib.GraphsageAmdError("%s: nprobe=%d must lie in [1, min(%d, %d clusters)]" % (who, nprobe, IVF_MAX_PROBE, C))
    if not 1 <= chunk <= RANK_CHUNK:
        raise _lib.GraphsageAmdError("%s: chunk=%d must lie in [1, %d]" % (who, chunk, RANK_CHUNK))
    if src is not None and (src.dtype != torch.int32 or src.numel() != Q):
        raise _lib.GraphsageAmdError("%s: src must be an int32 vector with one entry per query" % who)
    if (list_ptr.dtype, list_ids.dtype) != (torch.int64, torch.int32) or list_ptr.numel() != C + 1 or not (
            list_ptr.is_contiguous() and list_ids.is_contiguous()):
        raise _lib.GraphsageAmdError("%s: the lists are a dense int64 list_ptr [C + 1] with a dense int32 list_ids" % who)
    dev = Xq.buf.device
    ids = torch.empty((Q, k), dtype=torch.int32, device=dev) if ids is None else ids
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev) if scores is None else scores
    count = torch.empty(Q, dtype=torch.int32, device=dev) if count is None else count
    scanned = torch.empty(Q, dtype=torch.int64, device=dev) if scanned is None else scanned
    if tuple(ids.shape) != (Q, k) or tuple(scores.shape) != (Q, k) or count.numel() != Q or scanned.numel() != Q or not (
            ids.is_contiguous() and scores.is_contiguous() and count.is_contiguous() and scanned.is_contiguous()) or (
            ids.dtype, scores.dtype, count.dtype, scanned.dtype) != (torch.int32, torch.float32, torch.int32, torch.int64):
        raise _lib.GraphsageAmdError("%s: ids int32 [Q, k], scores float32 [Q, k], count int32 [Q] and scanned int64 [Q] must be "
                                     "dense" % who)
    need = max(ivf_ws_bytes(n, C, k, nprobe) for n in {min(Q, chunk), Q % chunk})        # the two chunk sizes that occur
    if ws is None:
        ws = torch.empty(max((need + 7) // 8, 2), dtype=torch.int64, device=dev)
    q.centers, q.ldc, q.list_ptr, q.list_ids, q.n_list = centers.ptr, centers.ld, ptr(list_ptr), ptr(list_ids), list_ids.numel()
    q.ws, q.ws_bytes, q.k, q.nprobe, q.n_clusters, q.stop_after = ptr(ws), ws.element_size() * ws.numel(), k, nprobe, C, stop_after
    for q0 in range(0, max(Q, 1), chunk):
        n = min(chunk, Q - q0)
        q.Q, q.Xq = n, Xq.ptr + 4 * q0 * Xq.ld
        q.src = ptr(src[q0:q0 + n]) if src is not None else None
        q.ids, q.scores, q.count, q.scanned = (ptr(ids[q0:q0 + n]), ptr(scores[q0:q0 + n]), ptr(count[q0:q0 + n]),
                                               ptr(scanned[q0:q0 + n]))
        call("gs_ivf_search", ctypes.addressof(q), _s(stream))
    return ids, scores, count, scanned


# ------------------------------------------------------------------------------------------ PROP
PROP_MAX_D = _lib.PROP_MAX_D        # widest table of gs_prop_step / gs_prop_correct


def prop_weights(rowptr, col, n_rows, pad, deg=None, w=None, stream=None):
    """gs_prop_weights: deg[r] = the entries of CSR row r that are not `pad` (deg[pad] = 0), w[r] = fp32(1 / sqrt((double)deg[r])),
    0 at deg 0.  Returns (deg int32 [n_rows], w float32 [n_rows])."""
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or rowptr.numel() != n_rows + 1:
        raise _lib.GraphsageAmdError("prop_weights: the CSR is an int64 rowptr [n_rows + 1] with an int32 col")
    deg = torch.empty(n_rows, dtype=torch.int32, device=rowptr.device) if deg is None else deg
    w = torch.empty(n_rows, dtype=torch.float32, device=rowptr.device) if w is None else w
    if (deg.dtype, w.dtype) != (torch.int32, torch.float32) or deg.numel() != n_rows or w.numel() != n_rows or not (
            deg.is_contiguous() and w.is_contiguous()):
        raise _lib.GraphsageAmdError("prop_weights: deg int32 [n_rows] and w float32 [n_rows] must be dense")
    call("gs_prop_weights", ptr(rowptr), ptr(col), n_rows, pad, ptr(deg), ptr(w), _s(stream))
    return deg, w


def prop_ws_bytes(n_slots, d):
    """Bytes of the partials workspace gs_prop_step needs for n_slots segments of cut rows at width d."""
    out = ctypes.c_int64(0)
    call("gs_prop_ws_bytes", n_slots, d, ctypes.byref(out))
    return out.value


def prop_step(rowptr, col, items, splits, n_rows, split_len, pad, w, X, out, R=None, alpha=1.0, lo=float("-inf"),
              hi=float("inf"), n_slots=0, ws=None, d=None, stream=None):
    """gs_prop_step: out[r] = clamp(fmaf(alpha, w[r] * sum_e w[col[e]] * X[col[e]], R[r])) for every row of a planned CSR graph
    (inference.FullGraph owns the plan: items / splits over all rows, n_slots partial slots), out[pad] = 0; a pad entry adds
    exactly 0.  X, out, R (nullable): Mats of n_rows rows, out not X; w: float32 [n_rows] (prop_weights); d: the width, X.d
    unless given."""
    for name, m in (("X", X), ("out", out), ("R", R)):
        if m is not None and m.rows < n_rows:
            raise _lib.GraphsageAmdError("prop_step: %s has %d rows, the graph %d" % (name, m.rows, n_rows))
    if w.dtype != torch.float32 or w.numel() != n_rows or not w.is_contiguous():
        raise _lib.GraphsageAmdError("prop_step: w must be a dense float32 vector of n_rows = %d entries" % n_rows)
    q = _lib.PropDesc()
    q.rowptr, q.col, q.items, q.splits = ptr(rowptr), ptr(col), ptr(items), ptr(splits)
    q.X, q.R, q.w, q.out, q.ws = X.ptr, (R.ptr if R is not None else None), ptr(w), out.ptr, ptr(ws)
    q.n_rows, q.nnz, q.n_items, q.n_split = n_rows, col.numel(), items.shape[0], (splits.shape[0] if splits is not None else 0)
    q.n_slots, q.pad, q.ldx, q.ldr, q.ldo = n_slots, pad, X.ld, (R.ld if R is not None else 0), out.ld
    q.ws_bytes = 4 * ws.numel() if ws is not None else 0
    q.alpha, q.lo, q.hi, q.d, q.split_len = alpha, lo, hi, (X.d if d is None else d), split_len
    call("gs_prop_step", ctypes.addressof(q), _s(stream))
    return out


def prop_correct(P, E, sigma, out, Y=None, known=None, n=None, stream=None):
    """gs_prop_correct: out[i] = known[i] ? Y[i] : P[i] + scale_i * E[i] for the first n rows, scale_i = sigma / sum_j |E[i][j]|,
    replaced by 1 where it is not finite or exceeds 1000.  known: int32 device flags [n]; Y, known None: no row is known."""
    n = P.rows if n is None else int(n)
    for name, m in (("P", P), ("E", E), ("out", out), ("Y", Y)):
        if m is not None and (m.rows < n or m.d != P.d):
            raise _lib.GraphsageAmdError("prop_correct: %s is [%d, %d], wanted [>= %d, %d]" % (name, m.rows, m.d, n, P.d))
    if (Y is None) != (known is None) or (known is not None and (known.dtype != torch.int32 or known.numel() < n
                                                                  or not known.is_contiguous())):
        raise _lib.GraphsageAmdError("prop_correct: Y comes with a dense int32 vector known of n = %d flags" % n)
    call("gs_prop_correct", P.ptr, P.ld, E.ptr, E.ld, (Y.ptr if Y is not None else None), (Y.ld if Y is not None else 0),
         ptr(known), n, P.d, sigma, out.ptr, out.ld, _s(stream))
    return out


# ------------------------------------------------------------------------------------------ NBR
NBR_TILE = _lib.NBR_TILE                        # candidate ids per LDS tile unless the caller overrides it
NBR_MIN_TILE, NBR_MAX_TILE = _lib.NBR_MIN_TILE, _lib.NBR_MAX_TILE
NBR_PARTNER_CHUNK = _lib.NBR_PARTNER_CHUNK      # partners of one source that are ranked per pass over a tile
NBR_CURSORS = _lib.NBR_CURSORS                  # neighbors of a source whose row cursors fit in LDS
NBR_KINDS = {"sum": _lib.NBR_SUM, "jaccard": _lib.NBR_JACCARD}


def nbr_rank_grid(n_groups, max_workgroups=0):
    """Workgroups gs_nbr_rank launches for n_groups source groups (max_workgroups > 0 caps them)."""
    out = ctypes.c_int64(0)
    call("gs_nbr_rank_grid", n_groups, max_workgroups, ctypes.byref(out))
    return out.value


def nbr_rank_ws_bytes(n_workgroups, max_src_degree):
    """Bytes of the cursor workspace gs_nbr_rank wants for sources of up to max_src_degree neighbors (0 while they fit in LDS)."""
    out = ctypes.c_int64(0)
    call("gs_nbr_rank_ws_bytes", n_workgroups, max_src_degree, ctypes.byref(out))
    return out.value


def nbr_rank(rowptr, col, n_nodes, group_ptr, group_src, dst, q=None, deg=None, f_rowptr=None, f_col=None, kind="sum", tile=0,
             max_workgroups=0, max_src_degree=0, t=None, n_gt=None, n_eq=None, ws=None, stream=None):
    """gs_nbr_rank over a SIMPLE CSR graph (rows strictly ascending, ids in [0, n_nodes), validated by the caller -- see
    link_heuristics.SimpleGraph): for the queries dst (int32, grouped by source: group g = group_src[g] with
    dst[group_ptr[g]:group_ptr[g + 1]]) t = s(src, dst) with s(u, x) = sum of q[w] over w in N(u) with x in N(w) (q uint32 [N]; None:
    1), and the numbers n_gt / n_eq of candidates (all nodes but dst, src and the filter row of src) that rank above / tie.
    kind "jaccard" ranks by s / (deg[u] + deg[x] - s) (deg int32 [N], q None).  max_src_degree: the longest source row (sizes the
    cursor workspace).  Returns (t uint32, n_gt int32, n_eq int32) in group order."""
    dev = rowptr.device
    G, Q = group_src.numel(), dst.numel()
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or rowptr.numel() != n_nodes + 1:
        raise _lib.GraphsageAmdError("nbr_rank: the CSR is an int64 rowptr [n_nodes + 1] with an int32 col")
    if group_ptr.dtype != torch.int64 or group_ptr.numel() != G + 1 or group_src.dtype != torch.int32 or dst.dtype != torch.int32:
        raise _lib.GraphsageAmdError("nbr_rank: group_ptr int64 [groups + 1], group_src and dst int32")
    if kind not in NBR_KINDS:
        raise _lib.GraphsageAmdError("nbr_rank: kind must be one of %s" % sorted(NBR_KINDS))
    for name, v in (("q", q), ("deg", deg)):           # q: the uint32 bits in an int32 tensor
        if v is not None and (v.numel() != n_nodes or not v.is_contiguous() or v.dtype != torch.int32):
            raise _lib.GraphsageAmdError("nbr_rank: %s must be a dense int32 vector of n_nodes = %d entries" % (name, n_nodes))
    if (f_rowptr is None) != (f_col is None) or (f_rowptr is not None and (
            f_rowptr.dtype != torch.int64 or f_rowptr.numel() != n_nodes + 1 or f_col.dtype != torch.int32)):
        raise _lib.GraphsageAmdError("nbr_rank: the filter is an int64 f_rowptr [n_nodes + 1] with an int32 f_col, or neither")
    t = torch.zeros(Q, dtype=torch.int32, device=dev) if t is None else t
    n_gt = torch.zeros(Q, dtype=torch.int32, device=dev) if n_gt is None else n_gt
    n_eq = torch.zeros(Q, dtype=torch.int32, device=dev) if n_eq is None else n_eq
    for name, v in (("t", t), ("n_gt", n_gt), ("n_eq", n_eq)):
        if v.numel() != Q or v.element_size() != 4 or not v.is_contiguous():
            raise _lib.GraphsageAmdError("nbr_rank: %s must be a dense 32-bit vector of %d entries" % (name, Q))
    grid = nbr_rank_grid(G, max_workgroups)
    stride = int(max_src_degree) if max_src_degree > NBR_CURSORS else 0
    if stride and ws is None:
        ws = torch.empty(nbr_rank_ws_bytes(grid, stride) // 4, dtype=torch.int32, device=dev)
    d = _lib.NbrRankDesc()
    d.rowptr, d.col, d.q, d.deg, d.f_rowptr, d.f_col = ptr(rowptr), ptr(col), ptr(q), ptr(deg), ptr(f_rowptr), ptr(f_col)
    d.group_ptr, d.group_src, d.dst, d.t, d.n_gt, d.n_eq, d.ws = (ptr(group_ptr), ptr(group_src), ptr(dst), ptr(t), ptr(n_gt),
                                                                   ptr(n_eq), ptr(ws) if stride else None)
    d.n_nodes, d.n_groups, d.n_queries, d.ws_stride = n_nodes, G, Q, stride
    d.ws_bytes = 4 * ws.numel() if (stride and ws is not None) else 0
    d.kind, d.tile, d.max_workgroups, d.reserved_ = NBR_KINDS[kind], tile, max_workgroups, 0
    call("gs_nbr_rank", ctypes.addressof(d), _s(stream))
    return t, n_gt, n_eq


# ------------------------------------------------------------------------------------------ graphs / events
class Stream(object):
    """A non-blocking HIP stream created by the library (capturable into a hipGraph)."""

    def __init__(self):
        import ctypes
        h = ctypes.c_void_p()
        call("gs_stream_create", ctypes.byref(h))
        self.handle = h.value

    def sync(self):
        call("gs_stream_sync", self.handle)

    def __del__(self):
        try:
            _lib.load().gs_stream_destroy(self.handle)
        except Exception:
            pass


class Graph(object):
    """hipGraph captured from the kernel chain enqueued between begin() and end()."""

    def __init__(self, stream):
        self.stream = stream
        self.exec_ = None

    def begin(self):
        call("gs_capture_begin", self.stream)

    def end(self):
        import ctypes
        h = ctypes.c_void_p()
        call("gs_capture_end", self.stream, ctypes.byref(h))
        self.exec_ = h.value

    def launch(self):
        call("gs_graph_launch", self.exec_, self.stream)

    def __del__(self):
        try:
            if self.exec_:
                _lib.load().gs_graph_destroy(self.exec_)
        except Exception:
            pass


class Event(object):
    def __init__(self):
        import ctypes
        h = ctypes.c_void_p()
        call("gs_event_create", ctypes.byref(h))
        self.handle = h.value

    def record(self, stream):
        call("gs_event_record", self.handle, stream)

    def wait(self, stream):
        """Make `stream` wait for this event (fork/join; a graph edge while capturing)."""
        call("gs_stream_wait_event", stream, self.handle)

    def elapsed_ms(self, stop):
        import ctypes
        ms = ctypes.c_float()
        call("gs_event_elapsed_ms", self.handle, stop.handle, ctypes.byref(ms))
        return ms.value

    def __del__(self):
        try:
            _lib.load().gs_event_destroy(self.handle)
        except Exception:
            pass


def build_csr_host(src, dst, n_nodes, symmetrize=True, keep_mask=None):
    """Host-side C++ CSR builder (gs_build_csr_host).  numpy in, numpy out."""
    import ctypes
    import numpy as np
    src = np.ascontiguousarray(src, dtype=np.int32)
    dst = np.ascontiguousarray(dst, dtype=np.int32)
    if keep_mask is not None:
        keep_mask = np.ascontiguousarray(keep_mask, dtype=np.uint8)
    cap = int(src.size) * (2 if symmetrize else 1)
    rowptr = np.zeros((n_nodes + 1,), dtype=np.int64)
    col = np.zeros((max(cap, 1),), dtype=np.int32)
    nnz = ctypes.c_int64()
    call("gs_build_csr_host", _lib.host_ptr(src), _lib.host_ptr(dst), _lib.host_ptr(keep_mask), src.size, n_nodes,
         1 if symmetrize else 0, _lib.host_ptr(rowptr), _lib.host_ptr(col), cap, ctypes.byref(nnz))
    return rowptr, col[: nnz.value].copy()
