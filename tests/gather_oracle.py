"""NumPy references for the gather + segmented mean (gather_mean_wave, csrc/gs_gather_dev.h: the stand-alone launches of
gs_gather.hip and the rider workgroups of every other launch) and for gs_segment_max_gather_fwd.  No GPU, no torch.

Three references, from loose to exact:
  * gemm_oracle.gather_mean (reused unchanged): the float64 mean and its derived bound (cnt + 3) u mag / cnt + u |want|;
  * gather_mean_dropout: the same with the keep mask of oracle/sampler_hash.dropout_mask.  A kept element is x * fp32(1 / keep)
    rounded to fp32 BEFORE it enters the sum: one rounding more per element, so the bound is (cnt + 4) u mag / cnt + u |want|
    with mag the sum of |x * scale| over the kept elements (the scale itself is the kernel's fp32 value, taken exactly);
  * ordered_f32: the fp32 restatement -- acc = +0; acc += X[idx[j]] for j = 0..s-1; acc += self; acc *= fp32(1) / fp32(cnt) --
    which every launch without dropout must match BIT FOR BIT, whatever its number of loads in flight U and whichever launch
    hosts it.  (The masked remainder acc += v * m with m in {0, 1} is exact, also contracted to an fma; acc starts at +0 and a
    round-to-nearest sum never turns +0 into -0, so adding v * 0 = +-0 changes nothing.)  Dropout is NOT bit-pinned: x * scale + acc
    may contract to an fma in one batch form and not in the other, so dropout is held to the bound only.
emulate_wave / emulate_launch restate the kernel and its rider dispatch as written (work item -> (row, chunk), id blocks of
64, full batches of U, the clamped and masked remainder, gs_mask_tail, the wave_start search) on padded buffers, with planted
faults by name; read_block holds the buffer checks that the GPU tests apply, so tests/test_gather_oracle.py can show on the CPU
that every fault fails one of them."""
import numpy as np

import gemm_oracle as go
from oracle import sampler_hash

U = go.U
SENTINEL, ISENTINEL = go.SENTINEL, go.ISENTINEL
NAN = np.float32("nan")

S_SWEEP = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 25, 63, 64, 65, 72, 77, 128, 130]
D_SWEEP = [1, 3, 4, 5, 255, 256, 257, 260, 602, 1024, 1028]
N_SWEEP = [1, 5]
US = [1, 4, 8, 13, 25]
DROP_S = [1, 3, 7, 8, 9, 25, 65, 77]
DROP_D = [5, 257, 602]
DROP_RATES = [0.4, 0.93]
SEGMAX_S = [1, 4, 5, 6, 12, 13, 14, 26, 27, 64, 65, 77]
SEGMAX_HIDDEN = [1, 3, 5, 255, 257, 512]
N_TABLE = 200

# (n, s, d, self term: None | "idx" | "pos", indexed?)  -- the rider lists.  Chunks per row: ceil(ceil(d / 4) / 64).
JOBS_SIX = [(5, 1, 7, None, True), (3, 7, 260, None, True), (2, 13, 602, "idx", True), (3, 25, 50, None, False),
            (1, 77, 1028, None, True), (4, 26, 4, "pos", True)]
JOBS_MULT8 = [(4, 9, 257, None, True), (2, 25, 5, "pos", False), (2, 70, 513, "idx", True)]
JOBS_ONE = [(3, 25, 602, None, True)]
JOB_LISTS = {"six": JOBS_SIX, "mult8": JOBS_MULT8, "one": JOBS_ONE}


def rup4(d):
    return (d + 3) // 4 * 4


def chunks(d):
    return ((d + 3) // 4 + 63) // 64


def wave_starts(specs):
    """Prefix sums of work items (waves) per job, as build_cojobs_s forms them."""
    ws = [0]
    for spec in specs:
        ws.append(ws[-1] + spec[0] * chunks(spec[2]))
    return ws


def rider_u(u, ubig, s):
    """run_gather_item<U, UBIG>'s dispatch."""
    if ubig != u and s >= ubig:
        return ubig
    return u if s >= 8 else 1


def standalone_u(s):
    """launch_gather_mean's dispatch (no dropout)."""
    return 8 if s >= 8 else (4 if s >= 4 else 1)


# ------------------------------------------------------------------------------------------------ operands
def table(rng, n_idx, d, n_table=N_TABLE, pad=8):
    """(buf [n_table, rup4(d) + pad] with NaN in every pad column and in every row that no index points at, idx [n_idx] int32
    with repeats, the clean [n_table, d] rows).  A quarter of the rows is never pointed at, whatever n_idx is."""
    clean = go.asym(rng, (n_table, d))
    live = rng.permutation(n_table)[:max(1, 3 * n_table // 4)]
    idx = live[rng.integers(0, len(live), size=n_idx)].astype(np.int32)
    if n_idx >= 3:
        idx[-1] = idx[1]
    buf = np.full((n_table, rup4(d) + pad), NAN, np.float32)
    hit = np.zeros(n_table, bool)
    hit[idx] = True
    buf[hit, :d] = clean[hit]
    return buf, idx, clean


def dense(rows, d, pad=8):
    """[rows, d] -> buffer with NaN pad columns."""
    rows = np.asarray(rows, np.float32)
    buf = np.full((rows.shape[0], rup4(d) + pad), NAN, np.float32)
    buf[:, :d] = rows
    return buf


def out_buffer(n, d, pad=8, sentinel=SENTINEL, dtype=np.float32):
    """[n + 4, rup4(d) + pad] full of the sentinel; the output view is rows [2, 2 + n)."""
    return np.full((n + 4, rup4(d) + pad), sentinel, dtype)


def read_block(big, n, d, tag, d4=None, sentinel=SENTINEL):
    """The logical [n, d] block of an out_buffer after the launch: rows outside the view and columns >= round_up(d, 4) still hold
    the sentinel, columns [d, round_up(d, 4)) are exact zeros."""
    d4 = rup4(d) if d4 is None else d4
    assert np.all(big[:2] == sentinel) and np.all(big[2 + n:] == sentinel), "%s: rows outside the view were written" % (tag,)
    assert np.all(big[:, d4:] == sentinel), "%s: columns beyond round_up(d, 4) were written" % (tag,)
    assert np.all(big[2:2 + n, d:d4] == 0), "%s: the pad columns of the last float4 must be exact zeros" % (tag,)
    return big[2:2 + n, :d]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, tag):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (tag, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, "%s: %d of %d elements differ in their bits, first at %s (got %r, want %r)" % (
        tag, len(bad), g.size, tuple(bad[0]), float(np.asarray(got)[tuple(bad[0])]), float(np.asarray(want)[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------ references
def group_ids(idx, n, s):
    return np.arange(n * s) if idx is None else np.asarray(idx)[:n * s]


def ordered_f32(X, idx, n, s, self_rows=None):
    """The kernel in fp32, order j = 0..s-1 (see the module docstring).  X: logical [rows, d]; idx None = contiguous groups;
    self_rows: the [n, d] self rows already picked (S[self_idx] or S[:n])."""
    g = np.asarray(X, np.float32)[group_ids(idx, n, s)].reshape(n, s, -1)
    acc = np.zeros((n, g.shape[2]), np.float32)
    for j in range(s):
        acc = acc + g[:, j]
    cnt = s
    if self_rows is not None:
        acc = acc + np.asarray(self_rows, np.float32)
        cnt = s + 1
    return acc * (np.float32(1) / np.float32(cnt))


def gather_mean(X, idx, n, s, self_rows=None):
    """gemm_oracle.gather_mean with idx None = contiguous groups."""
    return go.gather_mean(X, group_ids(idx, n, s), n, s, self_rows)


def drop_scale(rate):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def gather_mean_dropout(X, idx, n, s, mask, self_rows=None):
    """gs_gather_mean_dropout_fwd: (want [n, d], bound).  mask [n * s, d]: sampler_hash.dropout_mask's {0, fp32(1 / keep)} for the
    call's rows row0 .. row0 + n s - 1.  The float64 reference multiplies by that fp32 scale exactly; the kernel rounds each
    product x * scale to fp32 before summing, one rounding more than gemm_oracle.gather_mean counts: (cnt + 4) u mag / cnt + u |want|
    with mag = sum |x * scale| over the kept elements (+ |self|: the self row is not dropped)."""
    g = (go.f64(X)[group_ids(idx, n, s)] * go.f64(mask)).reshape(n, s, -1)
    tot, mag, cnt = g.sum(axis=1), np.abs(g).sum(axis=1), s
    if self_rows is not None:
        tot, mag, cnt = tot + go.f64(self_rows), mag + np.abs(go.f64(self_rows)), s + 1
    want = tot / cnt
    return want, (cnt + 4.0) * U * mag / cnt + U * np.abs(want)


def dropout_mask(seed, clock, site, row0, n_rows, d, rate):
    return sampler_hash.dropout_mask(seed, clock, site, row0, n_rows, d, rate)


def segment_max_gather(H, inv, n, s, last_tie=False):
    """gs_segment_max_gather_fwd: pooled = the exact fp32 maximum over rows H[inv[i s + j]], argmax = the FIRST j that attains it
    (the kernel starts at -inf and replaces on strict >).  last_tie: the planted fault (>=)."""
    g = np.asarray(H, np.float32)[np.asarray(inv)[:n * s]].reshape(n, s, -1)
    pooled = g.max(axis=1)
    if last_tie:
        arg = s - 1 - g[:, ::-1].argmax(axis=1)
    else:
        arg = g.argmax(axis=1)
    return pooled, arg.astype(np.int32)


def segmax_inputs(rng, n, s, hidden, n_table=N_TABLE):
    """(H buffer [n_table, rup4(hidden) + 8] of relu outputs with NaN pads and NaN dead rows, inv [n * s], clean H).  Planted:
    whole zero columns (every third), half-integer values (ties), the group maximum repeated at the first and at the last j, and
    for s > 64 a group whose maximum (repeated, too) sits in the second id block."""
    clean = np.maximum(np.round(go.asym(rng, (n_table, hidden)) * 2) / 2, 0).astype(np.float32)
    clean[:, ::3] = 0
    live = rng.permutation(n_table)[:3 * n_table // 4]
    top, top2 = live[0], live[1]
    clean[top] = np.where(np.arange(hidden) % 3 == 0, 0, 9.5)          # beats every half-integer normal
    clean[top2] = np.where(np.arange(hidden) % 3 == 0, 0, 9.5)         # a different row with the same values
    rest = live[2:]
    inv = rest[rng.integers(0, len(rest), size=n * s)].astype(np.int32).reshape(n, s)
    inv[0, 0], inv[0, s - 1] = top, top2                               # the maximum at the first and at the last j
    if n > 1 and s > 64:
        inv[1, 64], inv[1, s - 1] = top, top2                          # ... in the second id block
    if n > 2 and s > 2:
        inv[2, 1], inv[2, 2] = top2, top                               # ... in the middle
    inv = inv.reshape(-1)
    buf = np.full((n_table, rup4(hidden) + 8), NAN, np.float32)
    hit = np.zeros(n_table, bool)
    hit[inv] = True
    buf[hit, :hidden] = clean[hit]
    return buf, inv, clean


# ------------------------------------------------------------------------------------------------ the kernel, restated
def emulate_wave(u, Xbuf, idx, s, d, w, out, Sbuf=None, sidx=None, scale=None, fault=None):
    """gather_mean_wave<U> for work item w, all 64 lanes at once: writes out[row, cols] (out: the [n, ldo] VIEW).  Buffers are the
    padded ones (ld >= rup4(d)); the lanes' float4 cover columns [c * 256, min((c + 1) * 256, rup4(d))).
    fault: None | "remainder_unmasked" | "block_reuse" | "pad_not_zeroed" | "self_by_position"."""
    ch = chunks(d)
    row, c = divmod(w, ch)
    cols = np.arange(c * 256, min((c + 1) * 256, rup4(d)))              # the active lanes' columns
    acc = np.zeros(len(cols), np.float32)
    for jb in range(0, s, 64):
        cnt = min(64, s - jb)
        base = row * s + (0 if fault == "block_reuse" else jb)
        my = [(int(idx[base + lane]) if idx is not None else base + lane) for lane in range(cnt)]
        if len(cols) == 0:
            continue
        j = 0
        while j + u <= cnt:
            v = [Xbuf[my[j + k], cols] for k in range(u)]
            for k in range(u):
                acc = acc + v[k]
            j += u
        if j < cnt:
            v = [Xbuf[my[min(j + k, cnt - 1)], cols] for k in range(u)]
            for k in range(u):
                m = np.float32(1) if (j + k < cnt or fault == "remainder_unmasked") else np.float32(0)
                acc = acc + v[k] * m
    if len(cols) == 0:
        return
    if Sbuf is not None:
        sr = int(sidx[row]) if (sidx is not None and fault != "self_by_position") else row
        acc = acc + Sbuf[sr, cols]
    acc = acc * np.float32(scale)
    if fault != "pad_not_zeroed":
        acc = np.where(cols >= d, np.float32(0), acc)
    out[row, cols] = acc


class Job(object):
    """One gather+mean job on the host: padded operands, a sentinel-filled output buffer, the references."""

    def __init__(self, rng, n, s, d, self_kind=None, indexed=True, n_table=N_TABLE):
        self.n, self.s, self.d, self.self_kind, self.indexed = n, s, d, self_kind, indexed
        if indexed:
            self.Xbuf, self.idx, clean = table(rng, n * s, d, n_table)
        else:
            clean = go.asym(rng, (n * s, d))
            self.Xbuf, self.idx = dense(clean, d), None
            self.Xbuf = np.concatenate([self.Xbuf, np.full((3, self.Xbuf.shape[1]), NAN, np.float32)])   # rows behind the groups
        self.Sbuf = self.sidx = self_rows = None
        if self_kind == "idx":
            self.Sbuf, self.sidx, sclean = table(rng, n, d, 40)
            self_rows = sclean[self.sidx]
        elif self_kind == "pos":
            self_rows = go.asym(rng, (n, d))
            self.Sbuf = np.concatenate([dense(self_rows, d), np.full((2, rup4(d) + 8), NAN, np.float32)])
        self.clean, self.self_rows = clean, self_rows
        self.want32 = ordered_f32(clean, self.idx, n, s, self_rows)
        self.want64, self.bound = gather_mean(clean, self.idx, n, s, self_rows)
        self.scale = np.float32(1) / np.float32(s + 1 if self_kind else s)
        self.tag = "job n=%d s=%d d=%d self=%s indexed=%d" % (n, s, d, self_kind, indexed)
        self.big = out_buffer(n, d)

    def items(self):
        return self.n * chunks(self.d)

    def run_item(self, u, w, fault=None, scale=None):
        emulate_wave(u, self.Xbuf, self.idx, self.s, self.d, w, self.big[2:2 + self.n], self.Sbuf, self.sidx,
                     self.scale if scale is None else scale, fault)

    def check(self, tag=""):
        """What the GPU tests apply to a job's output buffer; returns err / bound."""
        got = read_block(self.big, self.n, self.d, tag + self.tag)
        assert_bits(got, self.want32, tag + self.tag)
        return go.assert_within(got, self.want64, self.bound, tag + self.tag)


def emulate_launch(jobs, u, ubig, waves_per_wg, fault=None):
    """The rider workgroups of a host: ceil(waves / waves_per_wg) workgroups, run_gather_item<U, UBIG> per wave.
    fault: those of emulate_wave, or "drop_last_item" (the grid one workgroup short / the last wave returning early),
    "boundary" (the wave_start search comparing with > where >= belongs: the first item of every later job goes to the job in front
    of it, which has no such item), "scale_s" (1 / s where a self term makes it 1 / (s + 1))."""
    ws = [0]
    for j in jobs:
        ws.append(ws[-1] + j.items())
    total = ws[-1]
    n_wg = -(-total // waves_per_wg)
    dead = n_wg * waves_per_wg - total
    for w in range(n_wg * waves_per_wg):
        if w >= total:
            continue
        if fault == "drop_last_item" and w == total - 1:
            continue
        k = 0
        while k + 1 < len(jobs) and (w > ws[k + 1] if fault == "boundary" else w >= ws[k + 1]):
            k += 1
        job = jobs[k]
        local = w - ws[k]
        if local >= job.items():
            continue                                   # ("boundary": row n of the job in front -- out of its view, nothing kept)
        scale = (np.float32(1) / np.float32(job.s)) if fault == "scale_s" else None
        job.run_item(rider_u(u, ubig, job.s), local, fault if fault not in ("drop_last_item", "boundary", "scale_s") else None, scale)
    return total, dead
