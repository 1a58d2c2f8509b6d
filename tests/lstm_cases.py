"""The cases of tests/test_lstm_edges_gpu.py (the recurrence kernels of csrc/gs_lstm.hip at their tile, length and layout edges),
shared with tests/test_seq_oracle.py, which checks on the CPU that the builder makes the lengths it claims and that the inputs are
well conditioned.

A case is a list of segments (n sequences, T steps).  Every segment gets as many of the PLANTED sequences as its n (and T) allow,
in this order, the rest run all T steps:
  0  all-zero rows                                            L = 1   (a degree-0 node)
  1  an interior zero row (t = 1)                  T >= 3:    L = T - 1
  2  a trailing zero row                           T >= 2:    L = T - 1
  3  a leading zero row                            T >= 2:    L = T - 1, step 0 runs on a zero input
  4  only the last row non-zero                               L = 1, the one step that runs is on a zero input
  5  row 0 normal, row 1 zero but for one fp32 subnormal (1e-40) in column d - 1, the rest zero   T >= 2:  L = 2
  6  every entry -0.0                                         L = 1   (-0.0 counts as zero)
A planted sequence whose T is too small is left as it is (L = T).  `short` names tiles (segment, tile of 16 sequences) all of whose
sequences stop early: L = 1 + r % (T - 2) < T - 1.

Gate pre-activations G = x . W_x + b (summed in float64, rounded to fp32 once) with weights uniform in +-0.15: at that scale the
25-step recurrence amplifies fp32 rounding to 1e-7 .. 2e-6 of the largest element (test_seq_oracle.py holds it below 1e-5)."""
import functools
import zlib

import numpy as np

import seq_oracle as so

D = 12                                  # input width of the recurrence cases (the recurrence itself only sees G)
TILE = 16                               # LSTM_TILE of csrc/gs_lstm.hip
SCALE = 0.15
SUBNORMAL = np.float32(1e-40)
N_PLANTED = 7
OUTPUTS = ("A", "C", "Hp", "hl", "dG")

# (segments, short tiles)
CASES = [
    ([(1, 1)], ()), ([(3, 2)], ()), ([(15, 25)], ()), ([(16, 3)], ()), ([(17, 5)], ()), ([(33, 7)], ()),
    ([(0, 4), (5, 3)], ()), ([(5, 3), (0, 4), (18, 2)], ()), ([(4, 6), (0, 1)], ()),      # an empty segment first, in the middle, last
    ([(4, 1), (5, 25), (16, 2), (3, 9)], ()),                                            # GS_LSTM_MAX_SEG segments
    ([(0, 3)], ()),                                                                      # nothing to do
    ([(33, 7)], ((0, 1),)),                                                              # second tile: tmax < T
]
CASES_256 = [0, 2, 4, 9, 11]            # H = 256: n = 1, n = 15 at T = 25, n = 17, four segments, the short tile
WIDTHS = [1, 63, 64, 65, 130, 602]      # gs_lstm_lengths: one lane, one wave of columns less one / exactly / plus one, three trips, Reddit


def case_id(i):
    segs, short = CASES[i]
    return "+".join("%dx%d" % s for s in segs) + ("-short" if short else "")


def segment_inputs(rng, n, T, d, last_col_only=False, short_tiles=()):
    """-> (x [n, T, d] fp32, the lengths L [n] it is built to have)."""
    x = rng.standard_normal((n, T, d)).astype(np.float32)
    assert (x != 0).all()
    L = np.full(n, T, np.int64)
    if last_col_only:                   # the only non-zero of every non-zero planted row lies in the last column
        x[:N_PLANTED, :, :d - 1] = 0.0
    if n > 0:
        x[0], L[0] = 0.0, 1
    if n > 1 and T >= 3:
        x[1, 1], L[1] = 0.0, T - 1
    if n > 2 and T >= 2:
        x[2, T - 1], L[2] = 0.0, T - 1
    if n > 3 and T >= 2:
        x[3, 0], L[3] = 0.0, T - 1
    if n > 4:
        x[4, :T - 1], L[4] = 0.0, 1
    if n > 5 and T >= 2:
        x[5, 1:] = 0.0
        x[5, 1, d - 1], L[5] = SUBNORMAL, 2
    if n > 6:
        x[6], L[6] = -0.0, 1
    for tile in short_tiles:
        assert tile >= 1 and T >= 3 and tile * TILE < n             # (tile 0 holds the planted sequences)
        for r in range(tile * TILE, min(n, (tile + 1) * TILE)):
            L[r] = 1 + r % (T - 2)
            x[r, L[r]:] = 0.0
    return x, L


def inputs(segs, d, last_col_only=False, short=(), seed=0):
    """Per segment: x and the claimed lengths."""
    rng = np.random.RandomState(zlib.crc32(repr((segs, d, last_col_only, short, seed)).encode()) & 0x7fffffff)
    out = [segment_inputs(rng, n, T, d, last_col_only, [t for k2, t in short if k2 == k]) for k, (n, T) in enumerate(segs)]
    return [x for x, _ in out], [L for _, L in out]


class Layout(object):
    """Where the step rows lie: segment k's sequence r, step t is row row0[k] + r*T + t, `gap` rows nobody owns before every segment
    and one behind the last; sequence rows (lengths, h_last, dh_last) are seq0[k] + r, one row nobody owns behind the last."""

    def __init__(self, segs, gap=0):
        self.segs, self.row0, self.seq0 = list(segs), [], []
        r = s = 0
        for n, T in segs:
            r += gap
            self.row0.append(r)
            self.seq0.append(s)
            r += n * T
            s += n
        self.rows, self.n_total = r + 1, s

    def scatter(self, parts, out):
        """Per-segment [n, T, w] -> the rows of out [rows, >= w] (the other elements keep what they hold)."""
        for (n, T), r0, p in zip(self.segs, self.row0, parts):
            out[r0:r0 + n * T, :p.shape[2]] = p.reshape(n * T, p.shape[2])
        return out

    def gather(self, arr, w):
        return [arr[r0:r0 + n * T, :w].copy().reshape(n, T, w) for (n, T), r0 in zip(self.segs, self.row0)]

    def step_mask(self, per_seg_nt, w, ld):
        """[rows, ld] bool: columns < w of the step rows where per_seg_nt[k] [n, T] holds."""
        m = np.zeros((self.rows, ld), bool)
        for (n, T), r0, p in zip(self.segs, self.row0, per_seg_nt):
            m[r0:r0 + n * T, :w] = np.asarray(p, bool).reshape(n * T, 1)
        return m


class Case(object):
    """Inputs of one recurrence case in fp32 (per segment: x, L, G, dh; W_h for all) and its oracle in either precision."""

    def __init__(self, segs, H, short=(), saturate=False):
        self.segs, self.H = list(segs), H
        self.xs, self.L = inputs(segs, D, short=short, seed=H)
        rng = np.random.RandomState(zlib.crc32(repr((segs, H, short)).encode()) & 0x7fffffff)
        kernel = rng.uniform(-SCALE, SCALE, (D + H, 4 * H)).astype(np.float32)
        bias = rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32)
        self.W_x, self.W_h, self.bias = kernel[:D], np.ascontiguousarray(kernel[D:]), bias
        self.G = [(x.astype(np.float64) @ kernel[:D].astype(np.float64) + bias).astype(np.float32) for x in self.xs]
        self.dh = [rng.standard_normal((n, H)).astype(np.float32) for n, _ in segs]
        if saturate:        # +-100 in eight units of each gate (gate g: units 8g .. 8g + 7), at every step
            for G in self.G:
                for g in range(4):
                    G[:, :, g * H + 8 * g:g * H + 8 * g + 8] = np.where(np.arange(8) % 2 == 0, 100.0, -100.0)

    @functools.lru_cache(maxsize=None)
    def oracle(self, dtype):
        """Per segment {A, C, Hp, hl, dG, ran} in `dtype`, from the fp32 inputs."""
        out = []
        W = self.W_h.astype(dtype)
        with np.errstate(over="ignore", under="ignore"):
            for G, L, dh in zip(self.G, self.L, self.dh):
                A, C, Hp, hl, ran = so.recurrence_fwd(G.astype(dtype), L, W)
                dG = so.recurrence_bwd(dh.astype(dtype), L, W, A, C)
                out.append({"A": A, "C": C, "Hp": Hp, "hl": hl, "dG": dG, "ran": ran})
        return out

    def e32(self):
        """{output: largest |fp32 oracle - fp64 oracle| over the case}."""
        o32, o64 = self.oracle(np.float32), self.oracle(np.float64)
        return {k: max([float(np.abs(a[k].astype(np.float64) - b[k]).max()) for a, b in zip(o32, o64) if a[k].size] or [0.0])
                for k in OUTPUTS}

    def largest(self):
        return {k: max([float(np.abs(b[k]).max()) for b in self.oracle(np.float64) if b[k].size] or [0.0]) for k in OUTPUTS}

    def tolerance(self):
        """The bound of the GPU test per output: max(8 e32, 8 * 2^-24 * max(1, max |want|))."""
        e, big = self.e32(), self.largest()
        return {k: max(8.0 * e[k], 8.0 * 2.0 ** -24 * max(1.0, big[k])) for k in OUTPUTS}

    def select(self, picks):
        """A case of the sequences picks = [(segment, indices)]: one segment per pick, the same weights (no oracle of its own)."""
        c = object.__new__(Case)
        c.H, c.W_x, c.W_h, c.bias = self.H, self.W_x, self.W_h, self.bias
        c.segs = [(len(idx), self.segs[k][1]) for k, idx in picks]
        for name in ("xs", "L", "G", "dh"):
            setattr(c, name, [getattr(self, name)[k][np.asarray(idx, np.int64)] for k, idx in picks])
        return c


@functools.lru_cache(maxsize=None)
def case(i, H):
    segs, short = CASES[i]
    return Case(segs, H, short)


@functools.lru_cache(maxsize=None)
def saturated_case():
    return Case([(5, 3)], 128, saturate=True)


def permutation(n):
    """A fixed shuffle of a segment's sequences (other tile slots, other neighbours); n = 2 swaps."""
    return np.random.RandomState(n).permutation(n) if n > 2 else np.arange(n)[::-1]


# ---------------------------------------------------------------------------------------------- gs_lstm_lengths through a row table
def id_table(xs, rng):
    """The step rows of all segments as ids into a larger table: the rows shuffled among five rows no id names, every all-zero step
    row drawn from ONE zero pad row (the last), and every other sequence of full length from index 8 on sharing its neighbour's
    rows.  -> (table [rows, d], per-segment ids [n*T] int32, per-segment x as gathered)."""
    d = xs[0].shape[2]
    flat = np.concatenate([x.reshape(-1, d) for x in xs])
    slot = rng.permutation(len(flat) + 5)[:len(flat)]
    table = rng.standard_normal((len(flat) + 6, d)).astype(np.float32)
    table[slot] = flat
    table[-1] = 0.0
    ids_all = slot.astype(np.int32)
    ids_all[~flat.any(axis=1) & ~np.signbit(flat).any(axis=1)] = len(table) - 1          # (the -0.0 rows stay rows of their own)
    ids, r = [], 0
    for x in xs:
        n, T = x.shape[:2]
        i = ids_all[r:r + n * T].reshape(n, T).copy()
        for q in range(9, n, 2):
            if x[q].any(axis=1).all() and x[q - 1].any(axis=1).all():
                i[q] = i[q - 1]
        ids.append(i.reshape(-1))
        r += n * T
    return table, ids, [table[i].reshape(x.shape) for i, x in zip(ids, xs)]
