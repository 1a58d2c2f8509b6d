"""NumPy float64 stage references, each with a DERIVED elementwise error bound, for the five fused tail kernels -- the supervised
tail of csrc/gs_tail.hip / gs_tail_dev.h (gs_sage_tail_fwd_bwd[_means], gs_sage_tail_z[_means], gs_sage_tail_dh0) and, in the second
half of this file, the link-prediction tail of csrc/gs_unsup_tail.hip (gs_linkpred_tail[_means], gs_linkpred_tail_neg) --, the cases
the GPU sweep runs and the buffers it runs them in.  No GPU, no torch.

CHAINED stages.  Every stage's reference is computed in float64 from the fp32 values the kernel itself STORED for the stage
before it, so that its bound is the bound of that one stage, derived from the operations as written:

    means <- h0            z <- h0, means_got        y <- z_got          logits <- y_got
    loss_rows, preds, dlogits <- logits_got          dz <- dlogits_got, y_got, z_got          d_h0 <- dz_got, h0

This is sound because the stored word and the word the next phase consumes are the same fp32 bits (read in sage_tail_kernel):
z is stored from the register that was loaded from the LDS word phase 2 normalises (`zv`), y from the value written back to
that LDS word (phase 3's A operand, phase 6's y), logits from x[m] (the value the loss phase works on), dlogits from `gv` (the
value written to DLs, phase 5's A operand), dz from g[m] (the value written to DZs, phase 7's A operand).  `means` is stored from
the float4 that goes to the contraction's LDS rows.  d_y (phase 5) is never stored: its error is carried into dz's bound.

Error model, as tests/gemm_oracle.py and tests/optim_oracle.py: u = 2^-24; a value computed with R roundings on its longest path
differs from the exact one by at most R u sum|terms| (first order; SLACK pays for the second).  Contractions take
gemm_oracle.product's (K + 8) u |A| |B| + u |want|: here a 16x16x4 MFMA chain per K-slice -- z: eight chains of D / 8 products
and seven additions of the partial tiles; logits: nks in {2, 4} chains of 2 O / nks products added to the bias in slice order;
d_y, d_self, d_means: one chain -- so every addend passes through at most K / 8 + 7 (z), K / nks + nks (logits) or K (the others)
roundings, all <= K + 8.  The hardware transcendentals v_exp_f32, v_log_f32, v_rcp_f32 and v_rsq_f32 are 1 ulp = 2 u each
(`ULP1`); they replace the library calls of gs_head.hip, so optim_oracle's factor LIB does not appear: every rounding is counted.
Results that may fall below 2^-126 get the absolute floor DENORM (subnormal spacing), and what passes through v_exp_f32 the floor
FLUSH = 2^-126 (the instruction flushes a subnormal result to zero).

No rtol / atol: the bounds below are the only tolerances of tests/test_tail_edges_gpu.py.  tests/test_tail_oracle.py shows on the
CPU that an fp32 emulation in the kernel's order lies inside each of them and that each planted fault is rejected."""
import numpy as np

import gemm_oracle as go
import gather_oracle as G
from optim_oracle import U, SLACK, DENORM

f64 = go.f64
NAN = np.float32("nan")
SENTINEL = G.SENTINEL
ULP1 = 2.0 * U                   # one ulp, relative: v_exp_f32 / v_log_f32 / v_rcp_f32 / v_rsq_f32
FLUSH = 2.0 ** -126
CLAMP = np.float64(np.float32(1e-12))      # the kernel's fmaxf(ss, 1e-12f)
TAIL_NB = 11

DO = [(128, 64), (128, 128), (256, 64), (256, 128)]
N_SWEEP = [1, 15, 16, 17, 33]
S_SWEEP = [1, 2, 10, 11]
C_SWEEP = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 96, 97, 121, 127, 128]
SWEEP_HEADS = [(41, False), (121, True)]   # (C, sigmoid) of the (D, O) x n x s sweep


def rup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ cases
class Case(object):
    """The logical operands of one launch.  h0 [n + n s, D] is relu output: positive normals, +0, -0 and a few positive
    subnormals; where n >= 2 root n - 1 has an all-zero self row and all-zero neighbor rows (z = 0: the clamp, y = 0,
    dz = g * 1e6); where n >= 3 root n - 2 is ~1e-9 throughout (0 < sum z^2 < 1e-12: the clamped branch with y != 0, which the
    unclamped formula gets wrong).  Labels: sigmoid multi-hot; softmax one-hot, and where n >= 3 row 0 all-zero and row 1 a
    non-normalised soft row.  wide: W_head at scale 16, |logit| reaches about 50.  gcn: ONE weight matrix W [D, 2 O],
    W_self = W[:, :O], W_neigh = W[:, O:]."""

    def __init__(self, D, O, n, s, C, sigmoid, seed=0, gcn=False, wide=False):
        self.D, self.O, self.n, self.s, self.C, self.sigmoid, self.gcn, self.wide = D, O, n, s, C, bool(sigmoid), bool(gcn), wide
        self.Z, self.rows = 2 * O, n + n * s
        rng = np.random.default_rng([seed, D, O, n, s, C, int(sigmoid)])
        h0 = np.maximum(go.asym(rng, (self.rows, D)), 0).astype(np.float32)
        zero = h0 == 0
        h0[zero & (rng.random(h0.shape) < 0.3)] = np.float32(-0.0)
        h0[zero & (rng.random(h0.shape) < 0.05)] = np.float32(1e-40)
        for root, scale in ((n - 1, 0.0), (n - 2, 1e-9))[:max(0, n - 1)]:
            rs = [root] + list(range(n + root * s, n + root * s + s))
            h0[rs] = (np.abs(h0[rs]) * scale).astype(np.float32)
        if n >= 2:
            h0[n - 1, ::3] = np.float32(-0.0)
        self.h0 = h0
        self.W = go.asym(rng, (D, 2 * O), 0.2)
        self.Ws, self.Wn = self.W[:, :O], self.W[:, O:]
        self.Wh = go.asym(rng, (self.Z, C), 16.0 if wide else 0.3)
        self.b = go.asym(rng, (C,), 0.1)
        if sigmoid:
            lab = (rng.random((n, C)) > 0.5).astype(np.float32)
        else:
            lab = np.eye(C, dtype=np.float32)[rng.integers(0, C, n)]
            if n >= 3:
                lab[0] = 0
                lab[1] = (rng.random(C) * 0.7 + 0.05).astype(np.float32)
        self.labels = lab

    def tag(self):
        return "D%d O%d n%d s%d C%d %s%s%s" % (self.D, self.O, self.n, self.s, self.C, "sigmoid" if self.sigmoid else "softmax",
                                                " gcn" if self.gcn else "", " wide" if self.wide else "")

    def mask(self):
        return self.h0 > 0

    # ---- buffers: inputs with ld = round_up(width, 4) + 8 and NaN everywhere outside the logical operand
    def in_h0(self):
        buf = np.full((self.rows + 4, self.D + 8), NAN, np.float32)        # four extra rows behind row n + n s
        buf[:self.rows, :self.D] = self.h0
        return buf

    def in_weights(self):
        """(W_self buffer, W_neigh buffer); gcn: (the [D, 2 O] buffer, None) -- W_neigh = W_self + O inside it."""
        if self.gcn:
            return G.dense(self.W, 2 * self.O), None
        return G.dense(self.Ws, self.O), G.dense(self.Wn, self.O)

    def in_head(self):
        """(W_head buffer: columns [C, ld) NaN, [C, round_up(C, 4)) among them; bias followed by NaN; labels buffer)."""
        return G.dense(self.Wh, self.C), np.concatenate([self.b, np.full(8, NAN, np.float32)]), G.dense(self.labels, self.C)

    def out_shapes(self):
        return {"means": (self.n, self.D), "z": (self.n, self.Z), "y": (self.n, self.Z), "logits": (self.n, self.C),
                "preds": (self.n, self.C), "dlogits": (self.n, self.C), "dz": (self.n, self.Z), "d_h0": (self.rows, self.D)}

    def out_buffers(self):
        """name -> sentinel-filled buffer, the view two rows down (gather_oracle.out_buffer); d_h0's logical block is NaN: every
        one of its n + n s rows must be written.  loss_rows: [4 + n + 4]."""
        bufs = {k: G.out_buffer(r, w) for k, (r, w) in self.out_shapes().items()}
        bufs["d_h0"][2:2 + self.rows, :self.D] = NAN
        bufs["loss_rows"] = np.full(self.n + 8, SENTINEL, np.float32)
        return bufs


def read_outputs(case, bufs, names):
    """The logical blocks of the named outputs after a launch, once gather_oracle.read_block has seen the frame intact: every word
    outside the view still the sentinel, columns [C, round_up(C, 4)) of logits / preds / dlogits exact zeros."""
    got = {}
    for k in names:
        if k == "loss_rows":
            big = bufs[k]
            assert np.all(big[:4] == SENTINEL) and np.all(big[4 + case.n:] == SENTINEL), "%s loss_rows: words outside the view were written" % case.tag()
            got[k] = big[4:4 + case.n]
        else:
            r, w = case.out_shapes()[k]
            got[k] = G.read_block(bufs[k], r, w, "%s %s" % (case.tag(), k))
        assert np.isfinite(got[k]).all(), "%s %s: non-finite output" % (case.tag(), k)
    return got


# ------------------------------------------------------------------------------------------------ stage references
def means(case):
    """gemm_oracle.gather_mean over the contiguous groups h0[n + i s + j] (+ the self row, / (s + 1): gcn); + DENORM: a mean of
    subnormals is rounded on the subnormal grid."""
    want, bound = go.gather_mean(case.h0, case.n + np.arange(case.n * case.s), case.n, case.s, case.h0[:case.n] if case.gcn else None)
    return want, bound * SLACK + DENORM


def z(case, means_got):
    """[h_self . W_self | means_got . W_neigh]; gcn: both halves contract means_got.  Each half is eight K-slices (one per wave) of
    D / 8 fmaf steps each, summed in wave order (seven additions): an addend passes through at most D / 8 + 7 roundings, which
    product()'s K + 8 covers with room; the final u |want| is the last addition's."""
    a_self = means_got if case.gcn else case.h0[:case.n]
    return go.product([(a_self, case.Ws), (means_got, case.Wn)], concat=True)


def l2norm(z_got):
    """(y, b_y, inv, e_inv (relative), clamped) from the stored z.  ss: per lane Z / 64 products and additions (2 Z / 64 roundings
    if the compiler does not fuse them, counted so), then tail_wave_sum: four DPP steps and two more additions on a path;
    max(ss, 1e-12f) is exact; v_rsq_f32 halves ss's relative error and adds its ulp; y = z * inv one more."""
    zz = f64(z_got)
    nj = zz.shape[1] // 64
    ss = (zz * zz).sum(axis=1)
    clamped = ss < CLAMP
    inv = 1.0 / np.sqrt(np.maximum(ss, CLAMP))
    e_inv = (0.5 * (2 * nj + 6) * U + ULP1) * SLACK
    y = zz * inv[:, None]
    return y, (e_inv + U) * np.abs(y) * SLACK + DENORM, inv, e_inv, clamped


def logits(case, y_got):
    """y_got . W_head + b: nks in {2, 4} partial chains of 2 O / nks steps, added to the bias in K-slice order."""
    return go.product([(y_got, case.Wh)], bias=case.b)


def wave_sum_r(C):
    """Roundings on the longest path of a per-lane sum over ceil(C / 64) class groups followed by tail_wave_sum."""
    return -(-C // 64) + 6


def class_loss(case, x_got):
    """loss_rows, preds, dlogits from the stored logits -> dict (values and b_* bounds).  optim_oracle.class_loss re-derived for
    phase 4 of sage_tail_kernel.

    __expf(a) = v_exp_f32(a * log2(e)): the product's rounding and the rounded constant move the exponent by 2 |a| u relative to
    the result; + ULP1; a result below 2^-126 is flushed (FLUSH).
    sigmoid, e = __expf(-|x|) (E_e = 2 |x| u + ULP1): term = max(x, 0) - x z + __logf(1 + e): x z rounded (labels need not be
    0 / 1), the subtraction, 1 + e (absolute u: log's slope there is <= 1), v_log_f32 and its product with ln 2 (ULP1 + 2 u on
    the value), the addition; e's error reaches the term scaled by e / (1 + e).  Sum: wave_sum_r(C) roundings on the terms'
    magnitudes; inv_c = 1 / C (correctly rounded division) and the product: 2.
    p = rcp(1 + e) (x >= 0) or e * rcp(1 + e): the addition, ULP1, the product (4 u), and E_e scaled by 1 - p.
    g = (p - z) * (inv_n * inv_c): p's error; the subtraction, two reciprocals, their product and the last product: 5 on |p - z|.
    softmax, m exact: e_c = __expf(x_c - m): the subtraction's rounding enters the exponent too: E_e = 3 |x_c - m| u + ULP1.
    se: wave_sum_r(C) more.  rse = v_rcp_f32(se): ULP1.  p = e * rse: E_p = E_e + E_se + ULP1 + u.
    zs = sum z, zx = sum z x (products rounded: + 1): wave_sum_r(C) on the magnitudes.
    loss = zs * (m + __logf(se)) - zx: log se is off by E_se (absolute) + (ULP1 + 2 u) |log se|, the addition u |lse|, the product
    u |zs lse| and zs's own error, the subtraction u (|zs lse| + |zx|).
    g = (p * zs - z) * inv_n: (E_p + E_zs + u) p zs, then the subtraction, the reciprocal and the product: 3 on |p zs - z|."""
    x, lab = f64(x_got), f64(case.labels)
    n, C = x.shape
    R = wave_sum_r(C)
    if case.sigmoid:
        ax = np.abs(x)
        e = np.exp(-ax)
        E_e = 2 * ax * U + ULP1
        sp = np.log1p(e)
        pos = np.maximum(x, 0)
        term = pos - x * lab + sp
        tmag = pos + np.abs(x * lab) + sp
        b_term = U * (np.abs(x * lab) + pos + np.abs(x * lab) + tmag) + U + (ULP1 + 2 * U) * sp + (e * E_e + FLUSH) / (1 + e)
        loss = term.mean(axis=1)
        b_loss = (b_term.mean(axis=1) + (R + 2) * U * tmag.mean(axis=1)) * SLACK + DENORM
        p = 1.0 / (1.0 + np.exp(-x))
        b_p = (p * (4 * U + (1 - p) * E_e) + FLUSH) * SLACK
        g = (p - lab) / (n * C)
        b_g = (b_p + 5 * U * np.abs(p - lab)) / (n * C) * SLACK + DENORM
    else:
        m = x.max(axis=1, keepdims=True)
        e = np.exp(x - m)
        se = e.sum(axis=1, keepdims=True)
        E_e = 3 * np.abs(x - m) * U + ULP1
        E_se = (e * E_e + FLUSH).sum(axis=1, keepdims=True) / se + R * U
        E_p = E_e + E_se + ULP1 + U
        p = e / se
        b_p = (p * E_p + FLUSH) * SLACK
        zs, zsm = lab.sum(axis=1, keepdims=True), np.abs(lab).sum(axis=1, keepdims=True)
        zx, zxm = (lab * x).sum(axis=1, keepdims=True), np.abs(lab * x).sum(axis=1, keepdims=True)
        E_zs = R * U
        lse = m + np.log(se)
        loss = (zs * lse - zx)[:, 0]
        b_loss = (zsm * (E_se + (ULP1 + 2 * U) * np.abs(np.log(se)) + U * np.abs(lse)) + (U + E_zs) * zsm * np.abs(lse)
                  + (R + 1) * U * zxm + U * (np.abs(zs * lse) + np.abs(zx)))[:, 0] * SLACK + DENORM
        g = (p * zs - lab) / n
        b_g = ((E_p + E_zs + U) * p * zsm + FLUSH * zsm + 3 * U * np.abs(p * zs - lab)) / n * SLACK + DENORM
    return {"loss_rows": loss, "b_loss_rows": b_loss, "preds": p, "b_preds": b_p, "dlogits": g, "b_dlogits": b_g}


def dz(case, dlogits_got, y_got, z_got):
    """l2norm_bwd of d_y = dlogits_got . W_head^T (one chain, K = round_up(C, 32): the operand is zero-padded), which is not
    stored: its bound travels."""
    dl, Wh = f64(dlogits_got), f64(case.Wh)
    g, b_g = go.product([(dl @ Wh.T, np.abs(dl) @ np.abs(Wh.T), rup(case.C, 32))])
    return l2norm_bwd(g, b_g, y_got, z_got)


def l2norm_bwd(g, b_g, y_got, z_got):
    """tail_l2norm_bwd_row on an upstream gradient g known to b_g, the stored y and the inv of the stored z.  g's bound travels
    through g itself and through dot = sum g y (one fma chain of Z / 64 + tail_wave_sum: Z / 64 + 6 roundings on sum |g y|).
    dz = inv * (g - y * dot): the product y dot, the subtraction and the product with inv (u each, on their operands), and inv's
    own relative error e_inv (l2norm) on |dz|.  Clamped rows (sum z^2 < 1e-12): dz = g * inv."""
    y = f64(y_got)
    _, _, inv, e_inv, clamped = l2norm(z_got)
    inv, cl = inv[:, None], clamped[:, None]
    nj = y.shape[1] // 64
    dot = (g * y).sum(axis=1, keepdims=True)
    b_dot = (np.abs(y) * b_g).sum(axis=1, keepdims=True) + (nj + 6) * U * np.abs(g * y).sum(axis=1, keepdims=True)
    want = np.where(cl, g * inv, inv * (g - y * dot))
    b_open = inv * (b_g + np.abs(y) * b_dot + U * np.abs(y * dot) + U * (np.abs(g) + np.abs(y * dot)))
    bound = np.where(cl, inv * b_g, b_open) + (e_inv + U) * np.abs(want)
    return want, bound * SLACK + DENORM


def d_h0(case, dz_got):
    """relu'(h0) * (d_self on the self rows, d_means * fp32(1 / s) on each neighbor row), d_self = dz[:, :O] . W_self^T and
    d_means = dz[:, O:] . W_neigh^T one chain of K = O each; the reciprocal and the product add 2 u.  gcn: every row gets
    (d_self + d_means) * fp32(1 / (s + 1)): one addition more.  The mask is a select on h0 > 0: masked elements are exact +0
    (-> mask, checked apart from the bound)."""
    n, s, O = case.n, case.s, case.O
    d = f64(dz_got)
    ds, b_ds = go.product([(d[:, :O], case.Ws.T)])
    dm, b_dm = go.product([(d[:, O:], case.Wn.T)])
    if case.gcn:
        tot = (ds + dm) / (s + 1)
        b = (b_ds + b_dm + U * np.abs(ds + dm)) / (s + 1) + 2 * U * np.abs(tot)
        self_w, self_b, nb_w, nb_b = tot, b, tot, b
    else:
        self_w, self_b, nb_w, nb_b = ds, b_ds, dm / s, b_dm / s + 2 * U * np.abs(dm / s)
    want = np.concatenate([self_w, np.repeat(nb_w, s, axis=0)])
    bound = np.concatenate([self_b, np.repeat(nb_b, s, axis=0)])
    m = case.mask()
    return np.where(m, want, 0.0), np.where(m, bound * SLACK + DENORM, 0.0)


# ------------------------------------------------------------------------------------------------ the checks
FWD = ("means", "z", "y", "logits", "loss_rows", "preds", "dlogits")
BWD = ("dz", "d_h0")


def check_stages(case, got, stages, means_in=None, note=None):
    """Every named stage of `got` (logical blocks, fp32) inside its bound, chained as in the module docstring.  means_in: the
    `means` the launch was GIVEN (means_ready) -- z is then derived from it.  Returns {stage: worst err / bound}."""
    out = {}

    def hold(k, want, bound):
        out[k] = go.assert_within(got[k], want, bound, "%s %s" % (case.tag(), k))
        if note is not None:
            note(k, out[k])

    if "means" in stages:
        hold("means", *means(case))
    if "z" in stages:
        hold("z", *z(case, means_in if means_in is not None else got["means"]))
    if "y" in stages:
        y, b_y = l2norm(got["z"])[:2]
        hold("y", y, b_y)
    if "logits" in stages:
        hold("logits", *logits(case, got["y"]))
    if "loss_rows" in stages:
        ref = class_loss(case, got["logits"])
        for k in ("loss_rows", "preds", "dlogits"):
            if k in stages:
                hold(k, ref[k], ref["b_" + k])
    if "dz" in stages:
        hold("dz", *dz(case, got["dlogits"], got["y"], got["z"]))
    if "d_h0" in stages:
        want, bound = d_h0(case, got["dz"])
        hold("d_h0", want, bound)
        masked = ~case.mask()
        assert np.all(G.bits(got["d_h0"])[masked] == 0), "%s d_h0: an element with h0 <= 0 is not an exact +0" % case.tag()
    return out


# ================================================================================================ the link-prediction tail
# gs_linkpred_tail[_means] + gs_linkpred_tail_neg (csrc/gs_unsup_tail.hip).  Rows: [batch1 (B) | batch2 (B) | negatives (n_neg)].
# Chain:  means <- h0     z <- h0, means_got     y <- z_got     aff_all <- y_got     loss_rows, rr_rows <- aff_all_got
#         dz[pairs], neg_slabs <- y_got, aff_all_got, z_got       dz[negatives] <- neg_slabs_got, z_got       d_h0 <- dz_got
#         loss_out <- loss_rows_got      mrr_out <- rr_rows_got
# Stored = consumed (read in sage_lp_tail_kernel): y from the LDS word the pair phase reads (the negatives' y by group 0 only, every
# main computes the same bits); aff / nav are stored from the registers the loss, the rank and the gradients use; dz from the value
# written to DZs; the slabs are launch 2's input.
B_SWEEP = [1, 7, 8, 9, 17]
NEG_SWEEP = [1, 3, 4, 5, 15, 16, 17, 32]


class LpCase(Case):
    """The logical operands of one link-prediction step.  h0 as Case's; where n_neg >= 3 the LAST negative is an all-zero root
    (z = 0: launch 2's clamp) and the one before it ~1e-9 throughout (clamped with y != 0)."""

    def __init__(self, D, O, B, n_neg, s, seed=0, neg_weight=0.7):
        self.D, self.O, self.B, self.n_neg, self.s, self.gcn = D, O, B, n_neg, s, False
        n = self.n = 2 * B + n_neg
        self.Z, self.rows = 2 * O, n + n * s
        self.neg_weight, self.scale = np.float32(neg_weight), np.float32(1.0 / B)
        rng = np.random.default_rng([seed, D, O, B, n_neg, s])
        h0 = np.maximum(go.asym(rng, (self.rows, D)), 0).astype(np.float32)
        zero = h0 == 0
        h0[zero & (rng.random(h0.shape) < 0.3)] = np.float32(-0.0)
        h0[zero & (rng.random(h0.shape) < 0.05)] = np.float32(1e-40)
        if n_neg >= 3:
            for root, scale in ((n - 1, 0.0), (n - 2, 1e-9)):
                rs = [root] + list(range(n + root * s, n + root * s + s))
                h0[rs] = (np.abs(h0[rs]) * scale).astype(np.float32)
        self.h0 = h0
        self.W = go.asym(rng, (D, 2 * O), 0.2)
        self.Ws, self.Wn = self.W[:, :O], self.W[:, O:]
        self.GP = (B + 7) // 8

    def tag(self):
        return "lp D%d O%d B%d neg%d s%d" % (self.D, self.O, self.B, self.n_neg, self.s)

    def out_shapes(self):
        return {"means": (self.n, self.D), "z": (self.n, self.Z), "y": (self.n, self.Z), "dz": (self.n, self.Z),
                "d_h0": (self.rows, self.D), "aff_all": (self.B, self.n_neg + 1)}

    def vec_shapes(self):
        return {"loss_rows": self.B, "rr_rows": self.B, "neg_slabs": self.GP * self.n_neg * self.Z, "loss_out": 1, "mrr_out": 1}

    def out_buffers(self):
        """As Case.out_buffers; aff_all's spare columns start at n_neg + 1 (no pad-zero promise); the vectors sit 4 words into
        [4 + len + 4] buffers."""
        bufs = {k: G.out_buffer(r, w) for k, (r, w) in self.out_shapes().items()}
        bufs["d_h0"][2:2 + self.rows, :self.D] = NAN
        for k, ln in self.vec_shapes().items():
            bufs[k] = np.full(ln + 8, SENTINEL, np.float32)
        return bufs


def lp_read_outputs(case, bufs, names):
    got = {}
    for k in names:
        if k in case.vec_shapes():
            ln, big = case.vec_shapes()[k], bufs[k]
            assert np.all(big[:4] == SENTINEL) and np.all(big[4 + ln:] == SENTINEL), "%s %s: words outside the view were written" % (case.tag(), k)
            got[k] = big[4:4 + ln]
        else:
            r, w = case.out_shapes()[k]
            got[k] = G.read_block(bufs[k], r, w, "%s %s" % (case.tag(), k), d4=w if k == "aff_all" else None)
        assert np.isfinite(got[k]).all(), "%s %s: non-finite output" % (case.tag(), k)
    return got


def sigmoid_lg(x):
    """gs_sigmoid_lg in float64 -> (sg, b_sg, lg, b_lg): class_loss's sigmoid pieces (e = __expf(-|x|), v_rcp_f32, __logf)."""
    x = f64(x)
    ax = np.abs(x)
    e = np.exp(-ax)
    E_e = 2 * ax * U + ULP1
    sg = 1.0 / (1.0 + np.exp(-x))
    lg = np.log1p(e)
    return (sg, (sg * (4 * U + (1 - sg) * E_e) + FLUSH) * SLACK,
            lg, (U + (ULP1 + 2 * U) * lg + (e * E_e + FLUSH) / (1 + e)) * SLACK)


def affinities(case, y_got):
    """aff_all [B, n_neg + 1]: columns [0, n_neg) <y1, neg_q>, column n_neg <y1, y2>.  Per lane Z / 64 products and additions
    (2 Z / 64 roundings unfused), then a 6-step reduction (tail_wave_sum, or the xor butterfly of the four-at-a-time path)."""
    B, y = case.B, f64(y_got)
    y1, y2, ng = y[:B], y[B:2 * B], y[2 * B:]
    want = np.concatenate([y1 @ ng.T, (y1 * y2).sum(axis=1, keepdims=True)], axis=1)
    mag = np.concatenate([np.abs(y1) @ np.abs(ng.T), np.abs(y1 * y2).sum(axis=1, keepdims=True)], axis=1)
    return want, (2 * (y.shape[1] // 64) + 6) * U * mag * SLACK + DENORM


def rank_interval(want, bound):
    """Per pair the ranks #{q: nav_q >= aff} consistent with every affinity moving by its bound -> (lo, hi)."""
    nav, b_nav, aff, b_aff = want[:, :-1], bound[:, :-1], want[:, -1:], bound[:, -1:]
    return (nav - b_nav >= aff + b_aff).sum(axis=1), (nav + b_nav >= aff - b_aff).sum(axis=1)


def lp_loss(case, aff_all_got):
    """loss_rows, rr_rows from the stored affinities.  loss = max(aff, 0) - aff + lg(aff) + neg_weight * sum_q (max(nav_q, 0) +
    lg(nav_q)): the first difference is exact, every addition rounds its result, the sum is one term per lane (tail_wave_sum: 6),
    the product with neg_weight and the last addition one each.  rank = #{q: nav_q >= aff} on the STORED bits is exact, and
    rr = 1 / (rank + 1) a correctly rounded division."""
    a = f64(aff_all_got)
    nav, aff = a[:, :-1], a[:, -1]
    nw = float(case.neg_weight)
    _, _, lga, b_lga = sigmoid_lg(aff)
    _, _, lgn, b_lgn = sigmoid_lg(nav)
    pos = np.maximum(aff, 0) - aff + lga
    terms = np.maximum(nav, 0) + lgn
    neg = terms.sum(axis=1)
    loss = pos + nw * neg
    b = b_lga + U * np.abs(pos) + nw * ((b_lgn + U * terms).sum(axis=1) + 7 * U * neg) + U * np.abs(loss)
    rr = 1.0 / ((nav >= aff[:, None]).sum(axis=1) + 1.0)
    return {"loss_rows": loss, "b_loss_rows": b * SLACK + DENORM, "rr_rows": rr, "b_rr_rows": U * rr}


def lp_pair_grads(case, y_got, aff_all_got, z_got):
    """(dz of the 2 B pair rows, its bound, neg_slabs [GP, n_neg, Z], its bound).  da = (sg(aff) - 1) * scale: sg's error, the
    subtraction and the product.  gq = (neg_weight * scale) * sg(nav_q): two products.  g1 = da y2 + sum_q gq neg_q: a chain of
    n_neg + 1 steps; g2 = da y1.  Each through l2norm_bwd.  Slab of main g: sum over its 8 pairs of y1[p] gq[p][q], a chain of 8
    (16 roundings unfused); pairs beyond B contribute exact zeros."""
    B, nn, Z = case.B, case.n_neg, case.Z
    y, a = f64(y_got), f64(aff_all_got)
    y1, y2, ng = y[:B], y[B:2 * B], y[2 * B:]
    nav, aff = a[:, :-1], a[:, -1:]
    sc, nw = float(case.scale), float(case.neg_weight)
    sa, b_sa, _, _ = sigmoid_lg(aff)
    sg, b_sg, _, _ = sigmoid_lg(nav)
    da, b_da = (sa - 1) * sc, (b_sa + 2 * U * np.abs(sa - 1)) * sc
    gq, b_gq = nw * sc * sg, (b_sg + 2 * U * sg) * nw * sc
    g1 = da * y2 + gq @ ng
    b_g1 = np.abs(y2) * b_da + b_gq @ np.abs(ng) + (nn + 1) * U * (np.abs(da * y2) + gq @ np.abs(ng))
    g2, b_g2 = da * y1, np.abs(y1) * b_da + U * np.abs(da * y1)
    d1, b_d1 = l2norm_bwd(g1, b_g1, y_got[:B], z_got[:B])
    d2, b_d2 = l2norm_bwd(g2, b_g2, y_got[B:2 * B], z_got[B:2 * B])
    slabs, b_slabs = np.zeros((case.GP, nn, Z)), np.zeros((case.GP, nn, Z))
    for g in range(case.GP):
        p = slice(8 * g, min(8 * g + 8, B))
        slabs[g] = gq[p].T @ y1[p]
        b_slabs[g] = b_gq[p].T @ np.abs(y1[p]) + 16 * U * (gq[p].T @ np.abs(y1[p]))
    return np.concatenate([d1, d2]), np.concatenate([b_d1, b_d2]), slabs, b_slabs * SLACK + DENORM


def lp_neg_dz(case, slabs_got, z_got_neg):
    """dz of the negatives (lp_neg_tail_kernel) from the stored slabs and the stored z: g = the slabs added in main order (GP
    roundings on sum |slab|); ss: per lane (x^2 + y^2) + (z^2 + w^2), three roundings on a path, + tail_wave_sum: 9; inv =
    v_rsq_f32: e_inv = 4.5 u + ULP1; dot = sum of ((g.z) four-term tree * inv) per lane: 4 + 6 roundings on inv sum |g z|, and
    inv's error; dz = (g - z * (inv * dot)) * inv: four roundings on their operands, inv's error on |dz|.  Clamped: g * inv."""
    s3 = f64(slabs_got).reshape(case.GP, case.n_neg, case.Z)
    g, b_g = s3.sum(axis=0), case.GP * U * np.abs(s3).sum(axis=0)
    z = f64(z_got_neg)
    ss = (z * z).sum(axis=1, keepdims=True)
    cl = ss < CLAMP
    inv = 1.0 / np.sqrt(np.maximum(ss, CLAMP))
    e_inv = (4.5 * U + ULP1) * SLACK
    dot = inv * (g * z).sum(axis=1, keepdims=True)
    b_dot = inv * ((np.abs(z) * b_g).sum(axis=1, keepdims=True) + 10 * U * np.abs(g * z).sum(axis=1, keepdims=True)) + e_inv * np.abs(dot)
    t = z * inv * dot
    want = np.where(cl, g * inv, (g - t) * inv)
    b_open = inv * (b_g + np.abs(z) * inv * b_dot + (e_inv + 2 * U) * np.abs(t) + U * (np.abs(g) + np.abs(t)))
    bound = np.where(cl, inv * b_g, b_open) + (e_inv + U) * np.abs(want)
    return want, bound * SLACK + DENORM


def lp_epilogue(rows_got, B, prev=None):
    """loss_out / mrr_out = sum(rows) * fp32(1 / B) (+ the previous value: accumulate), the step epilogue's order: per thread a
    chain of ceil(B / 256) additions, tail_wave_sum (6), three additions of the four waves' sums, the reciprocal and the product."""
    r = f64(rows_got)
    want = r.sum() / B + (0.0 if prev is None else float(prev))
    R = -(-B // 256) + 6 + 3 + 2
    return np.array([want]), np.array([(R * U * np.abs(r).sum() / B + (0.0 if prev is None else U * abs(want))) * SLACK + DENORM])


LP_FWD = ("means", "z", "y", "aff_all", "loss_rows", "rr_rows")
LP_BWD = ("dz", "neg_slabs", "d_h0")


def lp_check_stages(case, got, stages, means_in=None, prev_loss=None, note=None):
    """As check_stages, for the link-prediction tail (aff_all must be among the outputs).  Also holds the kernel's rank inside
    rank_interval of the affinities derived from y_got."""
    out = {}

    def hold(k, want, bound, g=None):
        out[k] = go.assert_within(got[k] if g is None else g, want, bound, "%s %s" % (case.tag(), k))
        if note is not None:
            note(k, out[k])

    B, n = case.B, case.n
    if "means" in stages:
        hold("means", *means(case))
    if "z" in stages:
        hold("z", *z(case, means_in if means_in is not None else got["means"]))
    if "y" in stages:
        hold("y", *l2norm(got["z"])[:2])
    if "aff_all" in stages:
        hold("aff_all", *affinities(case, got["y"]))
    if "loss_rows" in stages:
        ref = lp_loss(case, got["aff_all"])
        hold("loss_rows", ref["loss_rows"], ref["b_loss_rows"])
        hold("rr_rows", ref["rr_rows"], ref["b_rr_rows"])
        lo, hi = rank_interval(*affinities(case, got["y"]))
        rank = np.rint(1.0 / f64(got["rr_rows"])) - 1
        assert np.all((lo <= rank) & (rank <= hi)), "%s: a rank outside the interval its affinities allow" % case.tag()
    if "dz" in stages:
        d, b_d, slabs, b_slabs = lp_pair_grads(case, got["y"], got["aff_all"], got["z"])
        hold("dz pairs", d, b_d, got["dz"][:2 * B])
        hold("neg_slabs", slabs.reshape(-1), b_slabs.reshape(-1))
        hold("dz negatives", *lp_neg_dz(case, got["neg_slabs"], got["z"][2 * B:]), g=got["dz"][2 * B:])
    if "d_h0" in stages:
        hold("d_h0", *d_h0(case, got["dz"]))
        assert np.all(G.bits(got["d_h0"])[~case.mask()] == 0), "%s d_h0: an element with h0 <= 0 is not an exact +0" % case.tag()
    if "loss_out" in stages:
        hold("loss_out", *lp_epilogue(got["loss_rows"], B, prev_loss))
        hold("mrr_out", *lp_epilogue(got["rr_rows"], B))
    return out


def lp_sweep():
    """(D, O, B, n_neg, s) of the link-prediction sweep: every B x n_neg x s, the four (D, O) in rotation (each B, each n_neg and
    each s meets at least two of them)."""
    return [DO[(ib + iq + i_s) % 4] + (B, nn, s) for ib, B in enumerate(B_SWEEP) for iq, nn in enumerate(NEG_SWEEP)
            for i_s, s in enumerate([1, 11])]
