"""Float64 NumPy restatements of the gradient finaliser / optimizer (csrc/gs_optim.hip), the step epilogue (gs_common.h:
gs_step_epilogue_block) and the small backward kernels (gs_gather.hip, gs_head.hip), with the rounding-error bounds the GPU
tests hold the kernels to, and the shapes / inputs those tests run (shared with the CPU checks of test_optim_oracle.py).

Error model.  u = 2^-24 is the unit roundoff of fp32.  A value computed with R roundings on its longest path from terms
t_1..t_k differs from the exact result by at most R * u * sum|t_i| (first order; the (1 + 1e-6) below pays for the second).
Every bound here is R * u * (sum of the magnitudes of the terms), R counted from the kernel's code as written; the kernels
that call expf / logf / powf / sqrtf / a division get a factor LIB = 4 on top (those are a few ulp, not half an ulp)."""
import numpy as np

from oracle import graphsage_oracle as orc

U = 2.0 ** -24
LIB = 4.0
SLACK = 1.0 + 1e-6
DENORM = 2.0 ** -149          # spacing of the fp32 subnormals: the absolute floor of any fp32 result


def f32(x):
    """The fp32 value a float argument becomes at the C ABI, as float64."""
    return np.float64(np.float32(x))


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ slab sums
def slab_sum(slabs):
    """slabs [k, size] -> their sum over k (k = 0: zeros)."""
    return f64(slabs).sum(axis=0)


def slab_abs_sum(slabs):
    return np.abs(f64(slabs)).sum(axis=0)


def weight_decay_add(g, p, wd):
    return f64(g) + f32(wd) * f64(p)


def flat_grad(slabs, p, wd, decay):
    """Gradient of one variable of gs_flat_reduce_adam and its error bound.  The kernel adds the slabs in order z = 0, 1, ...
    into g = 0 (the first add is exact: max(k - 1, 0) roundings), then g + fl(wd * p): 2 more."""
    k = slabs.shape[0]
    g, mag = slab_sum(slabs), slab_abs_sum(slabs)
    if decay and wd != 0:
        g, mag = weight_decay_add(g, p, wd), mag + np.abs(f32(wd) * f64(p))
    return g, (max(k - 1, 0) + 2) * U * mag * SLACK


def reduce_slabs(slabs, wd, w, grad_prev):
    """gs_reduce_slabs on [k, rows, cols] slabs.  Thread group g of 8 adds slabs g, g + 8, ... in turn (ceil(k / 8) - 1
    roundings), the 8 partials are added in order (7), then + wd * w (2; 1 if contracted) and + the old grad (1)."""
    k = slabs.shape[0]
    g, mag = slab_sum(slabs), slab_abs_sum(slabs)
    if w is not None and wd != 0:
        g, mag = weight_decay_add(g, w, wd), mag + np.abs(f32(wd) * f64(w))
    if grad_prev is not None:
        g, mag = g + f64(grad_prev), mag + np.abs(f64(grad_prev))
    return g, ((k + 7) // 8 - 1 + 7 + 2 + 1) * U * mag * SLACK


def colsum_slabs(Z, n, n_slabs):
    """gs_colsum_slabs: slab b = column sums of rows [b * rps, min(n, (b + 1) * rps)), rps = ceil(n / n_slabs); slabs past
    the data are zero.  Wave w of 4 adds rows w, w + 4, ... of the slice (<= ceil(rps / 4) roundings), then two levels of
    pairwise adds (2)."""
    Z = f64(Z)[:n]
    rps = -(-n // n_slabs)
    out = np.zeros((n_slabs, Z.shape[1]))
    mag = np.zeros_like(out)
    for b in range(n_slabs):
        out[b] = Z[b * rps:(b + 1) * rps].sum(axis=0)
        mag[b] = np.abs(Z[b * rps:(b + 1) * rps]).sum(axis=0)
    return out, (-(-rps // 4) + 2) * U * mag * SLACK


def scaled_sum(rows, scale, prev, lanes):
    """loss_out = [prev +] scale * sum(rows) as the loss workgroups compute it: `lanes` threads (64 in gs_flat_reduce_adam, 256
    in finalize_step_kernel) stride the rows (ceil(n / lanes) - 1 roundings), a 6-step butterfly, 2 more adds for the 4 waves
    of the 256-thread form, the product with scale (1) and the accumulate (1)."""
    rows = f64(rows)
    n = rows.size
    val, mag = f32(scale) * rows.sum(), abs(f32(scale)) * np.abs(rows).sum()
    if prev is not None:
        val, mag = val + float(prev), mag + abs(float(prev))
    R = max(-(-n // lanes) - 1, 0) + 6 + (2 if lanes == 256 else 0) + 2
    return val, R * U * mag * SLACK


# ------------------------------------------------------------------------------------------------ Adam
def adam_t(step_dev, step_offset):
    """t as the kernels form it: (float)(step + offset)."""
    return float(np.float32(int(step_dev) + int(step_offset)))


def adam_lr_t(t, lr, b1, b2):
    lr, b1, b2 = f32(lr), f32(b1), f32(b2)
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adam_lr_t_roundings(t, b1, b2):
    """Roundings (units of u, relative) of fp32 lr_t = lr * sqrtf(1 - powf(b2, t)) / (1 - powf(b1, t)): powf's relative error is
    amplified by b^t / (1 - b^t) in 1 - b^t (the subtraction cancels), halved again by the sqrt; then the two subtractions (the
    first halved), sqrtf, the product and the division."""
    b1, b2 = f32(b1), f32(b2)
    a1, a2 = b1 ** t, b2 ** t
    return 0.5 * a2 / (1.0 - a2) + 0.5 + 1.0 + a1 / (1.0 - a1) + 1.0 + 1.0 + 1.0


def adam_step_size(m, v, t, lr, b1, b2, eps):
    """q = lr_t * m / (sqrt(v) + eps), the amount gs_adam_elem subtracts from p, and its bound: lr_t's roundings, the product,
    sqrtf, the add of eps and the division (4), times LIB; the subtraction p - q itself rounds to u * |p| (the caller adds)."""
    q = adam_lr_t(t, lr, b1, b2) * f64(m) / (np.sqrt(f64(v)) + f32(eps))
    return q, LIB * (adam_lr_t_roundings(t, b1, b2) + 4) * U * np.abs(q) * SLACK


def adam(p, g, m, v, t, lr, b1, b2, eps, clip, gscale):
    """gs_adam_elem (csrc/gs_common.h) in float64 on fp32-rounded hyper-parameters: g' = g * gscale, clipped to +-clip if
    clip > 0; m' = b1 m + (1 - b1) g'; v' = b2 v + (1 - b2) g'^2; p' = p - lr_t m' / (sqrt(v') + eps).
    Returns (p', m', v', q = p - p', bound_m, bound_v): m' takes 4 roundings (g * gscale, two products, the add), v' takes 6
    (g' enters twice, three products, the add), each relative to the sum of its two terms' magnitudes."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    b1, b2, clip = f32(b1), f32(b2), f32(clip)
    g = g * f32(gscale)
    if clip > 0:
        g = np.clip(g, -clip, clip)
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    q, _ = adam_step_size(m1, v1, t, lr, b1, b2, eps)
    bm = 4 * U * (np.abs(b1 * m) + np.abs((1.0 - b1) * g)) * SLACK
    bv = 6 * U * (b2 * v + (1.0 - b2) * g * g) * SLACK
    return p - q, m1, v1, q, bm, bv


# ------------------------------------------------------------------------------------------------ small backward kernels
def mean_bwd(dm, s, scale, mask_y=None):
    """repeat(dm * fp32(scale)) rows s times, zero where mask_y <= 0.  fp32 in, fp32 out: ONE rounding, the product."""
    g = np.repeat(np.asarray(dm, np.float32) * np.float32(scale), s, axis=0)
    return g if mask_y is None else np.where(mask_y > 0, g, np.float32(0))


def input_grad_pull(rows, d, d_self, n_self, segments, mask_y=None):
    """out[r] = d_self[r] (r < n_self) + sum over segments (src, row0, n, s, scale) covering r of scale * src[(r - row0) / s],
    rows covered by nothing are zero; then the relu mask.  float64 -> (out, bound): one rounding per product and one per add
    after the first term, times the sum of the terms' magnitudes (a row that only copies d_self has bound 0: bit-equal)."""
    out, mag, R = np.zeros((rows, d)), np.zeros((rows, d)), np.zeros((rows, 1))
    terms = np.zeros((rows, 1))
    if d_self is not None:
        out[:n_self] += f64(d_self)[:n_self]
        mag[:n_self] += np.abs(f64(d_self)[:n_self])
        terms[:n_self] += 1
    for src, row0, n, s, scale in segments:
        t = np.repeat(f64(src)[:n] * f32(scale), s, axis=0)
        out[row0:row0 + n * s] += t
        mag[row0:row0 + n * s] += np.abs(t)
        R[row0:row0 + n * s] += 1
        terms[row0:row0 + n * s] += 1
    R += np.maximum(terms - 1, 0)
    if mask_y is not None:
        out, mag = np.where(mask_y > 0, out, 0.0), np.where(mask_y > 0, mag, 0.0)
    return out, R * U * mag * SLACK


def segment_max_fwd(H, n, s):
    """fp32 max over each group of s rows and the FIRST index that attains it (np.argmax's rule)."""
    H3 = np.asarray(H, np.float32).reshape(n, s, -1)
    return H3.max(axis=1), H3.argmax(axis=1).astype(np.int32)


def segment_max_bwd(dP, pooled, arg, n, s):
    """dH[i * s + j, c] = dP[i, c] where j is the arg-max and pooled > 0 (the relu in front of the max), else 0."""
    dH = np.zeros((n, s, dP.shape[1]), np.float32)
    np.put_along_axis(dH, arg[:, None, :].astype(np.int64), np.where(pooled > 0, dP, np.float32(0))[:, None, :], axis=1)
    return dH.reshape(n * s, -1)


def l2norm_fwd(x):
    """orc.l2_normalize_fwd in float64 -> (y, inv, cache, bound_y, bound_inv).  ss: ceil(d / 64) products-and-adds per lane and
    a 6-step butterfly, R_ss = ceil(d / 64) + 7, all terms positive; the clamp constant 1e-12f is itself rounded (1); the sqrt
    halves those; then sqrtf, the division (inv: R_ss / 2 + 2.5) and the product x * inv (y: one more)."""
    x = f64(x)
    y, cache = orc.l2_normalize_fwd(x)
    inv = cache[1][:, 0]
    R = 0.5 * (-(-x.shape[1] // 64) + 7) + 2.5
    return y, inv, cache, LIB * (R + 1) * U * np.abs(y) * SLACK, LIB * R * U * inv * SLACK


def l2norm_bwd(dy, y, inv, ss):
    """orc.l2_normalize_bwd on the y and inv the backward kernel is GIVEN (its inputs, not the exact ones), the clamp decided by
    the exact ss.  dot = sum(dy * y): ceil(d / 64) + 7 roundings; then y * dot, the subtraction and the product with inv (3),
    relative to inv * (|dy| + |y| * sum|dy * y|).  A clamped row is dy * inv: one rounding."""
    dy, y, inv = f64(dy), f64(y), f64(inv)[:, None]
    dx = orc.l2_normalize_bwd(dy, (y / inv, inv, f64(ss).reshape(-1, 1), 1e-12))
    R = -(-dy.shape[1] // 64) + 7 + 3
    mag = inv * (np.abs(dy) + np.abs(y) * np.abs(dy * y).sum(axis=1, keepdims=True))
    return dx, LIB * R * U * mag * SLACK


def class_loss(x, z, sigmoid_loss):
    """Per-row classification loss, predictions and d(mean loss)/d(logits) for general label rows z (0/1 entries), float64
    (orc.classification_loss for the gradient, orc.sigmoid / orc.softmax for the predictions) -> dict of values and bounds.

    expf: the library's expansion forms ph = x * log2(e), n = rint(ph) and 2^n * exp2((ph - n) + pl), pl the product's rounding
    residual; under the build's -ffp-contract=fast the compiler fuses ph - n into fma(x, log2(e), -n), which is already exact, so
    adding pl puts the product's rounding BACK: expf(x) is off by up to |x| u relative (half an ulp of x * log2(e), times ln 2),
    on top of the instruction's own ulp.  Seen on the GPU: sigmoid(-30) off by 14.7 u.  That term is not a library ulp: it is
    counted as |x| u, outside the factor LIB.
    sigmoid: loss_r = mean_c [max(x, 0) - x z + log1p(exp(-|x|))]: 4 roundings per term (x z is exact for z in {0, 1}; the
    subtraction, expf, log1pf, the add) and expf's |x| u, which log1p scales by e / (1 + e), e = exp(-|x|);
    ceil(C / 64) + 6 for the wave's sum, 1 for / C, relative to the mean of the terms' magnitudes.
    p = 1 / (1 + exp(-x)): 3 roundings (expf, the add, the division) and expf's |x| u scaled by e / (1 + e) = 1 - p.
    g = (p - z) / (n C): p's error, then the subtraction, n * C, the reciprocal and the product (4) on |p - z|.
    softmax: the max is exact; e_c = exp(x_c - m) carries the rounding of x_c - m INTO the exponent: (|x_c - m| + 1) u
    relative (the factor LIB on this term also pays for expf's own |x_c - m| u); se = sum e_c adds ceil(C / 64) + 6.  p_c = e_c / se: e_c's, se's, the reciprocal and the product.
    loss_r = zs * lse - zx with lse = m + logf(se), zs = sum z exact, zx = sum z x (products exact, ceil(C / 64) + 6 for the sum):
    lse is off by u * (E_se + |log se| + |lse|), then the product and the subtraction round to u * (|zs lse| + |zx|) each.
    g = (p zs - z) / n: p's roundings + 1 on p zs, then the subtraction, the reciprocal of n and the product (3).
    Everywhere + DENORM: a result below 2^-126 is a subnormal with absolute, not relative, spacing."""
    x, z = f64(x), f64(z)
    n, C = x.shape
    Rs = -(-C // 64) + 6
    _, dlog = orc.classification_loss(x, z, sigmoid_loss)
    if sigmoid_loss:
        e = np.exp(-np.abs(x))
        sp = np.log1p(e)
        loss = (np.maximum(x, 0) - x * z + sp).mean(axis=1)
        lmag = (np.maximum(x, 0) + np.abs(x * z) + sp).mean(axis=1)
        p = orc.sigmoid(x)
        e_p = np.abs(x) * (1 - p) * p * U                        # expf's argument-proportional error, as it reaches p
        return {"loss": loss, "b_loss": (LIB * (4 + Rs + 1) * U * lmag + U * (np.abs(x) * e / (1 + e)).mean(axis=1)) * SLACK + DENORM,
                "preds": p, "b_preds": (LIB * 3 * U * p + e_p) * SLACK + LIB * DENORM,
                "dlogits": dlog, "b_dlogits": (LIB * U * (3 * p + 4 * np.abs(p - z)) + e_p) / (n * C) * SLACK + LIB * DENORM}
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    se = e.sum(axis=1, keepdims=True)
    E_e = np.abs(x - m) + 1
    E_se = (e * E_e).sum(axis=1, keepdims=True) / se + Rs
    p = orc.softmax(x)
    E_p = E_e + E_se + 2
    lse = m + np.log(se)
    zs, zx = z.sum(axis=1, keepdims=True), (z * x).sum(axis=1, keepdims=True)
    loss = (zs * lse - zx)[:, 0]
    b_loss = U * (zs * (E_se + 1 + np.abs(np.log(se)) + np.abs(lse)) + Rs * np.abs(z * x).sum(axis=1, keepdims=True)
                  + 2 * (np.abs(zs * lse) + np.abs(zx)))[:, 0]
    return {"loss": loss, "b_loss": LIB * b_loss * SLACK + DENORM,
            "preds": p, "b_preds": LIB * E_p * U * p * SLACK + LIB * DENORM,
            "dlogits": dlog, "b_dlogits": LIB * U * ((E_p + 1) * p * zs + 3 * np.abs(p * zs - z)) / n * SLACK + LIB * DENORM}


# ------------------------------------------------------------------------------------------------ the cases under test
SENTINEL = -12345.5
HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8)

# gs_flat_reduce_adam layouts: sizes in floats, slab counts, decay flags, the `clear` variable (n_slabs must be 1)
FLAT_LAYOUTS = {
    # several variables inside one wave (64 float4 = 256 floats), one wave spanning three or more; slab counts 0, one batch of
    # GS_OPT_SLAB_BATCH = 24, one batch + 1, two batches + 1
    "straddle": dict(sizes=[4, 4, 44, 4, 252, 8, 1028, 4], n_slabs=[1, 0, 3, 24, 25, 49, 2, 1],
                     decay=[1, 0, 1, 1, 0, 1, 1, 0], clear=[0, 0, 0, 0, 0, 0, 0, 1]),
    # GS_MAX_VARS = 24 variables of 4..68 floats: the unrolled offset search runs over every slot
    "vars24": dict(sizes=[4 + 4 * ((7 * i) % 17) for i in range(24)], n_slabs=[(5 * i) % 4 for i in range(24)],
                   decay=[i % 2 for i in range(24)], clear=[0] * 24),
    # grid-stride loop: 4096 * 256 float4 + 77 more, then a variable of 11 float4: the second, partial trip of the loop ends
    # inside another variable
    "past_cap": dict(sizes=[4096 * 256 * 4 + 4 * 77, 44], n_slabs=[2, 3], decay=[1, 0], clear=[0, 0]),
}
FLAT_TAIL = 64                  # `total` is this many floats larger than the variables cover: never written
FLAT_LOSS_N = [1, 63, 64, 65, 700]
ADAM_COUNTS = [1, 2048 * 256 + 77]
REDUCE_SLAB_COUNTS = [1, 8, 9, 127, 128, 129, 257]
REDUCE_SMALL = (5, 7, 8, 12)                # rows, cols, ld_slab, ldg: 35 outputs, the last workgroup's lanes 3..31 are clamped
REDUCE_BIG = (1030, 128, 128, 128)          # 131840 outputs, 3 slabs: the grid-stride loop
COLSUM_CASES = [(777, 41, 5, 44), (300, 130, 3, 132), (5, 64, 8, 64), (33, 65, 1, 68), (29, 7, 1, 8), (1, 1, 1, 4)]
FINALIZE_N = [0, 1, 63, 64, 255, 256, 257, 5000]

WIDTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 602]
ROWS = [1, 3, 4, 5, 257]
GROUPS = [1, 2, 25, 70]
CLASSES = [1, 3, 41, 64, 65, 121, 130]
# past-the-cap shapes at d = 5 (two float4 per row)
CAP_D = 5
CAP_MEAN_BWD = (37450, 7)       # n, s: 262150 rows
CAP_ACT_BWD = 262150            # rows
CAP_PULL_ROWS = 524293
CAP_SEGMAX_FWD = (524293, 2)    # n, s
CAP_SEGMAX_BWD = (524293, 2)    # n, s: 1048586 rows


def lds(d):
    d4 = (d + 3) // 4 * 4
    return [d4, d4 + 8]


def flat_inputs(name, seed=0):
    """p0 and the slabs of a layout.  Slab magnitudes differ by variable (10^-3 .. 10), so that some gradients exceed the clip
    of 5 and others stay far below; nothing is zero."""
    L = FLAT_LAYOUTS[name]
    rng = np.random.RandomState(seed)
    covered = sum(L["sizes"])
    p0 = (rng.standard_normal(covered) * 0.1).astype(np.float32)
    slabs = [(rng.standard_normal((max(k, 1), sz)) * 10.0 ** (((i + 3) % 5) - 3)).astype(np.float32)
             for i, (sz, k) in enumerate(zip(L["sizes"], L["n_slabs"]))]
    return p0, slabs


def l2_rows(n, d, seed):
    """Rows for the l2norm sweep: unit-scale rows, then (as far as n allows, from the LAST row backwards, so that n = 1 tests
    the all-zero row) an all-zero row, sum(x^2) = 1e-12 * (1 -+ 2^-10) (just clamped / just not) and a row of NORM 1e18 (the
    entries are 1e18 / sqrt(d): the fp32 sum of squares, 1e36, stays finite as it does in the float64 oracle)."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, d))
    unit = x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    special = [0.0, np.sqrt(1e-12 * (1 - 2.0 ** -10)), np.sqrt(1e-12 * (1 + 2.0 ** -10)), 1e18]
    for k, norm in enumerate(special[:n]):
        x[n - 1 - k] = unit[n - 1 - k] * norm
    return x.astype(np.float32)


def class_inputs(n, C, sigmoid_loss, seed):
    """Logits at scale 3 with planted +-30, +-88, +-200; labels: sigmoid 0/1 at random, softmax one-hot rows, then multi-hot
    rows and all-zero rows in turn (row r: r % 3)."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((n, C)) * 3).astype(np.float32)
    planted = [30.0, -30.0, 88.0, -88.0, 200.0, -200.0]
    for k, val in enumerate(planted):
        x[(5 * k + 1) % n, (7 * k + 3) % C] = val
    if sigmoid_loss:
        z = (rng.random_sample((n, C)) > 0.5).astype(np.float32)
    else:
        z = np.eye(C, dtype=np.float32)[rng.randint(0, C, n)]
        multi = (rng.random_sample((n, C)) > 0.6).astype(np.float32)
        r = np.arange(n) % 3
        z[r == 1] = multi[r == 1]
        z[r == 2] = 0
    return x, z


# ------------------------------------------------------------------------------------------------ comparison
WORST = {}


def check(kernel, what, got, want, bound):
    """assert |got - want| <= bound on EVERY element; prints (pytest -s) the worst error as a fraction of its bound, and keeps
    the worst per kernel in WORST."""
    got, want, bound = f64(got), f64(want), np.broadcast_to(f64(bound), np.shape(want))
    assert got.shape == want.shape, (kernel, what, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s %s: non-finite output" % (kernel, what)
    err = np.abs(got - want)
    frac = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
    k = int(np.argmax(frac)) if frac.size else 0
    worst = float(frac.reshape(-1)[k]) if frac.size else 0.0
    key = "%s %s" % (kernel, what)
    here = (worst, float(err.reshape(-1)[k]) if frac.size else 0.0, float(bound.reshape(-1)[k]) if frac.size else 0.0)
    if worst >= WORST.get(key, (-1.0,))[0]:
        WORST[key] = here
    print("[bound] %-44s worst err/bound %.3f (err %.3e, bound %.3e, %d elements)" % ((key,) + here + (err.size,)))
    assert worst <= 1.0, "%s: %d of %d elements beyond the derived bound; worst: err %.3e, bound %.3e, got %r want %r" % (
        key, int((frac > 1).sum()), err.size, err.reshape(-1)[k], bound.reshape(-1)[k], got.reshape(-1)[k], want.reshape(-1)[k])
