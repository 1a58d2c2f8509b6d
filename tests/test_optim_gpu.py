"""-m gpu: the gradient finaliser / optimizer (csrc/gs_optim.hip: gs_flat_reduce_adam, gs_adam_step, gs_reduce_slabs,
gs_colsum_slabs) and the step epilogue (gs_finalize_step, gs_finalize_step2) against the float64 oracle of
tests/optim_oracle.py, at the shapes where a float4 kernel with a masked tail, a clamped surplus load or a capped grid goes
wrong.  Every buffer a launch may write is larger than the written extent and pre-filled with a sentinel; every input pad a
launch must not read holds NaN.  Bounds: oo.* derive them from the kernels' code (roundings on the longest path x 2^-24 x the sum
of the terms' magnitudes, x 4 where expf / logf / powf / sqrtf / a division is involved); the numbers are in each docstring.
Copies, selects, counters, the `clear` slab and every repeat are bit-equal."""
import ctypes

import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
from graphsage_amd._lib import GraphsageAmdError
from graphsage_amd.ops import Mat
import optim_oracle as oo

pytestmark = pytest.mark.gpu
S = oo.SENTINEL
H = oo.HYPER
HARGS = (H["lr"], H["b1"], H["b2"], H["eps"])


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sync():
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- gs_flat_reduce_adam
class Flat(object):
    """One layout of oo.FLAT_LAYOUTS on the device: params / grads / m / v of covered + FLAT_TAIL + 32 floats (`total` passed is
    covered + FLAT_TAIL), the slabs of each variable with 16 sentinel floats behind them, the device step counter."""

    def __init__(self, dev, name, step0, seed=0):
        L = oo.FLAT_LAYOUTS[name]
        self.L, self.dev = L, dev
        self.sizes, self.k = L["sizes"], L["n_slabs"]
        self.covered = sum(self.sizes)
        self.total = self.covered + oo.FLAT_TAIL
        p0, slabs = oo.flat_inputs(name, seed)

        def buf(fill):
            a = np.full(self.total + 32, S, np.float32)
            a[:self.covered] = fill
            return _dev(a, dev)
        self.P, self.G, self.M, self.V = buf(p0), buf(S), buf(0.0), buf(0.0)
        self.slabs = [_dev(np.concatenate([s.reshape(-1), np.full(16, S, np.float32)]), dev) for s in slabs]
        self.step = torch.tensor([step0], dtype=torch.int64, device=dev)
        self.desc = self.descs(len(self.sizes))
        _sync()

    def descs(self, n):
        arr = (_lib.VarDesc * n)()
        off = 0
        for i in range(n):
            j = i % len(self.sizes)
            arr[i].offset, arr[i].size, arr[i].slabs, arr[i].n_slabs = off, self.sizes[j], self.slabs[j].data_ptr(), self.k[j]
            arr[i].decay, arr[i].clear = self.L["decay"][j], self.L["clear"][j]
            off += self.sizes[j]
        return arr

    def launch(self, fuse, wd, clip, gscale, offset, loss=None, desc=None):
        desc = self.desc if desc is None else desc
        lr, ln, ls, lo, la = loss if loss is not None else (None, 0, 0.0, None, 0)
        ops.call("gs_flat_reduce_adam", ctypes.addressof(desc), len(desc), ops.ptr(self.P), ops.ptr(self.G), ops.ptr(self.M),
                 ops.ptr(self.V), self.total, wd, fuse, *HARGS, clip, gscale, ops.ptr(self.step), offset, ops.ptr(lr), ln, ls,
                 ops.ptr(lo), la, ops.current_stream())

    def host(self):
        _sync()
        st = {n: getattr(self, n).cpu().numpy() for n in "PGMV"}
        st["slabs"] = [s.cpu().numpy() for s in self.slabs]
        st["step"] = int(self.step.item())
        return st


def check_flat(fl, b, a, fuse, wd, clip, gscale, offset, tag):
    """before-state b, after-state a of ONE launch against the oracle (see test_flat_reduce_adam_equals_the_oracle)."""
    c = fl.covered
    for n in "PGMV":
        assert np.all(a[n][c:] == S), "%s: %s written beyond the variables (the tail of `total` / the surplus)" % (tag, n)
    off = 0
    want_g, bound_g = np.zeros(c), np.zeros(c)
    for i, (sz, k) in enumerate(zip(fl.sizes, fl.k)):
        sl = b["slabs"][i][:max(k, 1) * sz].reshape(max(k, 1), sz)
        want_g[off:off + sz], bound_g[off:off + sz] = oo.flat_grad(sl[:k], b["P"][off:off + sz], wd, fl.L["decay"][i])
        if fl.L["clear"][i]:
            assert np.all(a["slabs"][i][:sz] == 0), "%s: the slab of the clear variable %d must be consumed" % (tag, i)
            assert np.all(a["slabs"][i][sz:] == S)
        else:
            assert np.array_equal(a["slabs"][i], b["slabs"][i]), "%s: slab %d changed" % (tag, i)
        off += sz
    oo.check("flat_reduce_adam", "grads", a["G"][:c], want_g, bound_g)
    if not fuse:
        for n in "PMV":
            assert np.array_equal(a[n], b[n]), "%s: fuse_adam = 0 must leave %s alone" % (tag, n)
        return
    t = oo.adam_t(b["step"], offset)
    _, m1, v1, _, bm, bv = oo.adam(b["P"][:c], a["G"][:c], b["M"][:c], b["V"][:c], t, clip=clip, gscale=gscale, **H)
    oo.check("flat_reduce_adam", "adam_m", a["M"][:c], m1, bm)
    oo.check("flat_reduce_adam", "adam_v", a["V"][:c], v1, bv)
    q, bq = oo.adam_step_size(a["M"][:c], a["V"][:c], t, **H)
    update = a["P"][:c].astype(np.float64) - b["P"][:c]
    oo.check("flat_reduce_adam", "update", update, -q, bq + oo.U * np.maximum(np.abs(a["P"][:c]), np.abs(b["P"][:c])))
    assert np.abs(update).max() > 0


FLAT_CONFIGS = {
    # fuse, wd, clip, gscale, step_offset, steps
    "three_steps-wd-clip5-offset1": (1, 0.01, 5.0, 1.0, 1, 3),
    "grads_only_fuse0-three_steps": (0, 0.01, 5.0, 1.0, 1, 3),
    "gscale_quarter-clip_off-wd0-offset0": (1, 0.0, 0.0, 0.25, 0, 1),
    "clip_off-wd": (1, 0.01, 0.0, 1.0, 1, 1),
}
FLAT_CASES = [(lay, cfg) for lay in ("straddle", "vars24") for cfg in sorted(FLAT_CONFIGS)] + [
    ("past_cap", "three_steps-wd-clip5-offset1"), ("past_cap", "grads_only_fuse0-three_steps")]


@pytest.mark.parametrize("layout,config", FLAT_CASES, ids=["%s-%s" % c for c in FLAT_CASES])
def test_flat_reduce_adam_equals_the_oracle(dev, layout, config):
    """gs_flat_reduce_adam against oo.flat_grad / oo.adam, the device step at 7, every launch checked from the state the device held
    before it (so m and v are non-zero on entry of the 2nd and 3rd step and each step's bound is that of ONE step).
    Layouts (oo.FLAT_LAYOUTS): `straddle` (variables inside one wave, a wave over >= 3 variables, n_slabs 0 / 1 / 24 / 25 / 49: the
    second and third batch of GS_OPT_SLAB_BATCH loads with their clamped surplus loads, a `clear` variable, a variable without
    slabs whose slab pointer holds data that must be ignored), `vars24` (GS_MAX_VARS variables: every slot of the offset search),
    `past_cap` (> 4096 * 256 float4: the grid-stride loop's second trip ends inside another variable; one step).  `total` is 64
    floats beyond the variables: that tail and 32 more floats keep the sentinel.
    Bounds.  grads: (max(n_slabs - 1, 0) + 2) u (sum_k |slab_k| + |wd p|): at n_slabs = 49 that is 50 u = 3.0e-6 of the terms'
    magnitudes (a dropped slab of 49 is ~ 1 / 49 of them).  m: 4 u (|b1 m| + |(1 - b1) g'|) = 2.4e-7; v: 6 u (b2 v + (1 - b2) g'^2) =
    3.6e-7.  update p_after - p_before against -lr_t m' / (sqrt(v') + eps) formed from the m', v' the launch stored: 4 (R_lr + 4) u
    |q| + u |p| with R_lr = 77 (t = 7), 68 (t = 8), 61 (9), 55 (10) roundings of lr_t (1 - 0.999^t cancels: powf's error is amplified
    by 0.999^t / (1 - 0.999^t) ~ 1 / (0.001 t), halved by the sqrt): 1.9e-5 |q| at t = 7, against a 2 % change of lr_t for a step
    count off by one."""
    fuse, wd, clip, gscale, offset, steps = FLAT_CONFIGS[config]
    if layout == "past_cap":
        steps = 1
    fl = Flat(dev, layout, 7)
    b = fl.host()
    if clip > 0:
        assert layout == "vars24" or any((np.abs(s[:-16]) * gscale > clip).any() for s in b["slabs"])
    for it in range(steps):
        fl.launch(fuse, wd, clip, gscale, offset)
        a = fl.host()
        check_flat(fl, b, a, fuse, wd, clip, gscale, offset, "%s/%s step %d" % (layout, config, it))
        ops.advance_counter(fl.step, 1)
        b = fl.host()
        assert b["step"] == 8 + it
    again = Flat(dev, layout, 7)
    again.launch(fuse, wd, clip, gscale, offset)
    first = Flat(dev, layout, 7)
    first.launch(fuse, wd, clip, gscale, offset)
    x, y = again.host(), first.host()
    for n in "PGMV":
        assert np.array_equal(x[n], y[n]), "two launches from the same inputs must agree bit for bit (%s)" % n


def test_flat_reduce_adam_clip_and_step_offset_change_the_step(dev):
    """clip = 0 against clip = 5 and step_offset 0 against 1 (device step 7: t = 7 against 8) are each checked against the oracle
    above; here: they DIFFER where they must (a clipped gradient, every update), so neither argument is ignored."""
    out = {}
    for key, (clip, offset) in {"c5o1": (5.0, 1), "c0o1": (0.0, 1), "c5o0": (5.0, 0)}.items():
        fl = Flat(dev, "straddle", 7)
        b = fl.host()
        fl.launch(1, 0.01, clip, 1.0, offset)
        a = fl.host()
        check_flat(fl, b, a, 1, 0.01, clip, 1.0, offset, key)
        out[key] = a
    c = sum(oo.FLAT_LAYOUTS["straddle"]["sizes"])
    g = out["c5o1"]["G"][:c]
    assert np.array_equal(out["c5o1"]["G"], out["c0o1"]["G"]) and (np.abs(g) > 5).any()
    assert np.all(out["c5o1"]["M"][:c][np.abs(g) > 5] != out["c0o1"]["M"][:c][np.abs(g) > 5])
    assert np.array_equal(out["c5o1"]["M"][:c][np.abs(g) <= 5], out["c0o1"]["M"][:c][np.abs(g) <= 5])
    assert np.array_equal(out["c5o1"]["M"], out["c5o0"]["M"]) and np.array_equal(out["c5o1"]["V"], out["c5o0"]["V"])
    moved = out["c5o1"]["M"][:c] != 0
    assert moved.any() and np.all(out["c5o1"]["P"][:c][moved] != out["c5o0"]["P"][:c][moved])


def test_flat_reduce_adam_refuses_25_variables_on_the_host(dev):
    """GS_MAX_VARS + 1 variables: refused with the limit in the message, nothing launched (grads keep the sentinel)."""
    fl = Flat(dev, "vars24", 7)
    with pytest.raises(GraphsageAmdError, match="24"):
        fl.launch(1, 0.01, 5.0, 1.0, 1, desc=fl.descs(25))
    a = fl.host()
    assert np.all(a["G"] == S) and np.all(a["M"][:fl.covered] == 0)
    bad = fl.descs(24)
    bad[3].offset += 4                                             # a gap: the variables must tile the buffer in order
    with pytest.raises(GraphsageAmdError, match="tile"):
        fl.launch(1, 0.01, 5.0, 1.0, 1, desc=bad)
    assert np.all(fl.host()["G"] == S)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("loss_n", oo.FLAT_LOSS_N)
def test_flat_reduce_adam_loss_rows(dev, loss_n, accumulate):
    """The scalar loss folded into the launch (a workgroup of its own, one wave): loss_out = [loss_out +] scale * sum(rows[0:n]), n
    around the wave (1, 63, 64, 65) and 700; the rows behind n hold NaN, loss_out's neighbours a sentinel; the gradients of the
    same launch still equal the oracle.  Bound: (ceil(n / 64) - 1 + 6 + 2) u (scale sum|rows| + |loss_out|): 18 u = 1.1e-6 at 700."""
    rng = np.random.RandomState(loss_n)
    rows = rng.random_sample(loss_n).astype(np.float32) * 3
    rows_d = _dev(np.concatenate([rows, np.full(8, np.nan, np.float32)]), dev)
    out = _dev(np.asarray([S, 7.0, S], np.float32), dev)
    scale = float(np.float32(1.0 / loss_n))
    fl = Flat(dev, "straddle", 7)
    b = fl.host()
    fl.launch(0, 0.01, 5.0, 1.0, 1, loss=(rows_d, loss_n, scale, out[1:2], accumulate))
    a = fl.host()
    check_flat(fl, b, a, 0, 0.01, 5.0, 1.0, 1, "loss")
    got = out.cpu().numpy()
    assert got[0] == S and got[2] == S
    want, bound = oo.scaled_sum(rows, scale, 7.0 if accumulate else None, 64)
    oo.check("flat_reduce_adam", "loss", got[1:2], [want], [bound])


# ----------------------------------------------------------------------------------------------- gs_adam_step
ADAM_CONFIGS = {
    # gscale, clip, device step, step_offset
    "gscale_half-clip5-step7-offset1": (0.5, 5.0, 7, 1),
    "gscale_half-clip_off-step7-offset0": (0.5, 0.0, 7, 0),
    "clip_off-step_2p33_plus_3-offset0": (1.0, 0.0, 2 ** 33 + 3, 0),
}


@pytest.mark.parametrize("config", sorted(ADAM_CONFIGS))
@pytest.mark.parametrize("count", oo.ADAM_COUNTS)
def test_adam_step_equals_the_oracle(dev, count, config):
    """gs_adam_step against oo.adam over 3 steps: m, v and the update p_after - p_before, each step from the device's own state
    before it; count = 1 and 2048 * 256 + 77 (the stride loop past the grid cap, a ragged end); 32 sentinel floats behind every
    buffer.  The device step is read through step_dev: 2^33 + 3 must not be truncated to 3 (t = 2^33: both powf are 0, lr_t = lr;
    truncated, lr_t would be 5 % of that).  Bounds as in test_flat_reduce_adam_equals_the_oracle: m 4 u, v 6 u of their terms,
    update 4 (R_lr + 4) u |q| + u |p| with R_lr = 77 / 68 / 61 / 55 at t = 7 / 8 / 9 / 10 and 4.5 at t = 2^33."""
    gscale, clip, step0, offset = ADAM_CONFIGS[config]
    rng = np.random.RandomState(count % 1000)

    def buf(a):
        return _dev(np.concatenate([a.astype(np.float32), np.full(32, S, np.float32)]), dev)
    g_h = (rng.standard_normal(count) * 8).astype(np.float32)
    P, G, M, V = buf(rng.standard_normal(count) * 0.1), buf(g_h), buf(np.zeros(count)), buf(np.zeros(count))
    step = torch.tensor([step0], dtype=torch.int64, device=dev)
    assert clip == 0 or count == 1 or (np.abs(g_h * gscale) > clip).any()
    for it in range(3):
        b = [x.cpu().numpy() for x in (P, M, V)]
        ops.adam_step(P, G, M, V, count, H["lr"], step, clip=clip, grad_scale=gscale, step_offset=offset)
        _sync()
        a = [x.cpu().numpy() for x in (P, M, V)]
        for x in a:
            assert np.all(x[count:] == S)
        assert np.array_equal(G.cpu().numpy()[:count], g_h)
        t = oo.adam_t(step0 + it, offset)
        _, m1, v1, _, bm, bv = oo.adam(b[0][:count], g_h, b[1][:count], b[2][:count], t, clip=clip, gscale=gscale, **H)
        oo.check("adam_step", "adam_m", a[1][:count], m1, bm)
        oo.check("adam_step", "adam_v", a[2][:count], v1, bv)
        q, bq = oo.adam_step_size(a[1][:count], a[2][:count], t, **H)
        oo.check("adam_step", "update", a[0][:count].astype(np.float64) - b[0][:count], -q,
                 bq + oo.U * np.maximum(np.abs(a[0][:count]), np.abs(b[0][:count])))
        ops.advance_counter(step, 1)
    _sync()
    assert int(step.item()) == step0 + 3


def test_adam_step_count_0_launches_nothing(dev):
    bufs = [torch.full((8,), S, dtype=torch.float32, device=dev) for _ in range(4)]
    step = torch.tensor([7], dtype=torch.int64, device=dev)
    ops.adam_step(*bufs, 0, H["lr"], step)
    _sync()
    assert all(np.all(x.cpu().numpy() == S) for x in bufs)
    with pytest.raises(GraphsageAmdError, match="gs_adam_step"):
        ops.adam_step(*bufs, -1, H["lr"], step)


@pytest.mark.parametrize("offset", [0, 1])
def test_fused_adam_equals_reduce_then_adam_step_on_the_straddle_layout(dev, offset):
    """fuse_adam = 1 == fuse_adam = 0 followed by gs_adam_step, bit for bit (params, grads, m, v, tails included), three steps, on
    the layout whose waves span variables (test_peer_gpu.py asserts it for one layout with wave-aligned boundaries)."""
    res = {}
    for mode in ("fused", "two"):
        fl = Flat(dev, "straddle", 7)
        out = []
        for it in range(3):
            if mode == "fused":
                fl.launch(1, 0.01, 5.0, 0.25, offset)
            else:
                fl.launch(0, 0.01, 5.0, 0.25, offset)
                ops.adam_step(fl.P, fl.G, fl.M, fl.V, fl.covered, H["lr"], fl.step, clip=5.0, grad_scale=0.25, step_offset=offset)
            ops.advance_counter(fl.step, 1)
            out.append(fl.host())
        res[mode] = out
    for it in range(3):
        for n in "PGMV":
            assert np.array_equal(res["fused"][it][n], res["two"][it][n]), (it, n)


# ----------------------------------------------------------------------------------------------- gs_reduce_slabs
def _reduce_case(dev, k, shape, wd, with_w, accumulate, seed):
    rows, cols, ld_slab, ldg = shape
    ldw = ldg + 4
    rng = np.random.RandomState(seed)
    stride = rows * ld_slab + 4
    sl = np.full((k, stride), np.nan, np.float32)                         # pad columns / the gap between slabs: never read
    data = (rng.standard_normal((k, rows, cols)) * 10.0 ** rng.randint(-2, 2, size=(k, 1, 1))).astype(np.float32)
    for z in range(k):
        sl[z, :rows * ld_slab].reshape(rows, ld_slab)[:, :cols] = data[z]
    w = np.full((rows, ldw), np.nan, np.float32)
    w[:, :cols] = rng.standard_normal((rows, cols))
    g0 = np.full((rows + 4, ldg), S, np.float32)
    prev = rng.standard_normal((rows, cols)).astype(np.float32)
    if accumulate:
        g0[2:2 + rows, :cols] = prev
    sl_d, w_d, g_d = _dev(sl, dev), _dev(w, dev), _dev(g0, dev)
    _sync()
    ops.reduce_slabs(sl_d, k, stride, rows, cols, ld_slab, wd, ops.ptr(w_d) if with_w else None, ldw,
                     g_d.data_ptr() + 2 * ldg * 4, ldg, accumulate=bool(accumulate))
    _sync()
    got = g_d.cpu().numpy()
    assert np.all(got[:2] == S) and np.all(got[2 + rows:] == S), "rows outside the gradient were written"
    assert np.all(got[:, cols:] == S), "columns [cols, ldg) were written"
    want, bound = oo.reduce_slabs(data, wd, w[:, :cols] if with_w else None, prev if accumulate else None)
    oo.check("reduce_slabs", "grad", got[2:2 + rows, :cols], want, bound)
    return got


REDUCE_VARIANTS = [(0.5, True, 0), (0.5, False, 0), (0.0, True, 0), (0.5, True, 1)]


@pytest.mark.parametrize("n_slabs", oo.REDUCE_SLAB_COUNTS)
def test_reduce_slabs_slab_counts(dev, n_slabs):
    """gs_reduce_slabs at (rows, cols, ld_slab, ldg) = (5, 7, 8, 12): 35 outputs, so lanes 3..31 of the second workgroup take the
    clamped tc = total - 1; n_slabs around the 8 slab groups (1, 8, 9) and the 128 slabs of one trip (127, 128, 129, 257: the
    `z0 += 128` second and third trip with clamped surplus loads).  wd with w, wd with w null (no decay), wd = 0 with w,
    accumulate onto known values.  Pad columns of slabs and w hold NaN; grad sits in a sentinel buffer.  Bound:
    (ceil(k / 8) - 1 + 7 + 2 + 1) u (sum_k |slab_k| + |wd w| + |grad|): 42 u = 2.5e-6 at 257 slabs (one dropped slab: ~ 1 / 257 = 3.9e-3)."""
    for v, (wd, with_w, acc) in enumerate(REDUCE_VARIANTS):
        a = _reduce_case(dev, n_slabs, oo.REDUCE_SMALL, wd, with_w, acc, 100 * n_slabs + v)
        b = _reduce_case(dev, n_slabs, oo.REDUCE_SMALL, wd, with_w, acc, 100 * n_slabs + v)
        assert np.array_equal(a, b), "fixed summation order: two launches must agree bit for bit"


@pytest.mark.parametrize("accumulate", [0, 1])
def test_reduce_slabs_past_the_grid_cap(dev, accumulate):
    """1030 x 128 = 131840 outputs > 4096 * 32: the grid-stride loop of reduce_slabs_kernel; 3 slabs.  Bound 10 u = 6.0e-7."""
    a = _reduce_case(dev, 3, oo.REDUCE_BIG, 0.5, True, accumulate, 7)
    b = _reduce_case(dev, 3, oo.REDUCE_BIG, 0.5, True, accumulate, 7)
    assert np.array_equal(a, b)


def test_reduce_slabs_refuses_overlapping_rows_on_the_host(dev):
    sl, g = torch.zeros(64, device=dev), torch.full((64,), S, dtype=torch.float32, device=dev)
    for ld_slab, ldw, ldg in ((4, 8, 8), (8, 4, 8), (8, 8, 4)):
        with pytest.raises(GraphsageAmdError, match="cols"):
            ops.reduce_slabs(sl, 1, 64, 2, 7, ld_slab, 0.5, ops.ptr(sl), ldw, ops.ptr(g), ldg)
    _sync()
    assert np.all(g.cpu().numpy() == S)


# ----------------------------------------------------------------------------------------------- gs_colsum_slabs
@pytest.mark.parametrize("n,n_cols,n_slabs,ld_slab", oo.COLSUM_CASES)
def test_colsum_slabs_slab_by_slab(dev, n, n_cols, n_slabs, ld_slab):
    """gs_colsum_slabs slab by slab (not only the sum over slabs): one and three column tiles of 64 (blockIdx.x > 0), slices
    of 156 / 100 rows (the 8-deep unrolled loop and its remainder), of 33 / 29 (one trip / none), of 1 row; n < n_slabs (5 rows, 8
    slabs: slabs 5..7 exact zeros).  Z is a row slice of a wider buffer whose other rows and pad columns hold NaN; the slabs sit
    in a sentinel buffer, columns [n_cols, ld_slab) keep it.  Bound: (ceil(rps / 4) + 2) u sum|Z|: 41 u = 2.4e-6 at rps = 156."""
    rng = np.random.RandomState(n + n_cols)
    ldz = ops.round_up(n_cols, 4) + 8
    z = rng.standard_normal((n, n_cols)).astype(np.float32)
    big = np.full((n + 4, ldz), np.nan, np.float32)
    big[2:2 + n, :n_cols] = z
    Z = Mat(_dev(big, dev)[2:2 + n], n_cols)
    out = torch.full(((n_slabs + 2) * ld_slab,), S, dtype=torch.float32, device=dev)
    _sync()
    runs = []
    for _ in range(2):
        ops.colsum_slabs(Z, n, n_cols, n_slabs, out[ld_slab:], ld_slab)
        _sync()
        runs.append(out.cpu().numpy().reshape(n_slabs + 2, ld_slab))
    got = runs[0]
    assert np.array_equal(runs[0], runs[1])
    assert np.all(got[0] == S) and np.all(got[-1] == S) and np.all(got[:, n_cols:] == S)
    want, bound = oo.colsum_slabs(z, n, n_slabs)
    oo.check("colsum_slabs", "slabs", got[1:-1, :n_cols], want, bound)
    rps = -(-n // n_slabs)
    assert np.all(got[1 + -(-n // rps):-1, :n_cols] == 0), "slabs past the data must be exact zeros"


# ----------------------------------------------------------------------------------------------- gs_finalize_step(2)
CW = -7777                                                       # sentinel words between the counters
DELTAS = (2 ** 32 + 5, 3, 2 ** 40 + 1)
START = (10, 2 ** 33, 0)


def _counters(dev):
    return torch.tensor([START[0], CW, START[1], CW, START[2], CW], dtype=torch.int64, device=dev)


def _cargs(ctr, which):
    args = []
    for i in range(3):
        args += [ctr.data_ptr() + 16 * i if i in which else None, DELTAS[i]]
    return args


def _want_counters(which, times=1):
    return [START[0] + times * DELTAS[0] * (0 in which), CW, START[1] + times * DELTAS[1] * (1 in which), CW,
            START[2] + times * DELTAS[2] * (2 in which), CW]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", oo.FINALIZE_N)
def test_finalize_step_loss_and_counters(dev, n, accumulate):
    """gs_finalize_step: loss_out = [loss_out +] scale * sum(rows[0:n]) for n = 0 and around the wave and the workgroup (63, 64,
    255, 256, 257) and 5000; the three counters (adjacent int64 words with sentinel words between them; deltas above 2^32) all
    together, each alone, none.  Rows behind n hold NaN.  Bound: (ceil(n / 256) - 1 + 6 + 2 + 2) u (scale sum|rows| + |loss_out|):
    29 u = 1.7e-6 at n = 5000.  Counters are exact."""
    rng = np.random.RandomState(n)
    rows = rng.random_sample(n).astype(np.float32) * 3
    rows_d = _dev(np.concatenate([rows, np.full(8, np.nan, np.float32)]), dev)
    scale = float(np.float32(1.0 / max(n, 1)))
    for which in ((0, 1, 2), (0,), (1,), (2,), ()):
        out, ctr = _dev(np.asarray([S, 7.0, S], np.float32), dev), _counters(dev)
        _sync()
        ops.call("gs_finalize_step", ops.ptr(rows_d), n, scale, ops.ptr(out[1:2]), accumulate, *_cargs(ctr, which), ops.current_stream())
        _sync()
        got = out.cpu().numpy()
        assert got[0] == S and got[2] == S
        want, bound = oo.scaled_sum(rows, scale, 7.0 if accumulate else None, 256)
        oo.check("finalize_step", "loss", got[1:2], [want], [bound])
        assert ctr.cpu().tolist() == _want_counters(which), which


@pytest.mark.parametrize("n", oo.FINALIZE_N)
def test_finalize_step2_loss_and_aux(dev, n):
    """gs_finalize_step2: a second mean (aux_rows, aux_scale distinct from the loss's) in the same launch; aux only (loss_rows
    null: loss_out untouched), loss only (aux null: aux_out untouched), both; gs_finalize_step with loss_rows null leaves loss_out
    alone and still advances the counters.  Bounds as in test_finalize_step_loss_and_counters (aux never accumulates)."""
    rng = np.random.RandomState(1000 + n)
    rows, aux = rng.random_sample(n).astype(np.float32) * 3, -rng.random_sample(n).astype(np.float32)
    nan8 = np.full(8, np.nan, np.float32)
    rows_d, aux_d = _dev(np.concatenate([rows, nan8]), dev), _dev(np.concatenate([aux, nan8]), dev)
    scale, aux_scale = float(np.float32(1.0 / max(n, 1))), float(np.float32(0.37 / max(n, 1)))
    for use_loss, use_aux in ((1, 1), (0, 1), (1, 0)):
        out, ctr = _dev(np.asarray([S, 7.0, S, -3.0, S], np.float32), dev), _counters(dev)
        _sync()
        ops.call("gs_finalize_step2", ops.ptr(rows_d) if use_loss else None, n, scale, ops.ptr(out[1:2]), 1,
                 ops.ptr(aux_d) if use_aux else None, aux_scale, ops.ptr(out[3:4]), *_cargs(ctr, (0, 1, 2)), ops.current_stream())
        _sync()
        got = out.cpu().numpy()
        assert got[0] == S and got[2] == S and got[4] == S
        if use_loss:
            want, bound = oo.scaled_sum(rows, scale, 7.0, 256)
            oo.check("finalize_step2", "loss", got[1:2], [want], [bound])
        else:
            assert got[1] == 7.0
        if use_aux:
            want, bound = oo.scaled_sum(aux, aux_scale, None, 256)
            oo.check("finalize_step2", "aux", got[3:4], [want], [bound])
        else:
            assert got[3] == -3.0
        assert ctr.cpu().tolist() == _want_counters((0, 1, 2))
    out, ctr = _dev(np.asarray([S, 7.0, S], np.float32), dev), _counters(dev)
    _sync()
    ops.call("gs_finalize_step", None, n, scale, ops.ptr(out[1:2]), 0, *_cargs(ctr, (0, 2)), ops.current_stream())
    _sync()
    assert out.cpu().tolist() == [S, 7.0, S] and ctr.cpu().tolist() == _want_counters((0, 2))


def test_finalize_step_in_a_captured_graph(dev):
    """The launch captured in ops.Graph and replayed 3 times: the counters advance by 3 x delta, the loss is recomputed from the
    rows as they are at each replay (accumulate = 0) and summed over the replays (accumulate = 1)."""
    n = 257
    st = ops.Stream()
    rows_d = torch.zeros(n, dtype=torch.float32, device=dev)
    out, ctr = _dev(np.asarray([S, 7.0, 7.0, S], np.float32), dev), _counters(dev)
    scale = float(np.float32(1.0 / n))
    _sync()
    g = ops.Graph(st.handle)
    g.begin()
    ops.call("gs_finalize_step", ops.ptr(rows_d), n, scale, ops.ptr(out[1:2]), 0, *_cargs(ctr, (0, 1, 2)), st.handle)
    ops.call("gs_finalize_step", ops.ptr(rows_d), n, scale, ops.ptr(out[2:3]), 1, None, 0, None, 0, None, 0, st.handle)
    g.end()
    total, err = 7.0, 0.0
    for it in range(3):
        rows = np.random.RandomState(it).random_sample(n).astype(np.float32) * (it + 1)
        rows_d.copy_(torch.from_numpy(rows))
        _sync()
        g.launch()
        st.sync()
        got = out.cpu().numpy()
        want, bound = oo.scaled_sum(rows, scale, None, 256)
        oo.check("finalize_step", "loss (graph replay)", got[1:2], [want], [bound])
        total, bound = oo.scaled_sum(rows, scale, total, 256)
        err += bound                                               # each replay rounds once more, onto the sum so far
        oo.check("finalize_step", "loss (graph replay, accumulate)", got[2:3], [total], [err])
        assert got[0] == S and got[3] == S
        assert ctr.cpu().tolist() == _want_counters((0, 1, 2), times=it + 1)
