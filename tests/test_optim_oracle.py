"""CPU checks of tests/optim_oracle.py, the yardstick of test_optim_gpu.py and test_elementwise_edges_gpu.py: the Adam
restatement against the project's oracle, every "past the cap" shape against the cap it is meant to exceed, and the oracle
finite and non-degenerate on every input the GPU tests feed it (no GPU test excludes an element from a comparison)."""
import numpy as np
import pytest

from oracle import graphsage_oracle as orc
import optim_oracle as oo

# launch caps and batch sizes of the kernels under test, restated (a changed cap must fail here, not silently untest a loop)
ADAM_CAP = 2048 * 256            # gs_optim.hip gs_adam_step: min(ceil(count / 256), 2048) blocks of 256 threads, one float each
FLAT_CAP = 4096 * 256            # gs_optim.hip flat_reduce_adam_impl: min(ceil(total4 / GS_OPT_THREADS), 4096) blocks, one float4 each
REDUCE_CAP = 4096 * 32           # gs_optim.hip gs_reduce_slabs: min(ceil(total / 32), 4096) blocks of 32 outputs
REDUCE_TRIP = 8 * 16             # gs_optim.hip reduce_slabs_kernel: `z0 += 8 * 16`, 128 slabs per trip of the loop
OPT_SLAB_BATCH = 24              # gs_optim.hip #define GS_OPT_SLAB_BATCH 24
MAX_VARS = 24                    # gs_optim.hip #define GS_MAX_VARS 24
MEAN_BWD_CAP = 2048 * 256        # gs_gather.hip gs_mean_bwd: min(ceil(total / 256), 2048) blocks, one float4 each
ACT_BWD_CAP = 2048 * 256         # gs_gemm.hip gs_act_bwd: min(ceil(total / 256), 2048)
PULL_CAP = 4096 * 256            # gs_gather.hip gs_input_grad_pull: min(ceil(total / 256), 4096)
SEGMAX_FWD_CAP = 4096 * 256      # gs_head.hip gs_segment_max_fwd: min(ceil(total / 256), 4096)
SEGMAX_BWD_CAP = 8192 * 256      # gs_head.hip gs_segment_max_bwd: min(ceil(total / 256), 8192)
WAVE4 = 64                       # float4 per wave of the flat launch


def test_adam_equals_the_projects_oracle_on_fp32_inputs():
    """oo.adam == orc.clip_by_value + orc.adam_tf_update run in fp32, to fp32 rounding, at gscale = 1, clip = 5, over 3 steps.
    One constant differs by more than a rounding and is allowed for by its own size: the kernel (and TF, whose beta is an
    fp32 tensor) forms 1 - fp32(beta), orc.adam_tf_update forms fp32(1 - beta).  For beta2 = 0.999 these are 0.00099998713 and
    0.0010000000475: d2 = 1.3e-5 relative, on v's second term, on 1 - beta2^t in lr_t and (halved) on sqrt(v); for beta1 = 0.9,
    d1 = 2.2e-7.  So m within (4 u + d1) and v within (6 u + d2) of the sum of their two terms' magnitudes, the step q (formed
    from the fp32 run's own moments) within (d2 + 2 d1 + 16 u) |q| + u |p|."""
    rng = np.random.RandomState(1)
    n = 4096
    p = rng.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    d1 = abs(np.float64(np.float32(0.1)) - (1 - oo.f32(0.9))) / 0.1
    d2 = abs(np.float64(np.float32(0.001)) - (1 - oo.f32(0.999))) / 0.001
    assert d1 < 2.3e-7 and 1.2e-5 < d2 < 1.4e-5
    for t in (1, 2, 3):
        g = (rng.standard_normal(n) * 8).astype(np.float32)
        assert (np.abs(g) > 5).any() and (np.abs(g) < 5).any()
        p1, m1, v1, q, bm, bv = oo.adam(p, g, m, v, float(t), clip=5.0, gscale=1.0, **oo.HYPER)
        p_before = p.copy()
        orc.adam_tf_update(p, orc.clip_by_value(g), m, v, t, 0.01)              # in place, fp32
        assert (np.abs(m - m1) <= bm * (1 + d1 / (4 * oo.U))).all()            # bm, bv: roundings x the terms' magnitudes
        assert (np.abs(v - v1) <= bv * (1 + d2 / (6 * oo.U))).all()
        q, _ = oo.adam_step_size(m, v, float(t), **oo.HYPER)                   # from the moments the fp32 run holds, as the GPU tests do
        err = np.abs((p.astype(np.float64) - p_before) + q)
        assert (err <= (d2 + 2 * d1 + 16 * oo.U) * np.abs(q) + oo.U * np.abs(p1)).all(), err.max()
        assert (bm >= 0).all() and (bv >= 0).all()


def test_every_past_the_cap_shape_exceeds_its_cap():
    L = oo.FLAT_LAYOUTS["past_cap"]
    q = [s // 4 for s in L["sizes"]]
    assert q[0] > FLAT_CAP and q[0] - FLAT_CAP < WAVE4 * 4 and sum(q) < 2 * FLAT_CAP      # a second, partial trip ...
    assert (sum(q) - 1) // WAVE4 == q[0] // WAVE4                                           # ... whose last wave spans both variables
    assert max(oo.ADAM_COUNTS) > ADAM_CAP and max(oo.ADAM_COUNTS) % 256 != 0 and min(oo.ADAM_COUNTS) == 1
    ks = oo.FLAT_LAYOUTS["straddle"]["n_slabs"]
    assert {0, 1, OPT_SLAB_BATCH, OPT_SLAB_BATCH + 1, 2 * OPT_SLAB_BATCH + 1} <= set(ks)
    assert len(oo.FLAT_LAYOUTS["vars24"]["sizes"]) == MAX_VARS
    assert all(4 <= s <= 68 and s % 4 == 0 for s in oo.FLAT_LAYOUTS["vars24"]["sizes"])
    for L in oo.FLAT_LAYOUTS.values():
        assert all(s % 4 == 0 and s > 0 for s in L["sizes"])
        assert all(k == 1 for k, c in zip(L["n_slabs"], L["clear"]) if c)
    # the straddle layout: some wave holds pieces of >= 3 variables, and some variable boundary is not a multiple of 64 float4
    off = np.cumsum([0] + oo.FLAT_LAYOUTS["straddle"]["sizes"]) // 4
    per_wave = [len({int(np.searchsorted(off, qq, side="right")) for qq in range(w * WAVE4, min((w + 1) * WAVE4, off[-1]))})
                for w in range(-(-int(off[-1]) // WAVE4))]
    assert max(per_wave) >= 3 and any(o % WAVE4 for o in off[1:-1])
    assert max(oo.REDUCE_SLAB_COUNTS) > 2 * REDUCE_TRIP and {REDUCE_TRIP - 1, REDUCE_TRIP, REDUCE_TRIP + 1} <= set(oo.REDUCE_SLAB_COUNTS)
    assert (oo.REDUCE_SMALL[0] * oo.REDUCE_SMALL[1]) % 32 != 0
    assert oo.REDUCE_BIG[0] * oo.REDUCE_BIG[1] > REDUCE_CAP
    d4 = (oo.CAP_D + 3) // 4
    assert d4 == 2
    assert oo.CAP_MEAN_BWD[0] * oo.CAP_MEAN_BWD[1] * d4 > MEAN_BWD_CAP
    assert oo.CAP_ACT_BWD * d4 > ACT_BWD_CAP
    assert oo.CAP_PULL_ROWS * d4 > PULL_CAP
    assert oo.CAP_SEGMAX_FWD[0] * d4 > SEGMAX_FWD_CAP
    assert oo.CAP_SEGMAX_BWD[0] * oo.CAP_SEGMAX_BWD[1] * d4 > SEGMAX_BWD_CAP
    # colsum: more than one column tile of 64, slabs past the data, slices too short for the 8-deep loop (< 32 rows) and not
    assert any(c > 64 for _, c, _, _ in oo.COLSUM_CASES) and any(n < k for n, _, k, _ in oo.COLSUM_CASES)
    assert any(-(-n // k) < 32 for n, _, k, _ in oo.COLSUM_CASES) and any(-(-n // k) > 64 for n, _, k, _ in oo.COLSUM_CASES)


def test_bias_correction_bound_stays_under_the_projects_tolerance():
    """The derived bound of the Adam update (oo.adam_step_size) at the steps the GPU tests use, t = 7 .. 10 and 2^33: 77 u .. 61 u
    (+ 4), times LIB = 4: 1.9e-5 and below, a fifth of the project's 1e-4; at t = 2^33 powf underflows to 0 and 8.5 u remain."""
    for t, want in ((7.0, 77.0), (8.0, 68.0), (9.0, 61.0), (10.0, 55.0), (float(np.float32(2 ** 33 + 3)), 4.5)):
        r = oo.adam_lr_t_roundings(t, 0.9, 0.999)
        assert abs(r - want) < 1.0, (t, r)
        assert oo.LIB * (r + 4) * oo.U < 2e-5
    assert oo.adam_t(2 ** 33 + 3, 0) == 2.0 ** 33 and np.isfinite(oo.adam_lr_t(2.0 ** 33, **{k: oo.HYPER[k] for k in ("lr", "b1", "b2")}))


def test_the_oracle_is_finite_and_non_degenerate_on_the_chosen_inputs():
    for name in oo.FLAT_LAYOUTS:
        L = oo.FLAT_LAYOUTS[name]
        p0, slabs = oo.flat_inputs(name)
        off = 0
        big = small = 0
        for sz, k, dec, sl in zip(L["sizes"], L["n_slabs"], L["decay"], slabs):
            g, b = oo.flat_grad(sl[:k], p0[off:off + sz], 0.01, dec)
            assert np.isfinite(g).all() and np.isfinite(b).all()
            assert k == 0 or (b > 0).all()
            big, small = big + int((np.abs(g) > 5).sum()), small + int((np.abs(g) < 5).sum())
            p1, m1, v1, q, bm, bv = oo.adam(p0[off:off + sz], g, 0 * g, 0 * g, 8.0, clip=5.0, gscale=1.0, **oo.HYPER)
            assert np.isfinite(p1).all() and np.isfinite(q).all() and (k == 0 and not dec or (v1 > 0).all())
            off += sz
        assert name == "vars24" or (big > 0 and small > 0), "the clip of 5 must cut some gradients and spare others"
    for d in oo.WIDTHS:
        for n in oo.ROWS:
            x = oo.l2_rows(n, d, d)
            y, inv, cache, by, binv = oo.l2norm_fwd(x)
            ss = cache[2][:, 0]
            assert np.isfinite(y).all() and np.isfinite(inv).all() and float(np.float32(ss.max())) < 3e38
            assert ss[n - 1] == 0 and (n < 2 or 0 < ss[n - 2] < 1e-12 * (1 - 2.0 ** -11))
            assert n < 3 or 1e-12 * (1 + 2.0 ** -11) < ss[n - 3] < 1.1e-12
            assert n < 4 or abs(np.sqrt(ss[n - 4]) / 1e18 - 1) < 1e-6
            dy = np.random.RandomState(d + 1).standard_normal((n, d)).astype(np.float32)
            dx, bdx = oo.l2norm_bwd(dy, y.astype(np.float32), inv.astype(np.float32), ss)
            assert np.isfinite(dx).all() and np.isfinite(bdx).all()
    for C in oo.CLASSES:
        for sig in (True, False):
            for n in oo.ROWS:
                x, z = oo.class_inputs(n, C, sig, C)
                r = oo.class_loss(x, z, sig)
                assert all(np.isfinite(v).all() for v in r.values())
                assert (r["b_loss"] > 0).all() and (r["b_preds"] > 0).all() and (r["b_dlogits"] > 0).all()
                assert (r["b_loss"] <= 1e-4 * np.maximum(1.0, np.abs(x).max())).all(), "the derived bound must stay under the project's"
            x, z = oo.class_inputs(257, C, sig, C)
            assert np.abs(x).max() == 200 and (C == 1 or {30.0, 88.0, 200.0} <= set(np.abs(x).reshape(-1).tolist()))
            if not sig and C > 1:
                zs = z.sum(axis=1)
                assert (zs == 0).any() and (zs == 1).any() and (zs > 1).any()


@pytest.mark.parametrize("n,n_slabs", [(777, 5), (5, 8), (1, 1)])
def test_colsum_slabs_oracle_partitions_the_rows(n, n_slabs):
    Z = np.random.RandomState(n).standard_normal((n + 3, 9))
    out, b = oo.colsum_slabs(Z, n, n_slabs)
    np.testing.assert_allclose(out.sum(axis=0), Z[:n].sum(axis=0), rtol=1e-12, atol=1e-12)
    rps = -(-n // n_slabs)
    assert (out[-(-n // rps):] == 0).all() and (b >= 0).all()
