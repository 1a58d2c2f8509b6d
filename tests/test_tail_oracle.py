"""CPU checks of tests/tail_oracle.py, the float64 stage references and bounds tests/test_tail_edges_gpu.py holds the fused tails
(supervised and link-prediction) to.  An np.float32 emulation of every stage in the kernel's order -- ordered neighbor sum, eight
K-slices summed in wave order, the per-lane chains and the tail_wave_sum tree, the logits' K-slices added to the bias in order; for
the link-prediction tail the pair phase, the per-main slabs, their sum in main order and the step epilogue -- lies inside every
bound at every shape of the GPU sweep; the rank intervals of every link-prediction case are decided; and each planted fault is
rejected by the very checks the GPU test runs (tail_oracle.read_outputs / check_stages, lp_read_outputs / lp_check_stages)."""
import numpy as np
import pytest

import gemm_oracle as go
import tail_oracle as T

F = np.float32
LOG2E, LN2 = F(1.4426950408889634), F(0.6931471805599453)


def r32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def fma(a, b, c):
    return r32(go.f64(a) * go.f64(b) + go.f64(c))


def lanes(a, fill):
    """[n, W] -> [ceil(W / 64), n, 64]: element [m, i, l] is column l + 64 m (fill beyond W)."""
    n, W = a.shape
    nj = -(-W // 64)
    p = np.full((n, 64 * nj), fill, np.float32)
    p[:, :W] = a
    return p.reshape(n, nj, 64).transpose(1, 0, 2)


def unlanes(v, W):
    return v.transpose(1, 0, 2).reshape(v.shape[1], -1)[:, :W]


def butterfly(v, op):
    """tail_wave_sum / tail_wave_max: xor 1, 2, 4, 8 inside each row of 16 lanes, then (r0 op r1) op (r2 op r3).  v [n, 64]."""
    for off in (1, 2, 4, 8):
        v = op(v, v[:, np.arange(64) ^ off])
    return op(op(v[:, 0], v[:, 16]), op(v[:, 32], v[:, 48]))


def kslices(A, B, nk):
    K = A.shape[1]
    return [go.chain(A, B, ks=range(w * K // nk, (w + 1) * K // nk)) for w in range(nk)]


def expf(a):
    """__expf: v_exp_f32 of the rounded product with log2(e)."""
    with np.errstate(under="ignore"):
        return r32(np.exp2(go.f64(a * LOG2E)))


def logf(a):
    return r32(np.log2(go.f64(a))) * LN2


def rcp(a):
    return r32(1.0 / go.f64(a))


def emu_mean_z(case, fault=None):
    """The z helpers: ordered neighbor sum (+ self, gcn), eight K-slices per half summed in wave order -> (means, z)."""
    n, s, D = case.n, case.s, case.D
    h0 = case.h0
    nb = h0[n:].reshape(n, s, D)
    acc = np.zeros((n, D), F)
    for j in range(s - 1 if fault == "drop_last_neighbor" else s):
        acc = acc + nb[:, j]
    if case.gcn:
        mean = (acc + h0[:n]) * (F(1) / F(s if fault == "gcn_inv_s" else s + 1))
    else:
        mean = acc * (F(1) / F(s))
    Ws, Wn = (case.Wn, case.Ws) if fault == "swap_w" else (case.Ws, case.Wn)
    halves = []
    for A, W in ((mean if case.gcn else h0[:n], Ws), (mean, Wn)):
        parts = kslices(A, W, 8)
        v = parts[0]
        for p in parts[1:]:
            v = v + p
        halves.append(v)
    return mean, np.concatenate(halves, axis=1)


def dots(a, b):
    """Row-wise <a, b>: one fma chain per lane over the 64-column groups, then the wave tree."""
    al, bl = lanes(a, 0), lanes(b, 0)
    acc = np.zeros((a.shape[0], 64), F)
    for m in range(al.shape[0]):
        acc = fma(al[m], bl[m], acc)
    return butterfly(acc, np.add)


def emu_l2norm(z):
    """tail_l2norm_row -> (y, inv)."""
    inv = r32(1.0 / np.sqrt(go.f64(np.maximum(dots(z, z), F(1e-12)))))
    return z * inv[:, None], inv


def emu_l2bwd(g, y, inv, fault=None):
    """tail_l2norm_bwd_row."""
    dot = dots(g, y)[:, None]
    clamped = (inv >= F(1.0e6))[:, None] & (fault != "no_clamp")
    return np.where(clamped, g * inv[:, None], inv[:, None] * (g - y * dot))


def emu_dh0(case, dz, fault=None):
    s, O, n = case.s, case.O, case.n
    d_self, d_mean = go.chain(dz[:, :O], np.ascontiguousarray(case.Ws.T)), go.chain(dz[:, O:], np.ascontiguousarray(case.Wn.T))
    if case.gcn:
        d_self = (d_self + d_mean) * (F(1) / F(s + 1))
        d_mean = d_self
    else:
        d_mean = d_mean * (F(1) / F(s))
    mask = case.h0 >= 0 if fault == "mask_ge" else case.h0 > 0
    if fault == "mask_self":
        mask[n:] = np.repeat(mask[:n], s, axis=0)
    return np.where(mask, np.concatenate([d_self, np.repeat(d_mean, s, axis=0)]), F(0))


def store(bufs, k, v, row0=2):
    bufs[k][row0:row0 + v.shape[0], :v.shape[1]] = v
    bufs[k][row0:row0 + v.shape[0], v.shape[1]:T.rup(v.shape[1], 4)] = 0


def emulate(case, fault=None, train=True):
    """One fused launch in np.float32, written into case.out_buffers() as the kernel stores it."""
    n, C = case.n, case.C
    mean, z = emu_mean_z(case, fault)
    y, inv = emu_l2norm(z)
    # phases 3-4
    nks = 4 if C <= 64 else 2
    x = np.broadcast_to(case.b, (n, C)).astype(F)
    for p in kslices(y, case.Wh, nks):
        x = x + p
    lab = case.labels.copy()
    if fault == "label_row":
        lab[n - 2] = lab[n - 1]
    inv_n, inv_c = F(1) / F(n), F(1) / F(C)
    xl, ll = lanes(x, 0), lanes(lab, 0)
    inside = lanes(np.ones((n, C), F), 0) > 0
    CW = xl.shape[0]
    if case.sigmoid:
        e = expf(-np.abs(xl))
        term = np.zeros((n, 64), F)
        for m in range(CW):
            t = np.maximum(xl[m], F(0)) - xl[m] * ll[m] + logf(F(1) + e[m])
            term = term + np.where(inside[m], t, F(0))
        r1 = rcp(F(1) + e)
        pr = np.where(xl >= 0, r1, e * r1)
        gl = (pr - ll) * (inv_n * inv_c)
        loss = butterfly(term, np.add) * inv_c
    else:
        mx = butterfly(np.where(inside, xl, -np.inf).max(axis=0), np.maximum)
        ex = np.where(inside, expf(xl - mx[None, :, None]), F(0))
        sel, zsl, zxl = np.zeros((n, 64), F), np.zeros((n, 64), F), np.zeros((n, 64), F)
        for m in range(CW):
            em = ex[m].copy()
            if fault == "last_class" and (C - 1) // 64 == m:
                em[:, (C - 1) % 64] = 0
            sel, zsl, zxl = sel + em, zsl + ll[m], fma(ll[m], xl[m], zxl)
        se, zs, zx = butterfly(sel, np.add), butterfly(zsl, np.add), butterfly(zxl, np.add)
        pr = ex * rcp(se)[None, :, None]
        gl = (pr * zs[None, :, None] - ll) * inv_n
        loss = zs * (mx + logf(se)) - zx
    preds, dl = unlanes(pr, C), unlanes(gl, C)
    bufs = case.out_buffers()
    store(bufs, "means", mean)
    store(bufs, "z", z)
    store(bufs, "y", y, 3 if fault == "store_low" else 2)
    store(bufs, "logits", x)
    store(bufs, "preds", preds)
    store(bufs, "dlogits", dl)
    bufs["loss_rows"][4:4 + n] = loss
    if not train:
        return bufs
    dy = go.chain(dl, np.ascontiguousarray(case.Wh.T))
    if fault == "pad_nan" and C % 4:
        dy = dy + F(0) * T.NAN
    dz = emu_l2bwd(dy, y, inv, fault)
    store(bufs, "dz", dz)
    store(bufs, "d_h0", emu_dh0(case, dz, fault))
    return bufs


def check(case, bufs, train=True):
    stages = T.FWD + (T.BWD if train else ())
    return T.check_stages(case, T.read_outputs(case, bufs, stages), stages)


# ------------------------------------------------------------------------------------------------ the emulation passes
@pytest.mark.parametrize("D,O", T.DO)
def test_emulation_inside_every_bound_fwd_bwd_sweep(D, O):
    worst = {}
    for C, sig in T.SWEEP_HEADS:
        for n in T.N_SWEEP:
            for s in T.S_SWEEP:
                case = T.Case(D, O, n, s, C, sig)
                for k, r in check(case, emulate(case)).items():
                    worst[k] = max(worst.get(k, 0.0), r)
    print("\nfp32 emulation, worst err/bound:", " ".join("%s %.3f" % kv for kv in sorted(worst.items())), end="")


@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("D,O", T.DO)
def test_emulation_inside_every_bound_class_sweep(D, O, sig):
    for C in T.C_SWEEP:
        case = T.Case(D, O, 17, 2, C, sig)
        check(case, emulate(case))


@pytest.mark.parametrize("D,O", [(256, 128), (128, 64)])
@pytest.mark.parametrize("s", [1, 11])
def test_emulation_inside_every_bound_forms(D, O, s):
    for C, sig in T.SWEEP_HEADS:
        check(T.Case(D, O, 17, s, C, sig), emulate(T.Case(D, O, 17, s, C, sig), train=False), train=False)
        gcn = T.Case(D, O, 17, s, C, sig, gcn=True)
        check(gcn, emulate(gcn))
        wide = T.Case(D, O, 17, s, C, sig, wide=True)
        bufs = emulate(wide)
        check(wide, bufs)
        assert np.abs(bufs["logits"][2:19, :C]).max() > 40, "the wide case must reach |logit| of about 50"


def test_cases_hold_what_the_edge_tests_rely_on():
    case = T.Case(128, 64, 17, 2, 41, False)
    n, s = case.n, case.s
    h0 = case.h0
    assert np.all(h0 >= 0) and np.signbit(h0).any() and ((h0 > 0) & (h0 < 2.0 ** -126)).any() and (h0 == 0).any()
    assert not h0[n - 1].any() and not h0[n + (n - 1) * s:].any()                      # the zero root
    z = T.z(case, T.means(case)[0])[0]
    ss = (z * z).sum(axis=1)
    assert ss[n - 1] == 0 and 0 < ss[n - 2] < 1e-3 * T.CLAMP and np.all(ss[:n - 2] > 1e3 * T.CLAMP)     # no row near the clamp
    assert not case.labels[0].any() and abs(case.labels[1].sum() - 1) > 0.1 and np.all(case.labels[2:].sum(axis=1) == 1)
    Wh = case.in_head()[0]
    assert Wh.shape[1] == T.rup(case.C, 4) + 8 and np.isnan(Wh[:, case.C:]).all() and np.isfinite(Wh[:, :case.C]).all()
    assert np.isnan(case.in_h0()[-4:]).all() and np.isnan(case.in_h0()[:, case.D:]).all()


# ------------------------------------------------------------------------------------------------ planted faults
FAULTS = ["drop_last_neighbor", "swap_w", "last_class", "label_row", "mask_self", "mask_ge", "no_clamp", "pad_nan", "store_low"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_rejected(fault):
    case = T.Case(128, 64, 17, 2, 41, False)
    assert not np.array_equal(case.labels[case.n - 2], case.labels[case.n - 1])
    check(case, emulate(case))
    with pytest.raises(AssertionError):
        check(case, emulate(case, fault))


def test_planted_gcn_scale_is_rejected():
    case = T.Case(128, 64, 17, 2, 41, False, gcn=True)
    check(case, emulate(case))
    with pytest.raises(AssertionError):
        check(case, emulate(case, "gcn_inv_s"))


def test_last_class_fault_is_rejected_with_two_class_groups():
    case = T.Case(128, 64, 17, 2, 121, False)
    with pytest.raises(AssertionError):
        check(case, emulate(case, "last_class"))


# ================================================================================================ the link-prediction tail
def sigmoid_lg(x):
    e = expf(-np.abs(x))
    r = rcp(F(1) + e)
    return np.where(x >= 0, r, e * r), logf(F(1) + e)


def wave_sum_cols(a):
    """tail_wave_sum of one value per lane: a [rows, <= 64]."""
    p = np.zeros((a.shape[0], 64), F)
    p[:, :a.shape[1]] = a
    return butterfly(p, np.add)


def emulate_lp(case, fault=None, train=True, prev_loss=None):
    """gs_linkpred_tail + gs_linkpred_tail_neg in np.float32, written into case.out_buffers()."""
    B, nn, Z, GP = case.B, case.n_neg, case.Z, case.GP
    mean, z = emu_mean_z(case)
    y, inv = emu_l2norm(z)
    y1, y2, ng = y[:B], y[B:2 * B], y[2 * B:]
    aff = dots(y1, y2)
    nav = np.stack([dots(y1, np.broadcast_to(ng[q], y1.shape)) for q in range(nn)], axis=1)
    sa, lga = sigmoid_lg(aff)
    sg, lg = sigmoid_lg(nav)
    nw = F(1) if fault == "no_neg_weight" else case.neg_weight
    loss = (np.maximum(aff, F(0)) - aff + lga) + nw * wave_sum_cols(np.maximum(nav, F(0)) + lg)
    rr = F(1) / ((nav >= aff[:, None]).sum(axis=1) + 1).astype(F)
    bufs = case.out_buffers()
    store(bufs, "means", mean)
    store(bufs, "z", z)
    store(bufs, "y", y)
    bufs["aff_all"][2:2 + B, :nn + 1] = np.concatenate([nav, aff[:, None]], axis=1)
    bufs["loss_rows"][4:4 + B], bufs["rr_rows"][4:4 + B] = loss, rr
    inv_b = F(1) / F(B)
    tot = wave_sum_cols(loss[None, :] if B <= 64 else None)[0]           # (B <= 17 here: one row per lane of the first wave)
    bufs["loss_out"][4] = tot * inv_b if prev_loss is None else F(prev_loss) + tot * inv_b
    bufs["mrr_out"][4] = wave_sum_cols(rr[None, :])[0] * inv_b
    if not train:
        return bufs
    da = (sa - F(1)) * case.scale
    gq = case.neg_weight * case.scale * sg
    g1 = da[:, None] * y2
    for q in range(nn):
        g1 = fma(gq[:, q, None], ng[q][None, :], g1)
    dz = np.zeros((case.n, Z), F)
    dz[:B] = emu_l2bwd(g1, y1, inv[:B])
    dz[B:2 * B] = emu_l2bwd(da[:, None] * y1, y2, inv[B:2 * B])
    slabs = np.zeros((GP, nn, Z), F)
    for g in range(GP):
        for p in range(8 * g, min(8 * g + 8, B)):
            slabs[g] = fma(gq[p][:, None], y1[p][None, :], slabs[g])
    bufs["neg_slabs"][4:4 + slabs.size] = slabs.reshape(-1)
    # launch 2
    gsum = np.zeros((nn, Z), F)
    for g in range(GP - 1 if fault == "drop_last_slab" else GP):
        gsum = gsum + slabs[g]
    zv = z[2 * B:]

    def lane4(a, b):                       # lane l holds columns 4 l .. 4 l + 3: (x x' + y y') + (z z' + w w')
        p = (a * b).reshape(nn, Z // 4, 4)
        return (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])
    ninv = r32(1.0 / np.sqrt(go.f64(np.maximum(wave_sum_cols(lane4(zv, zv)), F(1e-12)))))[:, None]
    dot = wave_sum_cols(lane4(gsum, zv) * ninv)[:, None]
    dz[2 * B:] = np.where(ninv >= F(1.0e6), gsum * ninv, (gsum - zv * (ninv * dot)) * ninv)
    store(bufs, "dz", dz)
    store(bufs, "d_h0", emu_dh0(case, dz))
    return bufs


LP_ALL = T.LP_FWD + T.LP_BWD + ("loss_out", "mrr_out")


def check_lp(case, bufs, train=True, prev_loss=None):
    stages = T.LP_FWD + (T.LP_BWD if train else ()) + ("loss_out", "mrr_out")
    return T.lp_check_stages(case, T.lp_read_outputs(case, bufs, stages), stages, prev_loss=prev_loss)


def test_lp_emulation_inside_every_bound_and_ranks_are_decided():
    """The emulation passes at every shape of the GPU sweep; and, on the reference alone, at most one pair in eight of any case has
    a rank interval wider than one rank (rr_rows is discrete: a case whose ranks the bounds cannot decide would check nothing)."""
    worst = {}
    for D, O, B, nn, s in T.lp_sweep():
        case = T.LpCase(D, O, B, nn, s)
        bufs = emulate_lp(case)
        for k, r in check_lp(case, bufs).items():
            worst[k] = max(worst.get(k, 0.0), r)
        y = T.l2norm(T.z(case, T.means(case)[0])[0].astype(np.float32))[0]
        lo, hi = T.rank_interval(*T.affinities(case, y))
        assert 8 * int((hi - lo > 1).sum()) <= B, "%s: %d of %d rank intervals wider than one rank" % (case.tag(), int((hi - lo > 1).sum()), B)
    print("\nfp32 emulation, worst err/bound:", " ".join("%s %.3f" % kv for kv in sorted(worst.items())), end="")


def test_lp_emulation_eval_and_accumulate():
    case = T.LpCase(128, 64, 9, 5, 11)
    check_lp(case, emulate_lp(case, train=False), train=False)
    check_lp(case, emulate_lp(case, prev_loss=2.5), prev_loss=2.5)


@pytest.mark.parametrize("fault", ["no_neg_weight", "drop_last_slab"])
def test_lp_planted_fault_is_rejected(fault):
    case = T.LpCase(128, 64, 9, 5, 2)          # two mains: two slabs
    check_lp(case, emulate_lp(case))
    with pytest.raises(AssertionError):
        check_lp(case, emulate_lp(case, fault))
