"""-m gpu: the five fused tail kernels -- csrc/gs_tail.hip, gs_tail_dev.h: gs_sage_tail_fwd_bwd[_means], gs_sage_tail_z[_means],
gs_sage_tail_dh0; csrc/gs_unsup_tail.hip: gs_linkpred_tail[_means], gs_linkpred_tail_neg -- against the float64 stage references of tests/tail_oracle.py, at the edge shapes of every mechanism.

Every case
  * reads inputs with ld = round_up(width, 4) + 8 in which EVERYTHING outside the logical operand is NaN: the pad columns of h0,
    W_self, W_neigh, W_head (columns [C, round_up(C, 4)) among them), the labels, dz (gs_sage_tail_dh0) and `means` (means_ready),
    four h0 rows behind row n + n s, the words behind the bias (gcn: one [D, 2 O] matrix, its pad behind column 2 O);
  * writes each output two rows down a sentinel-filled buffer with spare columns, passed as a row-sliced Mat; d_h0's logical block
    is pre-filled with NaN.  Afterwards every stage is finite and inside the bound tail_oracle derives for it (the only
    tolerances here), chained on the values the kernel stored for the stage before; columns [C, round_up(C, 4)) of logits / preds /
    dlogits are exact zeros, masked d_h0 elements exact +0, and every other word still holds the sentinel -- the buffers a form
    must not touch included (`means` under means_ready, z and `means` in the z_ready launch, dz / d_h0 with train = 0);
  * leaves the error word of the hand-over buffer 0 and advances the three device counters exactly once.
tests/test_tail_oracle.py shows on the CPU that these checks pass an fp32 emulation in the kernel's order and reject each planted
fault.  All indices and sizes are in range; n <= 33 and B <= 17, so every workgroup of a launch is resident.

Kernel -> cases
  sage_tail_kernel<D, O, CW, NH>   test_fwd_bwd_sweep ((D, O) x n x s at C = 41 softmax / C = 121 sigmoid: NH = 2 for D = 256),
                                   test_class_sweep ((D, O) x C x loss: round_up(C, 4) / round_up(C, 32) edges, CW = 1 / 2),
                                   test_forms (eval, logits / preds NULL, gcn, z_ready, means_ready, wide logits, buffer reuse)
  sage_tail_z_kernel<D, O>         test_tail_z_and_dh0_sweep (mean, gcn, means_ready), test_forms (split), test_ids_copy
  sage_tail_dh0_kernel<D, O>       test_tail_z_and_dh0_sweep
  sage_lp_tail_kernel<D, O>,       test_linkpred_tail_sweep (B x n_neg x s, the four (D, O) in rotation: train, a second step on the
  lp_neg_tail_kernel<D, O>         same hand-over buffer, eval, aff_all NULL + accumulate, means_ready + no epilogue; neg_slabs,
                                   loss_rows, rr_rows, loss_out, mrr_out in sentinel frames).  The rank is exact on the stored
                                   affinities and inside the interval the affinities derived from y allow.
  the host checks                  test_refusals

Every test prints the worst err / bound it met per stage (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
from graphsage_amd.ops import Mat
import gather_oracle as G
import gemm_oracle as go
import tail_oracle as T
from test_gather_edges_gpu import DevOut, _dev, _sync, _words

pytestmark = pytest.mark.gpu
S = T.SENTINEL
WORST = {}
DELTAS = (3, 5, 7)


@pytest.fixture(autouse=True)
def _print_worst():
    """Prints the largest err / bound per kernel and stage that the test met (pytest -s); a figure, not a check."""
    WORST.clear()
    yield
    for k in sorted(WORST):
        print("\nworst err/bound %-28s %.4f" % (k, WORST[k]), end="")


def _noter(kernel):
    def note(stage, r):
        key = "%s %s" % (kernel, stage)
        WORST[key] = max(WORST.get(key, 0.0), r)
    return note


class Launch(object):
    """A case's operands on the device and a fresh set of framed outputs; `q` is the gs_tail_desc over them."""

    def __init__(self, dev, case, means_in=None, dz_in=None, train=True, sync=None, counters=True):
        self.dev, self.case = dev, case
        n, D, O, C = case.n, case.D, case.O, case.C
        self.h0 = Mat(_dev(case.in_h0(), dev), D)
        wa, wb = case.in_weights()
        if case.gcn:
            W = Mat(_dev(wa, dev), 2 * O)
            self.Ws, self.Wn = W.cols_slice(0, O), W.cols_slice(O, 2 * O)
        else:
            self.Ws, self.Wn = Mat(_dev(wa, dev), O), Mat(_dev(wb, dev), O)
        wh, b, lab = case.in_head()
        self.Wh, self.b, self.lab = Mat(_dev(wh, dev), C), _dev(b, dev), Mat(_dev(lab, dev), C)
        self.out = {k: DevOut(dev, r, w) for k, (r, w) in case.out_shapes().items()}
        self.out["d_h0"].view[:, :D] = float("nan")
        self.loss_rows = torch.full((n + 8,), float(S), device=dev)
        self.means_in = means_in
        if means_in is not None:                       # an INPUT in a NaN frame (kept to compare the bits afterwards)
            big = np.full((n + 4, D + 8), T.NAN, np.float32)
            big[2:2 + n, :D] = means_in
            self.means_big = _dev(big, dev)
            self.means_before = _words(self.means_big)
        if dz_in is not None:
            self.dz_in = Mat(_dev(G.dense(dz_in, case.Z), dev), case.Z)
        self.sync = sync if sync is not None else torch.zeros(ops.tail_sync_words(n, O), dtype=torch.int32, device=dev)
        self.counters = [torch.tensor([100 + i], dtype=torch.int64, device=dev) for i in range(3)] if counters else None
        self.launches = 0
        q = self.q = _lib.TailDesc()
        q.h0, q.ldh, q.n = self.h0.ptr, self.h0.ld, n
        q.W_self, q.ldws, q.W_neigh, q.ldwn = self.Ws.ptr, self.Ws.ld, self.Wn.ptr, self.Wn.ld
        q.W_head, q.ldwh, q.b_head, q.labels, q.ldlab = self.Wh.ptr, self.Wh.ld, self.b.data_ptr(), self.lab.ptr, self.lab.ld
        o = self.out
        if means_in is not None:
            q.means, q.ldm = self.means_big.data_ptr() + 2 * (D + 8) * 4, D + 8
        else:
            q.means, q.ldm = o["means"].mat.ptr, o["means"].mat.ld
        q.z, q.ldz, q.y, q.ldy = o["z"].mat.ptr, o["z"].mat.ld, o["y"].mat.ptr, o["y"].mat.ld
        q.logits, q.ldlo, q.preds, q.ldp = o["logits"].mat.ptr, o["logits"].mat.ld, o["preds"].mat.ptr, o["preds"].mat.ld
        q.dlogits, q.lddl, q.loss_rows = o["dlogits"].mat.ptr, o["dlogits"].mat.ld, self.loss_rows.data_ptr() + 16
        if dz_in is not None:
            q.dz, q.lddz = self.dz_in.ptr, self.dz_in.ld
        else:
            q.dz, q.lddz = o["dz"].mat.ptr, o["dz"].mat.ld
        q.d_h0, q.lddh = o["d_h0"].mat.ptr, o["d_h0"].mat.ld
        if counters:
            (q.c0, q.d0), (q.c1, q.d1), (q.c2, q.d2) = [(c.data_ptr(), d) for c, d in zip(self.counters, DELTAS)]
        q.s, q.d_in, q.out_dim, q.C, q.sigmoid, q.train = case.s, D, O, C, int(case.sigmoid), int(train)
        q.sync, q.gcn = self.sync.data_ptr(), int(case.gcn)
        _sync()

    def call(self, entry="gs_sage_tail_fwd_bwd", counts=True):
        no_jobs = (_lib.GatherDesc * 1)()
        ops.call(entry, ctypes.addressof(self.q), ctypes.addressof(no_jobs), 0, ops.current_stream())
        self.launches += 1 if counts else 0

    def bufs(self):
        _sync()
        b = {k: o.numpy() for k, o in self.out.items()}
        b["loss_rows"] = self.loss_rows.cpu().numpy()
        return b

    def check(self, kernel, stages):
        """The named outputs inside their bounds and frames, every OTHER output untouched, means_ready's input unchanged."""
        bufs = self.bufs()
        got = T.read_outputs(self.case, bufs, stages)
        T.check_stages(self.case, got, stages, means_in=self.means_in, note=_noter(kernel))
        for k, big in bufs.items():
            if k not in stages:
                want = G.out_buffer(*self.case.out_shapes()[k]) if k != "loss_rows" else big * 0 + S
                if k == "d_h0":
                    want[2:2 + self.case.rows, :self.case.D] = T.NAN
                assert np.array_equal(G.bits(big), G.bits(want)), "%s %s: %s must not be touched" % (kernel, self.case.tag(), k)
        if self.means_in is not None:
            assert np.array_equal(_words(self.means_big), self.means_before), "%s: means_ready wrote `means`" % self.case.tag()
        return got

    def check_state(self, epochs=None):
        """Error word 0, the epoch words at `epochs`, the counters advanced once per counted launch."""
        n = self.case.n
        g = (n + 15) // 16
        sync = self.sync.cpu().numpy()
        assert sync[2 * g] == 0, "%s: hand-over error word %d" % (self.case.tag(), sync[2 * g])
        if epochs is not None:
            assert np.all(sync[g:2 * g] == epochs), "%s: epoch words %r, want %d" % (self.case.tag(), sync[g:2 * g], epochs)
        if self.counters:
            for i, (c, d) in enumerate(zip(self.counters, DELTAS)):
                assert int(c.item()) == 100 + i + d * self.launches, "%s: counter %d advanced %d, want %d x %d" % (
                    self.case.tag(), i, int(c.item()) - 100 - i, self.launches, d)


ALL = T.FWD + T.BWD


def _fused_train(dev, case):
    L = Launch(dev, case)
    L.call()
    L.check("fwd_bwd", ALL)
    L.check_state(epochs=1)
    return L


# ================================================================================================== the fused launch
@pytest.mark.parametrize("C,sig", T.SWEEP_HEADS)
@pytest.mark.parametrize("D,O", T.DO)
def test_fwd_bwd_sweep(dev, D, O, C, sig):
    for n in T.N_SWEEP:
        for s in T.S_SWEEP:
            _fused_train(dev, T.Case(D, O, n, s, C, sig))


@pytest.mark.parametrize("sig", [False, True])
@pytest.mark.parametrize("D,O", T.DO)
def test_class_sweep(dev, D, O, sig):
    for C in T.C_SWEEP:
        _fused_train(dev, T.Case(D, O, 17, 2, C, sig))


def _same_bits(a, b, names, tag):
    for k in names:
        G.assert_bits(a[k], b[k], "%s %s" % (tag, k))


@pytest.mark.parametrize("s", [1, 11])
@pytest.mark.parametrize("D,O", [(256, 128), (128, 64)])
def test_forms(dev, D, O, s):
    for C, sig in T.SWEEP_HEADS:
        case = T.Case(D, O, 17, s, C, sig)
        full = _fused_train(dev, case)
        ref = T.read_outputs(case, full.bufs(), ALL)
        # eval: train = 0 with dz / d_h0 GIVEN -- neither is touched
        L = Launch(dev, case, train=False)
        L.call()
        _same_bits(L.check("eval", T.FWD), ref, T.FWD, "eval vs train")
        L.check_state(epochs=1)
        # logits / preds NULL: every other output has the bits of the full launch
        L = Launch(dev, case)
        L.q.logits, L.q.preds = None, None
        L.call()
        rest = tuple(k for k in ALL if k not in ("logits", "preds"))
        got = T.read_outputs(case, L.bufs(), rest)
        _same_bits(got, ref, rest, "logits / preds NULL")
        L.out["logits"].untouched("logits NULL")
        L.out["preds"].untouched("preds NULL")
        L.check_state(epochs=1)
        # split form: gs_sage_tail_z, then z_ready (no hand-over buffer; z and means untouched by the second launch)
        L = Launch(dev, case, counters=False)
        L.q.sync, L.q.z_ready = None, 1
        L.call("gs_sage_tail_z")
        first = L.check("tail_z", ("means", "z"))
        zm = {k: _words(L.out[k].big) for k in ("means", "z")}
        L.call()
        split = L.check("z_ready", ALL)
        for k in zm:
            assert np.array_equal(_words(L.out[k].big), zm[k]), "z_ready wrote %s" % k
        _same_bits(split, ref, ALL, "split vs fused")
        _same_bits(first, ref, ("means", "z"), "gs_sage_tail_z vs fused")
        # means_ready
        L = Launch(dev, case, means_in=ref["means"])
        L.call("gs_sage_tail_fwd_bwd_means")
        _same_bits(L.check("means_ready", tuple(k for k in ALL if k != "means")), ref, tuple(k for k in ALL if k != "means"), "means_ready")
        L.check_state(epochs=1)
        # gcn, and the wide-logits case of this loss
        _fused_train(dev, T.Case(D, O, 17, s, C, sig, gcn=True))
        wide = T.Case(D, O, 17, s, C, sig, wide=True)
        assert np.abs(T.read_outputs(wide, _fused_train(dev, wide).bufs(), ("logits",))["logits"]).max() > 40
        # one hand-over buffer, three launches: the epochs advance by one each, launch 3 has the bits of launch 1
        A = _fused_train(dev, case)
        B = Launch(dev, case, sync=A.sync)
        B.call()
        B.check_state(epochs=2)
        Cc = Launch(dev, case, sync=A.sync)
        Cc.call()
        Cc.check_state(epochs=3)
        _same_bits(Cc.check("fwd_bwd", ALL), ref, ALL, "launch 3 vs launch 1")


# ================================================================================================== the two lean kernels
@pytest.mark.parametrize("D,O", T.DO)
def test_tail_z_and_dh0_sweep(dev, D, O):
    rng = np.random.default_rng(D + O)
    for n in T.N_SWEEP:
        for s in T.S_SWEEP:
            case = T.Case(D, O, n, s, 1, False)
            L = Launch(dev, case, counters=False)
            L.q.sync, L.q.z_ready = None, 1
            L.call("gs_sage_tail_z")
            got = L.check("tail_z", ("means", "z"))
            M = Launch(dev, case, means_in=got["means"], counters=False)
            M.q.sync, M.q.z_ready = None, 1
            M.call("gs_sage_tail_z_means")
            _same_bits(M.check("tail_z_means", ("z",)), got, ("z",), "gs_sage_tail_z_means vs gs_sage_tail_z")
            gcn = T.Case(D, O, n, s, 1, False, gcn=True)
            L = Launch(dev, gcn, counters=False)
            L.q.sync, L.q.z_ready = None, 1
            L.call("gs_sage_tail_z")
            L.check("tail_z gcn", ("means", "z"))
            dz = go.asym(rng, (n, case.Z))
            L = Launch(dev, case, dz_in=dz, counters=False)
            L.q.sync, L.q.z_ready = None, 1
            L.call("gs_sage_tail_dh0")
            bufs = L.bufs()
            got = T.read_outputs(case, bufs, ("d_h0",))
            got["dz"] = dz
            T.check_stages(case, got, ("d_h0",), note=_noter("tail_dh0"))
            for k in bufs:
                if k not in ("d_h0", "loss_rows"):
                    L.out[k].untouched("gs_sage_tail_dh0 %s" % k)


# ================================================================================================== ids_copy
@pytest.mark.parametrize("entry", ["gs_sage_tail_fwd_bwd", "gs_sage_tail_z"])
def test_ids_copy(dev, entry):
    """The helper workgroups' copy of the step's node ids: bit-equal, the words behind it untouched; ignored under z_ready."""
    case = T.Case(128, 64, 17, 2, 41, False)
    helpers = 2 * 2 * 512                                        # G = 2 groups x HP = 2 helper workgroups x 512 threads
    rng = np.random.default_rng(3)
    for count in (0, 1, 511, 512, 513, 2 * helpers + 77):
        src = rng.integers(-2 ** 31, 2 ** 31 - 1, size=count + 8, dtype=np.int64).astype(np.int32)
        src_d, dst_d = _dev(src, dev), torch.full((count + 8,), -77, dtype=torch.int32, device=dev)
        L = Launch(dev, case)
        L.q.ids_copy_src, L.q.ids_copy_dst, L.q.ids_copy_n = src_d.data_ptr(), dst_d.data_ptr(), count
        if entry == "gs_sage_tail_z":
            L.q.z_ready = 1
        L.call(entry)
        _sync()
        dst = dst_d.cpu().numpy()
        assert np.array_equal(dst[:count], src[:count]) and np.all(dst[count:] == -77), "%s ids_copy of %d" % (entry, count)
        L.check("fwd_bwd" if entry == "gs_sage_tail_fwd_bwd" else "tail_z", ALL if entry == "gs_sage_tail_fwd_bwd" else ("means", "z"))
    # the z_ready launch of the split form has no helpers: the copy is gs_sage_tail_z's
    L = Launch(dev, case, counters=False)
    L.q.z_ready = 1
    L.call("gs_sage_tail_z")
    dst_d = torch.full((600,), -77, dtype=torch.int32, device=dev)
    L.q.ids_copy_src, L.q.ids_copy_dst, L.q.ids_copy_n = src_d.data_ptr(), dst_d.data_ptr(), 513
    L.call()
    _sync()
    assert np.all(dst_d.cpu().numpy() == -77), "the z_ready launch copied ids"


# ================================================================================================== the link-prediction tail
class LpLaunch(object):
    """An LpCase's operands on the device, fresh framed outputs and the gs_lp_tail_desc over them."""

    def __init__(self, dev, case, means_in=None, train=True, aff_all=True, sync=None):
        self.dev, self.case, self.means_in = dev, case, means_in
        n, D, O, B, nn = case.n, case.D, case.O, case.B, case.n_neg
        self.h0 = Mat(_dev(case.in_h0(), dev), D)
        wa, wb = case.in_weights()
        self.Ws, self.Wn = Mat(_dev(wa, dev), O), Mat(_dev(wb, dev), O)
        self.out = {k: DevOut(dev, r, w) for k, (r, w) in case.out_shapes().items()}
        self.out["d_h0"].view[:, :D] = float("nan")
        self.vec = {k: torch.full((ln + 8,), float(S), device=dev) for k, ln in case.vec_shapes().items()}
        if means_in is not None:
            big = np.full((n + 4, D + 8), T.NAN, np.float32)
            big[2:2 + n, :D] = means_in
            self.means_big = _dev(big, dev)
            self.means_before = _words(self.means_big)
        self.sync = sync if sync is not None else torch.zeros(ops.lp_tail_sync_words(B, nn), dtype=torch.int32, device=dev)
        self.counters = [torch.tensor([100 + i], dtype=torch.int64, device=dev) for i in range(3)]
        self.launches = 0
        q = self.q = _lib.LpTailDesc()
        o = self.out
        q.h0, q.ldh, q.B, q.n_neg, q.s, q.d_in, q.out_dim, q.train = self.h0.ptr, self.h0.ld, B, nn, case.s, D, O, int(train)
        q.W_self, q.ldws, q.W_neigh, q.ldwn = self.Ws.ptr, self.Ws.ld, self.Wn.ptr, self.Wn.ld
        if means_in is not None:
            q.means, q.ldm = self.means_big.data_ptr() + 2 * (D + 8) * 4, D + 8
        else:
            q.means, q.ldm = o["means"].mat.ptr, o["means"].mat.ld
        q.z, q.ldz, q.y, q.ldy = o["z"].mat.ptr, o["z"].mat.ld, o["y"].mat.ptr, o["y"].mat.ld
        q.dz, q.lddz, q.d_h0, q.lddh = o["dz"].mat.ptr, o["dz"].mat.ld, o["d_h0"].mat.ptr, o["d_h0"].mat.ld
        q.loss_rows, q.rr_rows, q.neg_slabs = [self.vec[k].data_ptr() + 16 for k in ("loss_rows", "rr_rows", "neg_slabs")]
        if aff_all:
            q.aff_all, q.ld_aff = o["aff_all"].mat.ptr, o["aff_all"].mat.ld
        q.neg_weight, q.scale, q.sync = float(case.neg_weight), float(case.scale), self.sync.data_ptr()
        _sync()

    def call1(self, entry="gs_linkpred_tail"):
        no_jobs = (_lib.GatherDesc * 1)()
        ops.call(entry, ctypes.addressof(self.q), ctypes.addressof(no_jobs), 0, ops.current_stream())

    def call2(self, epilogue=True, accumulate=False):
        no_jobs = (_lib.GatherDesc * 1)()
        cs = [(c.data_ptr(), d) for c, d in zip(self.counters, DELTAS)] if epilogue else [(None, 0)] * 3
        ops.call("gs_linkpred_tail_neg", ctypes.addressof(self.q), self.vec["loss_out"].data_ptr() + 16 if epilogue else None,
                 int(accumulate), self.vec["mrr_out"].data_ptr() + 16 if epilogue else None, cs[0][0], cs[0][1], cs[1][0], cs[1][1],
                 cs[2][0], cs[2][1], ctypes.addressof(no_jobs), 0, ops.current_stream())
        self.launches += 1 if epilogue else 0

    def bufs(self):
        _sync()
        b = {k: o.numpy() for k, o in self.out.items()}
        b.update({k: v.cpu().numpy() for k, v in self.vec.items()})
        return b

    def check(self, kernel, stages, prev_loss=None):
        """As Launch.check: the named outputs inside bounds and frames, every other output untouched, the error word 0 and the
        counters advanced once per launch 2 with an epilogue."""
        case, bufs = self.case, self.bufs()
        names = tuple(k for k in stages if k in bufs)
        got = T.lp_read_outputs(case, bufs, names)
        if stages:
            T.lp_check_stages(case, got, stages, means_in=self.means_in, prev_loss=prev_loss, note=_noter(kernel))
        fresh = case.out_buffers()
        for k, big in bufs.items():
            if k not in names:
                assert np.array_equal(G.bits(big), G.bits(fresh[k])), "%s %s: %s must not be touched" % (kernel, case.tag(), k)
        if self.means_in is not None:
            assert np.array_equal(_words(self.means_big), self.means_before), "%s: means_ready wrote `means`" % case.tag()
        assert ops.lp_tail_sync_error(self.sync, case.B, case.n_neg) == 0, "%s: hand-over error word" % case.tag()
        for i, (c, d) in enumerate(zip(self.counters, DELTAS)):
            assert int(c.item()) == 100 + i + d * self.launches, "%s: counter %d" % (case.tag(), i)
        return got


LP_STEP = T.LP_FWD + T.LP_BWD + ("loss_out", "mrr_out")


@pytest.mark.parametrize("B", T.B_SWEEP)
def test_linkpred_tail_sweep(dev, B):
    for D, O, B_, nn, s in T.lp_sweep():
        if B_ != B:
            continue
        case = T.LpCase(D, O, B, nn, s)
        L = LpLaunch(dev, case)
        L.call1()
        L.call2()
        ref = L.check("linkpred", LP_STEP)
        # a second step on the same hand-over buffer: the same bits, no error
        L2 = LpLaunch(dev, case, sync=L.sync)
        L2.call1()
        L2.call2()
        _same_bits(L2.check("linkpred", LP_STEP), ref, LP_STEP, "second step on one sync buffer")
        # eval: dz / d_h0 / neg_slabs are given and not touched
        E = LpLaunch(dev, case, train=False)
        E.call1()
        E.call2()
        ev = T.LP_FWD + ("loss_out", "mrr_out")
        _same_bits(E.check("linkpred eval", ev), ref, ev, "eval vs train")
        # aff_all NULL: the bits of the launch that stores it; accumulate on top of a previous loss; means_ready
        A = LpLaunch(dev, case, aff_all=False)
        A.call1()
        A.vec["loss_out"][4] = 2.5
        A.call2(accumulate=True)
        rest = tuple(k for k in LP_STEP if k not in ("aff_all", "loss_out"))
        got = T.lp_read_outputs(case, A.bufs(), rest + ("loss_out",))
        _same_bits(got, ref, rest, "aff_all NULL")
        A.out["aff_all"].untouched("aff_all NULL")
        r = go.assert_within(got["loss_out"], *T.lp_epilogue(got["loss_rows"], B, 2.5), tag="%s loss_out accumulate" % case.tag())
        _noter("linkpred")("loss_out accumulate", r)
        M = LpLaunch(dev, case, means_in=ref["means"])
        M.call1("gs_linkpred_tail_means")
        M.call2(epilogue=False)                                      # loss_out NULL: no epilogue, no counter
        rest = tuple(k for k in T.LP_FWD + T.LP_BWD if k != "means")
        _same_bits(M.check("linkpred means_ready", rest), ref, rest, "means_ready")


# ================================================================================================== refusals
def test_refusals(dev):
    """Bad arguments come back as an error, nothing is launched and no output word is touched; n = 0 is fine and touches nothing."""
    fb, zz, dh = "gs_sage_tail_fwd_bwd", "gs_sage_tail_z", "gs_sage_tail_dh0"

    def sets(**kw):
        def f(L):
            for k, v in kw.items():
                setattr(L.q, k, v)
        return f

    def plus(field, nbytes):
        return lambda L: setattr(L.q, field, getattr(L.q, field) + nbytes)

    bad = [(e, sets(s=12)) for e in (fb, zz, dh)]
    bad += [(fb, sets(C=0)), (fb, sets(C=129)), (fb, sets(d_in=96)), (zz, sets(d_in=96)), (dh, sets(d_in=96)),
            (fb, sets(out_dim=32)), (zz, sets(out_dim=32)), (dh, sets(out_dim=32)),
            (fb, sets(ldh=128 + 6)), (fb, sets(ldwh=41 + 1)), (zz, sets(ldz=128 + 2)), (dh, sets(lddh=128 + 2)),        # ld % 4 != 0
            (fb, sets(ldh=124)), (fb, sets(ldwh=40)), (fb, sets(ldz=124)), (fb, sets(lddl=40)), (fb, sets(ldlab=40)),
            (fb, sets(ldlo=40)), (fb, sets(lddh=124)), (zz, sets(ldm=124)), (dh, sets(lddz=124)),                       # ld too small
            (fb, plus("h0", 4)), (fb, plus("W_head", 8)), (fb, plus("y", 4)), (zz, plus("z", 4)), (dh, plus("d_h0", 12)),  # alignment
            (fb, sets(sync=None)), (fb, plus("sync", 4)),
            (fb, sets(gcn=1)),                                                            # two matrices: W_neigh != W_self + O
            (dh, sets(gcn=1)),
            (fb, sets(ids_copy_n=5)), (fb, sets(ids_copy_n=-1))]
    case = T.Case(128, 64, 17, 2, 41, False)
    for entry, change in bad:
        L = Launch(dev, case)
        if entry != fb:
            L.q.z_ready = 1
        change(L)
        with pytest.raises(_lib.GraphsageAmdError):
            L.call(entry, counts=False)
        L.check("refused", ())
        L.check_state(epochs=0)
    gcn = T.Case(128, 64, 17, 2, 41, False, gcn=True)
    for entry in ("gs_sage_tail_fwd_bwd_means", "gs_sage_tail_z_means"):                  # the gcn form computes its own means
        L = Launch(dev, gcn)
        with pytest.raises(_lib.GraphsageAmdError):
            L.call(entry, counts=False)
        L.check("refused", ())
        L.check_state(epochs=0)
    lp = T.LpCase(128, 64, 9, 5, 2)
    for change in (sets(s=12), sets(n_neg=0), sets(n_neg=33), sets(d_in=96), sets(out_dim=32), sets(B=0), sets(ldz=124), sets(ldh=128 + 2),
                   plus("z", 4), plus("neg_slabs", 4), sets(sync=None), sets(rr_rows=None), sets(ld_aff=5)):
        for second in (False, True):
            L = LpLaunch(dev, lp)
            change(L)
            with pytest.raises(_lib.GraphsageAmdError):
                L.call2() if second else L.call1()
            L.launches = 0
            L.check("refused", ())
    L = LpLaunch(dev, lp)                                          # loss_out without mrr_out
    no_jobs = (_lib.GatherDesc * 1)()
    with pytest.raises(_lib.GraphsageAmdError):
        ops.call("gs_linkpred_tail_neg", ctypes.addressof(L.q), L.vec["loss_out"].data_ptr() + 16, 0, None, None, 0, None, 0, None, 0,
                 ctypes.addressof(no_jobs), 0, ops.current_stream())
    L.check("refused", ())
    for entry in (fb, zz, dh):
        L = Launch(dev, case)
        L.q.n = 0
        L.call(entry, counts=False)
        L.check("n = 0", ())
        L.check_state(epochs=0)
