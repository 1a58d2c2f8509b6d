"""-m gpu: the gather + segmented mean (gather_mean_wave, csrc/gs_gather_dev.h) at edge shapes -- stand-alone, and riding as extra
workgroups in every launch that hosts it -- and gs_segment_max_gather_fwd, against tests/gather_oracle.py.

Every case
  * reads tables with ld = round_up(d, 4) + 8 in which EVERYTHING outside the logical operand is NaN: pad columns, table rows no
    index points at (a quarter of each table), the rows behind a contiguous operand;
  * writes each output two rows down a sentinel-filled buffer with spare columns, passed as a row-sliced Mat: afterwards the
    logical block has the BITS of gather_oracle.ordered_f32 (acc = +0; += X[idx[j]], j = 0..s-1; += self; *= fp32(1) / fp32(cnt)) and lies
    inside the float64 bound of gemm_oracle.gather_mean, columns [d, round_up(d, 4)) are exact zeros and every other word still holds
    the sentinel (gather_oracle.Job.check / read_block: the checks tests/test_gather_oracle.py shows each planted fault to fail).
Dropout (gs_gather_mean_dropout_fwd) is held to gather_oracle.gather_mean_dropout's bound only (one rounding more per kept
element; fma contraction may differ between the batch forms).  No other tolerance appears here.  All indices are in range.

Host -> cases (loads in flight U, UBIG; waves per workgroup).  Every rider host runs the three job lists of gather_oracle.JOB_LISTS --
`six` (GS_MAX_COJOBS_S jobs, 29 waves: s = 1 / 7 / 13 / 25 / 26 / 77, 1 / 2 / 3 / 5 chunks, self by index / by position, contiguous;
boundaries inside a workgroup of 4 and of 8 waves; dead waves in the last one), `mult8` (16 waves: no dead wave) and `one` -- and must
give (a) each job the bits of the stand-alone launch of that job (= ordered_f32), sentinels and pad zeros intact, (b) inside the float64
bound, (c) its OWN outputs the bits of the same launch without jobs:
  gather_mean_kernel<1 | 4 | 8>            test_standalone_sweep (d x s x n: indexed, contiguous, self by index / position),
                                           test_gather_rows_sweep (a copy: bit-equal)
  gather_mean_kernel<1 | 8, dropout>       test_gather_mean_dropout_sweep, test_dropout_rows_sweep (dropout_rows_kernel)
  segment_max_gather_kernel<5 | 13>        test_segment_max_gather_sweep
  gs_sage_dense_fwd_tiled3 (8; 4)          test_riders[tiled3_fwd]            _tiled3_means: test_riders[tiled3_fwd_means]
  gs_dense_wgrad_grouped_tiled3 (8; 4)     test_riders[wgrad_tiled3_form0 | _form1]
  gs_dense_wgrad_grouped_tiled3_sample     test_riders[wgrad_tiled3_sample_B1 | _B5] (sampler roots in front of the riders; ids
                                           bit-equal to gs_sample_fanout_desc)
  gs_sage_dense_fwd_stream / _stream2 (8; 4), gs_dense_wgrad_grouped_stream (8; 4)
                                           test_riders[stream_fwd | stream2_fwd | wgrad_stream]
  gs_sage_tail_fwd_bwd (13; 8)             test_riders[tail_train_D256 | tail_train_D128 | tail_eval | tail_train_C65 | tail_split |
                                           tail_means]   (tail_split: jobs in the gs_sage_tail_z launch AND in the z_ready launch)
  gs_sage_tail_z / _z_means / _dh0 (8; 8)  test_riders[tail_z | tail_z_means | tail_dh0]
  gs_linkpred_tail / _means / _neg (13; 8) test_riders[lp_tail | lp_tail_means | lp_neg_train | lp_neg_eval]
  gs_flat_reduce_adam_sample (8, 25; 4)    test_riders[optim | optim_loss | optim_sampler | optim_loss_sampler]: parameters, Adam state,
                                           gradients and loss bit-identical to gs_flat_reduce_adam, ids to the stand-alone sampler
  gs_sage_dense_fwd_cogather, gs_dense_wgrad_grouped_cogather (gs_gemm.hip, 4 jobs): their rider cases stay in
                                           tests/test_gemm_edges_gpu.py (GatherJob.check compares with the stand-alone launch, too)
Refusals (test_rider_refusals): 7 jobs (5 on the gs_gemm.hip hosts), n = 0, ldo < round_up(d, 4), ld_self < round_up(d, 4) -- an
error, and neither a job output nor a host output is touched.

Every test prints the worst err / bound it met per host and per U body (pytest -s)."""
import ctypes

import numpy as np
import pytest
import torch

from graphsage_amd import _lib, ops
from graphsage_amd.ops import Mat
import gather_oracle as G
import gemm_oracle as go
from test_gemm_edges_gpu import In, Out as GemmOut, Slabs, _wgrad_problem
from test_optim_gpu import Flat, HARGS

pytestmark = pytest.mark.gpu
S, IS = G.SENTINEL, G.ISENTINEL
WORST = {}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sync():
    torch.cuda.synchronize()


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


@pytest.fixture(autouse=True)
def _print_worst():
    """Prints the largest err / bound per host and U body that the test met (pytest -s); a figure, not a check."""
    WORST.clear()
    yield
    for k in sorted(WORST):
        print("\nworst err/bound %-40s %.4f" % (k, WORST[k]), end="")


def _words(t):
    """A tensor's bytes (NaN payloads and the sign of zero included)."""
    return t.detach().cpu().contiguous().numpy().reshape(-1).view(np.uint8)


class DevOut(object):
    """[n, d] output two rows down a sentinel-filled [n + 4, round_up(d, 4) + 8] device buffer; `mat` is the row-sliced view."""

    def __init__(self, dev, n, d, dtype=torch.float32, sentinel=S, ld=None):
        self.n, self.d, self.sentinel = n, d, sentinel
        self.big = torch.full((n + 4, G.rup4(d) + 8 if ld is None else ld), float(sentinel) if dtype == torch.float32 else int(sentinel),
                              dtype=dtype, device=dev)
        self.view = self.big[2:2 + n]
        self.mat = Mat(self.view, d) if dtype == torch.float32 else None

    def numpy(self):
        _sync()
        return self.big.cpu().numpy()

    def read(self, tag, d4=None):
        return G.read_block(self.numpy(), self.n, self.d, tag, d4=d4, sentinel=self.sentinel)

    def untouched(self, tag):
        assert np.all(self.numpy() == self.sentinel), "%s: a refused call wrote an output" % tag


class DevJob(object):
    """A gather_oracle.Job with its operands on the device."""

    def __init__(self, dev, job):
        self.dev, self.job = dev, job
        self.X = Mat(_dev(job.Xbuf, dev), job.d)
        self.idx = _dev(job.idx, dev) if job.idx is not None else None
        self.S = Mat(_dev(job.Sbuf, dev), job.d) if job.Sbuf is not None else None
        self.sidx = _dev(job.sidx, dev) if job.sidx is not None else None
        self.alone = None
        self.fresh()

    def fresh(self):
        self.out = DevOut(self.dev, self.job.n, self.job.d)

    def desc(self):
        return ops.gather_job(self.X, self.idx, self.job.n, self.job.s, self.out.mat, self_src=self.S, self_idx=self.sidx)

    def standalone(self):
        ops.gather_mean_fwd(self.X, self.idx, self.job.n, self.job.s, out=self.out.mat, self_src=self.S, self_idx=self.sidx)

    def collect(self, tag):
        """The checks of gather_oracle.Job.check on what the device wrote -> (err / bound, the logical block)."""
        self.job.big = self.out.numpy()
        r = self.job.check(tag)
        return r, self.job.big[2:2 + self.job.n, :self.job.d]


# ================================================================================================== stand-alone launches
@pytest.mark.parametrize("d", G.D_SWEEP)
def test_standalone_sweep(dev, d):
    """gs_gather_mean_fwd, U = 1 (s < 4), 4 (s < 8), 8: every s of the sweep (remainders 0, 1, 7; 64-id block edge; two and three
    blocks) x n in {1, 5} x {indexed, contiguous, GCN self through self_idx, GCN self by position}: the bits of ordered_f32, inside
    the float64 bound ((cnt + 3) u mag / cnt + u |want|: 1.7e-6 of the mean magnitude at s = 25), pad zeros, sentinels."""
    for s in G.S_SWEEP:
        for n in G.N_SWEEP:
            rng = np.random.default_rng(100000 * d + 100 * s + n)
            for kind, indexed in ((None, True), (None, False), ("idx", True), ("pos", True)):
                j = DevJob(dev, G.Job(rng, n, s, d, self_kind=kind, indexed=indexed))
                j.standalone()
                r, _ = j.collect("stand-alone ")
                _note("standalone U=%d" % G.standalone_u(s), r)


@pytest.mark.parametrize("d", G.D_SWEEP)
def test_gather_rows_sweep(dev, d):
    """gs_gather_rows is a copy: bit-equal, pad zeros, sentinels; n in {1, 5, 77} ids with repeats."""
    for n in (1, 5, 77):
        rng = np.random.default_rng(1000 * d + n)
        buf, ids, clean = G.table(rng, n, d)
        out = DevOut(dev, n, d)
        ops.gather_rows(Mat(_dev(buf, dev), d), _dev(ids, dev), out=out.mat)
        G.assert_bits(out.read("gather_rows d=%d n=%d" % (d, n)), clean[ids], "gather_rows d=%d n=%d" % (d, n))


@pytest.mark.parametrize("rate", G.DROP_RATES)
@pytest.mark.parametrize("d", G.DROP_D)
def test_gather_mean_dropout_sweep(dev, d, rate):
    """gs_gather_mean_dropout_fwd (U = 1 below s = 8, else 8; row0 != 0; with and without a GCN self term) inside
    gather_mean_dropout's bound: (cnt + 4) u sum|x / keep| / cnt + u |want|; pad zeros and sentinels as everywhere."""
    clock = torch.tensor([3], dtype=torch.int64, device=dev)
    for s in G.DROP_S:
        n, row0 = 5, 4096 + s
        rng = np.random.default_rng(1000 * d + s)
        mask = G.dropout_mask(9, 3, 33, row0, n * s, d, rate)
        for kind in (None, "pos"):
            j = DevJob(dev, G.Job(rng, n, s, d, self_kind=kind))
            ops.gather_mean_fwd(j.X, j.idx, n, s, out=j.out.mat, self_src=j.S, drop=ops.dropout_desc(9, clock, 33, rate, row0))
            tag = "dropout rate=%.2f s=%d d=%d self=%s" % (rate, s, d, kind)
            want, bound = G.gather_mean_dropout(j.job.clean, j.job.idx, n, s, mask, j.job.self_rows)
            _note("dropout U=%d" % (8 if s >= 8 else 1), go.assert_within(j.out.read(tag), want, bound, tag))


@pytest.mark.parametrize("rate", G.DROP_RATES)
@pytest.mark.parametrize("d", G.DROP_D)
def test_dropout_rows_sweep(dev, d, rate):
    """gs_dropout_rows == X[ids] * fp32(1 / keep) where kept, +0 where dropped (a select, not a product by 0), bit-equal; row0 != 0."""
    clock = torch.tensor([3], dtype=torch.int64, device=dev)
    for n in (1, 5, 77):
        rng = np.random.default_rng(d + n)
        buf, ids, clean = G.table(rng, n, d)
        out = DevOut(dev, n, d)
        ops.dropout_rows(Mat(_dev(buf, dev), d), _dev(ids, dev), n, ops.dropout_desc(9, clock, 20, rate, 1000 + n), out.mat)
        tag = "dropout_rows rate=%.2f d=%d n=%d" % (rate, d, n)
        mask = G.dropout_mask(9, 3, 20, 1000 + n, n, d, rate)
        G.assert_bits(out.read(tag), np.where(mask > 0, clean[ids] * mask, np.float32(0)), tag)


@pytest.mark.parametrize("hidden", G.SEGMAX_HIDDEN)
def test_segment_max_gather_sweep(dev, hidden):
    """gs_segment_max_gather_fwd, U = 5 (s < 13) and 13, s around both and around the 64-id block: pooled and arg-max bit-equal to the
    oracle (first index of the maximum) on relu outputs with whole zero columns and the group maximum repeated at the first and the
    last j and in the second id block, and bit-equal to gs_segment_max_fwd on the expanded matrix; the arg-max has no pad columns
    (nothing outside [0, hidden) written), pooled's pad columns are zeros."""
    n = 5
    for s in G.SEGMAX_S:
        rng = np.random.default_rng(1000 * s + hidden)
        buf, inv, clean = G.segmax_inputs(rng, n, s, hidden)
        H, inv_d = Mat(_dev(buf, dev), hidden), _dev(inv, dev)
        tag = "segment_max_gather s=%d hidden=%d" % (s, hidden)
        got = []
        for gathered in (True, False):
            pooled = DevOut(dev, n, hidden)
            arg = DevOut(dev, n, hidden, dtype=torch.int32, sentinel=IS, ld=hidden + 3)
            if gathered:
                ops.call("gs_segment_max_gather_fwd", H.ptr, H.ld, inv_d.data_ptr(), n, s, hidden, pooled.mat.ptr, pooled.mat.ld,
                         arg.view.data_ptr(), arg.view.stride(0), ops.current_stream())
            else:
                ops.segment_max_fwd(Mat(_dev(G.dense(clean[inv], hidden), dev), hidden), n, s, pooled.mat, arg.view)
            got.append((pooled.read(tag), arg.read(tag, d4=hidden)))
        want_p, want_a = G.segment_max_gather(clean, inv, n, s)
        G.assert_bits(got[0][0], want_p, tag + " pooled")
        assert np.array_equal(got[0][1], want_a), tag + " arg-max"
        G.assert_bits(got[1][0], got[0][0], tag + " pooled vs gs_segment_max_fwd")
        assert np.array_equal(got[1][1], got[0][1]), tag + " arg-max vs gs_segment_max_fwd"


# ================================================================================================== riders
@pytest.fixture(scope="module")
def lists(dev):
    """The three job lists on the device, each job's stand-alone launch checked and kept: computed once, shared by every host."""
    out = {}
    for name in sorted(G.JOB_LISTS):
        rng = np.random.default_rng(sum(name.encode()))
        djs = [DevJob(dev, G.Job(rng, *spec)) for spec in G.JOB_LISTS[name]]
        for j in djs:
            j.standalone()
            _, block = j.collect("stand-alone ")
            j.alone = block.copy()
        out[name] = djs
    return out


def _asym(rng, shape, scale=1.0):
    return go.asym(rng, shape, scale)


def _relu_h0(rng, rows, D):
    return np.maximum(_asym(rng, (rows, D)), 0).astype(np.float32)


# Every host below is a factory(dev) -> prep; prep() -> (outs, go, after): `outs` the tensors the launch may write (freshly
# allocated), go(descs) the launch with those gather descriptors riding, after() further checks once it ran (or None).
def _tiled3_fwd(with_means):
    def factory(dev):
        rng = np.random.default_rng(11)
        n_roots, s, K, out = 20, 10, 50, 64
        n = n_roots * (1 + s)
        X = _asym(rng, (300, K))
        sid = _dev(rng.integers(0, 300, size=n).astype(np.int32), dev)
        Xd, md = Mat.from_numpy(X, dev, 32), Mat.from_numpy(_asym(rng, (n, K)), dev, 4)
        Wsd, Wnd = Mat.from_numpy(_asym(rng, (K, out), 0.1), dev), Mat.from_numpy(_asym(rng, (K, out), 0.1), dev)
        bd = _dev(_asym(rng, (2 * out,), 0.1), dev)

        def prep():
            h0 = Mat(torch.full((n, 2 * out + 4), float("nan"), device=dev), 2 * out)
            lm = Mat(torch.full((n_roots + 3, 2 * out + 8), float("nan"), device=dev), 2 * out)

            def launch(descs):
                if with_means:
                    ops.sage_dense_fwd_tiled3_means(Xd, sid, md, n, Wsd, Wnd, out, ops.ACT_RELU, bd, h0, n_roots, s, lm, descs)
                else:
                    ops.sage_dense_fwd_tiled3(Xd, sid, md, n, Wsd, Wnd, out, ops.ACT_RELU, bd, h0, descs)
            return [h0.buf, lm.buf], launch, None
        return prep
    return factory


def _small_csr(rng, N):
    deg = rng.integers(0, 12, size=N)
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr, rng.integers(0, N, size=int(rowptr[-1])).astype(np.int32)


class Sampler(object):
    """A two-hop fan-out sampler over a 300-node graph for B roots taken from an epoch order at a wrapping cursor: `desc(ids)`."""

    def __init__(self, dev, B):
        rng = np.random.default_rng(5 + B)
        self.N, self.B, self.fans, self.dev = 300, B, (3, 2), dev
        rowptr, col = _small_csr(rng, self.N)
        self.rowptr, self.col = _dev(rowptr, dev), _dev(col, dev)
        self.order = _dev(rng.permutation(self.N).astype(np.int32), dev)
        self.cursor = torch.tensor([self.N - 3], dtype=torch.int64, device=dev)
        self.clock = torch.tensor([5], dtype=torch.int64, device=dev)
        self.offsets = [0, B, B + 3 * B, B + 3 * B + 6 * B]

    def ids(self):
        return torch.full((self.offsets[-1] + 8,), -7, dtype=torch.int32, device=self.dev)

    def desc(self, ids):
        return ops.fanout_desc(self.rowptr, self.col, self.N, self.N, list(self.fans), self.offsets, ids, self.B, 123, step_dev=self.clock,
                               order=self.order, cursor_dev=self.cursor)

    def check(self, ids_rider, tag):
        alone = self.ids()
        ops.sample_fanout_desc(self.desc(alone))
        _sync()
        a, b = alone.cpu().numpy(), ids_rider.cpu().numpy()
        assert np.array_equal(a, b), "%s: the riding sampler's ids differ from gs_sample_fanout_desc's" % tag
        assert np.all(a[:self.offsets[-1]] >= 0) and np.all(a[self.offsets[-1]:] == -7)


WGRAD_SHAPES = [(200, 70, 41, 0, 3), (83, 6, 136, 128, 2)]


def _wgrad(entry, form=None, B=0):
    def factory(dev):
        rng = np.random.default_rng(77)
        probs = [_wgrad_problem(dev, rng, n, d, out, col0, slabs, gathered=(i == 0)) for i, (n, d, out, col0, slabs) in enumerate(WGRAD_SHAPES)]
        sampler = Sampler(dev, B) if B else None

        def prep():
            slabs = [Slabs(dev, sl.n_slabs, sl.d, sl.out) for (_, _, _, sl, _, _) in probs]
            arr = (_lib.WgradDesc * len(probs))()
            for q, (A, idx_d, Z, _, _, _), sl, (n, d, out, col0, ns) in zip(arr, probs, slabs, WGRAD_SHAPES):
                q.A, q.a_idx, q.dZ, q.slabs = A.ptr, ops.ptr(idx_d), Z.ptr, sl.ptr
                q.lda, q.ldz, q.ld_slab, q.n, q.d, q.col0, q.out_dim, q.n_slabs = A.ld, Z.ld, sl.ld, n, d, col0, out, ns
                q.a_rows = A.t.shape[0] - 1
            ids = sampler.ids() if sampler else None

            def launch(descs):
                jarr = (_lib.GatherDesc * max(len(descs), 1))(*descs)
                if form is not None:
                    _lib.set_wgrad_tiled3_form(form)
                try:
                    if sampler:
                        fd = sampler.desc(ids)
                        ops.call(entry, ctypes.addressof(arr), len(probs), ctypes.addressof(jarr), len(descs), ctypes.addressof(fd),
                                 ops.current_stream())
                    else:
                        ops.call(entry, ctypes.addressof(arr), len(probs), ctypes.addressof(jarr), len(descs), ops.current_stream())
                finally:
                    if form is not None:
                        _lib.set_wgrad_tiled3_form(_lib.WGRAD_TILED3_FORM_DEFAULT)

            def after():
                if "tiled3" in entry:                      # (as tests/test_wgrad_acut_gpu.py holds them; a figure of the HOST's work)
                    for sl, p, shape in zip(slabs, probs, WGRAD_SHAPES):
                        _note(entry + " slabs", sl.check(p[4], p[5], shape[0], "%s %r" % (entry, shape)))
                if sampler:
                    sampler.check(ids, entry)
            return [sl.t for sl in slabs] + ([ids] if sampler else []), launch, after
        return prep
    return factory


def _stream_fwd(two_lengths):
    def factory(dev):
        rng = np.random.default_rng(13)
        n, d_self, d_agg, out = (70, 602, 37, 6) if two_lengths else (70, 20, 20, 6)
        X = _asym(rng, (300, d_self))
        sid = _dev(rng.integers(0, 300, size=n).astype(np.int32), dev)
        Xd, md = Mat.from_numpy(X, dev, 32), Mat.from_numpy(_asym(rng, (n, d_agg)), dev)
        Wsd, Wnd = Mat.from_numpy(_asym(rng, (d_self, out), 0.1), dev), Mat.from_numpy(_asym(rng, (d_agg, out), 0.1), dev)
        bd = _dev(_asym(rng, (2 * out,), 0.1), dev)

        def prep():
            o = DevOut(dev, n, 2 * out)

            def launch(descs):
                f = ops.sage_dense_fwd_stream2 if two_lengths else ops.sage_dense_fwd_stream
                f(Xd, sid, md, n, Wsd, Wnd, out, ops.ACT_RELU, bd, o.mat, descs)
            return [o.big], launch, None
        return prep
    return factory


def _tail(n, s, D, O, C, sig, train, split=False, means_ready=False):
    def factory(dev):
        rng = np.random.default_rng(n + C + D)
        rows, Z = n + n * s, 2 * O
        h0n = _relu_h0(rng, rows, D)
        h0 = Mat.from_numpy(h0n, dev)
        Ws, Wn = Mat.from_numpy(_asym(rng, (D, O), 0.2), dev), Mat.from_numpy(_asym(rng, (D, O), 0.2), dev)
        Wh, bh = Mat.from_numpy(_asym(rng, (Z, C), 0.3), dev), _dev(_asym(rng, (C,), 0.1), dev)
        labn = (rng.random((n, C)) > 0.5).astype(np.float32) if sig else np.eye(C, dtype=np.float32)[rng.integers(0, C, n)]
        lab = Mat.from_numpy(labn, dev)
        means_in = G.ordered_f32(h0n[n:], None, n, s)          # what gs_sage_dense_fwd_tiled3_means writes
        assert ops.sage_tail_supported(D, O, C)

        def prep():
            means = Mat.from_numpy(means_in, dev) if means_ready else Mat.zeros(n, D, dev)
            z, y = Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev)
            lo, pr, dl = Mat.zeros(n, C, dev), Mat.zeros(n, C, dev), Mat.zeros(n, C, dev)
            lr, dz, dh0 = torch.zeros(n, device=dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
            sync = torch.zeros(ops.tail_sync_words(n, O), dtype=torch.int32, device=dev)
            _sync()

            def launch(descs):
                half = len(descs) // 2 if split else 0
                ops.sage_tail_fwd_bwd(h0, n, s, Ws, Wn, O, Wh, bh, lab, C, sig, means, z, y, lo, pr, dl, lr, dz=dz if train else None,
                                      d_h0=dh0 if train else None, jobs=descs[half:], split=split, jobs_z=descs[:half], sync=sync,
                                      means_ready=means_ready)

            def after():
                if not split:
                    assert ops.tail_sync_error(sync, n) == 0
                assert float(z.buf.abs().max().item()) > 0 and (not train or float(dh0.buf.abs().max().item()) > 0)
            return [m.buf for m in (means, z, y, lo, pr, dl, dz, dh0)] + [lr], launch, after
        return prep
    return factory


def _tail_half(which, means_ready=False):
    def factory(dev):
        rng = np.random.default_rng(41)
        n, s, D, O = 20, 3, 128, 64
        rows, Z = n + n * s, 2 * O
        h0n = _relu_h0(rng, rows, D)
        h0 = Mat.from_numpy(h0n, dev)
        Ws, Wn = Mat.from_numpy(_asym(rng, (D, O), 0.2), dev), Mat.from_numpy(_asym(rng, (D, O), 0.2), dev)
        dz = Mat.from_numpy(_asym(rng, (n, Z)), dev)
        means_in = G.ordered_f32(h0n[n:], None, n, s)

        def prep():
            if which == "z":
                means = Mat.from_numpy(means_in, dev) if means_ready else Mat.zeros(n, D, dev)
                z = Mat.zeros(n, Z, dev)
                return [means.buf, z.buf], (lambda descs: ops.sage_tail_z(h0, n, s, Ws, Wn, O, means, z, jobs=descs,
                                                                          means_ready=means_ready)), None
            dh0 = Mat.zeros(rows, D, dev)
            return [dh0.buf], (lambda descs: ops.sage_tail_dh0(h0, n, s, Ws, Wn, O, dz, dh0, jobs=descs)), None
        return prep
    return factory


def _lp_tail(jobs_in, train=True, means_ready=False):
    def factory(dev):
        B, nn, s, D, O = 12, 20, 3, 128, 64
        n = 2 * B + nn
        rng = np.random.default_rng(s + D + O)
        rows, Z = n + n * s, 2 * O
        h0n = _relu_h0(rng, rows, D)
        h0 = Mat.from_numpy(h0n, dev)
        Ws, Wn = Mat.from_numpy(_asym(rng, (D, O), 0.2), dev), Mat.from_numpy(_asym(rng, (D, O), 0.2), dev)
        means_in = G.ordered_f32(h0n[n:], None, n, s)
        assert ops.linkpred_tail_supported(D, O, nn)

        def prep():
            means = Mat.from_numpy(means_in, dev) if means_ready else Mat.zeros(n, D, dev)
            z, y, dz, dh0 = Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev), Mat.zeros(n, Z, dev), Mat.zeros(rows, D, dev)
            lr, rr, aff = torch.zeros(B, device=dev), torch.zeros(B, device=dev), Mat.zeros(B, nn + 1, dev)
            slabs = torch.zeros(((B + 7) // 8) * nn * Z, device=dev)
            loss, mrr = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
            sync = torch.zeros(ops.lp_tail_sync_words(B, nn), dtype=torch.int32, device=dev)
            _sync()
            desc = ops.linkpred_tail_desc(h0, B, nn, s, Ws, Wn, O, means, z, y, lr, rr, aff, 1.0, 1.0 / B, sync, dz=dz if train else None,
                                          d_h0=dh0 if train else None, neg_slabs=slabs if train else None)

            def launch(descs):
                ops.linkpred_tail(desc, jobs=descs if jobs_in == 1 else (), means_ready=means_ready)
                ops.linkpred_tail_neg(desc, loss_out=loss, accumulate=False, mrr_out=mrr, jobs=descs if jobs_in == 2 else ())

            def after():
                assert ops.lp_tail_sync_error(sync, B, nn) == 0
                assert np.isfinite(loss.cpu().numpy()).all() and float(y.buf.abs().max().item()) > 0
            return [m.buf for m in (means, z, y, dz, dh0, aff)] + [lr, rr, slabs, loss, mrr], launch, after
        return prep
    return factory


def _optim(with_loss, B):
    def factory(dev):
        sampler = Sampler(dev, B) if B else None
        rows = _dev(np.concatenate([np.random.default_rng(3).random(65).astype(np.float32) * 3, np.full(8, np.nan, np.float32)]), dev)
        cfg = dict(wd=0.01, clip=5.0, gscale=1.0, offset=1)

        def prep():
            fl, ref = Flat(dev, "straddle", 7), Flat(dev, "straddle", 7)
            lo, lo_ref = _dev(np.asarray([S, 7.0, S], np.float32), dev), _dev(np.asarray([S, 7.0, S], np.float32), dev)
            ids = sampler.ids() if sampler else None

            def launch(descs):
                ops.flat_reduce_adam_sample(fl.desc, fl.P, fl.G, fl.M, fl.V, fl.total, cfg["wd"], True, HARGS[0], fl.step, beta1=HARGS[1],
                                            beta2=HARGS[2], eps=HARGS[3], clip=cfg["clip"], grad_scale=cfg["gscale"], step_offset=cfg["offset"],
                                            loss=(rows, 65, 1.0 / 65, lo[1:2], True) if with_loss else None,
                                            sampler=sampler.desc(ids) if sampler else None, jobs=descs)

            def after():
                ref.launch(1, cfg["wd"], cfg["clip"], cfg["gscale"], cfg["offset"], loss=(rows, 65, 1.0 / 65, lo_ref[1:2], 1) if with_loss else None)
                a, b = fl.host(), ref.host()
                for k in "PGMV":
                    assert np.array_equal(_words(getattr(fl, k)), _words(getattr(ref, k))), "optimizer: %s differs from gs_flat_reduce_adam's" % k
                assert all(np.array_equal(x, y) for x, y in zip(a["slabs"], b["slabs"]))
                assert np.array_equal(_words(lo), _words(lo_ref)) and (float(lo[1].item()) != 7.0) == with_loss
                assert np.abs(a["P"][:fl.covered] - Flat(dev, "straddle", 7).host()["P"][:fl.covered]).max() > 0
                if sampler:
                    sampler.check(ids, "optimizer")
            return [fl.P, fl.G, fl.M, fl.V, lo] + fl.slabs + ([ids] if sampler else []), launch, after
        return prep
    return factory


# name -> (factory, (U, UBIG))
HOSTS = {
    "tiled3_fwd": (_tiled3_fwd(False), (8, 8)),
    "tiled3_fwd_means": (_tiled3_fwd(True), (8, 8)),
    "wgrad_tiled3_form0": (_wgrad("gs_dense_wgrad_grouped_tiled3", form=0), (8, 8)),
    "wgrad_tiled3_form1": (_wgrad("gs_dense_wgrad_grouped_tiled3", form=1), (8, 8)),
    "wgrad_tiled3_sample_B1": (_wgrad("gs_dense_wgrad_grouped_tiled3_sample", B=1), (8, 8)),
    "wgrad_tiled3_sample_B5": (_wgrad("gs_dense_wgrad_grouped_tiled3_sample", B=5), (8, 8)),
    "stream_fwd": (_stream_fwd(False), (8, 8)),
    "stream2_fwd": (_stream_fwd(True), (8, 8)),
    "wgrad_stream": (_wgrad("gs_dense_wgrad_grouped_stream"), (8, 8)),
    "tail_train_D256": (_tail(20, 3, 256, 128, 41, False, True), (13, 13)),          # two main workgroups per 16-row group
    "tail_train_D128": (_tail(20, 3, 128, 64, 7, True, True), (13, 13)),
    "tail_eval": (_tail(20, 3, 256, 128, 41, False, False), (13, 13)),
    "tail_train_C65": (_tail(20, 3, 256, 64, 65, True, True), (13, 13)),             # two class groups
    "tail_split": (_tail(20, 3, 256, 128, 41, False, True, split=True), (13, 13)),   # (its z launch: U = 8)
    "tail_means": (_tail(20, 3, 256, 128, 41, False, True, means_ready=True), (13, 13)),
    "tail_z": (_tail_half("z"), (8, 8)),
    "tail_z_means": (_tail_half("z", means_ready=True), (8, 8)),
    "tail_dh0": (_tail_half("dh0"), (8, 8)),
    "lp_tail": (_lp_tail(1), (13, 13)),
    "lp_tail_means": (_lp_tail(1, means_ready=True), (13, 13)),
    "lp_neg_train": (_lp_tail(2), (13, 13)),
    "lp_neg_eval": (_lp_tail(2, train=False), (13, 13)),
    "optim": (_optim(False, 0), (8, 25)),
    "optim_loss": (_optim(True, 0), (8, 25)),
    "optim_sampler": (_optim(False, 3), (8, 25)),
    "optim_loss_sampler": (_optim(True, 3), (8, 25)),
}


@pytest.mark.parametrize("host", sorted(HOSTS))
def test_riders(dev, lists, host):
    """(a), (b), (c) of the module docstring for one host and the three job lists."""
    factory, (u, ubig) = HOSTS[host]
    prep = factory(dev)
    for name in ("six", "mult8", "one"):
        djs = lists[name]
        outs0, go0, _ = prep()
        go0([])
        _sync()
        base = [_words(t) for t in outs0]
        for j in djs:
            j.fresh()
        outs, launch, after = prep()
        launch([j.desc() for j in djs])
        _sync()
        for k, (a, t) in enumerate(zip(base, outs)):
            assert np.array_equal(a, _words(t)), "%s with the `%s` jobs: its own output %d differs from the launch without jobs" % (host, name, k)
        for j in djs:
            tag = "%s / %s: " % (host, name)
            r, block = j.collect(tag)
            G.assert_bits(block, j.alone, tag + j.job.tag + " vs the stand-alone launch")
            _note("%s U=%d" % (host, G.rider_u(u, ubig, j.job.s)), r)
        if after is not None:
            after()


# ================================================================================================== refusals
def _gemm_fwd_cogather(dev):
    rng = np.random.default_rng(9)
    n, d, out = 2049, 16, 8
    X, W = In(_asym(rng, (n, d)), dev), In(_asym(rng, (d, out), 0.1), dev)

    def prep():
        o = GemmOut(dev, n, 2 * out)

        def launch(descs):
            jarr = (_lib.GatherDesc * max(len(descs), 1))(*descs)
            ops.call("gs_sage_dense_fwd_cogather", X.ptr, X.ld, None, d, X.ptr, X.ld, None, d, n, W.ptr, W.ld, W.ptr, W.ld, out, 1,
                     ops.ACT_RELU, None, o.ptr, o.ld, ctypes.addressof(jarr), len(descs), ops.current_stream())
        return [o.t], launch, None
    return prep


def _gemm_wgrad_cogather(dev):
    rng = np.random.default_rng(10)
    prob = _wgrad_problem(dev, rng, 83, 6, 136, 128, 2, gathered=False)

    def prep():
        A, _, Z, _, _, _ = prob
        sl = Slabs(dev, 2, 6, 136)
        q = _lib.WgradDesc()
        q.A, q.dZ, q.slabs, q.lda, q.ldz, q.ld_slab, q.n, q.d, q.col0, q.out_dim, q.n_slabs = A.ptr, Z.ptr, sl.ptr, A.ld, Z.ld, sl.ld, 83, 6, 128, 136, 2

        def launch(descs):
            jarr = (_lib.GatherDesc * max(len(descs), 1))(*descs)
            ops.call("gs_dense_wgrad_grouped_cogather", ctypes.addressof(q), 1, ctypes.addressof(jarr), len(descs), ops.current_stream())
        return [sl.t], launch, None
    return prep


# name -> (factory, the host's job limit).  Hosts of two launches are taken where the FIRST launch carries the jobs.
REFUSING = {k: (HOSTS[k][0], 6) for k in ("tiled3_fwd", "tiled3_fwd_means", "wgrad_tiled3_form0", "wgrad_tiled3_sample_B1", "stream_fwd",
                                          "stream2_fwd", "wgrad_stream", "tail_train_D128", "tail_z", "tail_dh0", "lp_tail",
                                          "optim_loss_sampler")}
REFUSING["gemm_fwd_cogather"] = (_gemm_fwd_cogather, 4)            # n = 2049: sage_dense_cogather_kernel
REFUSING["gemm_wgrad_cogather"] = (_gemm_wgrad_cogather, 4)


@pytest.mark.parametrize("host", sorted(REFUSING))
def test_rider_refusals(dev, host):
    """Bad job lists are refused on the host before anything is launched: one job too many (7; 5 on the gs_gemm.hip hosts), a job with
    n = 0, with ldo < round_up(d, 4), with a self term whose ld_self < round_up(d, 4).  The call raises, every job output keeps its
    sentinel and every tensor the host may write keeps what it held.  Every pointer is valid and the buffers are their full size: a
    narrow leading dimension only makes the rows overlap, so even a launch that was NOT refused would stay inside them."""
    factory, limit = REFUSING[host]
    prep = factory(dev)
    rng = np.random.default_rng(21)
    n, s, d = 3, 9, 10                                      # round_up(d, 4) = 12
    good = [DevJob(dev, G.Job(rng, n, s, d, self_kind="pos")) for _ in range(limit + 1)]

    def descs(k, **change):
        out = [j.desc() for j in good[:k]]
        for name, v in change.items():
            setattr(out[-1], name, v)
        return out

    bad = {"%d jobs" % (limit + 1): descs(limit + 1), "n = 0": descs(2, n=0), "ldo < round_up(d, 4)": descs(2, ldo=8),
           "ld_self < round_up(d, 4)": descs(limit, ld_self=8), "ldx < round_up(d, 4)": descs(1, ldx=8)}
    for what, dl in sorted(bad.items()):
        outs, launch, _ = prep()
        _sync()
        before = [_words(t) for t in outs]
        with pytest.raises(_lib.GraphsageAmdError):
            launch(dl)
        _sync()
        for k, (a, t) in enumerate(zip(before, outs)):
            assert np.array_equal(a, _words(t)), "%s refused `%s` but wrote its output %d" % (host, what, k)
        for j in good:
            j.out.untouched("%s, %s" % (host, what))
