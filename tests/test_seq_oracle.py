"""CPU checks of what tests/test_lstm_edges_gpu.py holds the recurrence kernels (csrc/gs_lstm.hip) to:
  * seq_oracle.recurrence_fwd / recurrence_bwd (the kernels' contract: G given, A, C, H_prev, h_last, dG out) equal, in float64 and
    to 1e-12, a masked torch loop with G as the leaf and dG = G.grad of (h_last * dh_last).sum() -- written independently, no BPTT by
    hand -- and reproduce seq_oracle.lstm_fwd / lstm_bwd (the functions the fixture replays rest on) through the contractions
    h_last, dx = dG W_x^T, d_kernel = [x^T dG ; H_prev^T dG], d_bias = sum dG;
  * lstm_cases builds exactly the lengths it claims: the whole L vector of every case is written out here;
  * the inputs are well conditioned: on every case the fp32 oracle lies within 1e-5 of the largest element of the fp64 oracle, per
    output (that difference, e32, is what the GPU test's bound is made of);
  * the checks bite on the CPU already: an oracle with the forget bias dropped, and the fp64 oracle rounded to bf16-like precision,
    fall outside the GPU test's bound."""
import numpy as np
import pytest
import torch

import lstm_cases as lc
import seq_oracle as so

ALL = [(i, 128) for i in range(len(lc.CASES))] + [(i, 256) for i in lc.CASES_256]
IDS = ["H%d-%s" % (H, lc.case_id(i)) for i, H in ALL]

# the lengths of every case, per segment (the planted sequences first: see lstm_cases)
LENGTHS = [
    [[1]],
    [[1, 2, 1]],
    [[1, 24, 24, 24, 1, 2, 1] + [25] * 8],
    [[1, 2, 2, 2, 1, 2, 1] + [3] * 9],
    [[1, 4, 4, 4, 1, 2, 1] + [5] * 10],
    [[1, 6, 6, 6, 1, 2, 1] + [7] * 26],
    [[], [1, 2, 2, 2, 1]],
    [[1, 2, 2, 2, 1], [], [1, 2, 1, 1, 1, 2, 1] + [2] * 11],
    [[1, 5, 5, 5], []],
    [[1, 1, 1, 1], [1, 24, 24, 24, 1], [1, 2, 1, 1, 1, 2, 1] + [2] * 9, [1, 8, 8]],
    [[]],
    [[1, 6, 6, 6, 1, 2, 1] + [7] * 9 + [2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2] + [7]],
]


def _torch_reference(G, L, W_h, dh_last):
    """dynamic_rnn's masked loop in float64 with autograd: -> A, C, H_prev (as computed at every step, masked or not), h_last, dG."""
    G = torch.tensor(G, dtype=torch.float64, requires_grad=True)
    W, Lt = torch.tensor(W_h, dtype=torch.float64), torch.tensor(np.asarray(L))
    n, T, H4 = G.shape
    H = H4 // 4
    h = c = torch.zeros((n, H), dtype=torch.float64)
    A, C, Hp = [], [], []
    for t in range(T):
        z = G[:, t] + h @ W
        i, j, f, o = torch.sigmoid(z[:, :H]), torch.tanh(z[:, H:2 * H]), torch.sigmoid(z[:, 2 * H:3 * H] + 1.0), torch.sigmoid(z[:, 3 * H:])
        nc = c * f + i * j
        nh = torch.tanh(nc) * o
        m = (t < Lt)[:, None]
        A.append(torch.cat([i, j, f, o], dim=1))
        C.append(nc)
        Hp.append(h)
        c, h = torch.where(m, nc, c), torch.where(m, nh, h)
    (h * torch.tensor(dh_last, dtype=torch.float64)).sum().backward()
    st = lambda v: torch.stack(v, dim=1).detach().numpy()
    return st(A), st(C), st(Hp), h.detach().numpy(), G.grad.numpy()


@pytest.mark.parametrize("i,H", ALL, ids=IDS)
def test_recurrence_equals_masked_torch_loop(i, H):
    c = lc.case(i, H)
    for k, o in enumerate(c.oracle(np.float64)):
        if not c.segs[k][0]:
            continue
        ran = o["ran"]
        A, C, Hp, hl, dG = _torch_reference(c.G[k], c.L[k], c.W_h, c.dh[k])
        for name, want in (("A", A), ("C", C), ("Hp", Hp), ("dG", dG)):
            assert np.abs(o[name][ran] - want[ran]).max() <= 1e-12, name
        assert np.abs(o["hl"] - hl).max() <= 1e-12
        assert not dG[~ran].any()                                       # autograd agrees: no gradient where the state is copied through
        for name in ("A", "C", "Hp", "dG"):
            assert not o[name][~ran].any(), name                        # exact zeros
        assert not o["Hp"][:, 0].any()


@pytest.mark.parametrize("i,H", ALL, ids=IDS)
def test_recurrence_reproduces_lstm_fwd_and_bwd(i, H):
    c = lc.case(i, H)
    k64 = np.concatenate([c.W_x, c.W_h]).astype(np.float64)
    for k, o in enumerate(c.oracle(np.float64)):
        n, T = c.segs[k]
        if not n:
            continue
        x = c.xs[k].astype(np.float64)
        G = x @ k64[:lc.D] + c.bias.astype(np.float64)
        assert np.abs(G - c.G[k]).max() <= 2.0 ** -24 * max(1.0, np.abs(G).max())          # the case's G is this, rounded once
        A, C, Hp, hl, ran = so.recurrence_fwd(G, c.L[k], k64[lc.D:])
        dG = so.recurrence_bwd(c.dh[k].astype(np.float64), c.L[k], k64[lc.D:], A, C)
        h_ref, cache = so.lstm_fwd(x, c.L[k], k64, c.bias.astype(np.float64))
        dx, dk, db = so.lstm_bwd(c.dh[k].astype(np.float64), cache)
        g2, hp2 = dG.reshape(n * T, -1), Hp.reshape(n * T, -1)
        for name, got, want in (("h_last", hl, h_ref), ("dx", (g2 @ k64[:lc.D].T).reshape(x.shape), dx),
                                ("d_kernel", np.concatenate([x.reshape(n * T, -1).T @ g2, hp2.T @ g2]), dk), ("d_bias", g2.sum(axis=0), db)):
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize("i", range(len(lc.CASES)), ids=[lc.case_id(i) for i in range(len(lc.CASES))])
def test_builder_makes_the_lengths_it_claims(i):
    segs, short = lc.CASES[i]
    assert [len(v) for v in LENGTHS[i]] == [n for n, _ in segs]
    for d in [lc.D] + lc.WIDTHS:
        for last in (False, True):
            xs, Ls = lc.inputs(segs, d, last_col_only=last, short=short, seed=d)
            for x, L, want, (n, T) in zip(xs, Ls, LENGTHS[i], segs):
                assert L.tolist() == want and (so.lengths(x).tolist() == want if n else True), (d, last)
                assert not n or L.max() <= T
                if last:
                    assert not x[:lc.N_PLANTED, :, :d - 1].any()
            table, ids, gathered = lc.id_table(xs, np.random.RandomState(d))
            for x, g, idx, want, (n, T) in zip(xs, gathered, ids, LENGTHS[i], segs):
                assert so.lengths(g).tolist() == want if n else g.size == 0
                assert idx.max(initial=0) < len(table) and not table[-1].any()
    c = lc.case(i, 128)
    assert [L.tolist() for L in c.L] == LENGTHS[i]


def test_cases_cover_the_tile_and_length_edges():
    every = [L for v in LENGTHS for L in v]
    segs = [s for ss, _ in lc.CASES for s in ss]
    assert {1, 15, 16, 17, 33} <= {n for n, _ in segs} and {1, 2, 25} <= {T for _, T in segs}
    assert max(len(ss) for ss, _ in lc.CASES) == 4 and any(n == 0 for n, _ in segs)
    assert any(1 in L[:lc.TILE] and 25 in L[:lc.TILE] for L in every)              # L = 1 and L = T = 25 in one tile
    assert max(LENGTHS[11][0][16:32]) < 7                                          # a whole tile with tmax < T
    x, L = lc.segment_inputs(np.random.RandomState(0), 7, 5, 9)
    assert x[5, 1, 8] == lc.SUBNORMAL and 0 < float(x[5, 1, 8]) < np.finfo(np.float32).tiny and not x[5, 1, :8].any() and not x[5, 2:].any()
    assert np.signbit(x[6]).all() and not x[6].any()
    assert x[4, 4].all() and not x[4, :4].any() and not x[3, 0].any() and x[3, 1:].all()
    s = lc.saturated_case()
    assert all((np.abs(G[:, :, g * 128 + 8 * g:g * 128 + 8 * g + 8]) == 100).all() for G in s.G for g in range(4))


@pytest.mark.parametrize("i,H", ALL, ids=IDS)
def test_inputs_are_well_conditioned(i, H):
    """e32 / largest element per output < 1e-5 (measured 1e-7 .. 2e-6)."""
    c = lc.case(i, H)
    e, big = c.e32(), c.largest()
    for k in lc.OUTPUTS:
        print("H=%d %s %s: e32 %.3g, largest %.3g" % (H, lc.case_id(i), k, e[k], big[k]))
        assert e[k] < 1e-5 * big[k] or big[k] == 0.0, k
    tol = c.tolerance()
    assert all(tol[k] >= 8 * 2.0 ** -24 for k in lc.OUTPUTS)


def test_the_bound_rejects_a_wrong_recurrence():
    """On the CPU already: without the forget bias, or with every saved activation rounded to 8 mantissa bits, the fp32 recurrence is
    outside the GPU test's bound on every output it reaches; the fp32 oracle itself is inside."""
    c = lc.case(4, 128)
    tol, o64 = c.tolerance(), c.oracle(np.float64)[0]
    for k in lc.OUTPUTS:
        assert np.abs(c.oracle(np.float32)[0][k].astype(np.float64) - o64[k]).max() <= tol[k]
    G, L, W = c.G[0], c.L[0], c.W_h
    G2 = G.copy()
    G2[:, :, 256:384] -= 1.0                                                    # sigma(f) instead of sigma(f + 1)
    A, C, Hp, hl, ran = so.recurrence_fwd(G2, L, W)
    assert np.abs(C - o64["C"]).max() > tol["C"] and np.abs(hl - o64["hl"]).max() > tol["hl"]
    A, C, Hp, hl, ran = so.recurrence_fwd(G, L, W)
    A8 = (A.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    assert np.abs(so.recurrence_bwd(c.dh[0], L, W, A8, C) - o64["dG"]).max() > tol["dG"]
