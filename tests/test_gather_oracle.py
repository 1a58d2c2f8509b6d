"""CPU: the evidence that tests/test_gather_edges_gpu.py is sensitive.  gather_oracle.emulate_wave / emulate_launch restate
gather_mean_wave<U> and run_gather_item (csrc/gs_gather_dev.h) as written, on the padded NaN-poisoned operands and the
sentinel-filled outputs of the GPU tests:
  * for U in {1, 4, 8, 13, 25} and every s of the sweep the restatement has the bits of ordered_f32 (so the bit-equality the GPU
    tests demand is what the kernel's text promises, for every number of loads in flight);
  * ordered_f32 -- and the dropout form with each product rounded -- lies inside the float64 bounds (so a correct kernel passes), the
    worst err / bound is printed;
  * each planted fault fails at least one of the checks of gather_oracle.Job.check / read_block (so a wrong kernel fails)."""
import numpy as np
import pytest

import gather_oracle as G
import gemm_oracle as go

# (U, UBIG, waves per workgroup) of the rider hosts: the tiled / stream launches, the tail and link-prediction launches, the optimizer
HOSTS = [(8, 8, 4), (13, 13, 8), (8, 25, 4)]


def _jobs(name, seed=0):
    rng = np.random.default_rng(seed)
    return [G.Job(rng, *spec) for spec in G.JOB_LISTS[name]]


def test_job_lists_have_the_properties_the_rider_tests_rely_on():
    ws = G.wave_starts(G.JOBS_SIX)
    assert len(G.JOBS_SIX) == 6 and ws[-1] % 4 != 0 and ws[-1] % 8 != 0
    assert any(b % 4 for b in ws[1:-1]) and any(b % 8 for b in ws[1:-1])              # boundaries inside a workgroup
    ss = [j[1] for j in G.JOBS_SIX]
    assert min(ss) < 8 and 13 in ss and 25 in ss and 26 in ss and max(ss) > 64
    assert {1, 2, 3, 5} <= {G.chunks(j[2]) for j in G.JOBS_SIX}
    kinds = {(j[3], j[4]) for j in G.JOBS_SIX}
    assert ("idx", True) in kinds and ("pos", True) in kinds and (None, False) in kinds
    assert G.wave_starts(G.JOBS_MULT8)[-1] % 8 == 0 and len(G.JOBS_ONE) == 1
    # U = 13 and U = 25 each meet an exact batch and a remainder
    for u in (13, 25):
        assert any(s >= u and min(s, 64) % u == 0 for s in ss) and any(s >= u and min(s, 64) % u for s in ss)


@pytest.mark.parametrize("u", G.US)
def test_emulated_wave_has_the_bits_of_ordered_f32(u):
    """Every s of the sweep (remainders 0 .. U - 1, one, two and three id blocks), d = 5 (a partial float4) and 257 (a one-lane second
    chunk), with and without a self term: U only batches the loads, the adds stay in j order."""
    for s in G.S_SWEEP:
        for d in (5, 257):
            rng = np.random.default_rng(1000 * s + d)
            job = G.Job(rng, 2, s, d, self_kind=("idx" if s % 2 else None), indexed=(s % 3 != 0))
            for w in range(job.items()):
                job.run_item(u, w)
            job.check("U=%d " % u)


def test_ordered_f32_inside_the_float64_bound():
    worst = 0.0
    for s in G.S_SWEEP:
        for d in G.D_SWEEP:
            rng = np.random.default_rng(77 * s + d)
            for kind in (None, "idx"):
                job = G.Job(rng, 5, s, d, self_kind=kind)
                worst = max(worst, go.assert_within(job.want32, job.want64, job.bound, job.tag))
    print("ordered_f32 vs float64 over the sweep: worst err / bound %.3f" % worst)
    assert worst > 0.0                                         # (fp32 rounding is there at all: the two references differ)


@pytest.mark.parametrize("rate", G.DROP_RATES)
def test_dropout_twin_bound(rate):
    """fp32 emulation of the dropout body (x * scale rounded, then the ordered sum) inside gather_mean_dropout's bound; a lost mask,
    a mask shifted by one row (row0 off by one) and a missing 1 / keep scale outside it."""
    worst = 0.0
    for s in G.DROP_S:
        for d in G.DROP_D:
            rng = np.random.default_rng(s + d)
            n, row0 = 5, 4096 + s
            buf, idx, clean = G.table(rng, n * s, d)
            mask = G.dropout_mask(9, 3, 33, row0, n * s, d, rate)
            assert set(np.unique(mask)) <= {np.float32(0), G.drop_scale(rate)}
            want, bound = G.gather_mean_dropout(clean, idx, n, s, mask)
            dropped = np.zeros_like(clean[idx])
            dropped[:] = clean[idx] * mask                                   # fp32 product, rounded
            emu = G.ordered_f32(dropped, None, n, s)
            worst = max(worst, go.assert_within(emu, want, bound, "dropout s=%d d=%d" % (s, d)))
            if n * s * d >= 64:
                assert not go.within(G.ordered_f32(clean, idx, n, s), want, bound)
                shifted = G.dropout_mask(9, 3, 33, row0 + 1, n * s, d, rate)
                assert not go.within(G.ordered_f32(clean[idx] * shifted, None, n, s), want, bound)
                assert not go.within(G.ordered_f32(clean[idx] * (mask > 0), None, n, s), want, bound)
    print("dropout rate %.2f: worst err / bound %.3f" % (rate, worst))


@pytest.mark.parametrize("u,ubig,wpw", HOSTS)
@pytest.mark.parametrize("name", sorted(G.JOB_LISTS))
def test_emulated_launch_passes(name, u, ubig, wpw):
    jobs = _jobs(name)
    total, dead = G.emulate_launch(jobs, u, ubig, wpw)
    assert total == G.wave_starts(G.JOB_LISTS[name])[-1]
    if name == "six":
        assert dead > 0                                        # dead waves in the last rider workgroup
    if name == "mult8":
        assert dead == 0
    for j in jobs:
        j.check()


FAULTS = ["drop_last_item", "remainder_unmasked", "block_reuse", "boundary", "pad_not_zeroed", "scale_s", "self_by_position"]


@pytest.mark.parametrize("u,ubig,wpw", HOSTS)
@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_fails_a_check(fault, u, ubig, wpw):
    """Each fault, planted in the restated rider launch of the six-job list, makes at least one job fail Job.check (the bit
    comparison, the bound, the pad zeros or the sentinels)."""
    jobs = _jobs("six")
    G.emulate_launch(jobs, u, ubig, wpw, fault=fault)
    failed = []
    for j in jobs:
        try:
            j.check()
        except AssertionError:
            failed.append(j.tag)
    print("%s (U=%d, UBIG=%d): fails %d of %d jobs" % (fault, u, ubig, len(failed), len(jobs)))
    assert failed, fault


def test_planted_faults_fail_the_standalone_sweep_too():
    """The stand-alone launch (one job, U by launch_gather_mean's dispatch) at sweep shapes where each fault bites."""
    for fault, (n, s, d, kind) in [("remainder_unmasked", (5, 9, 5, None)), ("block_reuse", (1, 65, 257, None)),
                                   ("pad_not_zeroed", (1, 1, 1, None)), ("self_by_position", (5, 3, 260, "idx")),
                                   ("drop_last_item", (5, 4, 257, None)), ("scale_s", (1, 2, 3, "pos"))]:
        for planted in (None, fault):
            job = G.Job(np.random.default_rng(5), n, s, d, self_kind=kind)
            G.emulate_launch([job], G.standalone_u(s), G.standalone_u(s), 4, fault=planted)
            if planted is None:
                job.check()
            else:
                with pytest.raises(AssertionError):
                    job.check()


def test_a_store_outside_the_view_fails():
    job = G.Job(np.random.default_rng(1), 3, 2, 5)
    G.emulate_launch([job], 1, 1, 4)
    job.check()
    for r, c in ((1, 0), (5, 0), (2, 8), (3, 5)):              # a row above, a row below, a column beyond round_up(d, 4), a pad column
        keep = job.big[r, c]
        job.big[r, c] = 1.0
        with pytest.raises(AssertionError):
            job.check()
        job.big[r, c] = keep
    job.check()


def test_segment_max_gather_first_index_wins():
    """The oracle's argmax is the first index of the maximum; the planted ties (first and last j, second id block, zero columns) tell
    it from the last-index rule on the very inputs of the GPU test."""
    for s in G.SEGMAX_S:
        for hidden in (3, 257):
            rng = np.random.default_rng(s * 1000 + hidden)
            n = 5
            buf, inv, clean = G.segmax_inputs(rng, n, s, hidden)
            assert np.isnan(buf[:, hidden:]).all() and np.isfinite(buf[inv, :hidden]).all()
            pooled, arg = G.segment_max_gather(clean, inv, n, s)
            assert np.array_equal(pooled, clean[inv].reshape(n, s, hidden).max(axis=1))
            assert (pooled[:, ::3] == 0).all() and (arg[:, ::3] == 0).all()              # zero columns: index 0
            if hidden > 1:
                assert (pooled[0, 1::3] == 9.5).all() and (arg[0, 1::3] == 0).all()
            if s > 64:
                assert (arg[1, 1::3] == 64).all()
            p2, a2 = G.segment_max_gather(clean, inv, n, s, last_tie=True)
            assert np.array_equal(p2, pooled)
            assert (s == 1) == np.array_equal(a2, arg)
