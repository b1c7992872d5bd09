"""AsymptoticAnalysis, MartingaleOptimization and BranchingProcesses on a SHARDED job and at the edge shapes of their
device-resident entry points, against the oracle (run with -m gpu on an MI355X).

The three pricers reduce per-rank sums through ctx->allreduce (kernels_asym.hip, kernels_martingale.hip, kernels_branching.hip)
and the C ABI lets an empty shard through when a collective is installed, but every other collective test of the suite prices
European, LSM or exotics.  A wrong sum here gives a plausible price, not a crash, so everything below is a comparison with
oracle.binding.Oracle on the WHOLE matrix (the single engine's matrix of all paths, downloaded):

  1. world size 3 over a callback collective, shards uneven, none a multiple of 256, the middle one EMPTY;
  2. world size 1 with an identity collective against no collective: the same bits;
  3. the jobs of 1. over the library's own shared-memory collective (mcg_comm_init_shm), order 15 included: a 48-double message
     where shm_allreduce had only ever carried 1, 3 and 8;
  4. one engine, no collective: 1 .. 1023 paths x 1, 2, 50 steps, five kinds of maturity, the quad boundaries of num_branches.

Rank threads: one PathEngine per thread of this process (run_ranks); no pricer here spins on the device, so the default
hardware queues suffice.  Nothing can wait forever: the threads' barrier has a time-out, a rank that raises aborts it -- its
peers' callbacks then return non-zero and they end with MCG_ERR_COMM --, every join has a time-out and a thread still alive
fails the test.

Tolerances are the project's own: AsymptoticAnalysis 1e-12 (test_asymptotic_matches_reference_goldens_and_oracle: per-path
values are bit-identical, only the summation order differs), MartingaleOptimization rtol 1e-8 below order 4, 2e-6 up to order 8,
5e-6 beyond (test_martingale_matches_oracle), BranchingProcesses rtol 1e-12, atol 1e-14 (test_branching_matches_oracle_philox_mode).
Reference: src/models/AsymptoticAnalysisPricer.cpp:38-113, MartingaleOptimizationPricer.cpp:21-189, BranchingProcessPricer.cpp:12-134.
"""
import os
import threading
import time

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd.engine import _DevView
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu

SEED, S0, R, SIGMA, DT, K = 20251031, 100.0, 0.04, 0.2, 0.02, 100.0
DIVIDEND = 0.08
MCG_ERR_COMM = 7
STEPS = 24
SHARDS = [(0, 70_001), (70_001, 0), (70_001, 60_002)]          # (begin, count): uneven, no multiple of 256, the middle one empty
BR_STEPS = 12
BR_SHARDS = [(0, 30_001), (30_001, 0), (30_001, 30_000)]
BR_SEED = 99
ASYM_CASES = [(is_call, maturity) for is_call in (False, True) for maturity in (STEPS * DT, 15.5 * DT)]
MO_CASES = [(False, 2, 5), (True, 2, 5), (False, 2, 1), (False, 6, 5), (False, 15, 5)]      # (is_call, order, iterations)
BR_CASES = [(False, 6), (False, 10), (True, 10)]                                            # (is_call, branches)


def mo_rtol(order):
    return 1e-8 if order < 4 else (2e-6 if order <= 8 else 5e-6)


def rel(got, want):
    """Largest relative difference of two tuples of numbers (0 where both are 0)."""
    g, w = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    d = np.abs(g - w)
    return float(np.max(np.where(d == 0.0, 0.0, d / np.maximum(np.abs(w), 1e-300))))


# ------------------------------------------------------------------------------------------------
# the rank-thread harness
# ------------------------------------------------------------------------------------------------
def run_ranks(world, job, collective="callback", shm_name=None, wait=60.0, check=True):
    """`world` ranks of one job as threads of this process, each with a PathEngine of its own.

    collective "callback": the engines run on torch's stream and all-reduce through set_allreduce -- the callback stages the
    buffer through the host and sums the parts in rank order between two waits of a threading.Barrier (the same bits on every
    rank).  "shm": the library's own node-local collective, init_shm(shm_name, rank, world).

    job(rank, engine, counts) -> anything; counts is the list the rank's callback appends every all-reduce's length to (it
    stays empty with "shm").  Returns (results, counts per rank, errors as (rank, exception)).

    The barrier times out after `wait` seconds; a rank that raises aborts it, so a peer inside a callback gets
    BrokenBarrierError, its callback returns non-zero and its pricer ends with MCG_ERR_COMM.  Over "shm" a peer left alone in
    a collective is released by the library's own barrier time-out (120 s), which the joins outlast.  A thread that is still
    alive after its join fails the test; check=True also fails it on any rank's error."""
    import torch
    bar, lock, parts = threading.Barrier(world, timeout=wait), threading.Lock(), {}
    res, errs, counts = [None] * world, [], [[] for _ in range(world)]

    def allreduce(rank):
        def fn(ptr, count, _stream):
            t = torch.as_tensor(_DevView(ptr, count), device="cuda:0")
            h = t.cpu().numpy().copy()                    # (waits for the producing kernel: the engine runs on torch's stream)
            with lock:
                parts[rank] = h
            bar.wait()                                    # all parts are in
            tot = np.zeros(count)
            for r in range(world):
                tot += parts[r]                           # rank order: the same bits on every rank
            bar.wait()                                    # everybody has summed before anybody overwrites its part
            t.copy_(torch.from_numpy(tot))
            counts[rank].append(count)
        return fn

    def work(rank):
        e = None
        try:
            if collective == "callback":
                torch.cuda.set_device(0)
                e = mc.PathEngine(0, stream=torch.cuda.current_stream().cuda_stream)
                e.set_allreduce(allreduce(rank))
            else:
                e = mc.PathEngine(0)
                e.init_shm(shm_name, rank, world)
            res[rank] = job(rank, e, counts[rank])
            e.synchronize()
            bar.wait()                                    # nobody closes its engine while a peer is still inside the job
        except BaseException as ex:   # noqa: BLE001
            errs.append((rank, ex))
            bar.abort()
        finally:
            if e is not None:
                try:
                    e.close()
                except Exception as ex:   # noqa: BLE001
                    errs.append((rank, ex))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    deadline = time.monotonic() + (wait + 30.0 if collective == "callback" else 180.0)
    for t in th:
        t.join(max(0.1, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(th) if t.is_alive()]
    assert not alive, f"rank threads {alive} still alive; errors so far: {errs}"
    if check:
        assert not errs, errs
    return res, counts, errs


def shard_paths(e, rank, shards, steps):
    b, c = shards[rank]
    return e.gbm(SEED, S0, R, SIGMA, DT, steps, c, path_begin=b)


def same_on_every_rank(res):
    assert all(r == res[0] for r in res[1:]), res


# ------------------------------------------------------------------------------------------------
# the whole matrices and the oracle's numbers on them: computed once, never changed
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc():
    return Oracle()


class Whole:
    """The single engine's matrix of all paths, step-major on the host, and a cache of what the oracle says about it."""

    def __init__(self, orc, steps, n):
        with mc.PathEngine(0) as e:
            P = e.gbm(SEED, S0, R, SIGMA, DT, steps, n)
            self.host = P.to_host_step_major()
            self.host.setflags(write=False)
            P.free()
        self.orc, self.steps, self.n, self._cache = orc, steps, n, {}

    def _memo(self, key, f):
        if key not in self._cache:
            self._cache[key] = f()
        return self._cache[key]

    def asymptotic(self, is_call, maturity):
        return self._memo(("a", is_call, maturity),
                          lambda: self.orc.asymptotic_price(self.host, R, K, maturity, DT, is_call, SIGMA, DIVIDEND))

    def martingale(self, is_call, order, iters):
        return self._memo(("m", is_call, order, iters),
                          lambda: self.orc.martingale_price(self.host, R, K, self.steps * DT, DT, is_call, order, iters))

    def branching_full(self, is_call, branches):
        ex = np.arange(self.steps, dtype=np.int32)
        return self._memo(("bf", is_call, branches),
                          lambda: self.orc.branching_price(self.host, R, K, self.steps * DT, DT, is_call, branches, ex, BR_SEED,
                                                           mode="philox", path_begin=0))

    def branching_sharded(self, is_call, branches, shards):
        """The device resamples WITHIN the local shard: (price, lower, upper) = the shards' own oracle bounds weighted by
        their path counts, the price their midpoint."""
        def f():
            ex = np.arange(self.steps, dtype=np.int32)
            lo = up = 0.0
            for b, c in shards:
                if c == 0:
                    continue
                w = self.orc.branching_price(np.ascontiguousarray(self.host[:, b:b + c]), R, K, self.steps * DT, DT, is_call, branches,
                                             ex, BR_SEED, mode="philox", path_begin=b)
                lo += c * w[1]
                up += c * w[2]
            lo, up = lo / self.n, up / self.n
            return 0.5 * (lo + up), lo, up
        return self._memo(("bs", is_call, branches, tuple(shards)), f)


@pytest.fixture(scope="module")
def whole(orc):
    return Whole(orc, STEPS, sum(c for _, c in SHARDS))


@pytest.fixture(scope="module")
def whole_br(orc):
    return Whole(orc, BR_STEPS, sum(c for _, c in BR_SHARDS))


# ------------------------------------------------------------------------------------------------
# the three jobs (the same under both collectives) and what they must return
# ------------------------------------------------------------------------------------------------
def asymptotic_job(rank, e, counts):
    P = shard_paths(e, rank, SHARDS, STEPS)
    out = [e.price_asymptotic(P, R, K, maturity, DT, is_call, SIGMA, DIVIDEND) for is_call, maturity in ASYM_CASES]
    shard = P.to_host_step_major()
    P.free()
    return out, shard, list(counts)


def check_asymptotic(res, want, label):
    same_on_every_rank([r[0] for r in res])
    worst = 0.0
    for got, w in zip(res[0][0], want):
        worst = max(worst, rel(got, w))
        assert abs(got - w) <= 1e-12 * abs(w), (got, w)
    print(f"[sharded] asymptotic {label}: worst rel {worst:.3e}")


def martingale_job(cases):
    def job(rank, e, counts):
        P = shard_paths(e, rank, SHARDS, STEPS)
        out, lists = [], []
        for is_call, order, iters in cases:
            n0 = len(counts)
            out.append(e.price_martingale(P, R, K, STEPS * DT, DT, is_call, order, iters))
            lists.append(counts[n0:])
        P.free()
        return out, lists
    return job


def check_martingale(res, cases, whole, label):
    same_on_every_rank([r[0] for r in res])
    worst = {}
    for (is_call, order, iters), got in zip(cases, res[0][0]):
        want = whole.martingale(is_call, order, iters)
        worst[order] = max(worst.get(order, 0.0), rel(got, want))
        print(f"[sharded] martingale {label} call={is_call} order={order} iters={iters}: got {got} want {want} rel {rel(got, want):.3e}")
        assert np.allclose(got, want, rtol=mo_rtol(order), atol=1e-12), (is_call, order, iters, got, want)
        assert abs(got[0] - 0.5 * (got[1] + got[2])) <= 1e-13 * abs(got[0])
    print(f"[sharded] martingale {label}: worst rel per order {worst}")


def branching_job(rank, e, counts):
    P = shard_paths(e, rank, BR_SHARDS, BR_STEPS)
    ex = np.arange(BR_STEPS, dtype=np.int32)
    out, lists = [], []
    for is_call, branches in BR_CASES:
        n0 = len(counts)
        out.append(e.price_branching(P, R, K, BR_STEPS * DT, DT, is_call, branches, ex, seed=BR_SEED))
        lists.append(counts[n0:])
    P.free()
    return out, lists


def check_branching(res, whole_br, label):
    same_on_every_rank([r[0] for r in res])
    worst = 0.0
    for (is_call, branches), got in zip(BR_CASES, res[0][0]):
        want = whole_br.branching_sharded(is_call, branches, BR_SHARDS)
        full = whole_br.branching_full(is_call, branches)
        worst = max(worst, rel(got, want), rel(got[1], full[1]))
        print(f"[sharded] branching {label} call={is_call} branches={branches}: got {got} want {want} (unsharded oracle {full})")
        assert np.allclose(got, want, rtol=1e-12, atol=1e-14), (is_call, branches, got, want)
        assert np.isclose(got[1], full[1], rtol=1e-12, atol=1e-14), (got[1], full[1])     # the lower bound does not resample
        # resampling over all N paths instead of the shard's own would give the unsharded upper bound: the two must differ,
        # or this case could not tell them apart
        assert abs(want[2] - full[2]) > 1e-9 * full[2], (want, full)
    print(f"[sharded] branching {label}: worst rel {worst:.3e}")


# ------------------------------------------------------------------------------------------------
# 1. sharded equals unsharded: callback collective, world size 3
# ------------------------------------------------------------------------------------------------
def test_asymptotic_sharded_over_three_ranks_equals_the_oracle_on_the_whole_matrix(whole):
    """price = sum of bests / sum of valid paths, both all-reduced, while finish_sums is handed the LOCAL n: without the
    all-reduce every rank would return its own shard's mean (and the empty one 0.0).  Each shard's matrix equals its columns of
    the single engine's matrix bit for bit, every rank returns the same bits, and they equal the oracle on the whole matrix to
    1e-12; one all-reduce of 3 doubles per price on every rank, the empty one included.
    Measured on an MI355X (worst relative difference over put / call, maturity on the last date / between two dates):
    1.6e-14."""
    res, counts, _ = run_ranks(3, asymptotic_job)
    for rank, (b, c) in enumerate(SHARDS):
        assert res[rank][1].shape == (STEPS + 1, c) and np.array_equal(res[rank][1], whole.host[:, b:b + c])
        assert res[rank][2] == [3] * len(ASYM_CASES) == counts[rank]
    check_asymptotic(res, [whole.asymptotic(*c) for c in ASYM_CASES], "callback")


def dirty_matrix(whole):
    """Row-major copy of the whole matrix with NaN, +inf and -inf in a few dozen cells of the LAST shard, one of its paths
    non-finite at every date."""
    a = np.ascontiguousarray(whole.host.T).copy()
    b, c = SHARDS[2]
    rs = np.random.RandomState(5)
    bad = [np.nan, np.inf, -np.inf]
    for k in range(40):
        a[b + rs.randint(c), rs.randint(STEPS + 1)] = bad[k % 3]
    a[b + 12_345, :] = [bad[j % 3] for j in range(STEPS + 1)]
    a[b + c - 1, STEPS] = np.nan                                   # the job's very last cell
    return a


def test_asymptotic_sharded_skips_non_finite_cells_like_the_oracle(whole, orc):
    """The same job with the shards uploaded (from_host) from a matrix with NaN, +inf and -inf in a few dozen cells of the last shard and
    one path non-finite at every date (AsymptoticAnalysisPricer.cpp:74, :89, :103-106); the middle shard stays empty.  The oracle
    sees the same dirty matrix.  Measured on an MI355X: worst relative difference 1.6e-14."""
    dirty = dirty_matrix(whole)
    assert 40 <= np.count_nonzero(~np.isfinite(dirty)) <= 42 + STEPS + 1

    def job(rank, e, counts):
        b, c = SHARDS[rank]
        P = e.from_host(dirty[b:b + c]) if c else shard_paths(e, rank, SHARDS, STEPS)
        out = [e.price_asymptotic(P, R, K, maturity, DT, is_call, SIGMA, DIVIDEND) for is_call, maturity in ASYM_CASES]
        P.free()
        return out, None, list(counts)

    res, _, _ = run_ranks(3, job)
    want = [orc.asymptotic_price(dirty, R, K, maturity, DT, is_call, SIGMA, DIVIDEND, step_major=False) for is_call, maturity in ASYM_CASES]
    clean = [whole.asymptotic(*c) for c in ASYM_CASES]
    assert any(w != c for w, c in zip(want, clean))                # (the dirt is where it matters)
    check_asymptotic(res, want, "callback, non-finite cells")


def test_martingale_sharded_over_three_ranks_equals_the_oracle_on_the_whole_matrix(whole):
    """Orders 2, 6 and 15 (5 iterations), order 2 with 1 iteration, put and call at order 2.  What is all-reduced: the 3 (order+1)
    doubles of the refit's moments with the primal sum behind them -- once, or twice when the first solve asks for the re-centred
    second pass (every rank must take that branch or none) --, then the offset sum and the dual sum with the path count, 3 doubles
    each.  offset = sum M(S_0) / N with the ALL-REDUCED N: the local N would move `upper`.  (price, lower, upper) on every rank:
    the same bits, equal to the oracle on the whole matrix at the tolerances of test_martingale_matches_oracle; every rank, the
    empty one included, records the same list of all-reduce lengths, and it is the list a single engine with an identity
    collective records on the whole matrix.
    Measured on an MI355X, worst relative difference of the three numbers: 3.8e-13 at order 2, 7.4e-13 at order 6,
    8.3e-13 at order 15 (the lists: [9, 3, 3] at order 2, [21, 21, 3, 3] and [48, 48, 3, 3] at orders 6 and 15)."""
    res, _, _ = run_ranks(3, martingale_job(MO_CASES))
    check_martingale(res, MO_CASES, whole, "callback")
    with mc.PathEngine(0) as e:
        single = []
        e.set_allreduce(lambda ptr, count, stream: single.append(count))
        P = e.gbm(SEED, S0, R, SIGMA, DT, STEPS, whole.n)
        for i, (is_call, order, iters) in enumerate(MO_CASES):
            n0 = len(single)
            e.price_martingale(P, R, K, STEPS * DT, DT, is_call, order, iters)
            lst = single[n0:]
            nm = 3 * (order + 1)
            assert lst in ([nm, 3, 3], [nm, nm, 3, 3]), (order, lst)
            for rank in range(3):
                assert res[rank][1][i] == lst, (rank, order, res[rank][1][i], lst)
        P.free()
    print("[sharded] martingale all-reduce lengths:", res[1][1])


def test_martingale_with_fewer_samples_than_coefficients_keeps_the_fit_at_zero(orc):
    """Shards of 1, 0 and 2 paths at order 6: 6 samples in all, fewer than order + 1 -- judged on the all-reduced count --, so
    M stays 0 (MartingaleOptimizationPricer.cpp:150-153), the dual equals the primal, and all three numbers are the oracle's on
    the 3-path matrix (three summands in another order: 1e-14)."""
    shards = [(0, 1), (1, 0), (1, 2)]
    k_itm = 105.0
    with mc.PathEngine(0) as e:
        P = e.gbm(SEED, S0, R, SIGMA, DT, STEPS, 3)
        host = P.to_host_step_major()
        P.free()
    want = orc.martingale_price(host, R, k_itm, STEPS * DT, DT, False, 6, 5)

    def job(rank, e, counts):
        P = shard_paths(e, rank, shards, STEPS)
        got = e.price_martingale(P, R, k_itm, STEPS * DT, DT, False, 6, 5)
        P.free()
        return got, list(counts)

    res, _, _ = run_ranks(3, job)
    same_on_every_rank(res)
    got = res[0][0]
    print(f"[sharded] martingale tiny total: got {got} want {want}")
    assert got[1] > 0.0 and got[2] == got[1]
    assert np.allclose(got, want, rtol=1e-14, atol=0.0), (got, want)
    assert res[0][1] == [21, 3, 3]


def test_branching_sharded_over_three_ranks_equals_the_oracle_shard_by_shard(whole_br):
    """12 steps, exercise list 0..11, seed 99, 6 and 10 branches (a call too at 10).  The device resamples within the LOCAL shard
    -- indices in [0, n_local) from counters keyed by path_begin + p --, so lower and upper are the shards' own oracle bounds
    weighted by their path counts and the price their midpoint; the lower bound, which does not resample, also equals the
    oracle's on the whole matrix.  The empty shard runs k_branch_suffix over no path, takes k_branch_bounds' early-out and still
    enters the one all-reduce of 3 doubles.
    Measured on an MI355X: worst relative difference 3.9e-15."""
    res, _, _ = run_ranks(3, branching_job)
    check_branching(res, whole_br, "callback")
    for rank in range(3):
        assert res[rank][1] == [[3]] * len(BR_CASES), (rank, res[rank][1])


def test_every_shard_empty():
    """World size 2, no path anywhere: AsymptoticAnalysis returns 0.0 (AsymptoticAnalysisPricer.cpp:47-49), the other two raise
    the reference's "Empty pricePaths." -- on BOTH ranks, after the collectives that tell them so, and nobody is left waiting."""
    def job(rank, e, counts):
        P = e.gbm(SEED, S0, R, SIGMA, DT, STEPS, 0, path_begin=0)
        out = [e.price_asymptotic(P, R, K, STEPS * DT, DT, False, SIGMA, DIVIDEND)]
        for f in (lambda: e.price_martingale(P, R, K, STEPS * DT, DT, False, 2, 5),
                  lambda: e.price_branching(P, R, K, STEPS * DT, DT, False, 10, np.arange(STEPS, dtype=np.int32), seed=BR_SEED)):
            try:
                out.append(f())
            except mc.McgError as ex:
                out.append((str(ex), ex.status))
        P.free()
        return out, list(counts)

    res, _, _ = run_ranks(2, job, wait=30.0)
    for out, lengths in res:
        assert out[0] == 0.0
        assert out[1] == ("MartingaleOptimization: Empty pricePaths.", 6)
        assert out[2] == ("BranchingProcesses: Empty pricePaths.", 6)
        assert lengths == [3, 9, 3, 3]


def test_a_rank_that_raises_ends_its_peers_with_a_comm_error():
    """The harness itself: rank 1 raises before it prices anything; ranks 0 and 2, inside their first all-reduce, get a broken
    barrier, their callbacks return non-zero and price_asymptotic ends with MCG_ERR_COMM -- at once, no thread left."""
    def job(rank, e, counts):
        if rank == 1:
            raise ValueError("rank 1 gives up")
        P = shard_paths(e, rank, [(0, 300), (300, 0), (300, 300)], 4)
        try:
            return e.price_asymptotic(P, R, K, 4 * DT, DT, False, SIGMA, DIVIDEND)
        finally:
            P.free()

    _, _, errs = run_ranks(3, job, wait=20.0, check=False)
    by_rank = dict(errs)
    assert sorted(by_rank) == [0, 1, 2] and isinstance(by_rank[1], ValueError)
    for rank in (0, 2):
        assert isinstance(by_rank[rank], mc.McgError) and by_rank[rank].status == MCG_ERR_COMM, by_rank[rank]


def test_argument_errors_raise_before_any_collective():
    """maxIterations = 0, sigma = 0 and an empty exercise list are refused before the first all-reduce: a rank that raised them
    after one would have left its peers a collective behind."""
    with mc.PathEngine(0) as e:
        calls = []
        e.set_allreduce(lambda ptr, count, stream: calls.append(count))
        P = e.gbm(SEED, S0, R, SIGMA, DT, STEPS, 1000)
        with pytest.raises(mc.McgError, match="MartingaleOptimization: maxIterations must be positive."):
            e.price_martingale(P, R, K, STEPS * DT, DT, False, 2, 0)
        with pytest.raises(mc.McgError, match="AsymptoticAnalysis: Volatility must be positive."):
            e.price_asymptotic(P, R, K, STEPS * DT, DT, False, 0.0, DIVIDEND)
        with pytest.raises(mc.McgError, match="BranchingProcesses: No exercise times."):
            e.price_branching(P, R, K, STEPS * DT, DT, False, 10, np.zeros(0, dtype=np.int32), seed=BR_SEED)
        assert calls == []
        P.free()


# ------------------------------------------------------------------------------------------------
# 2. an identity collective changes nothing (world size 1)
# ------------------------------------------------------------------------------------------------
def test_an_identity_collective_changes_no_bit():
    """20 000 x 24, an engine with set_allreduce(identity) against an engine without.  AsymptoticAnalysis and BranchingProcesses
    run identical launches.  MartingaleOptimization's solve is split (lsm_reduce_allreduce_solve: reduce, all-reduce, solve
    instead of one launch), but k_lsm_reduce_solve does the same arithmetic either way: the reduce leaves every moment both in
    `moments` and in LDS as the same double, and the solve -- one thread, the same code -- reads the one or the other.  So all
    three are held to identical bits (measured on an MI355X: all differences 0)."""
    def prices(e):
        P = e.gbm(SEED, S0, R, SIGMA, DT, STEPS, 20_000)
        ex = np.arange(STEPS, dtype=np.int32)
        out = [e.price_asymptotic(P, R, K, m, DT, c, SIGMA, DIVIDEND) for c, m in ASYM_CASES]
        out += [e.price_martingale(P, R, K, STEPS * DT, DT, c, order, iters) for c, order, iters in MO_CASES]
        out += [e.price_branching(P, R, K, STEPS * DT, DT, c, b, ex, seed=BR_SEED) for c, b in BR_CASES]
        P.free()
        return out

    with mc.PathEngine(0) as plain, mc.PathEngine(0) as ident:
        calls = []
        ident.set_allreduce(lambda ptr, count, stream: calls.append(count))
        a, b = prices(plain), prices(ident)
    assert len(calls) >= len(ASYM_CASES) + 3 * len(MO_CASES) + len(BR_CASES)
    worst = max(rel(x, y) for x, y in zip(a, b))
    print(f"[identity] worst rel {worst:.3e}")
    assert a == b, [(x, y) for x, y in zip(a, b) if x != y]


# ------------------------------------------------------------------------------------------------
# 3. the same jobs over the library's own shared-memory collective
# ------------------------------------------------------------------------------------------------
SHM_MO_CASES = [(False, 2, 5), (False, 15, 5)]


def test_asymptotic_sharded_over_the_shared_memory_collective(whole):
    """The job of test_asymptotic_sharded_over_three_ranks_... with init_shm instead of the callback, the empty middle shard
    included.  Measured on an MI355X: worst relative difference 1.6e-14 (the callback job's bits)."""
    res, _, _ = run_ranks(3, asymptotic_job, collective="shm", shm_name=f"/mcg_pricers_asym_{os.getpid()}")
    check_asymptotic(res, [whole.asymptotic(*c) for c in ASYM_CASES], "shm")


def test_martingale_sharded_over_the_shared_memory_collective(whole):
    """Orders 2 and 15 over init_shm: order 15 sends 48 doubles through shm_allreduce, which takes up to SHM_FLAG_SLOT - 1 = 62
    and had never carried more than 8.  Measured on an MI355X: worst relative difference 1.1e-13 at order 2, 8.3e-13 at order 15
    (the callback job's bits)."""
    res, _, _ = run_ranks(3, martingale_job(SHM_MO_CASES), collective="shm", shm_name=f"/mcg_pricers_mo_{os.getpid()}")
    check_martingale(res, SHM_MO_CASES, whole, "shm")


def test_branching_sharded_over_the_shared_memory_collective(whole_br):
    """The job of test_branching_sharded_over_three_ranks_... over init_shm.  Measured on an MI355X: worst relative difference
    3.9e-15 (the callback job's bits)."""
    res, _, _ = run_ranks(3, branching_job, collective="shm", shm_name=f"/mcg_pricers_br_{os.getpid()}")
    check_branching(res, whole_br, "shm")


# ------------------------------------------------------------------------------------------------
# 4. edge shapes of the device-resident entry points (one engine, no collective)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = mc.PathEngine(0)
    yield e
    e.close()


def maturities(n_steps):
    return [("last date", n_steps * DT), ("between two dates", (n_steps - 0.5) * DT), ("beyond the matrix", (n_steps + 3.5) * DT),
            ("smaller than dt", 0.5 * DT), ("negative", -DT)]


@pytest.mark.parametrize("n_steps", [1, 2, 50])
@pytest.mark.parametrize("n_paths", [1, 2, 63, 64, 65, 255, 256, 257, 1023])
def test_edge_shapes_of_the_device_resident_pricers(eng, orc, n_paths, n_steps):
    """k_asym_scan, k_mo_primal / k_mo_offset / k_mo_dual and k_branch_suffix / k_branch_bounds(_any) reduce with the 256-thread
    block_sum<.,4>: 1 .. 1023 paths are its partial-wave, one-wave, partial-workgroup and several-workgroup cases; 1, 2 and 50
    steps; a generator with a non-zero path_begin (BranchingProcesses keys its counters by it).  Maturities: on the last date,
    between two dates, beyond the matrix (every column a date; with 50 steps T - t > 1 makes early boundaries NaN), smaller than
    dt (column 0 alone) and negative (no date: the oracle's numbers, nothing read out of range).  num_branches 0, 1, 4, 5, 12, 13
    are the quad boundaries; 13 takes k_branch_bounds_any.  MartingaleOptimization at orders 0 and 2.  The matrix again through
    from_host with non-finite cells for AsymptoticAnalysis.  Rows are padded to whole 256-path blocks (paths_new), so ld differs
    from n_paths at every size here but 256 -- read from PathMatrix's info.
    Measured on an MI355X over all 27 shapes, worst relative difference: AsymptoticAnalysis 1.1e-15, BranchingProcesses
    2.3e-15, MartingaleOptimization 1.6e-13 (duals that are 0 but for the rounding of M(S_0) - offset: within 3.4e-15 absolute)."""
    begin = 1_000_003
    P = eng.gbm(SEED, S0, R, SIGMA, DT, n_steps, n_paths, path_begin=begin)
    assert P.n_paths == n_paths and P.n_steps == n_steps and P.ld == (n_paths + 255) // 256 * 256
    assert (P.ld != n_paths) == (n_paths % 256 != 0)
    host = P.to_host_step_major()
    assert rel(host, orc.paths_gbm(SEED, S0, R, SIGMA, DT, n_steps, begin, n_paths)) < 1e-11
    ex = np.arange(n_steps, dtype=np.int32)
    dirty = np.ascontiguousarray(host.T).copy()
    rs = np.random.RandomState(n_paths * 100 + n_steps)
    for k in range(min(12, dirty.size)):
        dirty[rs.randint(n_paths), rs.randint(n_steps + 1)] = [np.nan, np.inf, -np.inf][k % 3]
    dirty[n_paths // 2, :] = np.nan
    Q = eng.from_host(dirty)
    assert Q.ld == P.ld
    worst = dict(asym=0.0, mo=0.0, mo_abs_near_zero=0.0, br=0.0)
    for what, T in maturities(n_steps):
        for is_call in (False, True):
            for M, h, sm in ((P, host, True), (Q, dirty, False)):
                got = eng.price_asymptotic(M, R, K, T, DT, is_call, SIGMA, DIVIDEND)
                want = orc.asymptotic_price(h, R, K, T, DT, is_call, SIGMA, DIVIDEND, step_major=sm)
                worst["asym"] = max(worst["asym"], rel(got, want))
                assert abs(got - want) <= 1e-12 * abs(want), ("asymptotic", what, is_call, sm, got, want)
            for order in (0, 2):
                got = eng.price_martingale(P, R, K, T, DT, is_call, order, 5)
                want = orc.martingale_price(host, R, K, T, DT, is_call, order, 5)
                # (a dual that is 0 but for the rounding of M(S_0) - offset has no relative difference to speak of: reported apart)
                big = np.abs(want) > 1e-9
                worst["mo"] = max(worst["mo"], rel(np.asarray(got)[big], np.asarray(want)[big]) if big.any() else 0.0)
                worst["mo_abs_near_zero"] = max(worst["mo_abs_near_zero"], float(np.max(np.abs(np.asarray(got) - want)[~big], initial=0.0)))
                assert np.allclose(got, want, rtol=1e-8, atol=1e-12), ("martingale", what, is_call, order, got, want)
        for branches in (0, 1, 4, 5, 12, 13):
            got = eng.price_branching(P, R, K, T, DT, False, branches, ex, seed=BR_SEED)
            want = orc.branching_price(host, R, K, T, DT, False, branches, ex, BR_SEED, mode="philox", path_begin=begin)
            worst["br"] = max(worst["br"], rel(got, want))
            assert np.allclose(got, want, rtol=1e-12, atol=1e-14), ("branching", what, branches, got, want)
    print(f"[edge] {n_paths} x {n_steps}: worst rel {worst}")
    P.free()
    Q.free()
