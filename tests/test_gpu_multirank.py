"""C5 at its real shard size, and the N>1 PRODUCT path with two (and four) real ranks (run with -m gpu on an MI355X).

  * test_c5_shard_full_size: BASELINE.json configs[4] as one of its eight shards -- rBergomi (H = 0.1, eta = 1.9)
    8M paths x 252 steps, American put, LSM order 2 -- through the per-date kernels every sharded run takes, once
    without and once with a collective installed (a no-op: world size 1).
  * test_two_rank_processes_equal_single_rank: two fresh child processes on GPU 0 (tests/mp_rank_worker.py), gloo
    between them, mcg_set_allreduce on each ctx; European, GBM-LSM and rBergomi-LSM prices of the sharded job must
    equal the single-rank run on the same global path ids (European 1e-12: only the order of three additions
    differs; LSM 1e-9: the regression moments are summed in a different order).
"""
import json
import math
import os
import socket
import subprocess
import sys

import pytest

import montecarlooptionspricer_amd as mc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, DT = 20251031, 1.0 / 252.0
RB = dict(S0=100.0, r=0.04, xi=0.04, H=0.1, eta=1.9, rho=-0.9)


def test_c5_shard_full_size():
    n, steps = 8_000_000, 252
    T = steps * DT
    a = mc.PathEngine(0)
    P = a.rbergomi(SEED, RB["S0"], RB["r"], RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, steps, n, payoff=(100.0, False))
    eu, ese = a.price_european(P, 100.0, RB["r"], T, False)
    am, ase = a.price_lsm(P, RB["r"], 100.0, T, DT, False, 2)
    assert math.isfinite(am) and math.isfinite(ase) and ase > 0
    assert eu - 3.0 * ese < am < 100.0                      # American put >= European put on the same paths
    c, cse = a.price_european(P, 100.0, RB["r"], T, True)    # martingale through put-call parity on the same paths
    fwd = math.exp(RB["r"] * T) * (c - eu) + 100.0
    assert abs(fwd - 100.0 * math.exp(RB["r"] * T)) <= 2.0 * math.exp(RB["r"] * T) * math.hypot(cse, ese)
    P.free()
    a.trim()

    b = mc.PathEngine(0)
    calls = []
    b.set_allreduce(lambda ptr, count, stream: calls.append(count))   # world size 1: the sum over ranks is the identity
    Q = b.rbergomi(SEED, RB["S0"], RB["r"], RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, steps, n, payoff=(100.0, False))
    eu2, ese2 = b.price_european(Q, 100.0, RB["r"], T, False)
    am2, ase2 = b.price_lsm(Q, RB["r"], 100.0, T, DT, False, 2)
    Q.free()
    b.close()
    a.close()
    assert eu2 == eu and ese2 == ese
    assert abs(am2 - am) <= 1e-9 * am and abs(ase2 - ase) <= 1e-9 * ase
    # 3p+2 moments between two launches of the per-date kernel (exactly one launch per column: no spare launch, no spare
    # collective), the sweep's fault flag once, payoff + final sums
    assert calls.count(8) == per_date_launches(steps) - 1 and calls.count(3) == 2 and calls.count(1) == 1


def per_date_launches(steps, refits=0):
    """k_lsm_date launches of a sweep over `steps` + 1 columns: one per column, plus one per re-fitted date -- the host
    queues exactly those (kernels_lsm.hip: run_lsm reads the device-side state back and queues what is left)."""
    return steps + 1 + refits


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, world, worker_mode, tag="res"):
    port, out = _free_port(), str(tmp_path / f"{tag}.json")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "mp_rank_worker.py"), str(r), str(world), str(port), out, worker_mode],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return [json.load(open(f"{out}.{r}")) for r in range(world)], logs


@pytest.mark.parametrize("mode", ["gloo", "shm", "shm_timeout", "shm4", "ipc", "ipc4"])
def test_two_rank_processes_equal_single_rank(tmp_path, mode):
    """mode "gloo": a host all-reduce callback, the per-date LSM kernels (what RCCL runs use).  mode "shm": the
    library's node-local shared-memory communicator -- each rank's LSM sweep is ONE launch, and the two persistent
    kernels exchange their per-date moments through the device-mapped mailbox while both are resident on the GPU.
    mode "shm_timeout": the same with every hand-shake forced to give up: the ranks agree (sum of their time-out flags)
    to discard the sweep and answer from the per-date kernels over the segment's host all-reduce.  mode "shm4": FOUR ranks
    on the one GPU through the shared-memory communicator (four mailbox rows per round, four persistent grids resident
    together), unequal shards.  modes "ipc" / "ipc4": the mailbox in device memory, every rank's copy mapped into the
    peers by HIP IPC (on this one-GPU box the peers' copies are the same HBM; on a node they are reached over xGMI)."""
    sys.path.insert(0, HERE)
    from mp_rank_worker import JOBS

    world = 4 if mode in ("shm4", "ipc4") else 2
    worker_mode = {"shm4": "shm", "ipc4": "ipc"}.get(mode, mode)
    ranks, logs = _run_ranks(tmp_path, world, worker_mode)

    e = mc.PathEngine(0)
    P = e.gbm(SEED, 100.0, 0.04, 0.2, DT, 252, JOBS["euro_paths"], payoff=(100.0, True))
    want_euro = e.price_european(P, 100.0, 0.04, 1.0, True)
    P.free()
    P = e.gbm(SEED, 100.0, 0.04, 0.2, 0.02, JOBS["lsm_steps"], JOBS["lsm_paths"])
    want_lsm = e.price_lsm(P, 0.04, 100.0, 1.0, 0.02, False, 2)
    P.free()
    T = JOBS["rb_steps"] * DT
    P = e.rbergomi(SEED, RB["S0"], RB["r"], RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, JOBS["rb_steps"], JOBS["rb_paths"])
    want_rb = e.price_lsm(P, RB["r"], 100.0, T, DT, False, 2)
    want_rb_eu = e.price_european(P, 100.0, RB["r"], T, False)
    P.free()
    e.close()

    # near-degenerate dates: the sharded job must reproduce the reference's rank rule (oracle, 1e-6) on every route
    from mp_rank_worker import DEGENERATE, near_degenerate_matrix
    from oracle.binding import Oracle
    orc = Oracle()
    want_deg = [orc.lsm_price(near_degenerate_matrix(*d), 0.04, 100.0, 1.0, 0.5, False, 2, step_major=False) for d in DEGENERATE]
    for r, res in enumerate(ranks):
        for got, want, d in zip(res["degenerate_lsm"], want_deg, DEGENERATE):
            assert abs(got - want) <= 1e-6 * abs(want), (mode, r, d, got, want)

    for r, res in enumerate(ranks):                          # every rank holds the GLOBAL price
        for got, want, tol in ((res["euro"], want_euro, 1e-12), (res["rb_euro_put"], want_rb_eu, 1e-12),
                               (res["gbm_lsm"], want_lsm, 1e-9), (res["rb_lsm"], want_rb, 1e-9)):
            assert abs(got[0] - want[0]) <= tol * abs(want[0]), (r, got, want)
            assert abs(got[1] - want[1]) <= max(tol, 1e-9) * abs(want[1]), (r, got, want)
        if mode == "gloo":
            # one all-reduce BETWEEN two launches of the per-date kernel, nothing else per date
            # (plus the three near-degenerate matrices: three columns each, the middle date re-fitted, one final sum each)
            assert res["allreduce_calls"] == {"3": 4 + len(DEGENERATE),
                                              "8": per_date_launches(JOBS["lsm_steps"]) + per_date_launches(JOBS["rb_steps"]) - 2
                                                   + len(DEGENERATE) * (per_date_launches(2, refits=1) - 1)}
            assert res["stats"]["lsm_per_date_refits"] == len(DEGENERATE) and res["stats"]["lsm_per_date_faults"] == 0
            assert res["gbm_lsm_sweep_launches"] == per_date_launches(JOBS["lsm_steps"]) + 1   # + the final sums
            assert res["comm"]["kind"] == "callback"
        elif mode in ("shm", "shm4", "ipc", "ipc4"):
            assert res["one_launch_enabled"], "\n".join(logs)                       # no hand-shake ever timed out
            assert res["stats"]["lsm_one_launch_timeouts"] == 0 and res["stats"]["shm_barrier_failures"] == 0, res["stats"]
            assert res["gbm_lsm_sweep_launches"] == 1 and res["rb_lsm_sweep_launches"] == 1
            assert res["comm"]["n_ranks"] == world and res["comm"]["seen_ranks"] == world and res["comm"]["rank"] == r
            if mode.startswith("ipc"):   # every rank exported, opened and pinged: the mailbox is in device memory
                assert res["peer_mailbox"] and res["comm"]["kind"] == "shm+peer-memory mailbox", "\n".join(logs)
                # ... and switched back to the host mailbox the same job gives the same bits
                assert res["comm_after_disable"]["kind"] == "shm" and res["gbm_lsm_host_mailbox"] == res["gbm_lsm"]
            else:
                assert res["comm"]["kind"] == "shm"
        else:   # forced time-out: the void sweep (1 launch) is discarded on BOTH ranks, the per-date kernels answer
            assert not res["one_launch_enabled"]
            assert res["gbm_lsm_sweep_launches"] == 1 + per_date_launches(JOBS["lsm_steps"]) + 1
            assert res["rb_lsm_sweep_launches"] == per_date_launches(JOBS["rb_steps"]) + 1   # no second attempt straight away
    assert ranks[0]["shard"][0] == 0 and all(r["shard"][0] % 2 == 0 for r in ranks)
    assert sum(r["shard"][1] for r in ranks) == JOBS["rb_paths"]


def test_peer_memory_mailbox_equals_host_mailbox_bit_for_bit(tmp_path):
    """The same two-rank job once through the host mailbox and once through the peer-memory mailbox: the exchange
    carries the same doubles and sums them in the same rank order, so every price is the same to the last bit."""
    host, _ = _run_ranks(tmp_path, 2, "shm", "host")
    peer, logs = _run_ranks(tmp_path, 2, "ipc", "peer")
    assert all(p["peer_mailbox"] for p in peer), "\n".join(logs)
    for a, b in zip(host, peer):
        for key in ("euro", "gbm_lsm", "rb_lsm", "rb_euro_put"):
            assert a[key] == b[key], (key, a[key], b[key])


def test_bench_two_ranks_carries_c2_and_c5_with_the_ranks_seen(tmp_path):
    """The driver's N > 1 command, rehearsed with two ranks on GPU 0 (gloo between them: two RCCL ranks cannot share a
    device): ONE JSON line that carries the C2 headline AND BASELINE.json configs[4] (C5) through the host mailbox, the
    peer-memory mailbox and the RCCL route (here: its torch fall-back, the same per-date kernels), each row with the
    slowest and the fastest rank's time, the collective that actually ran and the ranks its communicator has seen -- and
    every price equal to the single-rank run on the same global path ids."""
    root = os.path.dirname(HERE)
    c2_paths, c5_paths = 1_000_000, 300_000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--paths", str(c2_paths), "--c5-paths", str(c5_paths)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["config"]["global_paths"] == 2 * c2_paths
    assert out["config"]["comm"]["kind"] == "callback"      # C2's collective here: torch.distributed behind mcg_set_allreduce
    rows = out["extra"]["configs"]
    assert [r["collective_requested"] for r in rows] == ["none", "shm", "ipc", "rccl"], rows
    for r in rows:
        assert "error" not in r, r
        assert r["global_paths"] == 2 * c5_paths
        assert r["ms_per_pass_slowest_rank"] >= r["ms_per_pass_fastest_rank"] > 0
    alone, shm, ipc, rccl = rows
    assert alone["comm"]["kind"] == "none" and alone["lsm_one_launch"]        # the baseline: no exchange, a local price
    rows = rows[1:]
    assert shm["collective"] == "shm" and shm["comm"]["kind"] == "shm" and shm["comm"]["seen_ranks_min_over_ranks"] == 2
    assert ipc["collective"] == "ipc" and ipc["comm"]["kind"] == "shm+peer-memory mailbox" and ipc["comm"]["seen_ranks_min_over_ranks"] == 2
    assert shm["comm"]["n_ranks"] == 2 and ipc["comm"]["n_ranks"] == 2
    assert shm["lsm_one_launch"] and ipc["lsm_one_launch"]
    assert shm["rank0_lsm_sweep_launches_per_pass"] == 1 and ipc["rank0_lsm_sweep_launches_per_pass"] == 1
    # two ranks on one device: the built-in RCCL communicator cannot form, the row says so and runs the same per-date
    # kernels over torch.distributed -- one launch per exercise date (+ spare + final sums), one all-reduce between two
    assert rccl["collective"].startswith("torch (built-in RCCL init failed") and rccl["comm"]["kind"] == "callback"
    assert not rccl["lsm_one_launch"] and rccl["rank0_lsm_sweep_launches_per_pass"] == per_date_launches(252) + 1
    assert ipc["price"] == shm["price"] and ipc["std_err"] == shm["std_err"]

    e = mc.PathEngine(0)
    P = e.gbm(SEED, 100.0, 0.04, 0.2, DT, 252, 2 * c2_paths, payoff=(100.0, True))
    want_c2 = e.price_european(P, 100.0, 0.04, 1.0, True)
    P.free()
    P = e.rbergomi(SEED, RB["S0"], RB["r"], RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, 252, 2 * c5_paths)
    want_c5 = e.price_lsm(P, RB["r"], 100.0, 252 * DT, DT, False, 2)
    P.free()
    e.close()
    assert abs(out["parity"]["price"] - want_c2[0]) <= 1e-12 * want_c2[0] and abs(out["parity"]["std_err"] - want_c2[1]) <= 1e-9 * want_c2[1]
    for r in rows:
        assert abs(r["price"] - want_c5[0]) <= 1e-9 * want_c5[0], (r["collective"], r["price"], want_c5)
        assert abs(r["std_err"] - want_c5[1]) <= 1e-9 * want_c5[1]


def test_bench_headline_survives_a_failing_c5_child_job():
    """The C5 rows of an N > 1 run are timed in a child job of their own: if that job dies (forced here), the parent's JSON
    line -- the C2 headline -- is still printed, with a row that says what happened."""
    root = os.path.dirname(HERE)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--paths", "500000", "--c5-paths", "100000"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MCG_BENCH_C5_CHILD_FAIL="1")
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["parity"]["abs_err_over_std_err"] < 4
    rows = out["extra"]["configs"]
    # (whichever parent sees its child's exit code 3 first has every parent end its child: rank 0's row says one or the other)
    assert len(rows) == 1 and ("child job failed (exit code 3)" in rows[0]["error"] or "child job ended by its parents" in rows[0]["error"])
    assert out["config"]["c5_rows"] == "child"


def test_bench_two_ranks_with_the_c5_rows_inline():
    """`--c5-rows inline` (what `auto` picks from four ranks on, where a child process per rank would put 2 x N processes on
    the GPUs): the rows run in the two rank processes themselves after the headline went to rank 0's guardian; same rows,
    same prices as the single-rank run, one JSON line, exit code 0."""
    root = os.path.dirname(HERE)
    c2_paths, c5_paths = 500_000, 200_000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--paths", str(c2_paths), "--c5-paths", str(c5_paths), "--c5-rows", "inline", "--c5-collectives", "none,ipc,rccl"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["config"]["c5_rows"] == "inline" and "aborted" not in out and out["value"] > 0
    rows = out["extra"]["configs"]
    assert [r["collective_requested"] for r in rows] == ["none", "ipc", "rccl"] and all("error" not in r for r in rows), rows
    e = mc.PathEngine(0)
    P = e.rbergomi(SEED, RB["S0"], RB["r"], RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, 252, 2 * c5_paths)
    want = e.price_lsm(P, RB["r"], 100.0, 252 * DT, DT, False, 2)
    P.free()
    e.close()
    assert rows[1]["comm"]["n_ranks"] == 2 and rows[1]["collective"] == "ipc"
    for r in rows[1:]:        # (two ranks on one card: the RCCL row runs its torch fall-back, a callback communicator)
        assert abs(r["price"] - want[0]) <= 1e-9 * want[0], r


def test_bench_four_ranks_take_the_rows_inline_by_themselves():
    """World size 4 on the one card (gloo): 2 x 4 processes would be over the pool's process guard, so `--c5-rows auto`
    must decide for `inline` -- four GPU processes, the rows in the rank processes, the line through rank 0's guardian --
    and every sharded row must carry the single-rank price of the same global path ids."""
    root = os.path.dirname(HERE)
    c2_paths, c5_paths = 400_000, 100_000
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--full", "--gpus", "4", "--steps", "2", "--warmup", "1",
           "--backend", "gloo", "--paths", str(c2_paths), "--c5-paths", str(c5_paths), "--c5-collectives", "none,shm"]
    # (four persistent sweeps spinning on ONE card take seconds per pass: one mailbox row is enough here; the peer-memory
    #  mailbox at four ranks is test_two_rank_processes_equal_single_rank[ipc4])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run(cmd, env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["config"]["c5_rows"] == "inline" and "aborted" not in out
    assert out["config"]["global_paths"] == 4 * c2_paths and out["parity"]["abs_err_over_std_err"] < 4
    rows = out["extra"]["configs"]
    assert [r["collective_requested"] for r in rows] == ["none", "shm"] and all("error" not in r for r in rows), rows
    assert rows[1]["comm"]["n_ranks"] == 4 and rows[1]["comm"]["seen_ranks_min_over_ranks"] == 4 and rows[1]["lsm_one_launch"]
    e = mc.PathEngine(0)
    P = e.rbergomi(SEED, RB["S0"], RB["r"], RB["xi"], RB["H"], RB["eta"], RB["rho"], DT, 252, 4 * c5_paths)
    want = e.price_lsm(P, RB["r"], 100.0, 252 * DT, DT, False, 2)
    P.free()
    e.close()
    for r in rows[1:]:
        assert abs(r["price"] - want[0]) <= 1e-9 * want[0], r
