"""The batched row kernels (csrc/kernels_batch.hip) against the oracle, elementwise and price by price, at every order, path
count and row length they serve.  The case lists, the numpy restatement of k_batch_weights and the proof that every pricer
case is well conditioned are in tests/test_batch_rows_reference.py (CPU).

(a) k_batch_weights: the amplitudes and the compensator of every row of one 100-row call, dumped (mcg_debug_batch_row_dump)
    and compared with Oracle.rbergomi_spectrum -- amplitudes on the scale of the row's largest, the compensator relatively.
(b) k_batch_paths<0..3> with the batch's own workgroup map: the dumped block of row i against Oracle.paths_rbergomi with
    path_begin = i << 32, relatively; column 0 is S0 exactly.
(c) the four columns of mcg_batch_price_rows against the oracle's four pricers applied to the DUMPED block: both sides see
    identical numbers, which is what allows tight bounds.
(d) the row kernels on uploaded matrices through the class API (coalesced_fallbacks == 0), against the oracle; and, as a
    second check, the same calls with coalescing off (the single-contract kernels) against the row kernels.
(e) the error paths of the dump hook.
(f) the two hosts of the row kernels (mcg_batch_price_rows and the class API's coalesced calls) on the same dumped blocks,
    one row per LDS class: byte-equal prices.

A price error is |got - want| / K (MartingaleOptimization's price is ~1e-16 where nothing is ever in the money: an error
relative to the price means nothing there).  Each bound is ten times the largest error observed on an MI355X against the
oracle over all cases of this file, and none exceeds what the project already states for the quantity
(test_batch_rows_reference.CAPS).

    quantity                                         observed    bound (test_batch_rows_reference.BOUNDS)
    amplitudes, of the row's largest                 2.93e-15    3e-14      (513 steps, H 0.6)
    compensator, relative                            2.22e-16    2.3e-15
    paths, relative                                  9.77e-15    1e-13      (250 paths, 1020 steps)
    AsymptoticAnalysis                               1.29e-16    1.3e-15
    BranchingProcesses                               6.32e-16    6.4e-15    (64 paths, 700 steps)
    LSM, orders 0..2                                 5.96e-13    6e-12      (4 paths, 128 steps)
    LSM, order 3                                     1.56e-10    1.6e-9     (3 paths, 100 steps: four coefficients on three paths)
    LSM, order 4                                     1.57e-11    1.6e-10
    MartingaleOptimization, orders 0..3              8.72e-13    8.8e-12    (2 paths, order 3)
    MartingaleOptimization, order 4                  2.48e-13    2.5e-12
    single-contract against row kernels              <= 2.6e-14 in every column (0 in most): inside the same bounds

The first run of this file found MartingaleOptimization 8.5e-4 K away from the oracle on a two-path row at order 3: both paths
stop at date 0, S0 enters the regression twice, four samples hold three distinct prices for four coefficients, and of the
least-squares cubics the row kernel (and the single-contract kernel, which agreed with it to the last bit) returned another
one than the reference's minimum-norm solve.  Fixed in lsm_device.hpp (lsm_solve_centered_everywhere); the figures above are
from the fixed kernels.

The issue's six one-line mutants, each in a scratch build: P[k] for P[(M - k) & (M - 1)] fails (a) and every case of (b);
e <= ex_last fails twelve calls of (c) and (d) BranchingProcesses; % n_dates fails five calls of (c); max_iterations >= 1
fails four calls of (c) and (d) MartingaleOptimization; j >= 2 in lsm_wave_body fails twelve calls of (c) and (d) LSM.
dsc = sm + n_cols in k_batch_asym passes everything, and must: the boundaries fill sm[0 .. n_cols) and the discount factors
sm[n_cols .. 2 n_cols), inside the launch's 2 (max_steps + 1) doubles and apart from each other -- any offset >= n_cols
computes the same numbers.
"""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from montecarlooptionspricer_amd.engine import make_rows
from oracle.binding import Oracle
from test_batch_rows_reference import (BOUNDS, D_SEED, DT, H_ETA, PATH_CALLS, R, SEED64, class_api_cases, column_of, four_columns,
                                       lds_class, next_pow2, oracle_four, oracle_price, path_rows, pricer_calls, row,
                                       spectrum_errors, degenerate_cases, weight_rows)

pytestmark = pytest.mark.gpu

observed = {}
second = {}     # the single-contract kernels against the row kernels: a second check, never the reference
worst_at = {}   # (table, column) -> the case of its largest error


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest errors against the oracle in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(observed.items())))
    print("largest differences between the single-contract and the row kernels: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(second.items())))
    for (table, column), where in sorted(worst_at.items(), key=lambda kv: kv[0][1]):
        print(f"  {'oracle' if table == id(observed) else 'single'} {column}: {where}")


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def price_error(got, want, K):
    if math.isnan(want) or math.isnan(got):
        return 0.0 if math.isnan(want) and math.isnan(got) else math.inf
    if math.isinf(want) or math.isinf(got):
        return 0.0 if got == want else math.inf
    return abs(got - want) / K


class Errors:
    """Every figure of a test is taken before the test asserts, so that a failing run still tells all of them."""

    def __init__(self, table=observed):
        self.table, self.missed = table, []

    def note(self, column, err, where):
        if not err <= self.table.get(column, 0.0):
            self.table[column] = err
            worst_at[(id(self.table), column)] = where
        if not err <= BOUNDS[column]:
            self.missed.append((column, err, where))

    def settle(self):
        assert not self.missed, (len(self.missed), sorted(self.missed, key=lambda m: -m[1])[:6])


BATCH = dict(r=R, dt=DT)


def test_weights_elementwise(eng, orc):
    rows = weight_rows()
    arr = make_rows(rows)
    kw = dict(n_paths=2, num_branches=3, poly_order=1, max_iterations=2, seed=SEED64, **BATCH)
    plain = eng.batch_price_rows(arr, **kw)
    errs = Errors()
    for i, d in enumerate(rows):
        out, amp, comp, block = eng.debug_batch_row_dump(arr, i, **kw)
        assert bits(out) == bits(plain), i
        want_amp, want_comp = orc.rbergomi_spectrum(d["H"], d["eta"], DT, d["n_steps"])
        assert amp.shape == want_amp.shape and comp.shape == want_comp.shape
        ea, ec = spectrum_errors(amp, comp, want_amp, want_comp)
        errs.note("amp", ea, (i, d["n_steps"], d["H"], d["eta"]))
        errs.note("comp", ec, (i, d["n_steps"], d["H"], d["eta"]))
    errs.settle()


@pytest.mark.parametrize("n_paths,steps", PATH_CALLS, ids=[str(n) for n, _ in PATH_CALLS])
def test_paths_elementwise(eng, orc, n_paths, steps):
    rows = path_rows(steps)
    arr = make_rows(rows)
    kw = dict(n_paths=n_paths, num_branches=10, poly_order=2, max_iterations=5, seed=SEED64, **BATCH)
    plain = eng.batch_price_rows(arr, **kw)
    errs = Errors()
    for i, d in enumerate(rows):
        out, amp, comp, block = eng.debug_batch_row_dump(arr, i, **kw)
        assert bits(out) == bits(plain), i
        want = orc.paths_rbergomi(SEED64, d["S0"], R, d["xi"], d["H"], d["eta"], d["rho"], DT, d["n_steps"], i << 32, n_paths)
        assert block.shape == want.shape == (d["n_steps"] + 1, n_paths)
        assert (block[0] == d["S0"]).all(), i
        assert np.isfinite(block).all() and (block > 0.0).all(), i
        errs.note("paths", float(np.abs(block / want - 1.0).max()), (n_paths, i, d["n_steps"]))
    errs.settle()


@pytest.mark.parametrize("c", range(15))
def test_batch_columns_on_the_dumped_matrix(eng, orc, c):
    call = pricer_calls()[c]
    rows = call["rows"]
    arr = make_rows(rows)
    kw = dict(n_paths=call["n_paths"], num_branches=call["num_branches"], poly_order=call["poly_order"],
              max_iterations=call["max_iterations"], seed=call["seed"], **BATCH)
    plain = eng.batch_price_rows(arr, **kw)
    assert np.isfinite(plain).all()
    errs = Errors()
    cols = four_columns(call["poly_order"])
    for i, d in enumerate(rows):
        out, amp, comp, block = eng.debug_batch_row_dump(arr, i, **kw)
        assert bits(out) == bits(plain), i
        want = oracle_four(orc, block, d, call, i)
        for col, g, w in zip(cols, plain[i], want):
            errs.note(col, price_error(float(g), float(w), d["strike"]),
                      (c, i, call["n_paths"], d["n_steps"], d["is_call"], d["strike"], d["maturity"], float(g), float(w)))
    errs.settle()


def class_api_price(d):
    a = (d["matrix"], d["r"], d["K"], d["T"], d["dt"], d["is_call"])
    if d["kind"] == "asym":
        return mc.AsymptoticAnalysis().PredictOptionPrice(*a, d["sigma"], d["dividend"])
    if d["kind"] == "branching":
        return mc.BranchingProcesses().PredictOptionPrice(*a, d["num_branches"], list(range(d["matrix"].shape[1] - 1)))
    if d["kind"] == "lsm":
        return mc.LSM().PredictOptionPrice(*a, d["poly_order"])
    return mc.MartingaleOptimization().PredictOptionPrice(*a, d["poly_order"], d["max_iterations"])


def where_of(k, d, got, want):
    return (d["kind"], k, d["matrix"].shape, d["is_call"], d["K"], d["T"], d["dt"], d["r"], d["poly_order"], d["max_iterations"],
            d["num_branches"], got, want)


@pytest.mark.parametrize("kind", ["asym", "branching", "lsm", "mart"])
def test_row_kernels_through_the_class_api(orc, kind):
    cases = class_api_cases(kind) + degenerate_cases(kind)
    errs, errs2 = Errors(), Errors(second)
    mc.set_compat_seed(D_SEED)
    try:
        mc.stats(reset=True)
        rowwise = [class_api_price(d) for d in cases]
        s = mc.stats()
        assert s["coalesced_fallbacks"] == 0 and s["coalesced_calls"] >= len(cases), s
        for k, (d, got) in enumerate(zip(cases, rowwise)):
            want = float(oracle_price(orc, d))
            errs.note(column_of(kind, d["poly_order"]), price_error(got, want, d["K"]), where_of(k, d, got, want))
        mc.set_compat_coalescing(False)
        for k, (d, got) in enumerate(zip(cases, rowwise)):
            single = class_api_price(d)
            errs2.note(column_of(kind, d["poly_order"]), price_error(single, got, d["K"]), where_of(k, d, single, got))
    finally:
        mc.set_compat_coalescing(True)
        mc.set_compat_seed(None)
    errs.settle()
    errs2.settle()


@pytest.mark.parametrize("n_paths", [2, 250])
def test_both_hosts_drive_the_kernels_alike(eng, n_paths):
    """The row kernels have two hosts: run_batch_chunk (mcg_batch_price_rows) and co::run_round (the class API's coalesced
    calls), which share one launch function per kernel.  One call of four rows, one per LDS class (31, 200, 500 and 1020 steps);
    each row's dumped block goes path-major to the class API with the row's own arguments.  AsymptoticAnalysis, LSM (order 2)
    and MartingaleOptimization (order 2, 5 iterations) draw nothing: both hosts launch the same kernel on the same doubles, so
    the prices must be byte-equal to columns 0, 2 and 3 of the batch call.  BranchingProcesses draws with the Philox id
    (row << 32) + path in the batch and with path ids 0 .. n_paths - 1 through the class API: row 0 is the one row whose ids
    agree, and set_compat_seed gives the class API the batch call's key, so column 1 of row 0 is compared as well.
    On the commit before the launch functions existed every one of these 26 prices was byte-equal too."""
    steps_list = (31, 200, 500, 1020)
    rows = [row(s, *H_ETA[i], strike=(95.0, 100.0, 104.0, 99.0)[i], maturity=(1.0, 0.69, 1.5, 1.0)[i] * s * DT, is_call=i % 2,
                s0=96.0 + 2.0 * i, xi=0.04 + 0.02 * i) for i, s in enumerate(steps_list)]
    assert [lds_class(next_pow2(d["n_steps"])) for d in rows] == [0, 1, 2, 3]
    arr = make_rows(rows)
    kw = dict(n_paths=n_paths, num_branches=10, poly_order=2, max_iterations=5, seed=SEED64, **BATCH)
    plain = eng.batch_price_rows(arr, **kw)
    assert np.isfinite(plain).all()
    differ, calls = [], 0
    mc.set_compat_seed(SEED64)
    try:
        mc.stats(reset=True)
        for i, d in enumerate(rows):
            out, amp, comp, block = eng.debug_batch_row_dump(arr, i, **kw)
            assert bits(out) == bits(plain), i
            matrix = np.ascontiguousarray(block.T)
            assert matrix.shape == (n_paths, d["n_steps"] + 1)
            a = (matrix, R, d["strike"], d["maturity"], DT, bool(d["is_call"]))
            got = {0: mc.AsymptoticAnalysis().PredictOptionPrice(*a, d["sigma"], d["dividend"]),
                   2: mc.LSM().PredictOptionPrice(*a, 2),
                   3: mc.MartingaleOptimization().PredictOptionPrice(*a, 2, 5)}
            if i == 0:
                got[1] = mc.BranchingProcesses().PredictOptionPrice(*a, 10, list(range(d["n_steps"])))
            calls += len(got)
            for col, g in sorted(got.items()):
                print(f"\nn_paths {n_paths} row {i} ({d['n_steps']} steps) column {col}: class API {g!r}, batch {float(plain[i][col])!r}", end="")
                if bits(g) != bits(plain[i][col]):
                    differ.append((i, col, g, float(plain[i][col])))
        s = mc.stats()
    finally:
        mc.set_compat_seed(None)
    assert s["coalesced_fallbacks"] == 0 and s["coalesced_calls"] >= calls, s
    assert calls == 13 and not differ, differ


def test_dump_hook_error_paths(eng):
    rows = path_rows((5, 40, 1100, 64))
    rows.append(dict(rows[0], sigma=0.0))             # AsymptoticAnalysis would throw: the call answers the row with zeros
    arr = make_rows(rows)
    kw = dict(n_paths=64, num_branches=10, poly_order=2, max_iterations=5, seed=SEED64, **BATCH)
    plain = eng.batch_price_rows(arr, **kw)
    assert (plain[4] == 0.0).all() and (plain[2] != 0.0).any()
    before = mc.stats()
    for index, words, other in ((2, "priced singly", {}), (4, "invalid", {}), (5, "not one of", {}), (-1, "not one of", {}),
                                (0, "priced singly", dict(n_paths=300)), (1, "priced singly", dict(poly_order=5))):
        with pytest.raises(mc.McgError, match=words):
            eng.debug_batch_row_dump(arr, index, **dict(kw, **other))
    assert mc.stats() == before
    assert bits(eng.batch_price_rows(arr, **kw)) == bits(plain)
    out, amp, comp, block = eng.debug_batch_row_dump(arr, 3, **kw)      # ... and a good row beside them is dumped
    assert bits(out) == bits(plain) and block.shape == (65, 64) and (block[0] == rows[3]["S0"]).all()
