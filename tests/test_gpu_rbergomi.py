"""The rBergomi generator on the GPU (mcg_paths_rbergomi, mcg_paths_rbergomi_payoff) against the high-precision reference of
tests/test_rbergomi_reference.py on the same (seed, path ids), element by element, in every stepping regime: the parameter sets
of PARITY_SETS, whose wave-tiles take expm1_small6_2, expm1_small9_2 and exp_full2 - 1 -- one of them alone, or all three within
one workgroup -- as asserted there on the reference's increments.

Shapes: 1, 7, 16 steps (k_rbergomi_small); 17, 40, 100, 252 (LG 1-4, two staging buffers); 300, 1000 (LG 5, 6, one buffer); 2048
(k_rbergomi_fft<6,3>); 2500 (the generic route).  Each as a launch of 2 rb_pairs_per_block(Mz) + 3 paths (two shares, the second
ragged and ending on a lone A path) and, per transform size of the FFT kernels, as a launch of more shares than the
n_cus * RB_WAVES resident workgroups, so that workgroups take a second trip and draw it from the ticket counter.  path_begin is
even, beyond 2^32 at 7 and 252 steps.  The reference is evaluated on a subset of the columns (at most 64): the first and last
pair of the first share, the ragged last share, the first and last pair of the first ticket-drawn share, and pairs drawn at random.

Bounds.  S is compared relatively, no path-step excluded.  The device evaluates the same definition with its own logarithm, sine
and cosine, exponentials and an FFT in place of the direct sum, so the difference is rounding: steps times a few ulp, plus |inc|
times the error of X.  S_BOUND[set] is ten times S_OBSERVED[set], the largest error observed on an MI355X over all cases of this
file (printed at the end of every run): 6.3e-15 (eta-zero) to 1.7e-14 (full), largest on the 2048- and 2500-step shapes -- what
steps times a few ulp predicts, and 1e-5 of the 1e-9 that the older tests allow.  The reference's own error is 4.1e-18 at most
against mpmath at 50 digits (held to OWN_ERROR_BOUND = 2e-16 there, under 1/100 of the smallest bound here).  The binary64 oracle
of the older 1e-9 comparisons is as good as the device on the same cases: 5.7e-15 (eta-zero) to 1.9e-14 (full) against the
reference (ORACLE_OBSERVED there).

Mutations this file catches and the older tests do not (scratch builds, nothing committed): the 1/2 coefficient of
expm1_small9_2 moved by 256 ulp takes `middle` to 1.1e-13 at 1000 steps and 2.2e-13 at 2048; `ea - (1.0 + 0x1p-40)` in the full
branch of rb_fft_block takes `full` to 1.8e-11 at 17 steps already."""
import math

import numpy as np
import pytest

import montecarlooptionspricer_amd as mc
from test_rbergomi_reference import (FFT_STEPS, LD, MIXED_PATHS, MIXED_STEPS, PARITY_SETS, R, S0, STEPS, columns_of, pair_budget,
                                     pairs_per_block, path_begin_of, pick_pairs, ragged_launch, reference_columns, seed_of,
                                     transform_size)

pytestmark = pytest.mark.gpu

RB_WAVES = 2        # workgroups per CU of the persistent FFT kernels (csrc/kernels_rbergomi.hip)
# largest relative error in S against the reference, observed on an MI355X over the cases of this file
S_OBSERVED = {"small": 9.18e-15, "middle": 6.79e-15, "full": 1.69e-14, "mixed": 8.65e-15, "large-x": 7.52e-15, "smooth": 6.68e-15,
              "eta-zero": 6.33e-15}
S_BOUND = {k: 10.0 * v for k, v in S_OBSERVED.items()}
observed = {k: 0.0 for k in PARITY_SETS}
K = 100.0


@pytest.fixture(scope="module")
def eng():
    with mc.PathEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def grid():
    """Resident workgroups of the persistent kernels: shares from this index on are drawn from the ticket counter."""
    import torch
    return RB_WAVES * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nlargest relative errors in S against the reference in this run: " + ", ".join(f"{k} {v:.2e}" for k, v in observed.items()))


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def launch(eng, name, seed, n_steps, n_paths, begin, payoff=None):
    p = PARITY_SETS[name]
    return eng.rbergomi(seed, S0, R, p["xi"], p["H"], p["eta"], -0.9, p["dt"], n_steps, n_paths, path_begin=begin, payoff=payoff)


def many_share_launch(n_steps, grid):
    """(n_paths, path_begin, seed, pairs): grid + 2 whole shares and a ragged one; the pairs are the first and last of the first
    share and of the first ticket-drawn share, one of the share after it, the two of the ragged share, and random ones."""
    M = transform_size(n_steps)
    ppb = pairs_per_block(M)
    n_paths = 2 * ppb * (grid + 2) + 3
    n_pairs = (n_paths + 1) // 2
    must = (0, ppb - 1, grid * ppb, grid * ppb + ppb - 1, (grid + 1) * ppb + 1, n_pairs - 2, n_pairs - 1)
    return n_paths, path_begin_of(n_steps) + 4096, seed_of(n_steps) + 1, pick_pairs(n_paths, M, must, max(len(must), pair_budget(M) // 2))


def check_parity(eng, name, n_steps, n_paths, begin, seed, pairs, payoff, where):
    S, _, _ = reference_columns(name, n_steps, seed, begin, pairs)
    P = launch(eng, name, seed, n_steps, n_paths, begin, payoff)
    assert (P.n_paths, P.n_steps) == (n_paths, n_steps)
    got = P.to_host_step_major()
    assert got.shape == (n_steps + 1, n_paths) and (got[0] == S0).all() and np.isfinite(got).all() and (got > 0.0).all(), where
    cols, ref_cols = columns_of(pairs, n_paths)
    err = float(np.abs(got[:, cols].astype(LD) / S[:, ref_cols] - 1).max())
    observed[name] = max(observed[name], err)
    print(f"{where}: {len(cols)} columns, largest relative error {err:.2e}")
    assert err <= S_BOUND[name], (where, err)
    if payoff is not None:
        # the fused sums against the exactly rounded sums of the downloaded last row
        strike, is_call = payoff
        T = n_steps * PARITY_SETS[name]["dt"]
        D = math.exp(-R * T)
        x = np.maximum(got[-1] - strike, 0.0) if is_call else np.maximum(strike - got[-1], 0.0)
        mean = math.fsum(x) / n_paths
        m, se = eng.price_european(P, strike, R, T, is_call)
        assert abs(m - D * mean) <= 1e-12 * max(D * mean, 1e-300), (where, "fused mean", m, D * mean)
        var = float(np.sum((x.astype(LD) - LD(mean)) ** 2)) / (n_paths - 1)
        if var > 0.0:
            want_se = D * math.sqrt(var / n_paths)
            cond = max(1.0, 0.5 + mean * mean / var)
            assert abs(se - want_se) <= 1e-9 * cond * want_se, (where, "fused std error", se, want_se, cond)
    P.free()
    return got


@pytest.mark.parametrize("name", list(PARITY_SETS))
def test_parity_with_the_reference(eng, grid, name):
    for k, n_steps in enumerate(STEPS):
        n_paths, begin, seed, pairs = ragged_launch(n_steps)
        plain = check_parity(eng, name, n_steps, n_paths, begin, seed, pairs, None, (name, n_steps, n_paths, "plain"))
        fused = check_parity(eng, name, n_steps, n_paths, begin, seed, pairs, (K, k % 2 == 0), (name, n_steps, n_paths, "payoff"))
        assert bits(plain) == bits(fused), (name, n_steps)          # the plain and the _payoff launch write the same bits
    for k, n_steps in enumerate(FFT_STEPS):
        n_paths, begin, seed, pairs = many_share_launch(n_steps, grid)
        assert (n_paths + 1) // 2 > grid * pairs_per_block(transform_size(n_steps))
        check_parity(eng, name, n_steps, n_paths, begin, seed, pairs, (K, k % 2 == 1) if k % 3 else None,
                     (name, n_steps, n_paths, "second trip"))


def test_repeats_and_splits_of_a_mixed_launch(eng):
    """On `mixed`, where the waves of one workgroup take different exponentials: repeated launches and a second context give
    the same bits; a split of the paths at a multiple of 2 rb_pairs_per_block(Mz) columns reproduces the one-call matrix bit for
    bit (the shares, and hence the waves, are the same sets of paths); a split at another even column regroups the waves, and a
    regrouped wave may take another exponential for a tile, so it agrees within the parity bound only.  On `small`, where every
    wave takes the shortest one whatever its paths, the same unaligned split is still bit-identical: that is what the multi-rank
    tests, all run in that regime, rely on."""
    n_steps, n = MIXED_STEPS, MIXED_PATHS
    begin, seed = path_begin_of(n_steps), seed_of(n_steps)
    share = 2 * pairs_per_block(transform_size(n_steps))
    aligned, unaligned = 2 * share, 2 * share - 2
    assert unaligned % 2 == 0 and unaligned % share
    whole = {}
    for name in ("mixed", "small"):
        P = launch(eng, name, seed, n_steps, n, begin)
        whole[name] = P.to_host_step_major()
        P.free()
        for cut in (aligned, unaligned):
            A, B = launch(eng, name, seed, n_steps, cut, begin), launch(eng, name, seed, n_steps, n - cut, begin + cut)
            both = np.hstack([A.to_host_step_major(), B.to_host_step_major()])
            A.free()
            B.free()
            same = bits(both) == bits(whole[name])
            err = float(np.abs(both / whole[name] - 1.0).max())
            print(f"{name}: split at column {cut}: {'bit-identical' if same else f'largest relative difference {err:.2e}'}")
            if name == "small" or cut == aligned:
                assert same, (name, cut, err)
            else:
                assert not same and 0.0 < err <= S_BOUND[name], (name, cut, err)
    # up to 16 and beyond 2048 steps a path is computed on its own: any even split has the same bits
    for steps in (16, 2500):
        P, A, B = (launch(eng, "mixed", seed, steps, *a) for a in ((11, begin), (6, begin), (5, begin + 6)))
        assert bits(np.hstack([A.to_host_step_major(), B.to_host_step_major()])) == bits(P.to_host_step_major()), steps
        for M in (P, A, B):
            M.free()
    Q = launch(eng, "mixed", seed, n_steps, n, begin)
    assert bits(Q.to_host_step_major()) == bits(whole["mixed"])
    Q.free()
    with mc.PathEngine(0) as other:
        Q = launch(other, "mixed", seed, n_steps, n, begin, payoff=(K, False))
        assert bits(Q.to_host_step_major()) == bits(whole["mixed"])
        Q.free()


def test_refusals_and_empty_launches(eng):
    """What launch_rbergomi, its entry point and host_rbergomi_spectrum refuse, each with its status (MCG_ERR_INVALID = 1) and
    message; nothing is launched.  n_paths = 0 is an empty matrix, not an error."""
    ok = dict(seed=1, S0=100.0, r=0.04, xi=0.04, H=0.1, eta=1.9, rho=-0.9, dt=1.0 / 252.0, n_steps=8, n_paths=100)
    eng.rbergomi(**ok).free()
    nan, inf = float("nan"), float("inf")
    cases = [(dict(path_begin=1), "rBergomi path_begin must be even (paths are generated in pairs)"),
             (dict(path_begin=2 ** 33 + 1), "rBergomi path_begin must be even (paths are generated in pairs)"),
             (dict(S0=0.0), "rBergomi needs S0 > 0 (log-space stepping)"),
             (dict(S0=-1.0), "rBergomi needs S0 > 0 (log-space stepping)"),
             (dict(S0=nan), "S0 must be finite"), (dict(S0=inf), "S0 must be finite"),
             (dict(xi=-0.01), "xi must be >= 0"), (dict(xi=nan), "xi must be >= 0"),
             (dict(H=-0.1), "H must be >= 0"), (dict(H=nan), "H must be >= 0"), (dict(H=inf), "H must be >= 0"),
             (dict(eta=nan), "eta must be finite"), (dict(eta=inf), "eta must be finite"), (dict(eta=-inf), "eta must be finite"),
             (dict(rho=1.5), "|rho| must be <= 1"), (dict(rho=nan), "|rho| must be <= 1"),
             (dict(dt=0.0), "dt must be > 0"), (dict(dt=-1.0 / 252.0), "dt must be > 0"), (dict(dt=nan), "dt must be > 0"),
             (dict(n_steps=0), "n_steps must be >= 1 (got 0)"), (dict(n_steps=-3), "n_steps must be >= 1 (got -3)"),
             (dict(n_steps=2 ** 24 + 1, n_paths=0), f"rBergomi n_steps must be <= 2^24 (got {2 ** 24 + 1})"),
             (dict(n_paths=-1), "n_paths must be >= 0 (got -1)")]
    for change, message in cases:
        for extra in (dict(), dict(payoff=(100.0, True))):
            with pytest.raises(mc.McgError) as e:
                eng.rbergomi(**dict(ok, **change), **extra)
            assert e.value.status == 1 and str(e.value) == message, (change, str(e.value))
    # the edges of the valid set
    for change in (dict(n_paths=0), dict(n_paths=0, path_begin=2), dict(n_paths=0, n_steps=2500), dict(xi=0.0), dict(H=0.0), dict(eta=0.0),
                   dict(rho=1.0), dict(n_paths=1), dict(path_begin=2 ** 63)):
        for extra in (dict(), dict(payoff=(100.0, False))):
            M = eng.rbergomi(**dict(ok, **change), **extra)
            assert (M.n_paths, M.n_steps) == (dict(ok, **change)["n_paths"], dict(ok, **change)["n_steps"])
            if M.n_paths:
                got = M.to_host_step_major()
                assert got.shape == (M.n_steps + 1, M.n_paths) and (got[0] == 100.0).all() and np.isfinite(got).all(), change
            M.free()


def test_launch_frame(eng):
    """One launch under the generator's kernel id, the fused sums and their reuse (test_gpu_parity.check_launch_frame)."""
    from montecarlooptionspricer_amd import _native as N
    from test_gpu_parity import FRAME_PATHS, FRAME_STEPS, check_launch_frame
    check_launch_frame(eng, N.K_RBERGOMI,
                       lambda payoff: eng.rbergomi(1, 100.0, 0.04, 0.04, 0.1, 1.9, -0.9, 1.0 / 252.0, FRAME_STEPS, FRAME_PATHS, payoff=payoff))
