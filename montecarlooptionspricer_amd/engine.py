"""PathEngine: explicit-parameter host API over the C ABI (include/mcgpu.h).

This is the (seed, S0, K, r, sigma | xi, H, eta, T, N_paths, N_steps) interface the north-star
names; the reference hard-codes these as literals (SURVEY.md section 5 "Config / flags").
Device memory is owned by libmcgpu; torch is only used (optionally) for the stream and for the
cross-rank all-reduce.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import Callable, Optional, Tuple

import numpy as np

from . import _native as N
from ._native import McgError, check


class _DevView:
    """Raw device pointer exposed through __cuda_array_interface__ (zero-copy torch view)."""

    def __init__(self, ptr: int, count: int):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False),
                                         "version": 3, "strides": None}


class PathMatrix:
    """Device-resident (n_steps+1) x n_paths price matrix, step-major (mcg_paths*)."""

    def __init__(self, engine: "PathEngine", handle: C.c_void_p):
        self._engine = engine
        self._h = handle
        n_paths, n_steps, ld, ptr = C.c_int64(), C.c_int(), C.c_int64(), C.c_void_p()
        check(engine._L.mcg_paths_info(handle, C.byref(n_paths), C.byref(n_steps), C.byref(ld), C.byref(ptr)))
        self.n_paths, self.n_steps, self.ld = n_paths.value, n_steps.value, ld.value
        self.device_ptr = ptr.value or 0
        engine._live.add(self)

    @property
    def nbytes_algorithmic(self) -> int:
        """8*(n_steps+1) bytes per path: the figure the HBM-write roofline is computed from."""
        return 8 * (self.n_steps + 1) * self.n_paths

    def to_host(self) -> np.ndarray:
        """Reference layout: [n_paths][n_steps+1] (what GenerateStockPricePaths returns)."""
        self._alive()
        out = np.empty((self.n_paths, self.n_steps + 1), dtype=np.float64)
        check(self._engine._L.mcg_paths_to_host(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def to_host_step_major(self) -> np.ndarray:
        """As stored: [n_steps+1][n_paths]."""
        self._alive()
        out = np.empty((self.n_steps + 1, self.n_paths), dtype=np.float64)
        check(self._engine._L.mcg_paths_to_host_step_major(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def free(self) -> None:
        """Give the device buffer back to the engine's pool.  Safe in any order with PathEngine.close(): close()
        frees the matrices that are still alive first, so a late free() (or the garbage collector) finds nothing
        left to do."""
        h, self._h = self._h, None
        if h is not None:
            self._engine._live.discard(self)
            self._engine._L.mcg_paths_free(h)

    def _alive(self):
        if self._h is None:
            raise McgError("PathMatrix already freed")

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PathEngine:
    """One context (device + stream + workspace); create one per process/GPU or per host thread."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._L = N.load_library()
        self._ctx = C.c_void_p()
        if stream is None:
            check(self._L.mcg_init(C.byref(self._ctx), int(device)))
        else:  # adopt the caller's stream; 0 is the legacy default stream (torch's default)
            check(self._L.mcg_init_on_stream(C.byref(self._ctx), int(device), C.c_void_p(int(stream))))
        self._cb = None  # keep the ctypes callback alive
        self.device = device
        self._live = weakref.WeakSet()  # PathMatrix objects whose device buffer belongs to this ctx

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self) -> None:
        if self._ctx:
            for m in list(self._live):  # matrices nobody freed (an exception skipped P.free()): before the ctx goes
                m.free()
            self._L.mcg_finalize(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self) -> None:
        check(self._L.mcg_synchronize(self._ctx))

    def trim(self) -> None:
        check(self._L.mcg_trim(self._ctx))

    # -- collectives ----------------------------------------------------------------------------
    def set_allreduce(self, fn: Optional[Callable[[int, int, int], None]]) -> None:
        """fn(device_ptr, count, stream_handle) must sum `count` doubles in place over all ranks."""
        if fn is None:
            self._cb = None
            check(self._L.mcg_set_allreduce(self._ctx, C.cast(None, N.ALLREDUCE_FN), None))
            return

        def _tramp(_user, buf, count, stream):
            try:
                fn(int(buf), int(count), int(stream or 0))
                return 0
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        self._cb = N.ALLREDUCE_FN(_tramp)
        check(self._L.mcg_set_allreduce(self._ctx, self._cb, None))

    def use_torch_distributed(self, group=None) -> None:
        """All-reduce through torch.distributed (backend "nccl" is RCCL on ROCm).  The ctx must run
        on torch's current stream (PathEngine(stream=torch.cuda.current_stream().cuda_stream))."""
        import torch
        import torch.distributed as dist

        views = {}  # (ptr, count) -> tensor aliasing the context's workspace (a handful of fixed addresses)

        def _ar(ptr: int, count: int, _stream: int) -> None:
            t = views.get((ptr, count))
            if t is None:
                t = views[(ptr, count)] = torch.as_tensor(_DevView(ptr, count), device=torch.device("cuda", self.device))
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)

        self.set_allreduce(_ar)

    def init_rccl(self, rank: int, world: int, broadcast_bytes: Callable[[Optional[bytes]], bytes]) -> None:
        """Built-in RCCL communicator.  broadcast_bytes(id_or_None) returns rank 0's 128-byte id on
        every rank (e.g. via torch.distributed.broadcast_object_list).  Rank 0 ALWAYS enters the broadcast: if it cannot
        create the id it sends an empty one, and every rank raises -- no rank is left alone in a collective."""
        uid, err = None, None
        if rank == 0:
            buf = C.create_string_buffer(128)
            if self._L.mcg_comm_unique_id(buf) != 0:
                msg = self._L.mcg_last_error()
                err = msg.decode() if msg else "mcg_comm_unique_id failed"
                uid = b""
            else:
                uid = buf.raw
        uid = broadcast_bytes(uid)
        if not uid:
            raise McgError("rank 0 could not create the RCCL id" + (f": {err}" if err else ""), 7)
        check(self._L.mcg_comm_init_rank(self._ctx, uid, int(world), int(rank)))

    def rccl_probe(self) -> None:
        """Raises McgError unless librccl loads and hands out an id on THIS rank.  A launcher calls it on every rank and
        lets the ranks agree BEFORE init_rccl: a rank that cannot load the library would otherwise leave its peers waiting
        inside ncclCommInitRank."""
        buf = C.create_string_buffer(128)
        check(self._L.mcg_comm_unique_id(buf))

    def init_shm(self, name: str, rank: int, world: int, peer_mailbox: bool = False) -> bool:
        """Node-local shared-memory collective (mcg_comm_init_shm): `name` starts with '/', is the same on every rank
        and unique to the job.  Host all-reduce for the sums; the one-launch LSM sweeps exchange their per-date moments
        between the GPUs inside the kernel.  peer_mailbox: ask for the in-kernel mailbox in the GPUs' own HBM, mapped
        into the peers by HIP IPC (mcg_comm_shm_peer_mailbox; every rank or none); returns whether it is in use."""
        check(self._L.mcg_comm_init_shm(self._ctx, name.encode(), int(world), int(rank)))
        return self.shm_peer_mailbox(True) if peer_mailbox else False

    def shm_peer_mailbox(self, enable: bool = True) -> bool:
        """Collective over the ranks of the segment: switch the in-kernel mailbox between peer-mapped device memory and
        the host segment.  True when the peer-memory mailbox is in use afterwards (all ranks agree)."""
        active = C.c_int()
        check(self._L.mcg_comm_shm_peer_mailbox(self._ctx, int(bool(enable)), C.byref(active)))
        return bool(active.value)

    # -- generation -----------------------------------------------------------------------------
    def gbm(self, seed: int, S0: float, r: float, sigma: float, dt: float, n_steps: int, n_paths: int,
            path_begin: int = 0, payoff: Optional[Tuple[float, bool]] = None) -> PathMatrix:
        h = C.c_void_p()
        if payoff is None:
            check(self._L.mcg_paths_gbm(self._ctx, seed, S0, r, sigma, dt, n_steps, path_begin, n_paths, C.byref(h)))
        else:
            K, is_call = payoff
            check(self._L.mcg_paths_gbm_payoff(self._ctx, seed, S0, r, sigma, dt, n_steps, path_begin, n_paths,
                                               K, int(bool(is_call)), C.byref(h)))
        return PathMatrix(self, h)

    def rbergomi(self, seed: int, S0: float, r: float, xi: float, H: float, eta: float, rho: float, dt: float,
                 n_steps: int, n_paths: int, path_begin: int = 0,
                 payoff: Optional[Tuple[float, bool]] = None) -> PathMatrix:
        h = C.c_void_p()
        if payoff is None:
            check(self._L.mcg_paths_rbergomi(self._ctx, seed, S0, r, xi, H, eta, rho, dt, n_steps, path_begin,
                                             n_paths, C.byref(h)))
        else:
            K, is_call = payoff
            check(self._L.mcg_paths_rbergomi_payoff(self._ctx, seed, S0, r, xi, H, eta, rho, dt, n_steps,
                                                    path_begin, n_paths, K, int(bool(is_call)), C.byref(h)))
        return PathMatrix(self, h)

    def heston(self, seed: int, S0: float, r: float, v0: float, kappa: float, theta: float, sigma_v: float, rho: float,
               dt: float, n_steps: int, n_paths: int, path_begin: int = 0,
               payoff: Optional[Tuple[float, bool]] = None, want_variance: bool = False, scheme: str = "euler"):
        """Heston paths by one of the schemes of include/mcgpu.h: "euler", the full-truncation log-Euler scheme
        (mcg_paths_heston*), or "qe", Andersen's quadratic-exponential scheme (mcg_paths_heston_qe*: sigma_v > 0).  Returns the
        price matrix, or (prices, variances) when want_variance; row n of the variances is v_n (Euler: untruncated; QE: never
        negative)."""
        if scheme not in ("euler", "qe"):
            raise ValueError(f'scheme must be "euler" or "qe", not {scheme!r}')
        plain, fused = ((self._L.mcg_paths_heston, self._L.mcg_paths_heston_payoff) if scheme == "euler" else
                        (self._L.mcg_paths_heston_qe, self._L.mcg_paths_heston_qe_payoff))
        h, hv = C.c_void_p(), C.c_void_p()
        var_out = C.byref(hv) if want_variance else None
        if payoff is None:
            check(plain(self._ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, C.byref(h),
                        var_out))
        else:
            K, is_call = payoff
            check(fused(self._ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, dt, n_steps, path_begin, n_paths, K,
                        int(bool(is_call)), C.byref(h), var_out))
        return (PathMatrix(self, h), PathMatrix(self, hv)) if want_variance else PathMatrix(self, h)

    def bates(self, seed: int, S0: float, r: float, v0: float, kappa: float, theta: float, sigma_v: float, rho: float,
              jump_intensity: float, jump_mean: float, jump_std: float, dt: float, n_steps: int, n_paths: int, path_begin: int = 0,
              payoff: Optional[Tuple[float, bool]] = None, want_variance: bool = False, scheme: str = "euler"):
        """Bates paths (mcg_paths_bates*): heston(scheme=...) plus compound-Poisson jumps in the price, jump_intensity a year
        (lambda; lambda dt <= 1), each log-normal with mean jump_mean and std deviation jump_std of the log-size.  Returns what
        heston returns; jump_intensity = 0 gives heston's matrices bit for bit."""
        if scheme not in ("euler", "qe"):
            raise ValueError(f'scheme must be "euler" or "qe", not {scheme!r}')
        h, hv = C.c_void_p(), C.c_void_p()
        var_out = C.byref(hv) if want_variance else None
        model = (self._ctx, seed, S0, r, v0, kappa, theta, sigma_v, rho, jump_intensity, jump_mean, jump_std, dt, n_steps, path_begin,
                 n_paths, int(scheme == "qe"))
        if payoff is None:
            check(self._L.mcg_paths_bates(*model, C.byref(h), var_out))
        else:
            K, is_call = payoff
            check(self._L.mcg_paths_bates_payoff(*model, K, int(bool(is_call)), C.byref(h), var_out))
        return (PathMatrix(self, h), PathMatrix(self, hv)) if want_variance else PathMatrix(self, h)

    def merton(self, seed: int, S0: float, r: float, sigma: float, jump_intensity: float, jump_mean: float, jump_std: float,
               dt: float, n_steps: int, n_paths: int, path_begin: int = 0,
               payoff: Optional[Tuple[float, bool]] = None) -> PathMatrix:
        """Merton's jump-diffusion: GBM with volatility sigma plus the jumps of bates -- the Euler scheme at
        v0 = theta = sigma^2, kappa = sigma_v = rho = 0."""
        return self.bates(seed, S0, r, sigma * sigma, 0.0, sigma * sigma, 0.0, 0.0, jump_intensity, jump_mean, jump_std, dt, n_steps,
                          n_paths, path_begin=path_begin, payoff=payoff)

    def gbm_multi(self, seed: int, S0, r: float, sigma, corr, dt: float, n_steps: int, n_paths: int, path_begin: int = 0, q=None,
                  combine=None, weights=None, want_assets: bool = True):
        """Correlated multi-asset GBM paths (mcg_paths_gbm_multi): S0, sigma, q (dividend yields; None: zeros) and weights
        (None: ones) hold one value per asset, corr is the n x n correlation matrix.  combine: None, or "basket", "best_of",
        "worst_of" (or _native.C_*) -- the combined matrix is built in the same launch from the prices in registers.  Returns
        (assets, combined): a list of PathMatrix, one per asset (None unless want_assets), and the combined PathMatrix (None
        unless combine is given)."""
        S0, sigma = _vec(S0), _vec(sigma)
        n = len(S0)
        corr = np.ascontiguousarray(corr, dtype=np.float64)
        if len(sigma) != n or corr.shape != (n, n):
            raise McgError(f"gbm_multi: {n} spots need {n} volatilities and an {n} x {n} correlation matrix", 1)
        q, weights = (None if v is None else _vec(v) for v in (q, weights))
        if any(v is not None and len(v) != n for v in (q, weights)):
            raise McgError(f"gbm_multi: q and weights hold one value per asset ({n})", 1)
        kind = N.C_NONE if combine is None else _combine_kind(combine)
        dp = C.POINTER(C.c_double)
        ptr = lambda v: None if v is None else v.ctypes.data_as(dp)  # noqa: E731
        handles, hc = (C.c_void_p * max(n, 1))(), C.c_void_p()
        check(self._L.mcg_paths_gbm_multi(self._ctx, seed, n, ptr(S0), r, ptr(q), ptr(sigma), ptr(corr), dt, n_steps, path_begin, n_paths,
                                          kind, ptr(weights), handles if want_assets else None, C.byref(hc) if combine is not None else None))
        assets = [PathMatrix(self, C.c_void_p(h)) for h in handles] if want_assets else None
        return assets, (PathMatrix(self, hc) if combine is not None else None)

    def combine(self, paths, kind, weights=None) -> PathMatrix:
        """One matrix from up to eight of this engine's matrices of equal shape, whatever made them (mcg_paths_combine):
        kind "basket" (sum of w_a S^a; negative weights give spreads), "best_of" (max) or "worst_of" (min)."""
        paths = list(paths)
        for P in paths:
            P._alive()
        weights = None if weights is None else _vec(weights)
        if weights is not None and len(weights) != len(paths):
            raise McgError(f"combine: {len(paths)} matrices need {len(paths)} weights", 1)
        handles = (C.c_void_p * max(len(paths), 1))(*[P._h.value for P in paths])
        h = C.c_void_p()
        check(self._L.mcg_paths_combine(self._ctx, handles, len(paths), _combine_kind(kind),
                                        None if weights is None else weights.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
        return PathMatrix(self, h)

    def local_vol(self, seed: int, S0: float, r: float, surface: "LocalVolSurface", dt: float, n_steps: int, n_paths: int,
                  path_begin: int = 0, q: float = 0.0, payoff: Optional[Tuple[float, bool]] = None) -> PathMatrix:
        """Local-volatility paths (mcg_paths_localvol*): dS = (r - q) S dt + sigma(t, S) S dW with sigma from `surface`, bilinear
        in time and ln(S / S0) and flat outside its grid.  The matrix is a plain one for greeks_european (no rho)."""
        dp = C.POINTER(C.c_double)
        model = (self._ctx, seed, S0, r, q, surface.times.ctypes.data_as(dp), surface.n_t, surface.x_min, surface.x_max, surface.n_x,
                 surface.sigma.ctypes.data_as(dp), dt, n_steps, path_begin, n_paths)
        h = C.c_void_p()
        if payoff is None:
            check(self._L.mcg_paths_localvol(*model, C.byref(h)))
        else:
            K, is_call = payoff
            check(self._L.mcg_paths_localvol_payoff(*model, K, int(bool(is_call)), C.byref(h)))
        return PathMatrix(self, h)

    def gbm_sobol(self, sobol: "Sobol", S0: float, r: float, sigma: float, dt: float, n_steps: int, n_paths: int,
                  path_begin: int = 0, payoff: Optional[Tuple[float, bool]] = None) -> PathMatrix:
        """GBM paths from a Sobol' point set (mcg_paths_gbm_sobol*): path i is point path_begin + i of `sobol`, one dimension per
        step (n_steps <= 1024, path_begin + n_paths <= 2^32), the law of gbm() and the same plain matrix for every pricer.
        price_european's own std_err on it is the iid formula and is NOT an error bar of a Sobol' estimate: generate a few
        replicates (Sobol(seed, replicate=0, 1, ...)), price each, and take rqmc_combine over the prices."""
        spec = sobol._spec()
        h = C.c_void_p()
        if payoff is None:
            check(self._L.mcg_paths_gbm_sobol(self._ctx, C.byref(spec), S0, r, sigma, dt, n_steps, path_begin, n_paths, C.byref(h)))
        else:
            K, is_call = payoff
            check(self._L.mcg_paths_gbm_sobol_payoff(self._ctx, C.byref(spec), S0, r, sigma, dt, n_steps, path_begin, n_paths,
                                                     K, int(bool(is_call)), C.byref(h)))
        return PathMatrix(self, h)

    def local_vol_sobol(self, sobol: "Sobol", S0: float, r: float, surface: "LocalVolSurface", dt: float, n_steps: int, n_paths: int,
                        path_begin: int = 0, q: float = 0.0, payoff: Optional[Tuple[float, bool]] = None) -> PathMatrix:
        """Local-volatility paths from a Sobol' point set (mcg_paths_localvol_sobol*): the step of local_vol() with the normals of
        `sobol`; limits as gbm_sobol.  price_european's own std_err on it is the iid formula and is NOT an error bar of a Sobol'
        estimate: the error bar is rqmc_combine over replicates."""
        dp = C.POINTER(C.c_double)
        spec = sobol._spec()
        model = (self._ctx, C.byref(spec), S0, r, q, surface.times.ctypes.data_as(dp), surface.n_t, surface.x_min, surface.x_max,
                 surface.n_x, surface.sigma.ctypes.data_as(dp), dt, n_steps, path_begin, n_paths)
        h = C.c_void_p()
        if payoff is None:
            check(self._L.mcg_paths_localvol_sobol(*model, C.byref(h)))
        else:
            K, is_call = payoff
            check(self._L.mcg_paths_localvol_sobol_payoff(*model, K, int(bool(is_call)), C.byref(h)))
        return PathMatrix(self, h)

    def from_host(self, row_major: np.ndarray) -> PathMatrix:
        """Upload [n_paths][n_steps+1] (the reference's pricePaths layout)."""
        a = np.ascontiguousarray(row_major, dtype=np.float64)
        if a.ndim != 2 or a.size == 0:
            raise McgError("LSM::PredictOptionPrice: Empty pricePaths.", 6)
        h = C.c_void_p()
        check(self._L.mcg_paths_from_host(self._ctx, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0],
                                          a.shape[1], C.byref(h)))
        return PathMatrix(self, h)

    # -- pricing --------------------------------------------------------------------------------
    def price_european(self, paths: PathMatrix, K: float, r: float, T: float, is_call: bool) -> Tuple[float, float]:
        paths._alive()
        m, se = C.c_double(), C.c_double()
        check(self._L.mcg_price_european(self._ctx, paths._h, K, r, T, int(bool(is_call)), C.byref(m), C.byref(se)))
        return m.value, se.value

    def price_lsm(self, paths: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool,
                  poly_order: int) -> Tuple[float, float]:
        paths._alive()
        m, se = C.c_double(), C.c_double()
        check(self._L.mcg_price_lsm(self._ctx, paths._h, r, K, maturity, dt, int(bool(is_call)), int(poly_order),
                                    C.byref(m), C.byref(se)))
        return m.value, se.value

    def price_lsm2(self, paths: PathMatrix, state: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool,
                   poly_order: int, return_dropped: bool = False):
        """LSM with the continuation value regressed on the price AND a second per-path state of the same shape (the
        variance matrix of heston(..., want_variance=True)): mcg_price_lsm2, poly_order in [0, 3].  Returns (mean, std_err),
        plus the number of basis columns the fit dropped over all dates when return_dropped."""
        paths._alive()
        state._alive()
        m, se, nd = C.c_double(), C.c_double(), C.c_int64()
        check(self._L.mcg_price_lsm2(self._ctx, paths._h, state._h, r, K, maturity, dt, int(bool(is_call)), int(poly_order),
                                     C.byref(m), C.byref(se), C.byref(nd)))
        return (m.value, se.value, nd.value) if return_dropped else (m.value, se.value)

    def fit_lsm(self, paths: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool, poly_order: int):
        """price_lsm's estimator on the per-date route, and the exercise rule the sweep fitted (mcg_lsm_fit): returns
        (price, std_err, LsmPolicy).  poly_order in [0, 15]."""
        paths._alive()
        m, se, hdr = C.c_double(), C.c_double(), N.LsmPolicyHdr()
        coef = np.zeros((paths.n_steps + 1, N.LSM_POLICY_STRIDE))
        check(self._L.mcg_lsm_fit(self._ctx, paths._h, r, K, maturity, dt, int(bool(is_call)), int(poly_order), C.byref(m),
                                  C.byref(se), C.byref(hdr), coef.ctypes.data_as(C.POINTER(C.c_double))))
        return m.value, se.value, LsmPolicy(hdr.n_steps, hdr.poly_order, hdr.is_call != 0, hdr.r, hdr.K, hdr.maturity, hdr.dt, coef)

    def apply_lsm(self, policy: "LsmPolicy", paths: PathMatrix, return_hist: bool = False, return_sums: bool = False):
        """The policy applied to (independent) paths: every path stops at the first date the rule says exercise and takes the
        discounted payoff there -- a lower bound on the American value whatever the rule (mcg_lsm_apply).  Returns (price,
        std_err), then tau_hist (n_steps + 1 counts of stopping dates) when return_hist, then sums3 = {sum v, sum v^2, n} when
        return_sums."""
        paths._alive()
        m, se = C.c_double(), C.c_double()
        dp = C.POINTER(C.c_double)
        hist = np.zeros(policy.n_steps + 1, dtype=np.int64)
        sums = np.zeros(3)
        hdr = policy._hdr()
        check(self._L.mcg_lsm_apply(self._ctx, C.byref(hdr), policy.coef.ctypes.data_as(dp), paths._h, C.byref(m), C.byref(se),
                                    sums.ctypes.data_as(dp) if return_sums else None,
                                    hist.ctypes.data_as(C.POINTER(C.c_int64)) if return_hist else None))
        out = (m.value, se.value)
        if return_hist:
            out += (hist,)
        if return_sums:
            out += (sums,)
        return out

    def dual_upper_lsm(self, policy: "LsmPolicy", paths: PathMatrix, sigma: float, n_inner: int, seed: int, q: float = 0.0,
                       path_begin: int = 0, return_cont: bool = False, return_d: bool = False) -> "DualResult":
        """The Andersen-Broadie dual upper bound of the policy by nested simulation (mcg_lsm_dual_upper): along every outer
        path of `paths`, n_inner GBM paths (sigma, q, the policy's r and dt; Philox key `seed`) from every date estimate the
        policy's continuation value, and the bound is the mean of the pathwise maximum of the discounted payoff less the
        martingale they build.  An upper bound for any policy, biased upwards by the inner noise -- the caller's bound only if
        the outer paths follow the same GBM.  path_begin: the global id of the first outer path (shards: add sums3 and
        inner_steps).  Returns a DualResult (upper, std_err, sums3, inner_steps), then cont [n_steps][n_paths] when return_cont,
        then d [n_paths] when return_d."""
        paths._alive()
        if not 1 <= int(n_inner) <= N.LSM_DUAL_MAX_INNER:
            raise McgError(f"dual_upper_lsm: n_inner must be in [1, {N.LSM_DUAL_MAX_INNER}] (got {n_inner})", 1)
        if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(path_begin) < 2 ** 64:
            raise McgError("dual_upper_lsm: seed and path_begin must be in [0, 2^64)", 1)
        up, se, steps = C.c_double(), C.c_double(), C.c_int64()
        dp = C.POINTER(C.c_double)
        sums = np.zeros(3)
        cont = np.empty((policy.n_steps, paths.n_paths)) if return_cont else None
        d = np.empty(paths.n_paths) if return_d else None
        hdr = policy._hdr()
        model = N.LsmDualModel(int(seed), float(sigma), float(q), int(path_begin), int(n_inner), 0)
        check(self._L.mcg_lsm_dual_upper(self._ctx, C.byref(hdr), policy.coef.ctypes.data_as(dp), paths._h, C.byref(model), C.byref(up),
                                         C.byref(se), sums.ctypes.data_as(dp), cont.ctypes.data_as(dp) if return_cont else None,
                                         d.ctypes.data_as(dp) if return_d else None, C.byref(steps)))
        return DualResult(up.value, se.value, sums, steps.value, cont, d)

    def debug_lsm_dual_executed(self) -> int:
        """Measurement hook (mcg_debug_lsm_dual_executed, include/mcgpu_debug.h; not part of the product surface): path-steps
        the wavefronts of the last dual_upper_lsm ran through, stopped inner paths included -- inner_steps over this is the
        share of live lane-steps that tools/bench_lsm_dual.py reports."""
        n = C.c_int64()
        check(self._L.mcg_debug_lsm_dual_executed(self._ctx, C.byref(n)))
        return n.value

    def debug_lsm_dual_workspace(self, doubles: int = 0) -> None:
        """Test hook (mcg_debug_lsm_dual_workspace): the workspace, in doubles, one batch of outer paths of dual_upper_lsm may
        use; 0: the default (2^24).  A batch is never smaller than 512 outer paths."""
        check(self._L.mcg_debug_lsm_dual_workspace(self._ctx, int(doubles)))

    def greeks_european(self, paths: PathMatrix, K: float, r: float, T: float, is_call: bool,
                        sigma: Optional[float] = None) -> dict:
        """European price, delta, gamma, vega, rho, dual delta and their std errors (mcg_greeks_european); NaN where a
        Greek is not defined for these inputs.  sigma: the GBM volatility the paths were generated with (gamma, vega)."""
        paths._alive()
        g = N.Greeks()
        check(self._L.mcg_greeks_european(self._ctx, paths._h, K, r, T, int(bool(is_call)),
                                          float(sigma) if sigma is not None else 0.0, C.byref(g)))
        return g.as_dict()

    def greeks_lsm(self, paths: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool,
                   poly_order: int) -> dict:
        """LSM price, dual delta (K-tangent through the sweep) and delta by homogeneity, with std errors
        (mcg_greeks_lsm); gamma, vega and rho are NaN."""
        paths._alive()
        g = N.Greeks()
        check(self._L.mcg_greeks_lsm(self._ctx, paths._h, r, K, maturity, dt, int(bool(is_call)), int(poly_order),
                                     C.byref(g)))
        return g.as_dict()

    def path_stats(self, paths: PathMatrix, first_row: int = 1) -> np.ndarray:
        """Per-path statistics over the monitoring rows first_row .. n_steps (mcg_path_stats): [5][n_paths] =
        S_T, arithmetic mean, geometric mean, min, max."""
        paths._alive()
        out = np.empty((5, paths.n_paths), dtype=np.float64)
        check(self._L.mcg_path_stats(self._ctx, paths._h, int(first_row), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def price_exotics(self, paths: PathMatrix, r: float, T: float, book, first_row: int = 1, return_sums: bool = False):
        """Asian, lookback and barrier contracts from one pass over the matrix (mcg_price_exotics).  book: a sequence of
        exotic(...) tuples (kind, is_call, K, barrier, rebate) or dicts with those keys; returns (price[n], std_err[n]),
        plus sums[2 n + 1] = {sum, sum^2} per contract then the path count when return_sums."""
        paths._alive()
        arr = make_book(book)
        n = len(arr)
        dp = C.POINTER(C.c_double)
        price, se, sums = np.empty(n), np.empty(n), np.empty(2 * n + 1)
        check(self._L.mcg_price_exotics(self._ctx, paths._h, r, T, int(first_row), arr, n, price.ctypes.data_as(dp),
                                        se.ctypes.data_as(dp), sums.ctypes.data_as(dp) if return_sums else None))
        return (price, se, sums) if return_sums else (price, se)

    def path_tangent_stats(self, paths: PathMatrix, first_row: int = 1, with_logs: bool = True) -> np.ndarray:
        """The ten per-path statistics behind greeks_exotics (mcg_path_tangent_stats): [10][n_paths], rows in the order of
        _native.TANGENT_STATS -- the five of path_stats bit for bit, then L = mean S_j ln S_j, J = mean j S_j, the row of the
        first minimum and of the first maximum, and Q = sum of squared log-returns over all steps.  with_logs=False skips the
        logarithms: L and Q are NaN."""
        paths._alive()
        out = np.empty((10, paths.n_paths), dtype=np.float64)
        check(self._L.mcg_path_tangent_stats(self._ctx, paths._h, int(first_row), int(bool(with_logs)),
                                             out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def greeks_exotics(self, paths: PathMatrix, r: float, T: float, book, sigma: float = 0.0, q: float = 0.0,
                       first_row: int = 1) -> list:
        """Price, delta, gamma, vega, rho, dual delta and their std errors of every contract of a price_exotics book
        (mcg_greeks_exotics): a list of dicts like greeks_european's, NaN where a Greek is not defined for these inputs.
        sigma, q: the GBM volatility and dividend yield the paths were generated with (vega, gamma, the barriers' Greeks)."""
        paths._alive()
        arr = make_book(book)
        n = len(arr)
        out = (N.Greeks * n)()
        check(self._L.mcg_greeks_exotics(self._ctx, paths._h, r, q, float(sigma), T, int(first_row), arr, n, out))
        return [g.as_dict() for g in out]

    @staticmethod
    def _bridge_variance(sigma, var):
        """(var handle or None, sigma) of the bridge calls: exactly one of sigma and var is given."""
        if (sigma is None) == (var is None):
            raise ValueError("give exactly one of sigma (the scalar route) and var (a variance matrix)")
        if var is None:
            return None, float(sigma)
        if not isinstance(var, PathMatrix):
            raise ValueError("var must be a PathMatrix (a generator's var_out, or from_host)")
        var._alive()
        return var._h, 0.0

    def barrier_survival(self, paths: PathMatrix, levels, dt: float, sigma: Optional[float] = None, var: Optional[PathMatrix] = None,
                         first_row: int = 0) -> np.ndarray:
        """Brownian-bridge survival probabilities of every path for every level (mcg_barrier_survival): [n_levels][n_paths].
        levels: a sequence of (barrier, is_up).  Rows first_row .. n_steps and the intervals between them are monitored; the
        step variance is sigma * sigma * dt, or max(var, 0) * dt row by row from a variance matrix of the paths' shape.
        Exactly one of sigma and var must be given (ValueError otherwise)."""
        paths._alive()
        var_h, sig = self._bridge_variance(sigma, var)
        levels = list(levels)
        n = len(levels)
        B = np.ascontiguousarray([float(lv[0]) for lv in levels], dtype=np.float64)
        up = (C.c_int * max(n, 1))(*[int(bool(lv[1])) for lv in levels])
        out = np.empty((n, paths.n_paths), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(self._L.mcg_barrier_survival(self._ctx, paths._h, var_h, sig, float(dt), int(first_row), B.ctypes.data_as(dp), up, n,
                                           out.ctypes.data_as(dp)))
        return out

    def price_barriers_bridge(self, paths: PathMatrix, r: float, T: float, book, sigma: Optional[float] = None,
                              var: Optional[PathMatrix] = None, first_row: int = 0, return_sums: bool = False):
        """Continuously monitored barrier contracts from Brownian-bridge survival probabilities (mcg_price_barriers_bridge).
        book: exotic(...) tuples of the four barrier kinds, as for price_exotics; returns (price[n], std_err[n]), plus
        sums[2 n + 1] when return_sums.  dt = T / n_steps; exactly one of sigma and var must be given (ValueError otherwise)."""
        paths._alive()
        var_h, sig = self._bridge_variance(sigma, var)
        arr = make_book(book)
        n = len(arr)
        dp = C.POINTER(C.c_double)
        price, se, sums = np.empty(n), np.empty(n), np.empty(2 * n + 1)
        check(self._L.mcg_price_barriers_bridge(self._ctx, paths._h, var_h, sig, r, T, int(first_row), arr, n, price.ctypes.data_as(dp),
                                                se.ctypes.data_as(dp), sums.ctypes.data_as(dp) if return_sums else None))
        return (price, se, sums) if return_sums else (price, se)

    def gbm_twin_stats(self, twin, n_steps: int, n_paths: int, first_row: int = 1) -> np.ndarray:
        """The five statistics of path_stats for the GBM twin computed in registers (mcg_gbm_twin_stats): twin is a dict or
        tuple of the mcg_gbm_twin fields (seed, S0, r, q, sigma, dt, path_begin).  No matrix is stored."""
        tw = make_twin(twin)
        out = np.empty((5, max(int(n_paths), 0)), dtype=np.float64)
        check(self._L.mcg_gbm_twin_stats(self._ctx, C.byref(tw), int(n_steps), int(first_row), int(n_paths),
                                         out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def price_exotics_cv(self, paths: PathMatrix, r: float, T: float, book, controls, ctrl, first_row: int = 1, twin=None,
                         return_sums: bool = False):
        """price_exotics with up to two control variates a contract, in the same pass (mcg_price_exotics_cv).  controls: a
        sequence of control(...) tuples; ctrl: per contract a pair (a, b) of indices into controls, -1 or None for none (a
        single int means (a, -1)).  twin: None, a PathMatrix of the same shape, or a dict / tuple of the mcg_gbm_twin fields
        (the twin computed in registers) -- what controls with on_twin read.  Returns a CvResult (price, std_err, beta[n][2],
        plain_price, plain_se, and sums[9 n + 1] when return_sums)."""
        paths._alive()
        arr = make_book(book)
        n = len(arr)
        ctl = make_controls(controls)
        idx = make_ctrl(ctrl, n)
        twin_h, twin_s = None, None
        if isinstance(twin, PathMatrix):
            twin._alive()
            twin_h = twin._h
        elif twin is not None:
            twin_s = C.byref(make_twin(twin))
        dp = C.POINTER(C.c_double)
        price, se, beta, pp, ps, sums = np.empty(n), np.empty(n), np.empty((n, 2)), np.empty(n), np.empty(n), np.empty(9 * n + 1)
        check(self._L.mcg_price_exotics_cv(self._ctx, paths._h, twin_h, twin_s, r, T, int(first_row), arr, n, ctl, len(ctl), idx,
                                           price.ctypes.data_as(dp), se.ctypes.data_as(dp), beta.ctypes.data_as(dp),
                                           pp.ctypes.data_as(dp), ps.ctypes.data_as(dp), sums.ctypes.data_as(dp) if return_sums else None))
        return CvResult(price, se, beta, pp, ps, sums if return_sums else None)

    def mlmc_level(self, seed: int, S0: float, r: float, surface: "LocalVolSurface", T: float, book, n_fine: int, n_paths: int,
                   has_coarse: bool = True, stride_fine: int = 1, stride_coarse: int = 1, first_obs: int = 1, path_begin: int = 0,
                   q: float = 0.0, return_stats: bool = False, scheme: str = "euler", bridge: bool = False,
                   return_survival: bool = False):
        """One level of multilevel Monte Carlo under local volatility in one launch (mcg_mlmc_localvol_level): a fine path of
        n_fine steps over [0, T] and, with has_coarse, a coarse one of n_fine / 2 steps from the same Brownian path, both reduced
        to the five statistics of path_stats in registers; no matrix is stored.  Returns sums[6 n + 1] = {sum Y, sum Y^2,
        sum P_f, sum P_f^2, sum P_c, sum P_c^2} per contract of `book` (Y = P_f - P_c), then the path count; with return_stats
        (sums, stats10): [10][n_paths], the fine statistics then the coarse ones ([5][n_paths] without a coarse path).
        scheme "milstein" adds the Milstein correction to both grids' steps; bridge samples the barrier contracts from the
        Brownian-bridge survival probability of their level along each grid (continuous monitoring; at most four distinct
        levels, mlmc_bridge_levels(book) lists them) -- mcg_mlmc_localvol_level_ex.  return_survival appends surv[(1 or 2)
        n_levels][n_paths] to the result: P per level on the fine grid, then on the coarse one (no rows without bridge)."""
        arr = make_book(book)
        n = len(arr)
        dp = C.POINTER(C.c_double)
        if scheme not in N.MLMC_SCHEMES:
            raise McgError(f"mlmc: scheme must be one of {sorted(N.MLMC_SCHEMES)} (got {scheme!r})", 1)
        lv = N.MlmcLevel(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_fine), int(bool(has_coarse)), int(stride_fine), int(stride_coarse),
                         int(first_obs), int(path_begin) & 0xFFFFFFFFFFFFFFFF, int(n_paths))
        sums = np.empty(6 * n + 1)
        stats = np.empty((10 if has_coarse else 5, max(int(n_paths), 0))) if return_stats else None
        surv = None
        if return_survival:
            n_levels = len(mlmc_bridge_levels(book)) if bridge else 0
            surv = np.empty(((2 if has_coarse else 1) * n_levels, max(int(n_paths), 0)))
        check(self._L.mcg_mlmc_localvol_level_ex(self._ctx, S0, r, q, surface.times.ctypes.data_as(dp), surface.n_t, surface.x_min,
                                                 surface.x_max, surface.n_x, surface.sigma.ctypes.data_as(dp), T, C.byref(lv),
                                                 N.MLMC_SCHEMES[scheme], int(bool(bridge)), arr, n, sums.ctypes.data_as(dp),
                                                 stats.ctypes.data_as(dp) if return_stats else None,
                                                 surv.ctypes.data_as(dp) if return_survival and surv.size else None))
        out = (sums,) + ((stats,) if return_stats else ()) + ((surv,) if return_survival else ())
        return out if len(out) > 1 else sums

    def mlmc_local_vol(self, seed: int, S0: float, r: float, surface: "LocalVolSurface", T: float, book, eps: float, n0: int = 4,
                       n_obs: Optional[int] = None, first_obs: int = 1, q: float = 0.0, n_pilot: int = 10_000, l_min: int = 2,
                       l_max: int = 10, scheme: str = "euler", bridge: bool = False) -> "MlmcResult":
        """The multilevel estimator of a price_exotics book under local volatility, to a root-mean-square error of about eps
        (undiscounted bias below eps / sqrt(2) by the estimate of mlmc_plan, variance eps^2 / 2 by Giles' rule).  Level l has
        n0 2^l fine steps (level 0 no coarse path) and draws with the Philox key seed + l (mod 2^64); every level starts with
        n_pilot paths, and further batches of a level continue at path_begin = paths already drawn, so the result is a function
        of the arguments alone.  The path counts are those of the worst contract of the book.  Levels l_min + 1, ... are added
        until every contract's bias test passes or l_max is reached (converged False then; no error).  n_obs None monitors each
        grid's own rows; an integer monitors that many equidistant dates on every grid and must divide n0 / 2.  scheme and
        bridge are mlmc_level's: with bridge the barrier contracts are continuously monitored ones, whatever n_obs is."""
        n = len(book)
        if not (eps > 0.0) or not math.isfinite(eps):
            raise McgError("mlmc: eps must be finite and > 0", 1)
        if n0 < 1 or n_pilot < 2 or l_min < 0 or l_max < l_min or l_max >= N.MLMC_MAX_LEVELS:
            raise McgError(f"mlmc: needs n0 >= 1, n_pilot >= 2 and 0 <= l_min <= l_max < {N.MLMC_MAX_LEVELS}", 1)
        if l_max > 0 and n0 % 2:
            raise McgError(f"mlmc: n0 must be even (got {n0})", 1)
        if n_obs is not None and (n_obs < 1 or n0 % 2 or (n0 // 2) % n_obs):
            raise McgError(f"mlmc: n_obs must divide n0 / 2 (got n_obs = {n_obs}, n0 = {n0})", 1)
        sums, paths = [], []           # per level: [n][6] sums, paths drawn

        def draw(l, count):
            n_fine = n0 << l
            n_coarse = n_fine // 2
            sf, sc = (1, 1) if n_obs is None else (n_fine // n_obs, max(n_coarse // n_obs, 1))
            s = self.mlmc_level((seed + l) & 0xFFFFFFFFFFFFFFFF, S0, r, surface, T, book, n_fine, count, has_coarse=l > 0,
                                stride_fine=sf, stride_coarse=sc, first_obs=first_obs, path_begin=paths[l], q=q, scheme=scheme, bridge=bridge)
            sums[l] += s[:-1].reshape(n, 6)
            paths[l] += count

        def add_level():
            sums.append(np.zeros((n, 6)))
            paths.append(0)
            draw(len(paths) - 1, n_pilot)

        def table():
            cnt = np.array(paths, dtype=np.float64)
            mean = np.array([[sums[l][c, 0] / paths[l] for l in range(len(paths))] for c in range(n)])
            var = np.array([[max((sums[l][c, 1] - paths[l] * mean[c, l] * mean[c, l]) / (paths[l] - 1.0), 0.0)
                             for l in range(len(paths))] for c in range(n)])
            cost = np.array([float((n0 << l) + ((n0 << l) // 2 if l else 0)) for l in range(len(paths))])
            return cnt, mean, var, cost

        for _ in range(l_min + 1):
            add_level()
        while True:
            for _round in range(8):  # top the levels up to Giles' counts; the variances move as paths are added
                cnt, mean, var, cost = table()
                want = np.max([mlmc_plan(cnt, mean[c], var[c], cost, eps)[0] for c in range(n)], axis=0)
                more = [int(want[l]) - paths[l] for l in range(len(paths))]
                if max(more) <= 0:
                    break
                for l, m in enumerate(more):
                    if m > 0:
                        draw(l, m)
            cnt, mean, var, cost = table()
            plans = [mlmc_plan(cnt, mean[c], var[c], cost, eps) for c in range(n)]
            bias = np.array([p[2] for p in plans])
            converged = all(p[3] for p in plans)
            if converged or len(paths) - 1 >= l_max:
                break
            add_level()
        price, se = np.empty(n), np.empty(n)
        for c in range(n):
            price[c], se[c] = mlmc_combine([sums[l][c, 0] for l in range(len(paths))], [sums[l][c, 1] for l in range(len(paths))], cnt, r, T)
        levels = [dict(n_fine=n0 << l, paths=paths[l], mean_y=mean[:, l].copy(), var_y=var[:, l].copy(),
                       mean_pf=sums[l][:, 2] / paths[l], cost=cost[l]) for l in range(len(paths))]
        return MlmcResult(price, se, levels, math.exp(-r * T) * bias, bool(converged), float(np.dot(cnt, cost)))

    def price_scheduled(self, paths: PathMatrix, r: float, dt: float, schedule, book, return_sums: bool = False,
                        return_hist: bool = False):
        """Autocallables and cliquets on an observation schedule (mcg_price_scheduled).  schedule: what schedule(...) takes;
        book: a sequence of autocall(...) / cliquet(...) tuples or dicts with the mcg_sched fields.  Returns (price[n],
        std_err[n]) of the paths' present values, then sums[2 n + 1] when return_sums and stop_hist[n][n_obs + 1] (int64: the
        paths that ended at each observation, the last column at maturity) when return_hist."""
        paths._alive()
        obs, arr = schedule_array(schedule), make_sched_book(book)
        n = len(arr)
        dp = C.POINTER(C.c_double)
        price, se, sums = np.empty(n), np.empty(n), np.empty(2 * n + 1)
        hist = np.zeros((n, len(obs) + 1), dtype=np.int64)
        check(self._L.mcg_price_scheduled(self._ctx, paths._h, r, float(dt), obs, len(obs), arr, n, price.ctypes.data_as(dp),
                                          se.ctypes.data_as(dp), sums.ctypes.data_as(dp) if return_sums else None,
                                          hist.ctypes.data_as(C.POINTER(C.c_int64)) if return_hist else None))
        return (price, se) + ((sums,) if return_sums else ()) + ((hist,) if return_hist else ())

    def sched_path_values(self, paths: PathMatrix, r: float, dt: float, schedule, book, return_stop: bool = True):
        """The present value of every path under every contract of a price_scheduled book (mcg_sched_path_values):
        values[n][n_paths], and stop[n][n_paths] (int32: the observation at which the note ended, n_obs at maturity) when
        return_stop."""
        paths._alive()
        obs, arr = schedule_array(schedule), make_sched_book(book)
        n = len(arr)
        values = np.empty((n, paths.n_paths), dtype=np.float64)
        stop = np.empty((n, paths.n_paths), dtype=np.int32)
        check(self._L.mcg_sched_path_values(self._ctx, paths._h, r, float(dt), obs, len(obs), arr, n,
                                            values.ctypes.data_as(C.POINTER(C.c_double)),
                                            stop.ctypes.data_as(C.POINTER(C.c_int32)) if return_stop else None))
        return (values, stop) if return_stop else values

    def lsm_one_launch_enabled(self) -> bool:
        """False once the one-launch LSM sweep's hand-shake has timed out on this ctx (mcg_lsm_one_launch_enabled)."""
        v = C.c_int()
        check(self._L.mcg_lsm_one_launch_enabled(self._ctx, C.byref(v)))
        return bool(v.value)

    def lsm_one_launch_reset(self) -> None:
        """Allow the one-launch sweep again at once after a time-out (mcg_lsm_one_launch_reset)."""
        check(self._L.mcg_lsm_one_launch_reset(self._ctx))

    def debug_lsm_hooks(self, spin_limit: int = -1, poll_delay: int = 0) -> None:
        """Test hooks of the one-launch sweeps' hand-shake (mcg_debug_lsm_hooks)."""
        check(self._L.mcg_debug_lsm_hooks(self._ctx, int(spin_limit), int(poll_delay)))

    def comm_info(self) -> dict:
        """Collective held by this ctx and the ranks it has seen (mcg_comm_info)."""
        k, n, r, seen = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self._L.mcg_comm_info(self._ctx, C.byref(k), C.byref(n), C.byref(r), C.byref(seen)))
        kinds = {0: "none", 1: "callback", 2: "rccl", 3: "shm", 4: "shm+peer-memory mailbox"}
        return {"kind": kinds.get(k.value, str(k.value)), "n_ranks": n.value, "rank": r.value, "seen_ranks": seen.value}

    def price_asymptotic(self, paths: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool,
                         sigma: float, dividend: float) -> float:
        paths._alive()
        p = C.c_double()
        check(self._L.mcg_price_asymptotic(self._ctx, paths._h, r, K, maturity, dt, int(bool(is_call)), sigma, dividend,
                                           C.byref(p)))
        return p.value

    def price_martingale(self, paths: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool,
                         poly_order: int, max_iterations: int = 5) -> Tuple[float, float, float]:
        """(price, lower, upper) of MartingaleOptimization::PredictOptionPrice."""
        paths._alive()
        p, lo, up = C.c_double(), C.c_double(), C.c_double()
        check(self._L.mcg_price_martingale(self._ctx, paths._h, r, K, maturity, dt, int(bool(is_call)), int(poly_order),
                                           int(max_iterations), C.byref(p), C.byref(lo), C.byref(up)))
        return p.value, lo.value, up.value

    def price_branching(self, paths: PathMatrix, r: float, K: float, maturity: float, dt: float, is_call: bool,
                        num_branches: int, exercise_times, seed: int) -> Tuple[float, float, float]:
        """(price, lower, upper) of BranchingProcesses::PredictOptionPrice; resampling = Philox stream 2 of seed."""
        paths._alive()
        ex = np.ascontiguousarray(exercise_times, dtype=np.int32)
        p, lo, up = C.c_double(), C.c_double(), C.c_double()
        check(self._L.mcg_price_branching(self._ctx, paths._h, r, K, maturity, dt, int(bool(is_call)), int(num_branches),
                                          ex.ctypes.data_as(C.POINTER(C.c_int)), len(ex), int(seed), C.byref(p),
                                          C.byref(lo), C.byref(up)))
        return p.value, lo.value, up.value

    def batch_price_rows(self, rows, n_paths: int = 250, r: float = 0.04, dt: float = 1.0 / 252.0,
                         num_branches: int = 10, poly_order: int = 2, max_iterations: int = 5,
                         seed: int = 0, features=None) -> np.ndarray:
        """mcg_batch_price_rows: rows = sequence of dicts with the mcg_row fields, or the array make_rows() built from
        one (what a caller that prices the same rows repeatedly -- or times the entry point -- holds on to); returns
        [n_rows][4] (asymptotic, branching, lsm, martingale), the driver's four model columns.  features = [n_rows][2]
        (twenty_day_vol, twenty_day_momentum of mcg_row_build): mcg_batch_price_rows6, [n_rows][6] -- the driver's six."""
        arr = rows if isinstance(rows, C.Array) else make_rows(rows)
        n = len(arr)
        dp = C.POINTER(C.c_double)
        if features is None:
            out = np.zeros((n, 4), dtype=np.float64)
            check(self._L.mcg_batch_price_rows(self._ctx, arr, n, int(n_paths), r, dt, int(num_branches),
                                               int(poly_order), int(max_iterations), int(seed), out.ctypes.data_as(dp)))
            return out
        f = np.ascontiguousarray(features, dtype=np.float64)
        if f.shape != (n, 2):
            raise McgError("features must be [n_rows][2]", 1)
        out = np.zeros((n, 6), dtype=np.float64)
        check(self._L.mcg_batch_price_rows6(self._ctx, arr, f.ctypes.data_as(dp), n, int(n_paths), r, dt, int(num_branches),
                                            int(poly_order), int(max_iterations), int(seed), out.ctypes.data_as(dp)))
        return out

    def debug_batch_row_dump(self, rows, row: int, n_paths: int = 250, r: float = 0.04, dt: float = 1.0 / 252.0,
                             num_branches: int = 10, poly_order: int = 2, max_iterations: int = 5, seed: int = 0):
        """Test hook (mcg_debug_batch_row_dump): batch_price_rows with the same arguments, and what the row kernels held for
        row `row`.  Returns (prices [n_rows][4], amp [M], comp [n_steps], block [n_steps + 1][n_paths], step-major)."""
        arr = rows if isinstance(rows, C.Array) else make_rows(rows)
        n = len(arr)
        dp = C.POINTER(C.c_double)
        steps = int(arr[row].n_steps) if 0 <= row < n else 0
        M = 1
        while M < steps:
            M <<= 1
        out = np.zeros((n, 4), dtype=np.float64)
        amp, comp = np.zeros(M), np.zeros(max(steps, 1))
        block = np.zeros((max(steps, 0) + 1, max(int(n_paths), 1)))
        check(self._L.mcg_debug_batch_row_dump(self._ctx, arr, n, int(n_paths), r, dt, int(num_branches), int(poly_order),
                                               int(max_iterations), int(seed), out.ctypes.data_as(dp), int(row),
                                               amp.ctypes.data_as(dp), comp.ctypes.data_as(dp), block.ctypes.data_as(dp)))
        return out, amp, comp[:steps], block

    def debug_batch_budget(self, nbytes: int) -> None:
        """Test hook (mcg_debug_batch_budget): workspace bytes of one chunk of the batched rows (0: the default)."""
        check(self._L.mcg_debug_batch_budget(self._ctx, int(nbytes)))

    def debug_lsm_date_fault(self, mode: int = 0, date: int = 0, workgroup: int = 0, delay: int = 0, spin_limit: int = -1) -> None:
        """Test hook of the per-date LSM route's exchange (mcg_debug_lsm_date_fault)."""
        check(self._L.mcg_debug_lsm_date_fault(self._ctx, int(mode), int(date), int(workgroup), int(delay), int(spin_limit)))

    def probe_write_ceiling(self, n_paths: int = 10_000_000, n_steps: int = 252, reps: int = 5) -> Tuple[float, float]:
        """(GB/s, ms per launch) this board writes with the path matrix's store pattern and no arithmetic
        (mcg_probe_write_ceiling)."""
        g, ms = C.c_double(), C.c_double()
        check(self._L.mcg_probe_write_ceiling(self._ctx, int(n_paths), int(n_steps), int(reps), C.byref(g), C.byref(ms)))
        return g.value, ms.value

    def generator_clock_arm(self, on: bool = True) -> None:
        """The next GBM generator launches stamp their shader clock (off by default; mcg_generator_clock_arm)."""
        check(self._L.mcg_generator_clock_arm(self._ctx, 1 if on else 0))

    def generator_clock(self) -> dict:
        """Shader clock of the last ARMED GBM generator launch, stamped in-kernel (mcg_generator_clock)."""
        med, lo, hi, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        check(self._L.mcg_generator_clock(self._ctx, C.byref(med), C.byref(n), C.byref(lo), C.byref(hi)))
        return {"GHz_median": med.value, "GHz_min": lo.value, "GHz_max": hi.value, "stamping_workgroups": n.value}

    def debug_eval(self, fn: int, x: np.ndarray) -> np.ndarray:
        """Test hook (mcg_debug_eval): one device math routine elementwise; returns [n][4]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty((len(x), 4), dtype=np.float64)
        check(self._L.mcg_debug_eval(self._ctx, int(fn), x.ctypes.data_as(C.POINTER(C.c_double)),
                                     y.ctypes.data_as(C.POINTER(C.c_double)), len(x)))
        return y

    def debug_eval_v(self, fn: int, x: np.ndarray, params=()) -> np.ndarray:
        """Test hook (mcg_debug_eval_v): one device routine with several inputs per element (x: [n][n_in]) and parameters
        shared by the launch; returns [n][4]."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
        y = np.empty((x.shape[0], 4), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(self._L.mcg_debug_eval_v(self._ctx, int(fn), x.ctypes.data_as(dp), x.shape[1], p.ctypes.data_as(dp), len(p),
                                       y.ctypes.data_as(dp), x.shape[0]))
        return y

    def debug_lsm_solve(self, fn: int, nb: int, moments: np.ndarray, params=None) -> np.ndarray:
        """Test hook (mcg_debug_lsm_solve): one regression solve of the LSM sweeps per element, on the moments given
        (moments: [n][n_moments]; params: [n][3] = min_count, K, mu per element, default {1, 1, 0}); returns [n][48]: the
        coefficient block (24 doubles) and the tangent's."""
        m = np.ascontiguousarray(moments, dtype=np.float64)
        if m.ndim == 1:
            m = m.reshape(-1, 1)
        p = np.tile([1.0, 1.0, 0.0], (m.shape[0], 1)) if params is None else np.ascontiguousarray(params, dtype=np.float64)
        if p.shape != (m.shape[0], 3):
            raise McgError("params must be [n][3]", 1)
        p = np.ascontiguousarray(p)
        out = np.empty((m.shape[0], 48), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(self._L.mcg_debug_lsm_solve(self._ctx, int(fn), int(nb), m.ctypes.data_as(dp), m.shape[1], p.ctypes.data_as(dp),
                                          out.ctypes.data_as(dp), m.shape[0]))
        return out

    def debug_gbm_route(self, route: int = -1) -> int:
        """Test hook (mcg_debug_gbm_route): 0 = the generators choose their kernel by size, 1 = the narrow kernel, 2 = the
        wide one, -1 = unchanged; returns what the last GBM launch took (1 or 2; 0: none yet)."""
        last = C.c_int()
        check(self._L.mcg_debug_gbm_route(self._ctx, int(route), C.byref(last)))
        return last.value

    def debug_branch_route(self, route: int = -1, slice_shift: int = 0) -> int:
        """Test hook (mcg_debug_branch_route): 0 = price_branching chooses its kernels by size, 1 = one launch, 2 = a launch
        per date, 3 = binned, 4 = XCD-affine, -1 = unchanged; slice_shift = log2 of the paths in a slice of the gathered row
        (0: 18); returns what the last price_branching took (1..4; 0: none yet)."""
        last = C.c_int()
        check(self._L.mcg_debug_branch_route(self._ctx, int(route), int(slice_shift), C.byref(last)))
        return last.value

    # -- measurement ----------------------------------------------------------------------------
    def timing_enable(self, on: bool = True) -> None:
        check(self._L.mcg_timing_enable(self._ctx, int(on)))

    def timing_select(self, kernels=None) -> None:
        """Bracket only these kernels (_native.K_*) while timing is enabled; None: all of them (mcg_timing_select)."""
        mask = 0xFFFFFFFF if kernels is None else sum(1 << int(k) for k in kernels)
        check(self._L.mcg_timing_select(self._ctx, mask))

    def timing_reset(self) -> None:
        check(self._L.mcg_timing_reset(self._ctx))

    def timing_get(self, kernel: int) -> Tuple[float, int]:
        """(total device ms, launches) for one of _native.K_* since the last reset."""
        ms, n = C.c_double(), C.c_int64()
        check(self._L.mcg_timing_get(self._ctx, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _vec(x) -> np.ndarray:
    return np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float64)))


def _combine_kind(kind) -> int:
    """enum mcg_combine_kind from its name or number; an unknown number goes to the library, which rejects it."""
    if isinstance(kind, str):
        if kind.lower() not in N.COMBINE_KINDS:
            raise McgError(f"unknown combination {kind!r}: one of {sorted(N.COMBINE_KINDS)}", 1)
        return N.COMBINE_KINDS[kind.lower()]
    return int(kind)


def cholesky_corr(corr) -> np.ndarray:
    """Lower Cholesky factor of a correlation matrix, as the multi-asset generator takes it (mcg_cholesky_corr; host only)."""
    L = N.load_library()
    c = np.ascontiguousarray(corr, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise McgError("cholesky_corr: corr must be a square matrix", 1)
    out = np.empty_like(c)
    dp = C.POINTER(C.c_double)
    check(L.mcg_cholesky_corr(c.ctypes.data_as(dp), c.shape[0], out.ctypes.data_as(dp)))
    return out


class LocalVolSurface:
    """A local-volatility surface sigma(t, x) on a rectangular grid (include/mcgpu.h): time knots `times` (strictly increasing,
    1 to 64 of them), n_x equidistant nodes of the log-moneyness x = ln(S / S0) from x_min to x_max (2 to 128), and
    sigma[i][j] >= 0 at (times[i], x_j).  A one-dimensional sigma is a surface without a time axis.  The library checks it."""

    def __init__(self, times, x_min: float, x_max: float, sigma):
        self.times = _vec(times)
        self.sigma = np.ascontiguousarray(np.atleast_2d(np.asarray(sigma, dtype=np.float64)))
        if self.sigma.ndim != 2 or self.sigma.shape[0] != len(self.times):
            raise McgError(f"LocalVolSurface: {len(self.times)} time knots need {len(self.times)} rows of sigma, "
                           f"not an array of shape {self.sigma.shape}", 1)
        self.x_min, self.x_max = float(x_min), float(x_max)

    n_t = property(lambda self: self.sigma.shape[0])
    n_x = property(lambda self: self.sigma.shape[1])

    @classmethod
    def flat(cls, sigma: float) -> "LocalVolSurface":
        """sigma everywhere: the law of PathEngine.gbm."""
        return cls([0.0], -1.0, 1.0, [[sigma, sigma]])

    @classmethod
    def cev(cls, sigma0: float, beta: float, x_min: float, x_max: float, n_x: int) -> "LocalVolSurface":
        """The CEV model dS = mu S dt + sigma0 S0^(1 - beta) S^beta dW sampled at the nodes: sigma(x) = sigma0 exp((beta - 1) x)."""
        x = [x_min + j * (x_max - x_min) / (n_x - 1) for j in range(n_x)]
        return cls([0.0], x_min, x_max, [[sigma0 * math.exp((beta - 1.0) * xj) for xj in x]])


class LsmPolicy:
    """An LSM exercise policy (include/mcgpu.h): the header fields n_steps, poly_order, is_call, r, K, maturity, dt, and coef,
    an (n_steps + 1, 20) array of rows {16 coefficients of y^t, y = (S/K - 1) - centre; regression rows at the fit; centre;
    kind; 0}.  Plain host data: PathEngine.fit_lsm returns one, from_arrays builds one by hand, PathEngine.apply_lsm reads
    one.  The library checks it where it is used."""

    def __init__(self, n_steps: int, poly_order: int, is_call: bool, r: float, K: float, maturity: float, dt: float, coef):
        self.n_steps, self.poly_order, self.is_call = int(n_steps), int(poly_order), bool(is_call)
        self.r, self.K, self.maturity, self.dt = float(r), float(K), float(maturity), float(dt)
        self.coef = np.ascontiguousarray(coef, dtype=np.float64)
        if self.coef.shape != (self.n_steps + 1, N.LSM_POLICY_STRIDE):
            raise McgError(f"LsmPolicy: {self.n_steps} steps need coef of shape ({self.n_steps + 1}, {N.LSM_POLICY_STRIDE}), "
                           f"not {self.coef.shape}", 1)

    @classmethod
    def from_arrays(cls, n_steps: int, poly_order: int, is_call: bool, r: float, K: float, maturity: float, dt: float,
                    coefficients=None, kinds=None, centres=None, counts=None) -> "LsmPolicy":
        """A hand-made policy.  coefficients: (n_steps + 1, <= 16), c_t of y^t per date (default 0); kinds: n_steps + 1 of
        POL_CONTINUE / POL_EXERCISE_RULE / POL_TERMINAL (default: EXERCISE_RULE on every date, TERMINAL on the last row);
        centres, counts: per date (default 0)."""
        rows = int(n_steps) + 1
        coef = np.zeros((max(rows, 0), N.LSM_POLICY_STRIDE))
        if coefficients is not None:
            c = np.atleast_2d(np.asarray(coefficients, dtype=np.float64))
            if c.shape[0] != rows or c.shape[1] > 16:
                raise McgError(f"LsmPolicy.from_arrays: coefficients must have shape ({rows}, <= 16), not {c.shape}", 1)
            coef[:, :c.shape[1]] = c
        if kinds is None:
            kinds = [N.POL_EXERCISE_RULE] * (rows - 1) + [N.POL_TERMINAL]
        coef[:, 18] = _vec(kinds)
        if counts is not None:
            coef[:, 16] = _vec(counts)
        if centres is not None:
            coef[:, 17] = _vec(centres)
        return cls(n_steps, poly_order, is_call, r, K, maturity, dt, coef)

    @property
    def kinds(self) -> np.ndarray:
        """Per date: POL_CONTINUE, POL_EXERCISE_RULE or POL_TERMINAL."""
        return self.coef[:, 18].astype(np.int64)

    def _hdr(self) -> "N.LsmPolicyHdr":
        return N.LsmPolicyHdr(self.n_steps, self.poly_order, int(self.is_call), 0, self.r, self.K, self.maturity, self.dt)

    def continuation(self, j: int, S) -> np.ndarray:
        """The continuation value of date j at the prices S (mcg_lsm_policy_continuation; host only): Horner for an
        EXERCISE_RULE date, +inf for a CONTINUE date, 0 for the terminal one."""
        L = N.load_library()
        s = _vec(S)
        out = np.empty_like(s)
        dp = C.POINTER(C.c_double)
        hdr = self._hdr()
        check(L.mcg_lsm_policy_continuation(C.byref(hdr), self.coef.ctypes.data_as(dp), int(j), s.ctypes.data_as(dp), s.size,
                                            out.ctypes.data_as(dp)))
        return out


def local_vol_table(surface: LocalVolSurface, dt: float, n_steps: int) -> np.ndarray:
    """The per-step slices of a surface as the path kernel reads them (mcg_localvol_table; host only):
    [n_slices][n_x - 1][2] = {a_j, a_{j+1} - a_j}, a = sigma sqrt(dt); one slice for a surface with one time knot, else n_steps."""
    L = N.load_library()
    n_slices = 1 if surface.n_t == 1 else max(int(n_steps), 0)
    out = np.empty((n_slices, max(surface.n_x - 1, 0), 2), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    check(L.mcg_localvol_table(surface.times.ctypes.data_as(dp), surface.n_t, surface.n_x, surface.sigma.ctypes.data_as(dp), dt, n_steps,
                               out.ctypes.data_as(dp)))
    return out


class Sobol:
    """A randomised Sobol' point set (mcg_sobol; include/mcgpu.h states every rule): Joe and Kuo's direction numbers with the
    scramble "plain" (none), "shift" (a digital shift) or "lms" (Matousek's linear matrix scramble and a shift), drawn from
    (seed, replicate); bridge: the dimensions go through a Brownian bridge (the first ones carry most of the variance) instead
    of time order.  Replicates of one seed are independent scrambles: price each and combine them with rqmc_combine -- that
    is the error bar of a Sobol' estimate, not price_european's std_err, which is the iid formula."""

    def __init__(self, seed: int, replicate: int = 0, scramble="lms", bridge: bool = True):
        self.seed, self.replicate, self.bridge = int(seed), int(replicate), bridge
        if isinstance(scramble, str):
            if scramble.lower() not in N.SOBOL_SCRAMBLES:
                raise McgError(f"unknown scramble {scramble!r}: one of {sorted(N.SOBOL_SCRAMBLES)}", 1)
            scramble = N.SOBOL_SCRAMBLES[scramble.lower()]
        self.scramble = int(scramble)  # (an unknown number goes to the library, which rejects it)

    def _spec(self) -> "N.SobolSpec":
        if not 0 <= self.seed < 2 ** 64 or not 0 <= self.replicate < 2 ** 32:
            raise McgError("Sobol: seed must fit 64 bits and replicate 32", 1)
        return N.SobolSpec(self.seed, self.replicate, self.scramble, int(self.bridge))


def sobol_table(sobol: Sobol, n_dims: int):
    """(V, shift) of a point set as the kernels read them (mcg_sobol_table; host only): V [n_dims][32] uint32 direction numbers,
    scrambled or not, and shift [n_dims]; coordinate d of point i is shift[d] ^ XOR of V[d][b] over the set bits b of i ^ (i >> 1)."""
    L = N.load_library()
    v = np.empty((max(int(n_dims), 0), 32), dtype=np.uint32)
    shift = np.empty(max(int(n_dims), 0), dtype=np.uint32)
    up = C.POINTER(C.c_uint32)
    spec = sobol._spec()
    check(L.mcg_sobol_table(C.byref(spec), int(n_dims), v.ctypes.data_as(up), shift.ctypes.data_as(up)))
    return v, shift


def sobol_bridge(n_steps: int, bridge: bool = True) -> np.ndarray:
    """The bridge schedule in dimension order (mcg_sobol_bridge; host only): a structured array of n_steps entries with the
    fields t, l, r, wl, wr, sd -- B(t) = wl B(l) + (wr B(r) + sd z_d), in units of sqrt(dt)."""
    L = N.load_library()
    out = (N.BridgeNode * max(int(n_steps), 1))()
    check(L.mcg_sobol_bridge(int(n_steps), int(bridge), out))
    dtype = np.dtype([("t", np.int32), ("l", np.int32), ("r", np.int32), ("wl", np.float64), ("wr", np.float64), ("sd", np.float64)])
    return np.array([(e.t, e.l, e.r, e.wl, e.wr, e.sd) for e in out[:int(n_steps)]], dtype=dtype)


def rqmc_combine(estimates) -> Tuple[float, float]:
    """(mean, standard error) of independent replicate estimates (mcg_rqmc_combine): std(ddof=1) / sqrt(n), n >= 2.  This is
    the error bar of a Sobol' estimate; price_european's own std_err is the iid formula and does not apply to a Sobol' matrix."""
    L = N.load_library()
    e = _vec(estimates)
    mean, se = C.c_double(), C.c_double()
    check(L.mcg_rqmc_combine(e.ctypes.data_as(C.POINTER(C.c_double)), e.size, C.byref(mean), C.byref(se)))
    return mean.value, se.value


def mlmc_combine(sum_y, sum_y2, n, r: float, T: float) -> Tuple[float, float]:
    """(price, std_err) of a multilevel estimator from its per-level sums of Y and Y^2 and path counts (mcg_mlmc_combine; host
    only): price = e^{-rT} sum_l mean Y_l, std_err = e^{-rT} sqrt(sum_l V_l / N_l) with V_l the unbiased sample variance."""
    L = N.load_library()
    a, b, c = _vec(sum_y), _vec(sum_y2), _vec(n)
    if not (len(a) == len(b) == len(c)):
        raise McgError("mlmc_combine: sum_y, sum_y2 and n hold one value per level", 1)
    dp = C.POINTER(C.c_double)
    price, se = C.c_double(), C.c_double()
    check(L.mcg_mlmc_combine(a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), len(a), r, T, C.byref(price), C.byref(se)))
    return price.value, se.value


def mlmc_bridge_levels(book):
    """The distinct bridge levels [(barrier, is_up), ...] of a price_exotics book in the order mlmc_level(bridge=True) holds them
    (mcg_mlmc_bridge_levels; host only): the barrier contracts' (barrier, up), compared bitwise, by first appearance; a down
    barrier at zero is never touched and takes no level.  Raises McgError for more than four levels or a barrier <= 0 otherwise."""
    arr = make_book(book)
    b, up, n = np.empty(N.MLMC_BRIDGE_L_MAX), (C.c_int * N.MLMC_BRIDGE_L_MAX)(), C.c_int(0)
    check(N.load_library().mcg_mlmc_bridge_levels(arr, len(arr), b.ctypes.data_as(C.POINTER(C.c_double)), up, C.byref(n)))
    return [(float(b[l]), bool(up[l])) for l in range(n.value)]


def mlmc_plan(n, mean, var, cost, eps: float):
    """(n_opt[n_levels], alpha, bias, converged) of mcg_mlmc_plan (host only): Giles' path counts for the target eps from the
    levels' variances and costs, the fitted weak rate, the estimate of the remaining (undiscounted) bias and whether it lies
    below eps / sqrt(2)."""
    L = N.load_library()
    a, b, c, d = _vec(n), _vec(mean), _vec(var), _vec(cost)
    if not (len(a) == len(b) == len(c) == len(d)):
        raise McgError("mlmc_plan: n, mean, var and cost hold one value per level", 1)
    dp = C.POINTER(C.c_double)
    n_opt = np.empty(max(len(a), 1))
    alpha, bias, conv = C.c_double(), C.c_double(), C.c_int()
    check(L.mcg_mlmc_plan(a.ctypes.data_as(dp), b.ctypes.data_as(dp), c.ctypes.data_as(dp), d.ctypes.data_as(dp), len(a), eps,
                          n_opt.ctypes.data_as(dp), C.byref(alpha), C.byref(bias), C.byref(conv)))
    return n_opt[:len(a)], alpha.value, bias.value, bool(conv.value)


class MlmcResult(tuple):
    """What mlmc_local_vol returns: (price[n], std_err[n]) as a pair, and as attributes the per-level table `levels` (dicts of
    n_fine, paths, mean_y[n], var_y[n], mean_pf[n], cost in path-steps a path), bias_estimate[n] (discounted), converged and
    cost, the total in path-steps."""

    def __new__(cls, price, std_err, levels, bias_estimate, converged, cost):
        self = super().__new__(cls, (price, std_err))
        self.price, self.std_err, self.levels = price, std_err, levels
        self.bias_estimate, self.converged, self.cost = bias_estimate, converged, cost
        return self


def make_rows(rows):
    """ctypes array of mcg_row from a sequence of dicts with its fields (built once, passed to batch_price_rows as is)."""
    arr = (N.Row * len(rows))()
    names = [k for k, _ in N.Row._fields_]
    for i, d in enumerate(rows):
        r = arr[i]
        for k in names:
            setattr(r, k, d[k])
    return arr


def exotic(kind, is_call: bool, K: float = 0.0, barrier: float = 0.0, rebate: float = 0.0) -> tuple:
    """One contract of a price_exotics book: (kind, is_call, K, barrier, rebate).  kind: one of _native.X_* or its name
    ("asian_arith_fixed", "lookback_float", "barrier_up_out", ...: _native.EXOTIC_KINDS)."""
    k = N.EXOTIC_KINDS.get(kind.lower()) if isinstance(kind, str) else (int(kind) if int(kind) in N.EXOTIC_KINDS.values() else None)
    if k is None:
        raise McgError(f"unknown exotic kind {kind!r}: one of {sorted(N.EXOTIC_KINDS)} or 0..9", 1)
    return (k, bool(is_call), float(K), float(barrier), float(rebate))


def make_book(book):
    """ctypes array of mcg_exotic from a sequence of exotic(...) tuples or dicts with the mcg_exotic fields (fields a
    dict leaves out are 0).  Kinds and counts are checked by the library."""
    names = [k for k, _ in N.Exotic._fields_]
    arr = (N.Exotic * len(book))()
    for i, c in enumerate(book):
        vals = [c.get(k, 0) for k in names] if isinstance(c, dict) else c
        arr[i] = N.Exotic(int(vals[0]), int(bool(vals[1])), float(vals[2]), float(vals[3]), float(vals[4]))
    return arr


def schedule(entries) -> list:
    """The observation schedule of price_scheduled as a list of (row, flags).  entries: a sequence of (row, flags) with flags
    an int (_native.OBS_* or-ed) or names joined by "|" or given as a sequence ("coupon|call", ("ki",): _native.OBS_FLAGS).
    Rows must be non-negative and strictly increasing; what the matrix allows is checked by the library."""
    out = []
    for e in entries:
        row, flags = e
        if isinstance(flags, str):
            flags = [f for f in flags.replace(" ", "").split("|") if f]
        if not isinstance(flags, (int, np.integer)):
            names = list(flags)
            unknown = [f for f in names if not isinstance(f, str) or f.lower() not in N.OBS_FLAGS]
            if unknown:
                raise McgError(f"unknown observation flag {unknown[0]!r}: one of {sorted(N.OBS_FLAGS)}", 1)
            flags = 0
            for f in names:
                flags |= N.OBS_FLAGS[f.lower()]
        flags = int(flags)
        if flags & ~(N.OBS_COUPON | N.OBS_CALL | N.OBS_KI | N.OBS_RESET) or flags < 0:
            raise McgError(f"observation flags {flags:#x} outside the mask 0xf", 1)
        if int(row) != row or int(row) < 0:
            raise McgError(f"observation row must be a non-negative integer (got {row!r})", 1)
        if out and int(row) <= out[-1][0]:
            raise McgError(f"observation rows must be strictly increasing ({int(row)} after {out[-1][0]})", 1)
        out.append((int(row), flags))
    if not out:
        raise McgError("a schedule needs at least one observation", 1)
    return out


def schedule_array(entries):
    """ctypes array of mcg_obs from what schedule(...) takes; an array of _native.Obs passes as it is (the library checks it)."""
    if isinstance(entries, C.Array) and entries._type_ is N.Obs:
        return entries
    obs = schedule(entries)
    return (N.Obs * len(obs))(*[N.Obs(row, flags) for row, flags in obs])


def autocall(call_level: float, coupon: float, coupon_level: float = 0.0, ki_level: float = 0.0, put_strike: float = 1.0,
             memory: bool = False) -> tuple:
    """One autocallable of a price_scheduled book, in the order of the mcg_sched fields.  Levels are fractions of the path's
    own row-0 value; call_level = inf: never called; ki_level = 0: no knock-in."""
    vals = (float(call_level), float(coupon_level), float(coupon), float(ki_level), float(put_strike))
    if math.isnan(vals[0]) or not all(math.isfinite(v) for v in vals[1:4]):
        raise McgError("autocall: coupon, coupon_level and ki_level must be finite, call_level not NaN", 1)
    if not vals[4] > 0.0:
        raise McgError(f"autocall: put_strike must be positive (got {put_strike!r})", 1)
    return (N.S_AUTOCALL, int(bool(memory))) + vals + (0.0, 0.0, 0.0, 0.0)


def cliquet(local_floor: float = -math.inf, local_cap: float = math.inf, global_floor: float = -math.inf,
            global_cap: float = math.inf) -> tuple:
    """One cliquet of a price_scheduled book, in the order of the mcg_sched fields: the sum of the period returns between the
    schedule's RESET dates, each clamped to [local_floor, local_cap], the sum to [global_floor, global_cap]."""
    vals = (float(local_floor), float(local_cap), float(global_floor), float(global_cap))
    if any(math.isnan(v) for v in vals):
        raise McgError("cliquet: a bound is NaN", 1)
    if vals[0] > vals[1] or vals[2] > vals[3]:
        raise McgError("cliquet: a floor lies above its cap", 1)
    return (N.S_CLIQUET, 0, 0.0, 0.0, 0.0, 0.0, 1.0) + vals


def make_sched_book(book):
    """ctypes array of mcg_sched from a sequence of autocall(...) / cliquet(...) tuples or dicts with the mcg_sched fields
    (fields a dict leaves out are 0).  Kinds, values and counts are checked by the library."""
    names = [k for k, _ in N.Sched._fields_]
    arr = (N.Sched * len(book))()
    for i, c in enumerate(book):
        vals = [c.get(k, 0) for k in names] if isinstance(c, dict) else c
        if len(vals) != len(names):
            raise McgError(f"contract {i}: expected the {len(names)} fields of mcg_sched (got {len(vals)})", 1)
        arr[i] = N.Sched(int(vals[0]), int(bool(vals[1])), *[float(v) for v in vals[2:]])
    return arr


class CvResult(tuple):
    """What price_exotics_cv and exotics_cv_from_sums return: (price, std_err, beta, plain_price, plain_se), each an array over
    the contracts (beta: [n][2]), with the same by name and .sums (None unless asked for)."""
    FIELDS = ("price", "std_err", "beta", "plain_price", "plain_se")

    def __new__(cls, price, std_err, beta, plain_price, plain_se, sums=None):
        self = super().__new__(cls, (price, std_err, beta, plain_price, plain_se))
        self.sums = sums
        return self

    price, std_err, beta, plain_price, plain_se = (property(lambda self, i=i: self[i]) for i in range(5))

    @property
    def variance_ratio(self):
        """(plain_se / std_err)^2: the factor in path count the controls are worth (inf where std_err is 0)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return (self.plain_se / self.std_err) ** 2


class DualResult(tuple):
    """What dual_upper_lsm returns: (upper, std_err, sums3, inner_steps), then cont and d where they were asked for, with the
    same by name (.cont and .d are None unless asked for)."""

    def __new__(cls, upper, std_err, sums3, inner_steps, cont=None, d=None):
        self = super().__new__(cls, (upper, std_err, sums3, inner_steps) + tuple(x for x in (cont, d) if x is not None))
        self.cont, self.d = cont, d
        return self

    upper, std_err, sums3, inner_steps = (property(lambda self, i=i: self[i]) for i in range(4))


def control(form, mean: Optional[float] = None, on_twin: bool = False, **exotic_fields) -> tuple:
    """One control of price_exotics_cv: (form, on_twin, (kind, is_call, K, barrier, rebate), mean).  form: "payoff", "vanilla",
    "st", "a", "g" or _native.CV_*; exotic_fields: the exotic(...) arguments the form reads (payoff: kind, is_call, K, ...;
    vanilla: is_call, K).  mean: the control's known undiscounted expectation; None leaves it to be filled (gbm_expectation
    returns the tuple completed)."""
    f = N.CONTROL_FORMS.get(form.lower()) if isinstance(form, str) else (int(form) if int(form) in N.CONTROL_FORMS.values() else None)
    if f is None:
        raise McgError(f"unknown control form {form!r}: one of {sorted(N.CONTROL_FORMS)} or 0..4", 1)
    unknown = set(exotic_fields) - {"kind", "is_call", "K", "barrier", "rebate"}
    if unknown:
        raise McgError(f"control: unknown fields {sorted(unknown)}", 1)
    if f == N.CV_PAYOFF and "kind" not in exotic_fields:
        raise McgError('control: form "payoff" needs kind=...', 1)
    x = exotic(exotic_fields.get("kind", N.X_ASIAN_ARITH_FIXED), exotic_fields.get("is_call", True), exotic_fields.get("K", 0.0),
               exotic_fields.get("barrier", 0.0), exotic_fields.get("rebate", 0.0))
    return (f, bool(on_twin), x, None if mean is None else float(mean))


def _control_struct(c, need_mean=True) -> "N.Control":
    form, on_twin, x, mean = (c.get("form"), c.get("on_twin", False), c.get("x"), c.get("mean")) if isinstance(c, dict) else c
    if mean is None and need_mean:
        raise McgError("control: mean is not set (pass mean=..., or complete the control with gbm_expectation)", 1)
    x = x if x is not None else (0, True, 0.0, 0.0, 0.0)
    return N.Control(int(form), int(bool(on_twin)), N.Exotic(int(x[0]), int(bool(x[1])), float(x[2]), float(x[3]), float(x[4])),
                     0.0 if mean is None else float(mean))


def make_controls(controls):
    """ctypes array of mcg_control from a sequence of control(...) tuples (at least one element long: an empty sequence gives
    an array the library is told holds none)."""
    arr = (N.Control * len(controls))()
    for i, c in enumerate(controls):
        arr[i] = _control_struct(c)
    return arr


def make_ctrl(ctrl, n_contracts: int):
    """ctypes int array [2 n] from per-contract pairs (a, b), single indices a, or None."""
    if len(ctrl) != n_contracts:
        raise McgError(f"ctrl holds {len(ctrl)} entries for {n_contracts} contracts", 1)
    arr = (C.c_int * (2 * max(n_contracts, 1)))()
    for i, pair in enumerate(ctrl):
        a, b = (pair, -1) if pair is None or isinstance(pair, (int, np.integer)) else (tuple(pair) + (-1, -1))[:2]
        arr[2 * i], arr[2 * i + 1] = (-1 if a is None else int(a)), (-1 if b is None else int(b))
    return arr


def make_twin(twin) -> "N.GbmTwin":
    """mcg_gbm_twin from a dict (seed, S0, r, sigma, dt; q and path_begin default to 0) or a tuple in the struct's order."""
    if isinstance(twin, N.GbmTwin):
        return twin
    if isinstance(twin, dict):
        unknown = set(twin) - {k for k, _ in N.GbmTwin._fields_}
        if unknown:
            raise McgError(f"twin: unknown fields {sorted(unknown)}", 1)
        try:
            return N.GbmTwin(int(twin["seed"]), float(twin["S0"]), float(twin["r"]), float(twin.get("q", 0.0)), float(twin["sigma"]),
                             float(twin["dt"]), int(twin.get("path_begin", 0)))
        except KeyError as e:
            raise McgError(f"twin: field {e.args[0]!r} is missing", 1) from None
    if len(twin) != 7:
        raise McgError("twin: a tuple holds (seed, S0, r, q, sigma, dt, path_begin)", 1)
    return N.GbmTwin(int(twin[0]), *(float(v) for v in twin[1:6]), int(twin[6]))


def gbm_expectation(ctl, S0: float, r: float, sigma: float, dt: float, n_steps: int, first_row: int = 1, q: float = 0.0) -> tuple:
    """The control completed with its closed-form mean under GBM on the dates first_row .. n_steps (mcg_gbm_expectation; host
    only): forms "st" and "a" (model-free: sigma is not read), "g", "vanilla", and "payoff" with kind asian_geo_fixed."""
    L = N.load_library()
    c = _control_struct(ctl, need_mean=False)
    m = C.c_double()
    check(L.mcg_gbm_expectation(C.byref(c), S0, r, q, sigma, dt, int(n_steps), int(first_row), C.byref(m)))
    form, on_twin, x, _ = (ctl.get("form"), ctl.get("on_twin", False), ctl.get("x"), None) if isinstance(ctl, dict) else ctl
    return (form, on_twin, x, m.value)


def exotics_cv_from_sums(sums, ctrl, r: float, T: float) -> CvResult:
    """The estimator of price_exotics_cv from its sums[9 n + 1] (mcg_exotics_cv_from_sums; host only) -- how a caller combines
    the sums of shards by hand.  ctrl as in price_exotics_cv (only which entries are set is read)."""
    L = N.load_library()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.ndim != 1 or len(s) < 10 or (len(s) - 1) % 9:
        raise McgError(f"sums holds 9 values per contract and then n, not {s.shape}", 1)
    n = (len(s) - 1) // 9
    idx = make_ctrl(ctrl, n)
    dp = C.POINTER(C.c_double)
    price, se, beta, pp, ps = np.empty(n), np.empty(n), np.empty((n, 2)), np.empty(n), np.empty(n)
    check(L.mcg_exotics_cv_from_sums(s.ctypes.data_as(dp), n, idx, r, T, price.ctypes.data_as(dp), se.ctypes.data_as(dp),
                                     beta.ctypes.data_as(dp), pp.ctypes.data_as(dp), ps.ctypes.data_as(dp)))
    return CvResult(price, se, beta, pp, ps, s)


def row_features(hist) -> Tuple[float, float]:
    """(twenty_day_vol, twenty_day_momentum) of a spot history (mcg_row_features; PredictionGen.cpp:313-347)."""
    L = N.load_library()
    h = np.ascontiguousarray(hist, dtype=np.float64)
    v, m = C.c_double(), C.c_double()
    check(L.mcg_row_features(h.ctypes.data_as(C.POINTER(C.c_double)), len(h), C.byref(v), C.byref(m)))
    return v.value, m.value


def row_build(hist, underlying_last: float, dte: float, strike_dist_pct: float, option_type: int, dividend: float = 0.08):
    """(row dict with the mcg_row fields, (twenty_day_vol, twenty_day_momentum)) from the driver's own inputs of one
    option row (mcg_row_build; PredictionGen.cpp:664-719)."""
    L = N.load_library()
    h = np.ascontiguousarray(hist, dtype=np.float64)
    row, f = N.Row(), (C.c_double * 2)()
    check(L.mcg_row_build(h.ctypes.data_as(C.POINTER(C.c_double)), len(h), underlying_last, dte, strike_dist_pct, int(option_type),
                          dividend, C.byref(row), f))
    return {k: getattr(row, k) for k, _ in N.Row._fields_}, (f[0], f[1])


def stats(reset: bool = False) -> dict:
    """Process-wide event counters of libmcgpu (mcg_stats): what ran and what fell back."""
    L = N.load_library()
    s = N.Stats()
    check(L.mcg_stats(C.byref(s), int(bool(reset))))
    return {k: int(getattr(s, k)) for k, _ in N.Stats._fields_}


def estimate_params(hist) -> dict:
    """Host-side estimators of the class API (RoughVolatility.cpp:324-331)."""
    L = N.load_library()
    h = np.ascontiguousarray(hist, dtype=np.float64)
    out = np.empty(5)
    check(L.mcg_estimate_params(h.ctypes.data_as(C.POINTER(C.c_double)), len(h), out.ctypes.data_as(C.POINTER(C.c_double))))
    return dict(xi=out[0], H=out[1], eta=out[2], rho=out[3], S0=out[4])


def rbergomi_spectrum(H: float, eta: float, dt: float, n_steps: int):
    """(amp[Mz], comp[n_steps]) -- the LDS-staged spectral amplitudes and compensator."""
    L = N.load_library()
    M = 1
    while M < n_steps:
        M *= 2
    amp, comp, mz = np.empty(M), np.empty(n_steps), C.c_int()
    check(L.mcg_rbergomi_spectrum(H, eta, dt, n_steps, amp.ctypes.data_as(C.POINTER(C.c_double)),
                                  comp.ctypes.data_as(C.POINTER(C.c_double)), C.byref(mz)))
    assert mz.value == M
    return amp, comp


def bates_constants(jump_intensity: float, jump_mean: float, jump_std: float, dt: float):
    """Test hook, host-only (mcg_debug_bates_constants): (comp, T[16]) as the Bates generators derive them -- the compensator
    of a step and the sixteen word thresholds of the jump count, as Python ints."""
    T, comp = (C.c_uint32 * 16)(), C.c_double()
    check(N.load_library().mcg_debug_bates_constants(float(jump_intensity), float(jump_mean), float(jump_std), float(dt), T,
                                                    C.byref(comp)))
    return comp.value, [int(t) for t in T]


def sincos2_tables():
    """Test hook, host-only (mcg_debug_sincos2_tables): (coarse[4096][2], fine[4096][2]), the {cos, sin} tables of the wide
    GBM generator's two-level sin/cos."""
    L = N.load_library()
    coarse, fine = np.empty((4096, 2)), np.empty((4096, 2))
    check(L.mcg_debug_sincos2_tables(coarse.ctypes.data_as(C.POINTER(C.c_double)), fine.ctypes.data_as(C.POINTER(C.c_double))))
    return coarse, fine
