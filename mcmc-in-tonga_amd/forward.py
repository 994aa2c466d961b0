"""Forward model -- drop-in mirror of MCsub.jl's ``evaluate`` / ``Interpolation``.

Same names, argument meaning and return values as the reference:

* ``evaluate(model, dataStruct, TD_parameters) -> (model, dataStruct, valid)``
  (MCsub.jl:123-185): mutates and returns the SAME model object, setting
  ``phi``, ``ptS`` (fresh array), ``tS`` (alias of dataStruct.tS) and
  ``likelihood``; honours ``debug_prior``.
* ``Interpolation(TD_parameters, model, X, Y, Z) -> ndarray`` (MCsub.jl:306-336).
* ``v_nearest(x, y, z, mx, my, mz, mv)`` (MCsub.jl:247-263).

All arithmetic runs in libtdstar's HIP kernels (``TdContext``); there is no
CPU path.  ``interp_style == 2`` (IDW) is broken in the reference (MCsub.jl:332
uses undefined names) and raises here too.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, f64, lib, ptr


def _pack_models(models, ncomp=4, empty_ok=True):
    """(cell offsets [nmodels + 1], the first ``ncomp`` arrays of every model behind one another).  Of no model:
    empty arrays where ``empty_ok`` (the library refuses the call), else the ValueError of the concatenation."""
    off = np.zeros(len(models) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(m[0]) for m in models])
    cat = [f64(np.concatenate([np.asarray(m[k], dtype=np.float64) for m in models])) if len(models) or not empty_ok
           else np.zeros(0) for k in range(ncomp)]
    return off, cat


def _chain_lens(chain_len):
    """The rows of each chain as the int64 array the library reads, or None."""
    return np.ascontiguousarray(chain_len, dtype=np.int64).ravel() if chain_len is not None else None


def _history_handles(histories, count=True):
    """(the td_history handles of chain.History objects as a C array, the samples they hold -- one library call per
    history -- or None unless ``count``)"""
    histories = list(histories)
    hs = (ctypes.c_void_p * len(histories))(*[h.h for h in histories])
    return hs, sum(len(h) for h in histories) if count else None


class TdContext:
    """A td_ctx: the device-resident copy of a DataStruct's ray geometry."""

    def __init__(self, rayX, rayY, rayZ, rayL, rayU, tS, allSig, device=-1):
        self.m, self.n = np.asarray(rayX).shape
        # column-major m x n == C-order of the n x m transpose
        cm = lambda a: f64(np.asarray(a, dtype=np.float64).T)
        self._arrays = [cm(rayX), cm(rayY), cm(rayZ), cm(rayL), cm(rayU), f64(tS), f64(allSig)]
        X, Y, Z, L, U, t, s = self._arrays
        h = ctypes.c_void_p()
        check(lib().td_create(ctypes.byref(h), int(device), ptr(X), ptr(Y), ptr(Z), ptr(L), ptr(U), self.m, self.n,
                              ptr(t), ptr(s)))
        self.h = h
        info = _lib.TdInfo()
        check(lib().td_get_info(self.h, ctypes.byref(info)), self.h)
        self.P = int(info.npoints)
        self.S = int(info.nsegments)
        self.likelihood_const = float(info.likelihood)
        self.arch = info.arch.decode()
        self.device = int(info.device)
        self.num_cus = int(info.num_cus)

    @classmethod
    def from_datastruct(cls, ds, device=-1):
        return cls(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, device)

    def close(self):
        if getattr(self, "h", None):
            lib().td_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sigma(self, allSig):
        s = f64(allSig)
        check(lib().td_set_sigma(self.h, ptr(s)), self.h)
        info = _lib.TdInfo()
        check(lib().td_get_info(self.h, ctypes.byref(info)), self.h)
        self.likelihood_const = float(info.likelihood)

    def misfit(self, ptS, tS, allSig):
        """(phi, likelihood) of a given ptS (MCsub.jl:169-182) on this device:
        the reduction step of a ray-sharded evaluate (td_misfit)."""
        p, t, s = f64(ptS), f64(tS), f64(allSig)
        if not (len(p) == len(t) == len(s)):
            raise ValueError("ptS, tS and allSig must have the same length")
        phi, lk = ctypes.c_double(), ctypes.c_double()
        check(lib().td_misfit(self.h, len(p), ptr(p), ptr(t), ptr(s), ctypes.byref(phi), ctypes.byref(lk)), self.h)
        return phi.value, lk.value

    INCR_FULL, INCR_LAUNCH, INCR_RESIDENT = 0, 1, 2

    def set_incremental(self, mode):
        """td_evaluate's incremental path: INCR_RESIDENT (default: a resident
        kernel answers every call), INCR_LAUNCH (one launch per call; use it when
        other GPU work, e.g. a collective, runs between evaluates) or INCR_FULL."""
        check(lib().td_set_incremental(self.h, int(mode)), self.h)

    NN_AUTO, NN_BRUTE, NN_GRID, NN_BRUTE_SPLIT = 0, 1, 2, 3

    def set_nn_method(self, method):
        """Nearest-cell search: NN_AUTO (bucket grid from 256 cells on), NN_BRUTE
        (every point x every cell, the reference's loop: one launch of k_nn_tile
        where it fits), NN_GRID, NN_BRUTE_SPLIT (brute force through k_nn_partial
        + k_nn_merge).  Same answer."""
        check(lib().tdt_set_nn_method(self.h, int(method)), self.h)

    def timing(self, enable=None, reset=False, kernel=None):
        """Per-kernel HIP-event timing: enable/reset, or read (launches, total_ms) of `kernel`."""
        if enable is not None:
            check(lib().td_timing_enable(self.h, int(bool(enable))), self.h)
        if reset:
            check(lib().td_timing_reset(self.h), self.h)
        if kernel is not None:
            n = ctypes.c_int64()
            ms = ctypes.c_double()
            check(lib().td_timing_get(self.h, kernel.encode(), ctypes.byref(n), ctypes.byref(ms)), self.h)
            return n.value, ms.value
        return None

    def evaluate(self, cells, debug_prior=0, want_nearest=False):
        """-> (ptS[n], phi, likelihood, nearest[P] or None)"""
        xc, yc, zc, ze = (f64(c) for c in cells)
        ptS = np.zeros(self.n)
        phi = ctypes.c_double()
        lk = ctypes.c_double()
        near = np.empty(max(self.P, 1), dtype=np.int32) if want_nearest else None
        check(lib().td_evaluate(self.h, ptr(xc), ptr(yc), ptr(zc), ptr(ze), len(xc), int(debug_prior), ptr(ptS),
                                ctypes.byref(phi), ctypes.byref(lk),
                                ptr(near, _lib._pi32) if near is not None else None), self.h)
        return ptS, phi.value, lk.value, (near[:self.P] if near is not None else None)

    def evaluate_batch(self, models):
        """Several cell sets -> (ptS[k, n], phi[k], likelihood[k])."""
        off = np.zeros(len(models) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(m[0]) for m in models])
        cat = [f64(np.concatenate([m[i] for m in models])) if len(models) else np.zeros(0) for i in range(4)]
        ptS = np.zeros((len(models), self.n))
        phi = np.zeros(len(models))
        lk = np.zeros(len(models))
        check(lib().td_evaluate_batch(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), ptr(ptS),
                                      ptr(phi), ptr(lk)), self.h)
        return ptS, phi, lk

    def rasterize(self, models, qx, qy, qz, want_values=False):
        """td_rasterize: -> (mean[nq], std[nq], values[nmodels, nq] or None).
        models: list of (x, y, z, zeta) cell arrays in model_hist order."""
        off, cat = _pack_models(models, empty_ok=False)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        mean, std = np.empty(nq), np.empty(nq)
        vals = np.empty((len(models), nq)) if want_values else None
        check(lib().td_rasterize(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), ptr(qx), ptr(qy),
                                 ptr(qz), nq, ptr(mean), ptr(std), ptr(vals) if want_values else None), self.h)
        return mean, std, vals

    def rasterize_history(self, histories, qx, qy, qz, want_values=False):
        """td_history_rasterize: ``rasterize`` on the samples of the histories (chain.History), history
        by history in sample order, without the models visiting the host."""
        hs, nm = _history_handles(histories)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        mean, std = np.empty(nq), np.empty(nq)
        vals = np.empty((nm, nq)) if want_values else None
        check(lib().td_history_rasterize(self.h, hs, len(hs), ptr(qx), ptr(qy), ptr(qz), nq, ptr(mean),
                                         ptr(std), ptr(vals) if want_values else None), self.h)
        return mean, std, vals

    MARG_AUTO, MARG_RESIDENT, MARG_STREAMING = 0, 1, 2

    def set_marginals_method(self, method):
        """How ``marginals`` selects the order statistics: MARG_AUTO (columns sorted in LDS up to
        ``marginals_resident_max()`` models, a radix select over device memory beyond), MARG_RESIDENT,
        MARG_STREAMING.  Same answer."""
        check(lib().tdt_set_marginals_method(self.h, int(method)), self.h)

    def marginals_resident_max(self):
        m = ctypes.c_int64()
        check(lib().tdt_marginals_resident_max(self.h, ctypes.byref(m)), self.h)
        return m.value

    @staticmethod
    def marginals_plan(nmodels, nq, num_cus, method=0, nprob=1):
        """(resident, Mp, W, threads, dynamic LDS bytes) of the quantile kernel ``marginals`` launches for
        ``nmodels`` x ``nq`` values on ``num_cus`` compute units under ``method``; needs no GPU."""
        out = np.zeros(5, dtype=np.int64)
        check(lib().tdt_marginals_plan(int(nmodels), int(nq), int(num_cus), int(method), int(nprob),
                                       ptr(out, _lib._pi64)))
        return bool(out[0]), int(out[1]), int(out[2]), int(out[3]), int(out[4])

    @staticmethod
    def _marginals_want(nq, probs, bins):
        """(td_marginals, the arrays it points to, quantiles or None, hist or None)"""
        probs = f64(np.ravel(np.asarray(probs, dtype=np.float64)))
        nbins, lo, hi = (int(bins[0]), float(bins[1]), float(bins[2])) if bins is not None else (0, 0.0, 0.0)
        quant = np.empty((len(probs), nq)) if len(probs) else None
        hist = np.zeros((nq, nbins + 3), dtype=np.int64) if nbins > 0 else None
        want = _lib.TdMarginals(len(probs), ptr(probs) if len(probs) else None, ptr(quant), nbins, lo, hi,
                                ptr(hist, _lib._pi64))
        return want, (probs, quant, hist), quant, hist

    def marginals(self, models, qx, qy, qz, probs=(), bins=None):
        """td_rasterize_marginals: -> dict(mean[nq], std[nq], quantiles[nprob, nq] or None,
        hist[nq, nbins + 3] or None).  ``probs``: probabilities in [0, 1] (Julia's default quantile
        over the models at each point); ``bins`` = (nbins, lo, hi): per-point counts below lo, in the
        nbins equal bins of [lo, hi), at or above hi, and NaN.  models as for ``rasterize``."""
        off, (cx, cy, cz, cv) = _pack_models(models, empty_ok=False)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        mean, std = np.empty(nq), np.empty(nq)
        want, held, quant, hist = self._marginals_want(nq, probs, bins)
        check(lib().td_rasterize_marginals(self.h, len(models), ptr(off, _lib._pi64), ptr(cx), ptr(cy), ptr(cz),
                                           ptr(cv), ptr(qx), ptr(qy), ptr(qz), nq, ptr(mean), ptr(std),
                                           ctypes.byref(want)), self.h)
        del held
        return dict(mean=mean, std=std, quantiles=quant, hist=hist)

    def marginals_history(self, histories, qx, qy, qz, probs=(), bins=None):
        """td_history_marginals: ``marginals`` on the samples of the histories (chain.History), history by
        history in sample order, without the models visiting the host."""
        hs, _ = _history_handles(histories, count=False)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        mean, std = np.empty(nq), np.empty(nq)
        want, held, quant, hist = self._marginals_want(nq, probs, bins)
        check(lib().td_history_marginals(self.h, hs, len(hs), ptr(qx), ptr(qy), ptr(qz), nq, ptr(mean),
                                         ptr(std), ctypes.byref(want)), self.h)
        del held
        return dict(mean=mean, std=std, quantiles=quant, hist=hist)

    def zeta_hist(self, histories, bins):
        """td_history_zeta_hist: -> dict(zeta_hist[nbins + 3], ncells[samples]) over every sample of the
        histories; ``bins`` = (nbins, lo, hi), slots as in ``marginals``."""
        nbins, lo, hi = int(bins[0]), float(bins[1]), float(bins[2])
        hist = np.zeros(max(nbins, 0) + 3, dtype=np.int64)
        hs, nm = _history_handles(histories)
        ncells = np.zeros(max(nm, 1), dtype=np.int64)
        check(lib().td_history_zeta_hist(self.h, hs, len(hs), nbins, lo, hi, ptr(hist, _lib._pi64),
                                         ptr(ncells, _lib._pi64)), self.h)
        return dict(zeta_hist=hist, ncells=ncells[:nm])

    CONV_ALL = ("rhat", "ess", "lags")

    def set_convergence_round(self, R):
        """The lags ``convergence`` computes per round (0: auto; else even, >= 2).  Same answer."""
        check(lib().tdt_set_convergence_round(self.h, int(R)), self.h)

    def set_convergence_lag_block(self, LB):
        """The lags one wave of the autocovariance kernel accumulates (0: auto; 8; 16).  Same answer."""
        check(lib().tdt_set_convergence_lag_block(self.h, int(LB)), self.h)

    @staticmethod
    def _convergence_want(ncol, max_lag, want):
        """(td_convergence, dict of the arrays it points to)"""
        out = {}
        if "rhat" in want:
            out["rhat"] = np.empty(ncol)
        if "ess" in want:
            out["ess"] = np.empty(ncol)
        if "lags" in want:
            out["lags"] = np.zeros(ncol, dtype=np.int32)
        w = _lib.TdConvergence(int(max_lag), ptr(out.get("rhat")), ptr(out.get("ess")),
                               ptr(out.get("lags"), _lib._pi32))
        return w, out

    def _stat_wants(self, ncol, probs, bins, conv, max_lag):
        """The marginals and convergence parts of a request on ``ncol`` columns -> (address of the td_marginals or
        None, address of the td_convergence or None, the result entries: quantiles, hist and with ``conv`` rhat, ess,
        lags; what the addresses point into: keep it until the call has returned)."""
        entries = dict(quantiles=None, hist=None)
        marg = cw = arrays = None
        if len(np.ravel(probs)) or bins is not None:
            marg, arrays, entries["quantiles"], entries["hist"] = self._marginals_want(ncol, probs, bins)
        if conv:
            cw, out = self._convergence_want(ncol, max_lag, self.CONV_ALL)
            entries.update(out)
        return (ctypes.addressof(marg) if marg is not None else None, ctypes.addressof(cw) if cw is not None else None,
                entries, (marg, cw, arrays))

    def convergence(self, values, chain_len, max_lag=0, want=CONV_ALL):
        """td_convergence_values: -> dict(rhat[ncol], ess[ncol], lags[ncol]) of the columns of
        ``values`` [M, ncol] (or [M]: one column), whose rows are the chains' samples, chain after chain
        with ``chain_len`` rows each.  Split R-hat over the halves of every chain's last 2n rows
        (n = min(chain_len) // 2) and the effective sample size by Geyer's initial monotone sequence
        over at most ``max_lag`` lags (0: n - 1); ``lags``: the last lag summed, negative where the cap
        or n ended the sum (ess is then an upper bound).  ``want``: the subset to compute."""
        V = f64(values)
        if V.ndim == 1:
            V = V.reshape(-1, 1)
        lens = np.ascontiguousarray(chain_len, dtype=np.int64).ravel()
        w, out = self._convergence_want(V.shape[1], max_lag, want)
        check(lib().td_convergence_values(self.h, ptr(V), V.shape[0], V.shape[1], len(lens), ptr(lens, _lib._pi64),
                                          ctypes.byref(w)), self.h)
        return out

    def convergence_models(self, models, chain_len, qx, qy, qz, max_lag=0, want=CONV_ALL):
        """td_rasterize_convergence: ``convergence`` of the value matrix of ``rasterize`` (models as
        there, chain after chain), which stays on the device; also ``mean`` and ``std``."""
        off, cat = _pack_models(models, empty_ok=False)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        lens = np.ascontiguousarray(chain_len, dtype=np.int64).ravel()
        mean, std = np.empty(nq), np.empty(nq)
        w, out = self._convergence_want(nq, max_lag, want)
        check(lib().td_rasterize_convergence(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), ptr(qx),
                                             ptr(qy), ptr(qz), nq, len(lens), ptr(lens, _lib._pi64), ptr(mean),
                                             ptr(std), ctypes.byref(w)), self.h)
        return dict(out, mean=mean, std=std)

    def convergence_history(self, histories, qx, qy, qz, max_lag=0, want=CONV_ALL):
        """td_history_convergence: ``convergence_models`` on the samples of the histories
        (chain.History) where they lie: one history is one chain (one without samples is skipped)."""
        hs, _ = _history_handles(histories, count=False)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        mean, std = np.empty(nq), np.empty(nq)
        w, out = self._convergence_want(nq, max_lag, want)
        check(lib().td_history_convergence(self.h, hs, len(hs), ptr(qx), ptr(qy), ptr(qz), nq, ptr(mean),
                                           ptr(std), ctypes.byref(w)), self.h)
        return dict(out, mean=mean, std=std)

    VOL_AUTO, VOL_GRID, VOL_BRUTE = 0, 1, 2

    def set_volume_slab_nodes(self, n):
        """The nodes ``volume`` sweeps per slab (0: auto, what 1 GiB of values holds).  Same answer."""
        check(lib().tdt_set_volume_slab_nodes(self.h, int(n)), self.h)

    def set_volume_method(self, method):
        """How ``volume`` sweeps a slab: VOL_AUTO (bucket grids unless the models are small), VOL_GRID,
        VOL_BRUTE (``rasterize``'s kernel).  Same answer."""
        check(lib().tdt_set_volume_method(self.h, int(method)), self.h)

    def set_volume_counting(self, on):
        """Run the instance of the search kernel that counts its paths (``volume_counters``); off by
        default: its atomics cost more than the search.  Same answer."""
        check(lib().tdt_set_volume_counting(self.h, int(bool(on))), self.h)

    def volume_counters(self):
        """The (model, node) pairs of the last ``volume`` call decided by the 3x3x3 block, the 5x5x5 block,
        a full scan of the model (-1 each unless ``set_volume_counting(True)``), and the brute-force kernel."""
        out = np.zeros(4, dtype=np.int64)
        check(lib().tdt_volume_counters(self.h, ptr(out, _lib._pi64)), self.h)
        return tuple(int(v) for v in out)

    @staticmethod
    def volume_plan(nmodels, nq, budget=0, forced=0):
        """(nodes per slab, slabs) of a ``volume`` call (budget in bytes, 0: 1 GiB); needs no GPU."""
        out = np.zeros(2, dtype=np.int64)
        check(lib().tdt_volume_plan(int(nmodels), int(nq), int(budget), int(forced), ptr(out, _lib._pi64)))
        return int(out[0]), int(out[1])

    def _volume(self, call, nmodels, qx, qy, qz, probs, bins, conv, max_lag, want_values):
        """The td_volume request around ``call(byref(vol))`` -> dict of the outputs asked for."""
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        if not (len(qy) == len(qz) == nq):
            raise ValueError("qx, qy and qz must have the same length")
        mean, std = np.empty(nq), np.empty(nq)
        vals = np.empty((nmodels, nq)) if want_values else None
        out = dict(mean=mean, std=std, values=vals, quantiles=None, hist=None)
        marg, cw, entries, held = self._stat_wants(nq, probs, bins, conv, max_lag)
        out.update(entries)
        vol = _lib.TdVolume(ptr(qx), ptr(qy), ptr(qz), nq, ptr(mean), ptr(std), ptr(vals), marg, cw)
        call(ctypes.byref(vol))
        del held
        return out

    def volume(self, models, qx, qy, qz, probs=(), bins=None, chain_len=None, max_lag=0, want_values=False):
        """td_rasterize_volume: ``rasterize`` / ``marginals`` / ``convergence_models`` in one call at ANY
        number of nodes (a whole lattice, x fastest): one search structure for all models, the nodes swept
        slab by slab.  -> dict(mean[nq], std[nq], values[nmodels, nq] or None, quantiles[nprob, nq] or
        None, hist[nq, nbins + 3] or None and, with ``chain_len`` (the rows of each chain), rhat, ess,
        lags [nq]); every number is the section calls', bit for bit.  models as for ``rasterize``."""
        off, cat = _pack_models(models, empty_ok=False)
        lens = _chain_lens(chain_len)

        def call(vol):
            check(lib().td_rasterize_volume(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat),
                                            len(lens) if lens is not None else 0, ptr(lens, _lib._pi64), vol), self.h)

        return self._volume(call, len(models), qx, qy, qz, probs, bins, lens is not None, max_lag, want_values)

    def volume_history(self, histories, qx, qy, qz, probs=(), bins=None, convergence=False, max_lag=0,
                       want_values=False):
        """td_history_volume: ``volume`` on the samples of the histories (chain.History) where they lie;
        with ``convergence`` one history is one chain (one without samples is skipped)."""
        hs, nm = _history_handles(histories)

        def call(vol):
            check(lib().td_history_volume(self.h, hs, len(hs), vol), self.h)

        return self._volume(call, nm, qx, qy, qz, probs, bins, convergence, max_lag, want_values)

    def set_predict_plan(self, slab_points=0, model_chunk=0):
        """The ray points ``predict`` sweeps per slab and the models per sweep (0: auto).  Same answer."""
        check(lib().tdt_set_predict_plan(self.h, int(slab_points), int(model_chunk)), self.h)

    def set_predict_placement(self, xcd):
        """Run the ray-sum workgroups of model m on XCD m % 8 (default: off).  Same answer."""
        check(lib().tdt_set_predict_placement(self.h, int(bool(xcd))), self.h)

    @staticmethod
    def predict_plan(nmodels, ray_points, budget=0, forced_points=0, forced_chunk=0):
        """(points per slab, models per sweep, the slabs' ray edges [slabs + 1]) of a ``predict`` call on
        rays of ``ray_points`` points each (budget in bytes, 0: 1 GiB); needs no GPU."""
        rp = np.ascontiguousarray(ray_points, dtype=np.int64).ravel()
        out = np.zeros(3, dtype=np.int64)
        edges = np.zeros(len(rp) + 1, dtype=np.int64)
        check(lib().tdt_predict_plan(int(nmodels), len(rp), ptr(rp, _lib._pi64), int(budget), int(forced_points),
                                     int(forced_chunk), ptr(out, _lib._pi64), ptr(edges, _lib._pi64)))
        return int(out[0]), int(out[1]), [int(e) for e in edges[:int(out[2]) + 1]]

    def _predict(self, call, nmodels, probs, bins, conv, max_lag, want_values):
        """The td_predict request around ``call(byref(out))`` -> dict of the outputs."""
        n = self.n
        res = dict(phi=np.empty(nmodels), mean=np.empty(n), std=np.empty(n), quantiles=None, hist=None,
                   ptS=np.empty((nmodels, n)) if want_values else None)
        marg, cw, entries, held = self._stat_wants(n, probs, bins, conv, max_lag)
        res.update(entries)
        req = _lib.TdPredict(ptr(res["ptS"]), ptr(res["phi"]), ptr(res["mean"]), ptr(res["std"]), marg, cw)
        call(ctypes.byref(req))
        del held
        return res

    def predict(self, models, probs=(), bins=None, chain_len=None, max_lag=0, want_values=False):
        """td_rasterize_predict: every model's predicted t* on THIS context's rays (which need not be the
        rays the models were fitted to) in one sweep.  -> dict(phi[nmodels], the models' chi^2 against this
        context's tS / allSig; mean[n], std[n] over the models per ray; quantiles[nprob, n] or None;
        hist[n, nbins + 3] or None; with ``chain_len`` (the rows of each chain) rhat, ess, lags [n];
        ptS[nmodels, n] or None).  Row k of ptS and phi[k] are ``evaluate`` of model k, bit for bit; the
        statistics are ``rasterize`` / ``marginals`` / ``convergence`` of the matrix ptS.  models as for
        ``rasterize``."""
        off, cat = _pack_models(models)
        lens = _chain_lens(chain_len)

        def call(req):
            check(lib().td_rasterize_predict(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat),
                                             len(lens) if lens is not None else 0, ptr(lens, _lib._pi64), req), self.h)

        return self._predict(call, len(models), probs, bins, lens is not None, max_lag, want_values)

    def predict_history(self, histories, probs=(), bins=None, convergence=False, max_lag=0, want_values=False):
        """td_history_predict: ``predict`` on the samples of the histories (chain.History) where they lie;
        the histories may have been recorded on another context of this device.  With ``convergence`` one
        history is one chain (one without samples is skipped)."""
        hs, nm = _history_handles(histories)

        def call(req):
            check(lib().td_history_predict(self.h, hs, len(hs), req), self.h)

        return self._predict(call, nm, probs, bins, convergence, max_lag, want_values)

    @staticmethod
    def covariance_group():
        """G: the targets ``covariance`` keeps in registers at a time (a slab of the value matrix is read once
        per G targets); needs no GPU."""
        return int(lib().tdt_covariance_group())

    def _covariance(self, call, nmodels, qx, qy, qz, targets, series, want):
        """The td_covariance request around ``call(byref(req))`` -> dict of the outputs."""
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        if not (len(qy) == len(qz) == nq):
            raise ValueError("qx, qy and qz must have the same length")
        tg = f64(np.reshape(targets, (-1, 3)).T) if targets is not None else np.zeros((3, 0))  # [3][nt]
        nt = tg.shape[1]
        ser = None
        if series is not None:
            ser = f64(series)
            if ser.ndim == 1:
                ser = ser.reshape(-1, 1)
            if ser.ndim != 2 or ser.shape[0] != nmodels:
                raise ValueError("series must be [nmodels = %d][nseries], row = model; got %s" % (nmodels, ser.shape))
            if ser.shape[1] == 0:
                ser = None
        nser = ser.shape[1] if ser is not None else 0
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= {"cov", "corr"}:
            raise ValueError("want: 'cov' and / or 'corr'")
        T = nt + nser
        res = dict(cov=np.empty((T, nq)) if "cov" in want else None, corr=np.empty((T, nq)) if "corr" in want else None,
                   mean=np.empty(nq), std=np.empty(nq), target_mean=np.empty(T), target_std=np.empty(T))
        req = _lib.TdCovariance(ptr(qx), ptr(qy), ptr(qz), nq, ptr(tg[0]) if nt else None, ptr(tg[1]) if nt else None,
                                ptr(tg[2]) if nt else None, nt, ptr(ser), nser, ptr(res["cov"]), ptr(res["corr"]),
                                ptr(res["mean"]), ptr(res["std"]), ptr(res["target_mean"]), ptr(res["target_std"]))
        call(ctypes.byref(req))
        return res

    def covariance(self, models, qx, qy, qz, targets=None, series=None, want=("cov", "corr")):
        """td_rasterize_covariance: the covariance and the correlation, over the models, between zeta at each
        target and zeta at every node -- the ensemble's point-spread function.  ``targets``: points [nt, 3]
        (x, y, z), whose series is the nearest-cell value there; ``series``: [nmodels, nseries] (row = model),
        any per-model numbers (a ray's predicted t* out of ``predict``, the phi trace, ...).  -> dict(cov[T, nq],
        corr[T, nq] (each None unless in ``want``), mean[nq], std[nq] (``volume``'s), target_mean[T],
        target_std[T]); rows: the points, then the series.  cov = sum((v - mean)(a - target_mean)) / (M - 1) in
        ``rasterize``'s association without FMA, corr = cov / (std * target_std), unclamped.  Any number of
        nodes, swept slab by slab as by ``volume``.  models as for ``rasterize``."""
        off, cat = _pack_models(models)

        def call(req):
            check(lib().td_rasterize_covariance(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), req),
                  self.h)

        return self._covariance(call, len(models), qx, qy, qz, targets, series, want)

    def covariance_history(self, histories, qx, qy, qz, targets=None, series=None, want=("cov", "corr")):
        """td_history_covariance: ``covariance`` on the samples of the histories (chain.History) where they
        lie, history by history (one without samples is skipped); they may have been recorded on another
        context of this device."""
        hs, nm = _history_handles(histories)

        def call(req):
            check(lib().td_history_covariance(self.h, hs, len(hs), req), self.h)

        return self._covariance(call, nm, qx, qy, qz, targets, series, want)

    IFACE_ALL = ("count", "any", "exceed", "jump", "stats", "density")

    @staticmethod
    def interfaces_plan(nmodels, nx, ny, nz, budget=0, forced=0):
        """(the nodes a slab owns, slabs, the most columns of a slab's value matrix) of an ``interfaces`` call
        on an nx x ny x nz lattice (budget in bytes, 0: 1 GiB); needs no GPU."""
        out = np.zeros(3, dtype=np.int64)
        check(lib().tdt_interfaces_plan(int(nmodels), int(nx), int(ny), int(nz), int(budget), int(forced),
                                        ptr(out, _lib._pi64)))
        return int(out[0]), int(out[1]), int(out[2])

    def _interfaces(self, call, xs, ys, zs, thresholds, want):
        """The td_interfaces request around ``call(byref(req))`` -> dict of the flat outputs."""
        xs, ys, zs = (f64(np.ravel(a)) for a in (xs, ys, zs))
        thr = f64(np.ravel(thresholds))
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= set(self.IFACE_ALL):
            raise ValueError("want: a subset of %s" % (self.IFACE_ALL,))
        nx, ny, nz, nthr = len(xs), len(ys), len(zs), len(thr)
        nq = nx * ny * nz
        res = dict(count=np.empty((3, nq), dtype=np.int64) if "count" in want else None,
                   any=np.empty(nq, dtype=np.int64) if "any" in want else None,
                   exceed=np.empty((nthr, 3, nq), dtype=np.int64) if "exceed" in want and nthr else None,
                   jump=np.empty((3, nq)) if "jump" in want else None,
                   mean=np.empty(nq) if "stats" in want else None, std=np.empty(nq) if "stats" in want else None,
                   density=np.empty(nq, dtype=np.int64) if "density" in want else None, skipped=None)
        skipped = np.zeros(1, dtype=np.int64) if "density" in want else None
        send_thr = res["exceed"] is not None
        i64 = _lib._pi64
        req = _lib.TdInterfaces(ptr(xs), ptr(ys), ptr(zs), nx, ny, nz, ptr(thr) if send_thr else None,
                                nthr if send_thr else 0, ptr(res["count"], i64), ptr(res["any"], i64),
                                ptr(res["exceed"], i64), ptr(res["jump"]), ptr(res["mean"]), ptr(res["std"]),
                                ptr(res["density"], i64), ptr(skipped, i64))
        call(ctypes.byref(req))
        if skipped is not None:
            res["skipped"] = int(skipped[0])
        return res

    def interfaces(self, models, xs, ys, zs, thresholds=(), want=IFACE_ALL):
        """td_rasterize_interfaces: where the models put their Voronoi boundaries on the lattice ``xs`` x ``ys``
        x ``zs`` (node n = i + nx (j + ny k), x fastest), how large the jump across them is, and where the cells
        lie.  With d = V[m][n + s_a] - V[m][n] on the forward face of node n along axis a (x, y, z) -> dict of
        flat arrays: count[3, nq] the models whose value differs across the face, any[nq] the models that differ
        across at least one of the node's faces, exceed[nthr, 3, nq] the models with abs(d) > thresholds[t], jump[3,
        nq] the mean of abs(d) over the models in ``rasterize``'s association (-1 / NaN where there is no face),
        mean[nq], std[nq] (``volume``'s), density[nq] the cells of all models whose nucleus lies in the node's voxel
        (bounded by the midpoints between nodes, the edge voxels open outwards) and skipped, the cells with a NaN
        coordinate.  ``want``: the subset of IFACE_ALL to compute ("stats": mean and std); what is not asked
        for, and exceed without thresholds, is None.  Any number of nodes, swept slab by slab as by ``volume``
        with the halo of the forward neighbours.  models as for ``rasterize``."""
        off, cat = _pack_models(models)

        def call(req):
            check(lib().td_rasterize_interfaces(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), req),
                  self.h)

        return self._interfaces(call, xs, ys, zs, thresholds, want)

    def interfaces_history(self, histories, xs, ys, zs, thresholds=(), want=IFACE_ALL):
        """td_history_interfaces: ``interfaces`` on the samples of the histories (chain.History) where they lie,
        history by history (one without samples is skipped); they may have been recorded on another context of
        this device."""
        hs, _ = _history_handles(histories, count=False)

        def call(req):
            check(lib().td_history_interfaces(self.h, hs, len(hs), req), self.h)

        return self._interfaces(call, xs, ys, zs, thresholds, want)

    RES_SUMMARY = ("footprint", "run", "extent", "censored", "stats")
    RES_ALL = ("cov", "corr") + RES_SUMMARY

    @staticmethod
    def resolution_plan(nmodels, nq, reach, budget=0, forced=0):
        """(ns: the nodes of a block, R: the resident blocks, the blocks) of a ``resolution`` call on ``nq`` nodes
        whose largest flat offset is ``reach`` (budget in bytes of the resident blocks, 0: 2 GiB); needs no GPU."""
        out = np.zeros(3, dtype=np.int64)
        check(lib().tdt_resolution_plan(int(nmodels), int(nq), int(reach), int(budget), int(forced), ptr(out, _lib._pi64)))
        return int(out[0]), int(out[1]), int(out[2])

    RES_FORM_KEPT, RES_FORM_PLAIN, RES_FORM_XRUNS = 0, 1, 2

    def set_resolution(self, budget=0, form=RES_FORM_KEPT):
        """``resolution``'s budget in bytes of the resident blocks (0: 2 GiB) and the form of its pair kernel
        (RES_FORM_PLAIN: one partner load per offset; RES_FORM_XRUNS: a run of offsets that differ in di alone is
        served from one staged segment; RES_FORM_KEPT: runs of two offsets and more as x-runs, the lone ones plain).  Same
        answer."""
        check(lib().tdt_set_resolution(self.h, int(budget), int(form)), self.h)

    def _resolution(self, call, xs, ys, zs, offsets, threshold, weights, want):
        """The td_resolution request around ``call(byref(req))`` -> dict of the flat outputs."""
        xs, ys, zs = (f64(np.ravel(a)) for a in (xs, ys, zs))
        off = np.ascontiguousarray(np.reshape(offsets, (-1, 3)), dtype=np.int32)
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= set(self.RES_ALL):
            raise ValueError("want: a subset of %s" % (self.RES_ALL,))
        nx, ny, nz, noff = len(xs), len(ys), len(zs), len(off)
        nq = nx * ny * nz
        wts = None
        if weights is not None:
            wts = f64(np.ravel(weights))
            if len(wts) != nq:
                raise ValueError("weights must hold nx ny nz = %d numbers, x fastest; got %d" % (nq, len(wts)))
        res = dict(cov=np.empty((noff, nq)) if "cov" in want else None, corr=np.empty((noff, nq)) if "corr" in want else None,
                   footprint=np.empty(nq) if "footprint" in want else None,
                   run=np.empty((3, 2, nq), dtype=np.int32) if "run" in want else None,
                   extent=np.empty((3, nq)) if "extent" in want else None,
                   censored=np.empty(nq, dtype=np.int32) if "censored" in want else None,
                   mean=np.empty(nq) if "stats" in want else None, std=np.empty(nq) if "stats" in want else None)
        i32 = _lib._pi32
        req = _lib.TdResolution(ptr(xs), ptr(ys), ptr(zs), nx, ny, nz, ptr(off, i32) if noff else None, noff, float(threshold),
                                ptr(wts), ptr(res["cov"]), ptr(res["corr"]), ptr(res["footprint"]), ptr(res["run"], i32),
                                ptr(res["extent"]), ptr(res["censored"], i32), ptr(res["mean"]), ptr(res["std"]))
        call(ctypes.byref(req))
        return res

    def resolution(self, models, xs, ys, zs, offsets, threshold=0.5, weights=None, want=RES_SUMMARY):
        """td_rasterize_resolution: for every node n of the lattice ``xs`` x ``ys`` x ``zs`` (n = i + nx (j + ny k), x
        fastest) the correlation, over the models, of zeta there with zeta at each neighbour n + f(o) of the window
        ``offsets`` [noff, 3] = forward (di, dj, dk) (``posterior.resolution_offsets``), and what it reduces to ->
        dict of flat arrays: cov[noff, nq], corr[noff, nq] (NaN where the pair leaves the lattice; ``covariance``'s
        numbers for a point target at n, bit for bit), footprint[nq] the sum of ``weights`` [nq] (None: 1.0 each) over
        the node and the neighbours, forwards and backwards, tied to it at corr >= ``threshold``, run[3, 2, nq]
        (int32) the contiguous steps along +a / -a that pass, extent[3, nq] the distance between the ends of the two
        runs, censored[nq] (int32; bit 2a / 2a + 1: the run along +a / -a ended on the lattice's or the window's edge
        and not on a failing correlation), mean[nq], std[nq] (``volume``'s).  ``want``: the subset of RES_ALL to
        compute ("stats": mean and std); what is not asked for is None.  Every node is swept once, in a ring of
        blocks (``resolution_plan``).  models as for ``rasterize``."""
        off, cat = _pack_models(models)

        def call(req):
            check(lib().td_rasterize_resolution(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), req),
                  self.h)

        return self._resolution(call, xs, ys, zs, offsets, threshold, weights, want)

    def resolution_history(self, histories, xs, ys, zs, offsets, threshold=0.5, weights=None, want=RES_SUMMARY):
        """td_history_resolution: ``resolution`` on the samples of the histories (chain.History) where they lie,
        history by history (one without samples is skipped); they may have been recorded on another context of
        this device."""
        hs, _ = _history_handles(histories, count=False)

        def call(req):
            check(lib().td_history_resolution(self.h, hs, len(hs), req), self.h)

        return self._resolution(call, xs, ys, zs, offsets, threshold, weights, want)

    @staticmethod
    def regions_plan(nmodels, npoints, budget=0, forced=0):
        """(the points a slab sweeps, slabs) of a ``regions`` call on ``npoints`` points (budget in bytes, 0:
        1 GiB): ``volume_plan``'s numbers with the point list in the place of the nodes; needs no GPU."""
        out = np.zeros(2, dtype=np.int64)
        check(lib().tdt_regions_plan(int(nmodels), int(npoints), int(budget), int(forced), ptr(out, _lib._pi64)))
        return int(out[0]), int(out[1])

    def _regions(self, call, nmodels, px, py, pz, reg_off, w, normalize, probs, bins, conv, max_lag, greater):
        """The td_regions request around ``call(byref(req))`` -> dict of the outputs."""
        px, py, pz = (f64(np.ravel(a)) for a in (px, py, pz))
        npts = len(px)
        if not (len(py) == len(pz) == npts):
            raise ValueError("px, py and pz must have the same length")
        wv = f64(np.ravel(w)) if w is not None else None
        if wv is not None and len(wv) != npts:
            raise ValueError("w must have one weight per point")
        off = np.ascontiguousarray(reg_off, dtype=np.int64).ravel()
        R = len(off) - 1
        if R < 1:
            raise ValueError("reg_off must hold nreg + 1 >= 2 offsets")
        res = dict(series=np.empty((nmodels, R)), weight=np.empty(R), mean=np.empty(R), std=np.empty(R),
                   greater=np.empty((R, R), dtype=np.int64) if greater else None, quantiles=None, hist=None)
        marg, cw, entries, held = self._stat_wants(R, probs, bins, conv, max_lag)
        res.update(entries)
        req = _lib.TdRegions(ptr(px), ptr(py), ptr(pz), ptr(wv), npts, ptr(off, _lib._pi64), R, int(bool(normalize)),
                             ptr(res["series"]), ptr(res["weight"]), ptr(res["mean"]), ptr(res["std"]),
                             ptr(res["greater"], _lib._pi64), marg, cw)
        call(ctypes.byref(req))
        del held
        return res

    def regions(self, models, px, py, pz, reg_off, w=None, normalize=True, probs=(), bins=None, chain_len=None,
                max_lag=0, greater=True):
        """td_rasterize_regions: one number per model and region.  Region r is the points ``reg_off[r] ..
        reg_off[r + 1] - 1`` of ``px``, ``py``, ``pz`` with the weights ``w`` (None: 1.0; a point may be listed in
        several regions, a weight may be negative).  With V[m][p] the nearest-cell value of model m at point p
        (``volume``'s) -> dict(series[nmodels, R] = the sum over the region of w[p] * V[m][p] in ``rasterize``'s
        association over the index within the region, divided by weight[R] (the sum of w in the same association)
        when ``normalize``; mean[R], std[R] over the models; greater[R, R] = the models with series[m, a] >
        series[m, b] (None unless ``greater``); quantiles[nprob, R] or None; hist[R, nbins + 3] or None; with ``chain_len`` (the rows of
        each chain) rhat, ess, lags [R]) -- the statistics are ``volume``'s with the regions in the place of the
        nodes.  Any number of points, swept slab by slab as by ``volume``.  models as for ``rasterize``."""
        off, cat = _pack_models(models)
        lens = _chain_lens(chain_len)

        def call(req):
            check(lib().td_rasterize_regions(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat),
                                             len(lens) if lens is not None else 0, ptr(lens, _lib._pi64), req), self.h)

        return self._regions(call, len(models), px, py, pz, reg_off, w, normalize, probs, bins, lens is not None, max_lag,
                             greater)

    def regions_history(self, histories, px, py, pz, reg_off, w=None, normalize=True, probs=(), bins=None,
                        convergence=False, max_lag=0, greater=True):
        """td_history_regions: ``regions`` on the samples of the histories (chain.History) where they lie, history
        by history (one without samples is skipped); they may have been recorded on another context of this
        device.  With ``convergence`` one history is one chain."""
        hs, nm = _history_handles(histories)

        def call(req):
            check(lib().td_history_regions(self.h, hs, len(hs), req), self.h)

        return self._regions(call, nm, px, py, pz, reg_off, w, normalize, probs, bins, convergence, max_lag, greater)

    GRAM_MAX_MODELS = 11585  # 8 M^2 bytes of a matrix within 1 GiB (include/tdstar_gram.h)

    @staticmethod
    def gram_plan(nmodels, npoints, budget=0, forced=0):
        """(the points a slab sweeps, slabs) of a ``gram`` call on ``npoints`` points (budget in bytes, 0: 1 GiB):
        ``volume_plan``'s numbers with the point list in the place of the nodes; needs no GPU."""
        out = np.zeros(2, dtype=np.int64)
        check(lib().tdt_gram_plan(int(nmodels), int(npoints), int(budget), int(forced), ptr(out, _lib._pi64)))
        return int(out[0]), int(out[1])

    @staticmethod
    def set_gram_form(form=0):
        """Testing hook, process-wide: the pair kernel's register tile (0: the kept one, 1: 4 x 4 pairs a lane, 2:
        8 x 8); no answer depends on it."""
        check(lib().tdt_set_gram_form(int(form)))

    @staticmethod
    def gram_tile(form=0):
        """The rows of the tile of the lower triangle a workgroup of the pair kernel owns under ``form``; needs no GPU."""
        return int(lib().tdt_gram_tile(int(form)))

    def _gram(self, call, nmodels, px, py, pz, w, want):
        """The td_gram request around ``call(byref(req))`` -> dict of the outputs."""
        px, py, pz = (f64(np.ravel(a)) for a in (px, py, pz))
        npts = len(px)
        if not (len(py) == len(pz) == npts):
            raise ValueError("px, py and pz must have the same length")
        wv = f64(np.ravel(w)) if w is not None else None
        if wv is not None and len(wv) != npts:
            raise ValueError("w must have one weight per point")
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= {"gram", "dist2"}:
            raise ValueError("want: 'gram' and / or 'dist2'")
        res = dict(gram=np.empty((nmodels, nmodels)) if "gram" in want else None,
                   dist2=np.empty((nmodels, nmodels)) if "dist2" in want else None, mean=np.empty(npts), std=np.empty(npts),
                   wsum=np.empty(1))
        req = _lib.TdGram(ptr(px), ptr(py), ptr(pz), ptr(wv), npts, ptr(res["gram"]), ptr(res["dist2"]), ptr(res["mean"]),
                          ptr(res["std"]), ptr(res["wsum"]))
        call(ctypes.byref(req))
        res["wsum"] = float(res["wsum"][0])
        return res

    def gram(self, models, px, py, pz, w=None, want=("gram", "dist2")):
        """td_rasterize_gram: the M x M matrices of inner products and of squared distances between the models'
        volumes on the points ``px``, ``py``, ``pz`` with the weights ``w`` >= 0 (None: 1.0).  With V[m][p] the
        nearest-cell value of model m at point p (``volume``'s), mean[p] its mean over the models and X[m][p] =
        sqrt(w[p]) * (V[m][p] - mean[p]) -> dict(gram[M, M] = sum_p X[a][p] X[b][p], dist2[M, M] = sum_p (X[a][p] -
        X[b][p])^2 (each None unless in ``want``), mean[np], std[np] (``volume``'s), wsum = sum(w)).  Both sums run over
        the points in order in blocks of 64 without FMA (include/tdstar_gram.h): the matrices are symmetric bit for bit
        and depend on neither the slabs nor the kernel's tiling.  Any number of points, swept slab by slab as by
        ``volume``; at most 11585 models (1 GiB a matrix).  models as for ``rasterize``."""
        off, cat = _pack_models(models)

        def call(req):
            check(lib().td_rasterize_gram(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat), req), self.h)

        return self._gram(call, len(models), px, py, pz, w, want)

    def gram_history(self, histories, px, py, pz, w=None, want=("gram", "dist2")):
        """td_history_gram: ``gram`` on the samples of the histories (chain.History) where they lie, history by
        history (one without samples is skipped); they may have been recorded on another context of this device."""
        hs, nm = _history_handles(histories)

        def call(req):
            check(lib().td_history_gram(self.h, hs, len(hs), req), self.h)

        return self._gram(call, nm, px, py, pz, w, want)

    def _recovery(self, call, nmodels, px, py, pz, truth, reg_off, w, normalize, probs, bins, conv, max_lag):
        """The td_recovery request around ``call(byref(req))`` -> dict of the outputs."""
        px, py, pz, tr = (f64(np.ravel(a)) for a in (px, py, pz, truth))
        npts = len(px)
        if not (len(py) == len(pz) == len(tr) == npts):
            raise ValueError("px, py, pz and truth must have the same length")
        wv = f64(np.ravel(w)) if w is not None else None
        if wv is not None and len(wv) != npts:
            raise ValueError("w must have one weight per point")
        off = (np.ascontiguousarray(reg_off, dtype=np.int64).ravel() if reg_off is not None
               else np.array([0, npts], dtype=np.int64))
        R = len(off) - 1
        if R < 1:
            raise ValueError("reg_off must hold nreg + 1 >= 2 offsets")
        res = dict(below=np.empty(npts, dtype=np.int64), equal=np.empty(npts, dtype=np.int64),
                   above=np.empty(npts, dtype=np.int64), dmean=np.empty(npts), dstd=np.empty(npts),
                   series=np.empty((nmodels, R)), weight=np.empty(R), mean=np.empty(R), std=np.empty(R), quantiles=None,
                   hist=None)
        marg, cw, entries, held = self._stat_wants(R, probs, bins, conv, max_lag)
        res.update(entries)
        i64 = _lib._pi64
        req = _lib.TdRecovery(ptr(px), ptr(py), ptr(pz), ptr(wv), npts, ptr(off, i64), R, ptr(tr), int(bool(normalize)),
                              ptr(res["below"], i64), ptr(res["equal"], i64), ptr(res["above"], i64), ptr(res["dmean"]),
                              ptr(res["dstd"]), ptr(res["series"]), ptr(res["weight"]), ptr(res["mean"]), ptr(res["std"]),
                              marg, cw)
        call(ctypes.byref(req))
        del held
        return res

    def recovery(self, models, px, py, pz, truth, reg_off=None, w=None, normalize=True, probs=(), bins=None,
                 chain_len=None, max_lag=0):
        """td_rasterize_recovery: the models against a known model whose value at point p is ``truth[p]``.  The
        points, the regions (``reg_off=None``: all points are one region) and the weights are ``regions``'.  With
        V[m][p] the nearest-cell value of model m at point p (``volume``'s) and D = V - truth -> dict(below[np],
        equal[np], above[np] = the models with V <, ==, > truth (a NaN V counts in none); dmean[np], dstd[np] the
        mean and sigma of D over the models (``rasterize``'s); series[nmodels, R] = the sum over the region of w[p]
        * (D * D) in ``rasterize``'s association over the index within the region, divided by weight[R] when
        ``normalize``: the weighted mean square distance of every model to the truth; mean[R], std[R], quantiles
        [nprob, R] or None, hist[R, nbins + 3] or None and, with ``chain_len``, rhat, ess, lags [R] of the series, as
        ``regions`` gives them).  Any number of points, swept slab by slab as by ``volume``.  models as for
        ``rasterize``."""
        off, cat = _pack_models(models)
        lens = _chain_lens(chain_len)

        def call(req):
            check(lib().td_rasterize_recovery(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat),
                                              len(lens) if lens is not None else 0, ptr(lens, _lib._pi64), req), self.h)

        return self._recovery(call, len(models), px, py, pz, truth, reg_off, w, normalize, probs, bins, lens is not None,
                              max_lag)

    def recovery_history(self, histories, px, py, pz, truth, reg_off=None, w=None, normalize=True, probs=(), bins=None,
                         convergence=False, max_lag=0):
        """td_history_recovery: ``recovery`` on the samples of the histories (chain.History) where they lie, history
        by history (one without samples is skipped); they may have been recorded on another context of this
        device.  With ``convergence`` one history is one chain."""
        hs, nm = _history_handles(histories)

        def call(req):
            check(lib().td_history_recovery(self.h, hs, len(hs), req), self.h)

        return self._recovery(call, nm, px, py, pz, truth, reg_off, w, normalize, probs, bins, convergence, max_lag)

    CMP_COUNTS, CMP_KS, CMP_STATS = "counts", "ks", "stats"
    CMP_ALL = (CMP_COUNTS, CMP_KS, CMP_STATS)

    def _compare(self, call, ncol, qx, qy, qz, exceed, probs, bins, want):
        """The td_compare request around ``call(byref(req))`` -> dict of the outputs."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if not set(want) <= set(self.CMP_ALL):
            raise ValueError("want: a subset of %s" % (self.CMP_ALL,))
        pairs = f64(np.reshape(np.asarray(exceed, dtype=np.float64), (-1, 2)))
        scale, shift = f64(pairs[:, 0]), f64(pairs[:, 1])
        ne = len(scale)
        i64 = _lib._pi64
        counts, ks, stats = (k in want for k in self.CMP_ALL)
        cnt = lambda on: np.zeros(ncol, dtype=np.int64) if on else None  # noqa: E731
        res = dict(less=cnt(counts), equal=cnt(counts), greater=cnt(counts),
                   exceed=np.zeros((ne, ncol), dtype=np.int64) if ne else None, ks_plus=cnt(ks), ks_minus=cnt(ks),
                   ks_at=np.full(ncol, np.nan) if ks else None)
        for side in "ab":
            res["mean_" + side], res["std_" + side] = (np.empty(ncol), np.empty(ncol)) if stats else (None, None)
        held, marg = [], {}
        for side in "ab":
            m, mw, entries, keep = self._stat_wants(ncol, probs, bins, False, 0)
            held.append(keep)
            marg[side] = m
            res["quantiles_" + side], res["hist_" + side] = entries["quantiles"], entries["hist"]
        req = _lib.TdCompare(ptr(qx), ptr(qy), ptr(qz), ncol if qx is not None else 0, ne, ptr(scale) if ne else None,
                             ptr(shift) if ne else None, ptr(res["less"], i64), ptr(res["equal"], i64), ptr(res["greater"], i64),
                             ptr(res["exceed"], i64), ptr(res["ks_plus"], i64), ptr(res["ks_minus"], i64), ptr(res["ks_at"]),
                             ptr(res["mean_a"]), ptr(res["std_a"]), ptr(res["mean_b"]), ptr(res["std_b"]), marg["a"], marg["b"])
        call(ctypes.byref(req))
        del held
        return res

    def compare(self, models_a, models_b, qx, qy, qz, exceed=(), probs=(), bins=None, want=CMP_ALL):
        """td_rasterize_compare: one ensemble against another.  With a_i, b_j the nearest-cell values (``volume``'s) of
        the models of side A and side B at a node -> dict, per node: less, equal, greater[nq] = the pairs (i, j) with
        a_i <, ==, > b_j (IEEE: a NaN counts in nothing, -0.0 == 0.0); exceed[nexceed, nq] = the pairs with a_i > s_k *
        b_j + t_k for ``exceed`` = [(s_k, t_k)], two rounded operations (None without pairs); ks_plus, ks_minus[nq] =
        max(0, max of +-T) with T(x) = #{a <= x} MB - #{b <= x} MA over the values x of both sides, and ks_at[nq] the
        smallest x at which abs(T) is largest (NaN where T is 0 throughout); mean_a, std_a, mean_b, std_b[nq],
        quantiles_a, quantiles_b[nprob, nq] or None and hist_a, hist_b[nq, nbins + 3] or None: ``volume``'s of each
        side alone, bit for bit.  All counts are int64 and exact.  ``want``: the subset of CMP_ALL to compute.  The two
        sides are swept as one ensemble, slab by slab as by ``volume``; at most 16384 models a side.  models as for
        ``rasterize``."""
        offa, cata = _pack_models(models_a)
        offb, catb = _pack_models(models_b)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        if not (len(qy) == len(qz) == len(qx)):
            raise ValueError("qx, qy and qz must have the same length")

        def call(req):
            check(lib().td_rasterize_compare(self.h, len(models_a), ptr(offa, _lib._pi64), *(ptr(c) for c in cata),
                                             len(models_b), ptr(offb, _lib._pi64), *(ptr(c) for c in catb), req), self.h)

        return self._compare(call, len(qx), qx, qy, qz, exceed, probs, bins, want)

    def compare_history(self, histories_a, histories_b, qx, qy, qz, exceed=(), probs=(), bins=None, want=CMP_ALL):
        """td_history_compare: ``compare`` on the samples of two lists of histories (chain.History) where they lie,
        history by history (one without samples is skipped); they may have been recorded on another context of this
        device."""
        ha, _ = _history_handles(histories_a, count=False)
        hb, _ = _history_handles(histories_b, count=False)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        if not (len(qy) == len(qz) == len(qx)):
            raise ValueError("qx, qy and qz must have the same length")

        def call(req):
            check(lib().td_history_compare(self.h, ha, len(ha), hb, len(hb), req), self.h)

        return self._compare(call, len(qx), qx, qy, qz, exceed, probs, bins, want)

    def compare_values(self, values_a, values_b, exceed=(), probs=(), bins=None, want=CMP_ALL):
        """td_compare_values: ``compare`` on the columns of two host matrices ``values_a`` [MA, ncol] and ``values_b``
        [MB, ncol] (or [MA], [MB]: one column) with no search: traces of phi or nCells, ``regions``' series, predicted
        t*.  Every output has ncol columns."""
        A, B = f64(values_a), f64(values_b)
        A = A.reshape(-1, 1) if A.ndim == 1 else A
        B = B.reshape(-1, 1) if B.ndim == 1 else B
        if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
            raise ValueError("values_a [MA, ncol] and values_b [MB, ncol] must have the same columns")

        def call(req):
            check(lib().td_compare_values(self.h, ptr(A), A.shape[0], ptr(B), B.shape[0], A.shape[1], req), self.h)

        return self._compare(call, A.shape[1], None, None, None, exceed, probs, bins, want)

    @staticmethod
    def set_compare_form(plain=False, sort_threads=0, count_threads=0):
        """The columns the workgroups of ``compare``'s sort kernel take -- eight neighbouring ones per XCD (default), or
        ``plain``: the column of the workgroup's index -- and the threads of a workgroup of its two kernels (a power of
        two 64 .. 1024; 0: by the larger side).  Same answer.  Process-wide."""
        check(lib().tdt_set_compare_form(int(bool(plain)), int(sort_threads), int(count_threads)))

    SUP_AUTO, SUP_LDS, SUP_GLOBAL = 0, 1, 2

    @staticmethod
    def support_lds_cells():
        """The most cells of a model whose sums ``support``'s scatter kernel keeps in LDS; needs no GPU."""
        return int(lib().tdt_support_lds_cells())

    def set_support_scatter(self, mode):
        """How ``support`` adds a model's ray points to its cells: SUP_AUTO, SUP_LDS (in LDS where the model's cells
        fit ``support_lds_cells()``), SUP_GLOBAL (atomics on the global arrays).  Same answer.  Set it back to
        SUP_AUTO before ``close``."""
        check(lib().tdt_set_support_scatter(self.h, int(mode)), self.h)

    def _support(self, call, nmodels, total, w, qx, qy, qz, thresholds, probs, bins, conv, max_lag, want_values,
                 want_cells):
        """The td_support request around ``call(byref(req))`` -> dict of the outputs."""
        wv = f64(np.ravel(w)) if w is not None else None
        if wv is not None and len(wv) != self.P:
            raise ValueError("w must have one weight per valid ray point (%d)" % self.P)
        if qx is None:
            qx = qy = qz = np.zeros(0)
        qx, qy, qz = (f64(np.ravel(a)) for a in (qx, qy, qz))
        nq = len(qx)
        if not (len(qy) == len(qz) == nq):
            raise ValueError("qx, qy and qz must have the same length")
        thr = f64(np.ravel(thresholds))
        if nq == 0 and (len(thr) or len(np.ravel(probs)) or bins is not None or conv or want_values):
            raise ValueError("thresholds, probs, bins, convergence and the values need nodes")
        res = dict(cell=np.empty(total) if want_cells else None,
                   count=np.empty(total, dtype=np.int64) if want_cells else None, barren=np.empty(nmodels, dtype=np.int64),
                   orphans=np.empty(nmodels, dtype=np.int64), mean=np.empty(nq) if nq else None,
                   std=np.empty(nq) if nq else None, values=np.empty((nmodels, nq)) if want_values else None,
                   exceed=np.empty((len(thr), nq), dtype=np.int64) if len(thr) else None, quantiles=None, hist=None)
        marg, cw, entries, held = self._stat_wants(nq, probs, bins, conv, max_lag)
        res.update(entries)
        req = _lib.TdSupport(ptr(wv), ptr(qx), ptr(qy), ptr(qz), nq, ptr(thr) if len(thr) else None, len(thr),
                             ptr(res["cell"]), ptr(res["count"], _lib._pi64), ptr(res["barren"], _lib._pi64),
                             ptr(res["orphans"], _lib._pi64), ptr(res["values"]), ptr(res["mean"]), ptr(res["std"]),
                             ptr(res["exceed"], _lib._pi64), marg, cw)
        call(ctypes.byref(req))
        del held
        return res

    def support(self, models, w=None, qx=None, qy=None, qz=None, thresholds=(), probs=(), bins=None, chain_len=None,
                max_lag=0, want_values=False, want_cells=True):
        """td_rasterize_support: which cells, and through them which nodes, this context's rays constrain.  With
        owner[m][p] the cell ``evaluate`` picks for ray point p (``want_nearest`` order) in model m and ``w`` one
        weight per point (None: 1.0; quantised once to exact integer multiples of a power of two, so every sum is
        independent of its order) -> dict(cell[total cells] = the sum of w over the points the cell owns,
        count[total cells] the points it owns, barren[nmodels] the cells that own none, orphans[nmodels] the points
        no cell owns; with nodes: mean[nq], std[nq] over the models of U[m][q] = cell[the cell ``rasterize`` picks
        for node q], values[nmodels, nq] = U or None, exceed[nthr, nq] = the models with U > thresholds[t] or None,
        quantiles[nprob, nq] or None, hist[nq, nbins + 3] or None, with ``chain_len`` rhat, ess, lags [nq]).
        ``want_cells=False`` leaves cell and count None (16 bytes per cell of every model stay on the device).
        models: list of (x, y, z[, zeta]) cell arrays; zeta is not read."""
        off, cat = _pack_models(models, ncomp=3)
        lens = _chain_lens(chain_len)

        def call(req):
            check(lib().td_rasterize_support(self.h, len(models), ptr(off, _lib._pi64), *(ptr(c) for c in cat),
                                             len(lens) if lens is not None else 0, ptr(lens, _lib._pi64), req), self.h)

        return self._support(call, len(models), int(off[-1]), w, qx, qy, qz, thresholds, probs, bins, lens is not None,
                             max_lag, want_values, want_cells)

    def support_history(self, histories, w=None, qx=None, qy=None, qz=None, thresholds=(), probs=(), bins=None,
                        convergence=False, max_lag=0, want_values=False, want_cells=True):
        """td_history_support: ``support`` on the samples of the histories (chain.History) where they lie, history
        by history (one without samples is skipped); they may have been recorded on another context of this
        device.  With ``convergence`` one history is one chain."""
        histories = list(histories)
        hs, _ = _history_handles(histories, count=False)
        counts = [h.count() for h in histories]  # (samples, cells used)
        nm, total = sum(c[0] for c in counts), sum(c[1] for c in counts)

        def call(req):
            check(lib().td_history_support(self.h, hs, len(hs), req), self.h)

        return self._support(call, nm, total, w, qx, qy, qz, thresholds, probs, bins, convergence, max_lag, want_values,
                             want_cells)

    def interpolate(self, cells, X, Y, Z, want_nearest=False):
        """-> (zeta[npoints], nearest[npoints] or None)"""
        xc, yc, zc, ze = (f64(c) for c in cells)
        X, Y, Z = (f64(np.atleast_1d(a)) for a in (X, Y, Z))
        out = np.empty(max(len(X), 1))
        near = np.empty(max(len(X), 1), dtype=np.int32) if want_nearest else None
        npo = ctypes.c_int64()
        check(lib().td_interpolate(self.h, ptr(xc), ptr(yc), ptr(zc), ptr(ze), len(xc), ptr(X), len(X), ptr(Y),
                                   len(Y), ptr(Z), len(Z), ptr(out),
                                   ptr(near, _lib._pi32) if near is not None else None, ctypes.byref(npo)), self.h)
        k = npo.value
        return out[:k].copy(), (near[:k].copy() if near is not None else None)


def context_for(dataStruct):
    """The (cached) device context of a DataStruct; geometry never changes
    during a chain (deepcopy(dataStruct) only duplicates values)."""
    if dataStruct._td_ctx is None:
        dataStruct._td_ctx = TdContext.from_datastruct(dataStruct)
    return dataStruct._td_ctx


def evaluate(model, dataStruct, TD_parameters):
    """MCsub.jl:123-185."""
    valid = 1
    model.phi = 1
    model.likelihood = 1
    if TD_parameters.debug_prior == 1:  # :134-136
        return model, dataStruct, valid
    if TD_parameters.interp_style != 1:
        raise NotImplementedError("interp_style=2 (IDW) is broken in the reference (MCsub.jl:332)")
    ctx = context_for(dataStruct)
    ptS, phi, lk, _ = ctx.evaluate(model.cells())
    model.phi = phi
    model.ptS = ptS
    model.tS = dataStruct.tS
    model.likelihood = lk
    return model, dataStruct, valid


def Interpolation(TD_parameters, model, X, Y, Z, dataStruct=None):  # noqa: N802 -- reference name
    """MCsub.jl:306-336 (interp_style 1).  The reference needs no DataStruct here;
    any context works (geometry is not used), so one is created on demand."""
    if TD_parameters.interp_style != 1:
        raise NotImplementedError("interp_style=2 (IDW) is broken in the reference (MCsub.jl:332)")
    ctx = context_for(dataStruct) if dataStruct is not None else _scratch_context()
    z, _ = ctx.interpolate(model.cells(), X, Y, Z)
    return z


def v_nearest(x, y, z, mx, my, mz, mv, dataStruct=None):
    """MCsub.jl:247-263 for one point (value of the first nearest cell, 0.0 if none < 1e9)."""
    ctx = context_for(dataStruct) if dataStruct is not None else _scratch_context()
    v, _ = ctx.interpolate((mx, my, mz, mv), [x], [y], [z])
    return float(v[0])


_scratch = None


def _scratch_context():
    """A context with no rays, for Interpolation calls that carry no DataStruct."""
    global _scratch
    if _scratch is None:
        e = np.zeros((1, 0))
        _scratch = TdContext(e, e, e, np.zeros((0, 0)), np.zeros((0, 0)), np.zeros(0), np.zeros(0))
    return _scratch
