"""The convergence diagnostics of include/tdstar.h ("Convergence diagnostics") restated in numpy: split
R-hat and Geyer's initial-monotone-sequence ESS per column.  Every sum is a Python loop over the summed
index, starting at 0.0, vectorised over the columns only, so the association is the stated one and the
device results can be compared bit for bit.  Slow; fine at test sizes."""
import math

import numpy as np


def plan(chain_len, max_lag=0):
    """-> dict(n, m, T, seq_start[m], tau_floor)"""
    lens = [int(v) for v in chain_len]
    n = min(lens) // 2
    m = 2 * len(lens)
    T = n - 1 if max_lag == 0 else min(n - 1, max_lag)
    seq, pos = [], 0
    for L in lens:
        seq += [pos + L - 2 * n, pos + L - n]
        pos += L
    return dict(n=n, m=m, T=T, seq_start=seq, tau_floor=1.0 / math.log10(float(m * n)))


def convergence(V, chain_len, max_lag=0):
    """-> dict(rhat[ncol], ess[ncol], lags[ncol] int32) of V[M, ncol]"""
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 1:
        V = V.reshape(-1, 1)
    p = plan(chain_len, max_lag)
    n, m, T = p["n"], p["m"], p["T"]
    ncol = V.shape[1]
    with np.errstate(all="ignore"):
        means, varis, devs = [], [], []
        for s0 in p["seq_start"]:
            x = V[s0:s0 + n]
            a = np.zeros(ncol)
            for i in range(n):
                a = a + x[i]
            mean = a / float(n)
            d = x - mean
            q = np.zeros(ncol)
            for i in range(n):
                q = q + d[i] * d[i]
            means.append(mean)
            varis.append(q / float(n - 1))
            devs.append(d)
        W = np.zeros(ncol)
        mu = np.zeros(ncol)
        for s in range(m):
            W = W + varis[s]
            mu = mu + means[s]
        W = W / float(m)
        mu = mu / float(m)
        Bn = np.zeros(ncol)
        for s in range(m):
            e = means[s] - mu
            Bn = Bn + e * e
        Bn = Bn / float(m - 1)
        vp = (float(n - 1) / float(n)) * W + Bn
        rhat = np.sqrt(vp / W)

        def rho(t):
            A = np.zeros(ncol)
            for s in range(m):
                d = devs[s]
                acc = np.zeros(ncol)
                for i in range(n - t):
                    acc = acc + d[i] * d[i + t]
                A = A + acc / float(n)
            A = A / float(m)
            return 1.0 - (W - A) / vp

        Pprev = 1.0 + rho(1)
        S = Pprev.copy()
        last = np.ones(ncol, dtype=np.int64)
        going = np.ones(ncol, dtype=bool)  # still inside the loop; at the end: capped
        k = 1
        while 2 * k + 1 <= T and going.any():
            P = rho(2 * k) + rho(2 * k + 1)
            going &= P > 0  # a NaN stops too
            P = np.where(P > Pprev, Pprev, P)
            S = np.where(going, S + P, S)
            Pprev = np.where(going, P, Pprev)
            last = np.where(going, 2 * k + 1, last)
            k += 1
        tau = -1.0 + 2.0 * S
        tau = np.where(tau < p["tau_floor"], p["tau_floor"], tau)  # a NaN tau stays NaN
        ess = float(m * n) / tau
        lags = np.where(going, -last, last).astype(np.int32)
    return dict(rhat=rhat, ess=ess, lags=lags)


def ar1(rng, phi, nrows, ncol):
    """A stationary AR(1) column set, unit innovation variance."""
    x = np.empty((nrows, ncol))
    x[0] = rng.standard_normal(ncol) / math.sqrt(1.0 - phi * phi)
    for i in range(1, nrows):
        x[i] = phi * x[i - 1] + rng.standard_normal(ncol)
    return x
