"""The posterior covariance's definition (include/tdstar.h, "Posterior covariance"), restated in numpy on
oracle_np.rasterize (the value matrix, its mean and sigma) and oracle_np.julia_mapreduce_arrays (the sum S):
    cov[t][q]  = S / (M - 1),  S = mapreduce over k of (v_q[k] - m_q) * (a_t[k] - m_t)
    corr[t][q] = cov[t][q] / (s_q * s_t)
numpy multiplies and subtracts element by element, each rounded once (no FMA)."""
import numpy as np

from oracle import oracle_np


def column_stats(A):
    """mean and sigma (corrected) over the rows of A[M][n], the way oracle_np.rasterize forms them."""
    A = np.asarray(A, dtype=np.float64)
    rows = [A[k] for k in range(len(A))]
    n = len(rows)
    mean = oracle_np.julia_mapreduce_arrays(rows) / float(n)
    dev = [(v - mean) * (v - mean) for v in rows]
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(oracle_np.julia_mapreduce_arrays(dev) / np.float64(n - 1))
    return mean, std


def cross_moment(V, mean, std, A, tmean, tstd):
    """(cov, corr) [T][nq] of the value matrix V[M][nq] against the target matrix A[M][T]."""
    V, A = np.asarray(V, dtype=np.float64), np.asarray(A, dtype=np.float64)
    M = len(V)
    terms = [np.multiply.outer(A[k] - tmean, V[k] - mean) for k in range(M)]  # [T][nq], one rounding each
    S = oracle_np.julia_mapreduce_arrays(terms)
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = S / np.float64(M - 1)
        corr = cov / np.multiply.outer(tstd, std)
    return cov, corr


def covariance(models, qx, qy, qz, tx=None, ty=None, tz=None, series=None):
    """-> dict(cov, corr [T][nq], mean, std [nq], target_mean, target_std [T], values [M][nq], targets [M][T]);
    the target points (tx, ty, tz) first, then the columns of series[M][nseries]."""
    qx, qy, qz = (np.asarray(a, dtype=np.float64).ravel() for a in (qx, qy, qz))
    mean, std, V = oracle_np.rasterize(models, qx, qy, qz)
    M = len(models)
    cols = []
    if tx is not None and len(np.ravel(tx)):
        tx, ty, tz = (np.asarray(a, dtype=np.float64).ravel() for a in (tx, ty, tz))
        cols.append(oracle_np.rasterize(models, tx, ty, tz)[2])
    if series is not None:
        cols.append(np.asarray(series, dtype=np.float64).reshape(M, -1))
    A = np.concatenate(cols, axis=1)
    tmean, tstd = column_stats(A)
    cov, corr = cross_moment(V, mean, std, A, tmean, tstd)
    return dict(cov=cov, corr=corr, mean=mean, std=std, target_mean=tmean, target_std=tstd, values=V, targets=A)
