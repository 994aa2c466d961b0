"""Posterior cross-sections -- the numbers behind plot_model_hist (MCsub.jl:753-825).

For every y-slice (xz maps, MCsub.jl:756-785) and z-slice (xy maps,
MCsub.jl:789-820) the reference evaluates every saved model at every grid
node with v_nearest (`[v_nearest(xs, l0, zs, ...) for xs in xVec, zs in zVec]`,
an nx x nz matrix, xs fastest), then takes the mean and standard deviation
over the models and masks nodes whose std exceeds 5.  Here the model sweep
and both statistics run on the GPU (td_rasterize); plotting is out of scope.
"""
import dataclasses

import numpy as np

from .defstruct import Model
from .forward import context_for, evaluate


def _flatten(model_hist):
    """model_hist[i][j] (chain i, saved model j, MCsub.jl:761-763) or a flat list."""
    out = []
    for item in model_hist:
        if isinstance(item, (list, tuple)):
            out.extend(item)
        else:
            out.append(item)
    return out


def _section_nodes(xs, ys, zs, axis):
    """The nodes of a cross-section, xs fastest: (qx, qy, qz, (len(second), len(first)))."""
    if axis == "xz":
        a, b = np.asarray(xs, dtype=np.float64), np.asarray(zs, dtype=np.float64)
        qx, qz = np.tile(a, len(b)), np.repeat(b, len(a))
        qy = np.full(qx.shape, float(ys))
    elif axis == "xy":
        a, b = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
        qx, qy = np.tile(a, len(b)), np.repeat(b, len(a))
        qz = np.full(qx.shape, float(zs))
    else:
        raise ValueError(axis)
    return qx, qy, qz, (len(b), len(a))


def _on_device(models):
    return bool(models) and all(hasattr(m, "read_arrays") for m in models)


def section(ctx, models, xs, ys, zs, axis):
    """One cross-section: axis "xz" (ys a scalar) or "xy" (zs a scalar); ``models``: Model objects, or
    device histories (chain.History).
    Returns (mean, std) as len(first) x len(second) matrices."""
    qx, qy, qz, shape = _section_nodes(xs, ys, zs, axis)
    if _on_device(models):  # chain.History: rasterised where they lie
        mean, std, _ = ctx.rasterize_history(models, qx, qy, qz)
    else:
        mean, std, _ = ctx.rasterize([m.cells() for m in models], qx, qy, qz)
    # shape: column-major nx x n2 matrix, xs fastest
    return mean.reshape(shape).T.copy(), std.reshape(shape).T.copy()


def _sections(model_hist, dataStruct, TD_parameters):
    """plot_model_hist's loop (MCsub.jl:756, :789): (the models, the grid vectors, [(axis, slice)])."""
    if hasattr(model_hist, "read_arrays"):
        model_hist = [model_hist]
    models = _flatten(model_hist)
    vecs = tuple(np.asarray(v, dtype=np.float64) for v in (dataStruct.xVec, dataStruct.yVec, dataStruct.zVec))
    todo = []
    if TD_parameters.xzMap:
        todo += [("xz", l0) for l0 in TD_parameters.ySlice]
    if TD_parameters.xyMap:
        todo += [("xy", l0) for l0 in TD_parameters.zSlice]
    return models, vecs, todo


def plot_model_hist(model_hist, dataStruct, TD_parameters, cmax=None):  # noqa: N802 -- reference name
    """MCsub.jl:753-825 without the plots: {("xz", y) | ("xy", z): {"mean",
    "std", "masked"}} with masked = mean where std <= 5, NaN elsewhere (:776-781).
    ``model_hist`` may also be a ``History`` or a list of them (one per chain): their samples, history
    by history, are the models, and stay on the device (td_history_rasterize)."""
    ctx = context_for(dataStruct)
    models, (xv, yv, zv), todo = _sections(model_hist, dataStruct, TD_parameters)
    maps = {}
    for axis, l0 in todo:
        if axis == "xz":
            mean, std = section(ctx, models, xv, l0, zv, "xz")
        else:
            mean, std = section(ctx, models, xv, yv, l0, "xy")
        mask = np.where(std > 5, np.nan, 1.0)
        maps[(axis, l0)] = {"mean": mean, "std": std, "masked": mask * mean}
    return maps


def credible_maps(model_hist, dataStruct, TD_parameters, probs=(0.05, 0.5, 0.95), bins=None):
    """Quantile maps of the ensemble over plot_model_hist's sections: the posterior of a
    trans-dimensional run is a mixture over partitions, often bimodal at a boundary, which a mean and a
    standard deviation do not describe.  Same inputs as ``plot_model_hist`` (Models, nested lists, a
    ``History`` or a list of them); for each ("xz", y) / ("xy", z): ``quantiles`` [nprob, nx, n2]
    (Julia's Statistics.quantile over the models at each node, m[i, j] orientation), ``width`` = the
    last minus the first quantile, ``mean``, ``std`` and, with ``bins`` = (nbins, lo, hi), ``hist``
    [nx, n2, nbins + 3] (below lo | nbins bins of [lo, hi) | at or above hi | NaN).  All computed on
    the device (td_rasterize_marginals / td_history_marginals)."""
    ctx = context_for(dataStruct)
    models, (xv, yv, zv), todo = _sections(model_hist, dataStruct, TD_parameters)
    maps = {}
    for axis, l0 in todo:
        if axis == "xz":
            qx, qy, qz, shape = _section_nodes(xv, l0, zv, "xz")
        else:
            qx, qy, qz, shape = _section_nodes(xv, yv, l0, "xy")
        if _on_device(models):
            r = ctx.marginals_history(models, qx, qy, qz, probs, bins)
        else:
            r = ctx.marginals([m.cells() for m in models], qx, qy, qz, probs, bins)
        out = {"mean": r["mean"].reshape(shape).T.copy(), "std": r["std"].reshape(shape).T.copy()}
        q = r["quantiles"]
        if q is not None:
            out["quantiles"] = q.reshape((len(q),) + shape).transpose(0, 2, 1).copy()
            out["width"] = out["quantiles"][-1] - out["quantiles"][0]
        if r["hist"] is not None:
            out["hist"] = r["hist"].reshape(shape + (r["hist"].shape[1],)).transpose(1, 0, 2).copy()
        maps[(axis, l0)] = out
    return maps


def model_distributions(histories, bins):
    """The ensemble distributions plot_distribution.jl:66-80 draws, of every sample of a ``History`` or a
    list of them: ``zeta_hist`` [nbins + 3], the pooled histogram of all cells' zeta (``bins`` = (nbins,
    lo, hi), slots as in ``credible_maps``) counted where the samples lie, and ``ncells``, each sample's
    nCells, history by history."""
    if hasattr(histories, "read_arrays"):
        histories = [histories]
    histories = list(histories)
    return histories[0].ctx.zeta_hist(histories, bins)


def _chains(model_hist):
    """(the models or histories in order, the chain lengths): a nested model_hist[i][j] gives one chain per
    inner list, a list of ``History`` one chain per history (one without samples is skipped), a flat
    list of Models or a single ``History`` one chain."""
    if hasattr(model_hist, "read_arrays"):
        model_hist = [model_hist]
    model_hist = list(model_hist)
    if _on_device(model_hist):
        return model_hist, [len(h) for h in model_hist if len(h) > 0]
    if model_hist and all(isinstance(c, (list, tuple)) for c in model_hist):
        return [m for c in model_hist for m in c], [len(c) for c in model_hist]
    return model_hist, [len(model_hist)]


def _conv_summary(rhat, ess, lags, lens):
    """The ``summary`` of ``convergence_maps`` over the columns of rhat, ess and lags; ``lens``: the chains' lengths."""
    with np.errstate(invalid="ignore"):
        return {
            "rhat_max": float(np.nanmax(rhat)) if not np.all(np.isnan(rhat)) else float("nan"),
            "ess_min": float(np.nanmin(ess)) if not np.all(np.isnan(ess)) else float("nan"),
            "frac_rhat_above_1_01": float(np.mean(rhat > 1.01)),
            "frac_capped": float(np.mean(lags < 0)),
            "nan_columns": int(np.sum(np.isnan(rhat) | np.isnan(ess))),
            "n": min(lens) // 2, "m": 2 * len(lens)}


def convergence_maps(model_hist, dataStruct, TD_parameters, max_lag=0):
    """Whether the maps of ``plot_model_hist`` / ``credible_maps`` can be trusted: per node of the same
    sections (m[i, j] orientation) ``rhat``, the split Gelman-Rubin statistic over the chains' halves,
    ``ess``, the effective sample size (Geyer's initial monotone sequence over at most ``max_lag`` lags,
    0: all), ``lags``, the last lag summed (negative: the cap or the chain length ended the sum, ess is an
    upper bound), and ``mean``, ``std``; ``summary``: rhat_max (NaN ignored), ess_min, frac_rhat_above_1_01,
    frac_capped, nan_columns, n (rows per half chain), m (half chains).  Chains: see ``_chains``; every chain
    gives its last 2n samples, n = min length // 2.  All computed on the device (td_rasterize_convergence /
    td_history_convergence)."""
    ctx = context_for(dataStruct)
    _, (xv, yv, zv), todo = _sections(model_hist, dataStruct, TD_parameters)
    models, lens = _chains(model_hist)
    maps = {}
    for axis, l0 in todo:
        if axis == "xz":
            qx, qy, qz, shape = _section_nodes(xv, l0, zv, "xz")
        else:
            qx, qy, qz, shape = _section_nodes(xv, yv, l0, "xy")
        if _on_device(models):
            r = ctx.convergence_history(models, qx, qy, qz, max_lag)
        else:
            r = ctx.convergence_models([m.cells() for m in models], lens, qx, qy, qz, max_lag)
        out = {f: r[f].reshape(shape).T.copy() for f in ("rhat", "ess", "lags", "mean", "std")}
        out["summary"] = _conv_summary(r["rhat"], r["ess"], r["lags"], lens)
        maps[(axis, l0)] = out
    return maps


def posterior_volume(model_hist, dataStruct, TD_parameters, probs=(0.05, 0.5, 0.95), bins=None, convergence=False,
                     max_lag=0, xs=None, ys=None, zs=None):
    """The posterior as a volume: what ``plot_model_hist``, ``credible_maps`` and ``convergence_maps`` give
    section by section, at every node of the lattice ``xs`` x ``ys`` x ``zs`` (default: dataStruct.xVec /
    yVec / zVec) in one call, as [nx, ny, nz] arrays -- ``mean``, ``std``, ``masked`` (mean where std <= 5,
    NaN elsewhere), ``quantiles`` [nprob, nx, ny, nz] and ``width`` (the last minus the first quantile),
    ``hist`` [nx, ny, nz, nbins + 3] with ``bins`` = (nbins, lo, hi) and, with ``convergence``, ``rhat``,
    ``ess``, ``lags`` and ``summary`` as in ``convergence_maps``; ``x``, ``y``, ``z``: the lattice vectors.
    ``vol["mean"][:, j, :]`` is the xz section at ys[j], ``[:, :, k]`` the xy section at zs[k], bit for bit.
    Same inputs as ``plot_model_hist`` (Models, nested lists, a ``History`` or a list of them); computed on
    the device slab by slab, whatever the lattice's size (td_rasterize_volume / td_history_volume)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    models, lens = _chains(model_hist)
    if _on_device(models):
        r = ctx.volume_history(models, qx, qy, qz, probs, bins, convergence, max_lag)
    else:
        r = ctx.volume([m.cells() for m in models], qx, qy, qz, probs, bins, lens if convergence else None, max_lag)
    out = {"x": xv, "y": yv, "z": zv}
    for f in ("mean", "std") + (("rhat", "ess", "lags") if convergence else ()):
        out[f] = r[f].reshape(shape).transpose(2, 1, 0).copy()
    out["masked"] = np.where(out["std"] > 5, np.nan, 1.0) * out["mean"]
    q = r["quantiles"]
    if q is not None:
        out["quantiles"] = q.reshape((len(q),) + shape).transpose(0, 3, 2, 1).copy()
        out["width"] = out["quantiles"][-1] - out["quantiles"][0]
    if r["hist"] is not None:
        out["hist"] = r["hist"].reshape(shape + (r["hist"].shape[1],)).transpose(2, 1, 0, 3).copy()
    if convergence:
        out["summary"] = _conv_summary(r["rhat"], r["ess"], r["lags"], lens)
    return out


def posterior_covariance(model_hist, dataStruct, TD_parameters, targets, series=None, xs=None, ys=None, zs=None):
    """What trades off against what: the covariance and the correlation, over the models, between zeta at each
    target and zeta at every node of the lattice ``xs`` x ``ys`` x ``zs`` (default: dataStruct.xVec / yVec /
    zVec) -- the ensemble's own point-spread function, the Bayesian stand-in for a checkerboard test.
    ``targets``: points [nt, 3] (x, y, z; None for none); ``series``: [nmodels, nseries] per-model numbers
    (row = model: a ray's predicted t* out of ``posterior_predictive(values=True)["ptS"]``, the phi trace,
    ...).  Same inputs as ``posterior_volume`` (Models, nested lists, a ``History`` or a list of them).
    -> dict: ``cov``, ``corr`` [T, nx, ny, nz] (rows: the points, then the series), ``mean``, ``std`` [nx, ny,
    nz] (``posterior_volume``'s), ``target_mean``, ``target_std`` [T], ``node_volume`` (the product of the
    lattice's mean spacings, km^3; an axis of one node counts 1), ``footprint`` [T]: the nodes with corr >=
    0.5 times node_volume, and ``x``, ``y``, ``z``.  Computed on the device slab by slab
    (td_rasterize_covariance / td_history_covariance)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    models, _ = _chains(model_hist)
    if _on_device(models):
        r = ctx.covariance_history(models, qx, qy, qz, targets, series)
    else:
        r = ctx.covariance([m.cells() for m in models], qx, qy, qz, targets, series)
    out = {"x": xv, "y": yv, "z": zv, "target_mean": r["target_mean"], "target_std": r["target_std"]}
    for f in ("mean", "std"):
        out[f] = r[f].reshape(shape).transpose(2, 1, 0).copy()
    for f in ("cov", "corr"):
        out[f] = r[f].reshape((len(r[f]),) + shape).transpose(0, 3, 2, 1).copy()
    out["node_volume"] = float(np.prod([(v[-1] - v[0]) / (len(v) - 1) for v in (xv, yv, zv) if len(v) > 1]))
    out["footprint"] = np.sum(r["corr"] >= 0.5, axis=1) * out["node_volume"]
    return out


def posterior_interfaces(model_hist, dataStruct, TD_parameters, thresholds=(5.0,), xs=None, ys=None, zs=None):
    """Where the ensemble puts boundaries: what the other posterior products smooth over.  On the lattice
    ``xs`` x ``ys`` x ``zs`` (default: dataStruct.xVec / yVec / zVec), with d the difference of a model's
    nearest-cell zeta across the forward face of a node along axis a (0: x, 1: y, 2: z), -> dict of [nx, ny, nz]
    arrays: ``prob`` [3, ...] the share of the models with a Voronoi boundary on the face (the value differs),
    ``prob_any`` the share with one on any of the node's forward faces, ``exceed`` [nthr, 3, ...] the share with
    abs(d) > thresholds[t], ``jump`` [3, ...] the expected abs(d) (NaN where the lattice ends and there is no
    face), ``count`` [3, ...] and ``any`` the raw counts (-1 without a face), ``density`` the cells of all models
    whose nucleus lies in the node's voxel, ``density_per_model`` (= density / M: where the sampler spends its
    cells), ``skipped`` (cells with a NaN coordinate), ``mean``, ``std`` (``posterior_volume``'s) and ``x``,
    ``y``, ``z``, ``thresholds``.  Same inputs as ``posterior_volume`` (Models, nested lists, a ``History`` or a
    list of them); computed on the device slab by slab (td_rasterize_interfaces / td_history_interfaces)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, _, _, _ = _lattice(dataStruct, xs, ys, zs)
    thr = np.asarray(thresholds, dtype=np.float64).ravel()
    models, lens = _chains(model_hist)
    if _on_device(models):
        r = ctx.interfaces_history(models, xv, yv, zv, thr)
    else:
        r = ctx.interfaces([m.cells() for m in models], xv, yv, zv, thr)
    M = sum(lens)

    def share(c):
        return np.where(c < 0, np.nan, c / np.float64(M))

    out = {"x": xv, "y": yv, "z": zv, "thresholds": thr, "skipped": r["skipped"]}
    for f in ("count", "any", "jump", "mean", "std", "density"):
        out[f] = _grid(r[f], shape)
    out["prob"] = share(out["count"])
    out["prob_any"] = share(out["any"])
    out["exceed"] = share(_grid(r["exceed"], shape)) if r["exceed"] is not None else np.empty((0, 3) + shape[::-1])
    out["density_per_model"] = out["density"] / np.float64(M)
    return out


def resolution_offsets(lags=(2, 1, 2), window="box"):
    """The window of ``posterior_resolution`` as forward lattice offsets [noff, 3] (di, dj, dk), int32.  ``lags`` =
    (Lx, Ly, Lz) >= 0.  ``window="axes"``: (l, 0, 0), l = 1 .. Lx, then (0, l, 0), then (0, 0, l).  ``"box"``: every
    forward offset (dk > 0, or dk == 0 and dj > 0, or dk == dj == 0 and di > 0) with abs(di) <= Lx, abs(dj) <= Ly, 0 <=
    dk <= Lz -- the axes' offsets first, in that order, so that the runs can use them, then the others with di
    fastest and dk slowest."""
    Lx, Ly, Lz = (int(v) for v in lags)
    if min(Lx, Ly, Lz) < 0:
        raise ValueError("lags must be >= 0")
    if window not in ("axes", "box"):
        raise ValueError("window: 'axes' or 'box'")
    out = [(l, 0, 0) for l in range(1, Lx + 1)] + [(0, l, 0) for l in range(1, Ly + 1)] + [(0, 0, l) for l in range(1, Lz + 1)]
    if window == "box":
        on_axis = set(out)
        out += [(di, dj, dk) for dk in range(0, Lz + 1) for dj in range(-Ly, Ly + 1) for di in range(-Lx, Lx + 1)
                if (dk, dj, di) > (0, 0, 0) and (di, dj, dk) not in on_axis]
    return np.asarray(out, dtype=np.int32).reshape(-1, 3)


def posterior_resolution(model_hist, dataStruct, TD_parameters, lags=(2, 1, 2), window="box", threshold=0.5, weights="volume",
                         xs=None, ys=None, zs=None, want=None):
    """The ensemble's point-spread function at EVERY node: how far from a node the models tie zeta together, in which
    direction, and where that is unknown because the lattice or the window ends -- what ``posterior_covariance`` gives
    at a handful of targets.  On the lattice ``xs`` x ``ys`` x ``zs`` (default: dataStruct.xVec / yVec / zVec), with
    the window ``resolution_offsets(lags, window)``, -> dict: ``offsets`` [noff, 3]; ``corr``, ``cov`` [noff, nx, ny,
    nz], the correlation and covariance of the node's zeta with the neighbour's at the offset (NaN where the pair
    leaves the lattice), only when named in ``want``; ``footprint`` [nx, ny, nz], the weight of the node and of the
    neighbours, forwards and backwards, with corr >= ``threshold`` (``weights="volume"``: ``voxel_weights``, km^3;
    None: a count of nodes; an array [nx, ny, nz]); ``run`` [3, 2, nx, ny, nz], the contiguous steps along +a / -a that
    pass; ``extent`` [3, nx, ny, nz], the distance between the two runs' ends; ``censored`` [nx, ny, nz] (bit 2a / 2a
    + 1: the run along +a / -a ended on the lattice's or the window's edge, not on a failing correlation); ``mean``,
    ``std`` (``posterior_volume``'s); ``x``, ``y``, ``z``, ``threshold``.  ``want`` (default: everything but corr and
    cov): the subset of TdContext.RES_ALL to compute; an output that was not asked for is None.  Same inputs as
    ``posterior_volume``; every node is swept once on the device (td_rasterize_resolution / td_history_resolution)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, _, _, _ = _lattice(dataStruct, xs, ys, zs)
    off = resolution_offsets(lags, window)
    if isinstance(weights, str):
        if weights != "volume":
            raise ValueError("weights: 'volume', None or an array [nx, ny, nz]")
        weights = voxel_weights(xv, yv, zv)
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64)
        if w.shape != shape[::-1]:
            raise ValueError("weights must be [nx, ny, nz] = %s; got %s" % (shape[::-1], w.shape))
        weights = w.transpose(2, 1, 0).ravel()  # x fastest
    want = ctx.RES_SUMMARY if want is None else want
    models, _ = _chains(model_hist)
    if _on_device(models):
        r = ctx.resolution_history(models, xv, yv, zv, off, threshold, weights, want)
    else:
        r = ctx.resolution([m.cells() for m in models], xv, yv, zv, off, threshold, weights, want)
    out = {"x": xv, "y": yv, "z": zv, "offsets": off, "threshold": float(threshold)}
    for f in ("corr", "cov", "footprint", "extent", "run", "censored", "mean", "std"):
        out[f] = _grid(r[f], shape) if r[f] is not None else None
    return out


def voxel_weights(xs, ys, zs):
    """The volume of every node's voxel, [nx, ny, nz]: (dx_i * dy_j) * dz_k.  Along an axis of n >= 2 nodes v the
    widths are the differences of the edges [v_0, the midpoints 0.5 (v_l + v_{l+1}) ..., v_{n-1}] (the end nodes
    own half a cell); an axis of one node has width 1.0."""
    def widths(v):
        v = np.asarray(v, dtype=np.float64).ravel()
        if len(v) < 2:
            return np.ones(len(v))
        return np.diff(np.concatenate(([v[0]], 0.5 * (v[:-1] + v[1:]), [v[-1]])))

    dx, dy, dz = widths(xs), widths(ys), widths(zs)
    return (dx[:, None] * dy[None, :])[:, :, None] * dz[None, None, :]


def depth_layers(zs, edges):
    """Masks of the depth layers [edges[l], edges[l + 1]) of the lattice's ``zs``: {"z lo-hi": mask [1, 1, nz]},
    which ``posterior_regions`` broadcasts over x and y.  A layer without a node is left out."""
    zv = np.asarray(zs, dtype=np.float64).ravel()
    e = np.asarray(edges, dtype=np.float64).ravel()
    out = {}
    for lo, hi in zip(e[:-1], e[1:]):
        mask = (zv >= lo) & (zv < hi)
        if mask.any():
            out["z %g-%g" % (lo, hi)] = mask.reshape(1, 1, -1)
    return out


def box_region(xs, ys, zs, lo, hi):
    """The mask [nx, ny, nz] of the lattice's nodes with lo[a] <= coordinate <= hi[a] on every axis a."""
    inside = [(np.asarray(v, dtype=np.float64).ravel() >= float(a)) & (np.asarray(v, dtype=np.float64).ravel() <= float(b))
              for v, a, b in zip((xs, ys, zs), lo, hi)]
    return inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :]


def region_points(regions, xs, ys, zs, weights="volume"):
    """``posterior_regions``' regions as one point list: (names, px, py, pz, w or None, reg_off [R + 1]).  A mask
    gives its nodes in the lattice's order (x fastest) with the voxel weights (``weights="volume"``) or none; a
    tuple (px, py, pz[, w]) gives its points as they stand, w defaulting to 1.0."""
    if weights not in ("volume", None):
        raise ValueError("weights: 'volume' or None")
    xv, yv, zv = (np.asarray(v, dtype=np.float64).ravel() for v in (xs, ys, zs))
    shape = (len(xv), len(yv), len(zv))
    vol = voxel_weights(xv, yv, zv) if weights == "volume" else None
    names, pts, ws, off = [], [], [], [0]
    for name, reg in regions.items():
        if isinstance(reg, tuple):
            p = [np.asarray(a, dtype=np.float64).ravel() for a in reg[:3]]
            wr = np.asarray(reg[3], dtype=np.float64).ravel() if len(reg) > 3 else None
            if not (len(p[0]) == len(p[1]) == len(p[2])) or (wr is not None and len(wr) != len(p[0])):
                raise ValueError("region %r: px, py, pz and w must have the same length" % (name,))
        else:
            mask = np.broadcast_to(np.asarray(reg, dtype=bool), shape)
            k, j, i = np.nonzero(mask.transpose(2, 1, 0))  # x fastest
            p = [xv[i], yv[j], zv[k]]
            wr = vol[i, j, k] if vol is not None else None
        if len(p[0]) == 0:
            raise ValueError("region %r holds no point" % (name,))
        names.append(name)
        pts.append(p)
        ws.append(wr)
        off.append(off[-1] + len(p[0]))
    if not names:
        raise ValueError("no region")
    px, py, pz = (np.concatenate([p[a] for p in pts]) for a in range(3))
    w = None
    if any(wr is not None for wr in ws):
        w = np.concatenate([wr if wr is not None else np.ones(len(p[0])) for wr, p in zip(ws, pts)])
    return names, px, py, pz, w, np.asarray(off, dtype=np.int64)


def posterior_regions(model_hist, dataStruct, TD_parameters, regions, weights="volume", normalize=True,
                      probs=(0.05, 0.5, 0.95), bins=None, convergence=False, xs=None, ys=None, zs=None):
    """Questions about regions: is the wedge more attenuating than the back-arc, and with what probability; the
    lateral average of each depth layer with its credible band; the average along a ray path.  The average of a
    region is one number per SAMPLE, and its distribution over the samples depends on how the nodes co-vary, so
    none of this can be read off the per-node maps.  ``regions``: {name: a boolean mask [nx, ny, nz] on the
    lattice ``xs`` x ``ys`` x ``zs`` (default: dataStruct.xVec / yVec / zVec; anything that broadcasts to it, see
    ``depth_layers`` and ``box_region``) | a tuple (px, py, pz[, w]) of free points -- a profile, a ray path}.
    With masks and ``weights="volume"`` a node's weight is its voxel's volume (``voxel_weights``); ``weights=None``
    gives plain averages; ``normalize=False`` the weighted sums.  -> dict: ``names``, ``series`` [M, R] (shaped
    for ``posterior_covariance(..., series=...)``), ``weight`` [R], ``mean``, ``std`` [R], ``quantiles`` [nprob,
    R], ``hist`` [R, nbins + 3] with ``bins`` = (nbins, lo, hi), with ``convergence`` ``rhat``, ``ess``, ``lags``
    [R], ``greater`` [R, R] (the samples with series[:, a] > series[:, b]) and ``prob_greater`` = greater / M.
    Same inputs as ``posterior_interfaces`` (Models, nested lists, a ``History`` or a list of them); computed on
    the device slab by slab (td_rasterize_regions / td_history_regions)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature)
    xv, yv, zv = _lattice(dataStruct, xs, ys, zs)[:3]
    names, px, py, pz, w, off = region_points(regions, xv, yv, zv, weights)
    models, lens = _chains(model_hist)
    if _on_device(models):
        r = ctx.regions_history(models, px, py, pz, off, w, normalize, probs, bins, convergence)
    else:
        r = ctx.regions([m.cells() for m in models], px, py, pz, off, w, normalize, probs, bins,
                        lens if convergence else None)
    out = {"names": names, "prob_greater": r["greater"] / np.float64(sum(lens))}
    for f in ("series", "weight", "mean", "std", "greater") + (("rhat", "ess", "lags") if convergence else ()):
        out[f] = r[f]
    if r["quantiles"] is not None:
        out["quantiles"] = r["quantiles"]
    if r["hist"] is not None:
        out["hist"] = r["hist"]
    return out


def support_weights(dataStruct, kind="tstar"):
    """One weight per valid ray point of ``dataStruct`` in ``evaluate``'s ``want_nearest`` order, for
    ``TdContext.support``: ``"count"`` -> None (every point counts 1); ``"tstar"`` -> g[p], half the sum of
    rayL * rayU / 1000 of the segments that adjoin the point, so that the sum over the points of g[p] *
    zeta(owner of p) is the sum of ptS over the rays (MCsub.jl:147-160) and a cell's support is the derivative
    of the total predicted t* with respect to its zeta; ``"length"`` -> the same with rayL alone, in km."""
    if kind == "count":
        return None
    if kind not in ("tstar", "length"):
        raise ValueError("kind must be 'count', 'tstar' or 'length'")
    rayX, rayL, rayU = (np.asarray(a, dtype=np.float64) for a in (dataStruct.rayX, dataStruct.rayL, dataStruct.rayU))
    out = []
    for i in range(rayX.shape[1]):
        nan = np.flatnonzero(np.isnan(rayX[:, i]))
        c = int(nan[0]) if len(nan) else rayX.shape[0]
        if c == 0:
            continue
        seg = rayL[:c - 1, i] * rayU[:c - 1, i] / 1000.0 if kind == "tstar" else rayL[:c - 1, i].copy()
        out.append(0.5 * (np.concatenate((seg, [0.0])) + np.concatenate(([0.0], seg))))
    return np.concatenate(out) if out else np.zeros(0)


def _lattice(dataStruct, xs, ys, zs):
    """(xv, yv, zv, the shape x fastest, qx, qy, qz) of the lattice ``posterior_volume`` sweeps."""
    xv, yv, zv = (np.asarray(v if v is not None else d, dtype=np.float64).ravel()
                  for v, d in ((xs, dataStruct.xVec), (ys, dataStruct.yVec), (zs, dataStruct.zVec)))
    qx = np.tile(xv, len(yv) * len(zv))
    qy = np.tile(np.repeat(yv, len(xv)), len(zv))
    qz = np.repeat(zv, len(xv) * len(yv))
    return xv, yv, zv, (len(zv), len(yv), len(xv)), qx, qy, qz


def _grid(a, shape):
    """[..., nq] in the lattice's node order (``shape``, x fastest) -> [..., nx, ny, nz]"""
    lead = a.shape[:-1]
    k = len(lead)
    return a.reshape(lead + shape).transpose(tuple(range(k)) + (k + 2, k + 1, k)).copy()


def posterior_support(model_hist, dataStruct, TD_parameters, weights="tstar", thresholds=(0.0,), probs=None, bins=None,
                      convergence=False, xs=None, ys=None, zs=None):
    """Did the data say anything about this node, or is it the prior?  A Voronoi cell that owns no ray point does
    not enter ``evaluate``: its zeta is a prior draw in every sample.  Per sample, every cell's support is the sum
    of ``weights`` (a kind of ``support_weights``, an array of one weight per valid ray point, or None: a count)
    over the ray points it owns, and a node's support is its owning cell's.  On the lattice ``xs`` x ``ys`` x
    ``zs`` (default: dataStruct.xVec / yVec / zVec) -> dict of [nx, ny, nz] arrays ``mean``, ``std`` of the node
    support over the samples, ``share`` [nthr, ...] the share of the samples whose support exceeds thresholds[t]
    (0.0: the node's cell touches the data at all), ``exceed`` the raw counts, ``quantiles`` [nprob, ...],
    ``hist`` [..., nbins + 3], with ``convergence`` ``rhat``, ``ess``, ``lags``; per sample ``barren`` (cells that
    own no ray point), ``orphans`` (ray points no cell owns), ``cells`` and ``barren_share`` = barren / cells: the
    part of nCells that is not structure; ``x``, ``y``, ``z``, ``thresholds``.  Same inputs as ``posterior_volume``
    (Models, nested lists, a ``History`` or a list of them); computed on the device slab by slab
    (td_rasterize_support / td_history_support)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    w = support_weights(dataStruct, weights) if isinstance(weights, str) else weights
    thr = np.asarray(thresholds, dtype=np.float64).ravel()
    probs = () if probs is None else probs
    models, lens = _chains(model_hist)
    if _on_device(models):
        r = ctx.support_history(models, w, qx, qy, qz, thr, probs, bins, convergence, want_cells=False)
        cells = np.concatenate([h.traces()[:, 1] for h in models]).astype(np.int64)
    else:
        r = ctx.support([m.cells() for m in models], w, qx, qy, qz, thr, probs, bins, lens if convergence else None,
                        want_cells=False)
        cells = np.array([len(m.cells()[0]) for m in models], dtype=np.int64)
    M = sum(lens)
    out = {"x": xv, "y": yv, "z": zv, "thresholds": thr, "barren": r["barren"], "orphans": r["orphans"], "cells": cells}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["barren_share"] = r["barren"] / cells.astype(np.float64)
    for f in ("mean", "std") + (("rhat", "ess", "lags") if convergence else ()):
        out[f] = _grid(r[f], shape)
    out["exceed"] = _grid(r["exceed"], shape) if r["exceed"] is not None else np.empty((0,) + shape[::-1], dtype=np.int64)
    out["share"] = out["exceed"] / np.float64(M)
    if r["quantiles"] is not None:
        out["quantiles"] = _grid(r["quantiles"], shape)
    if r["hist"] is not None:
        out["hist"] = r["hist"].reshape(shape + (r["hist"].shape[1],)).transpose(2, 1, 0, 3).copy()
    return out


def ray_density(dataStruct, xs=None, ys=None, zs=None, weights="length"):
    """The classical ray-density map: every valid ray point of ``dataStruct`` gives its weight (a kind of
    ``support_weights``, an array, or None: a count) to the nearest node of the lattice ``xs`` x ``ys`` x ``zs``
    (default: dataStruct.xVec / yVec / zVec) -- one ``TdContext.support`` call with a single model whose cells are
    the nodes.  -> dict(``density`` [nx, ny, nz], ``count`` [nx, ny, nz], ``orphans``: the points farther than the
    search's sentinel from every node, ``x``, ``y``, ``z``)."""
    ctx = context_for(dataStruct)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    w = support_weights(dataStruct, weights) if isinstance(weights, str) else weights
    r = ctx.support([(qx, qy, qz)], w)
    return {"x": xv, "y": yv, "z": zv, "density": r["cell"].reshape(shape).transpose(2, 1, 0).copy(),
            "count": r["count"].reshape(shape).transpose(2, 1, 0).copy(), "orphans": int(r["orphans"][0])}


def checkerboard_model(xs, ys, zs, blocks, lo, hi):
    """The known model of a checkerboard test: a ``Model`` whose nuclei are the centres of a regular ``blocks`` =
    (bx, by, bz) division of the box of the lattice ``xs`` x ``ys`` x ``zs`` (cell i + bx (j + by k), x fastest),
    zeta = ``lo`` where i + j + k is even and ``hi`` where it is odd.  The nuclei are equally spaced along every
    axis, so the Voronoi cells are the blocks; a point on a face goes to the lower index, as everywhere."""
    bx, by, bz = (int(b) for b in blocks)
    if min(bx, by, bz) < 1:
        raise ValueError("blocks: at least one block along every axis")
    centres = []
    for v, b in zip((xs, ys, zs), (bx, by, bz)):
        v = np.asarray(v, dtype=np.float64).ravel()
        a, width = float(v.min()), (float(v.max()) - float(v.min())) / b
        centres.append(a + (np.arange(b) + 0.5) * width)
    k, j, i = np.meshgrid(np.arange(bz), np.arange(by), np.arange(bx), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    zeta = np.where((i + j + k) % 2 == 0, float(lo), float(hi))
    return Model(float(bx * by * bz), centres[0][i], centres[1][j], centres[2][k], zeta)


def synthetic_data(dataStruct, model, TD_parameters, noise=1.0, seed=0):
    """The data a known model would have given: a copy of ``dataStruct`` with tS = ptS(model) + noise * allSig *
    N(0, 1), ptS being ``evaluate``'s prediction on the rays of ``dataStruct`` and the draws
    numpy.random.default_rng(seed)'s.  ``noise=0`` gives the exact data.  Neither input is modified; the copy gets
    a device context of its own on first use."""
    prm = TD_parameters.replace(debug_prior=0) if TD_parameters.debug_prior == 1 else TD_parameters
    m, _, valid = evaluate(model.copy(), dataStruct, prm)
    if valid != 1:
        raise ValueError("the model cannot be evaluated on these rays")
    pt = np.asarray(m.ptS, dtype=np.float64).ravel()
    sig = np.asarray(dataStruct.allSig, dtype=np.float64).ravel()
    draws = np.random.default_rng(seed).standard_normal(len(pt))
    tS = pt + (float(noise) * sig) * draws
    return dataclasses.replace(dataStruct, tS=tS.reshape(np.shape(dataStruct.tS)), _td_ctx=None)


def posterior_recovery(model_hist, dataStruct, TD_parameters, truth, regions=None, weights="volume", band=(0.05, 0.95),
                       probs=(0.05, 0.5, 0.95), bins=None, convergence=False, xs=None, ys=None, zs=None):
    """The ensemble against a model that is KNOWN: a checkerboard or spike test, a synthetic recovery, another
    study's volume.  ``truth``: a ``Model`` (rasterised on the lattice ``xs`` x ``ys`` x ``zs``, default
    dataStruct.xVec / yVec / zVec, by the nearest search of the samples) or an array [nx, ny, nz] of node values.
    ``regions`` as in ``posterior_regions`` (default: one region "all" of every node, with ``voxel_weights`` when
    ``weights="volume"``); free points need a ``Model`` as the truth.  -> dict, per node [nx, ny, nz]: ``truth``;
    ``bias``, ``std`` (the mean and sigma over the samples of zeta - truth), ``zscore`` = bias / std; ``below``,
    ``equal``, ``above`` (the samples with zeta <, ==, > truth); ``pit`` = (below + 0.5 equal) / M, the mid-rank
    probability integral transform; ``inside`` = band[0] <= pit <= band[1]; ``pit_hist``: ten equal bins of pit
    over the nodes (flat when the ensemble is calibrated).  Per region: ``names``, ``weight`` [R], ``coverage``
    [R], the weighted share of the region's points that are inside; ``msd`` [M, R], every sample's weighted mean
    square distance to the truth, ``rms`` = sqrt(msd) with ``rms_mean``, ``rms_std``, ``rms_quantiles`` [nprob, R]
    (numpy on the M x R matrix); the device's statistics of msd ``msd_mean``, ``msd_std``, ``msd_quantiles``,
    ``msd_hist`` [R, nbins + 3] with ``bins`` = (nbins, lo, hi) in msd's units and, with ``convergence``, ``rhat``,
    ``ess``, ``lags`` [R] and ``summary`` as in ``convergence_maps`` (R-hat is that of the msd trace: burn-in in
    model space); ``mean_model_rms`` [R] = sqrt(sum w bias^2 / W), the distance of the MEAN model, which with
    weights >= 0 is never above the root of msd_mean.  Same inputs as ``posterior_regions``; computed on the device slab by slab
    (td_rasterize_recovery / td_history_recovery).  With ``regions`` given the per-node outputs come from one more
    region that lists every node once."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    nq = len(qx)
    vol = voxel_weights(xv, yv, zv).transpose(2, 1, 0).ravel() if weights == "volume" else None
    if weights not in ("volume", None):
        raise ValueError("weights: 'volume' or None")
    if regions is None:
        names, px, py, pz, w, off = ["all"], qx, qy, qz, vol, np.array([0, nq], dtype=np.int64)
    else:  # the named regions, then every node once
        names, px, py, pz, w, off = region_points(regions, xv, yv, zv, weights)
        if w is not None or vol is not None:
            w = np.concatenate((w if w is not None else np.ones(len(px)), vol if vol is not None else np.ones(nq)))
        px, py, pz = np.concatenate((px, qx)), np.concatenate((py, qy)), np.concatenate((pz, qz))
        off = np.concatenate((off, [off[-1] + nq]))
    R = len(names)
    if isinstance(truth, Model):
        tp = ctx.rasterize([truth.cells()], px, py, pz, want_values=True)[2][0]
    else:
        tn = np.asarray(truth, dtype=np.float64)
        if tn.shape != (len(xv), len(yv), len(zv)):
            raise ValueError("truth: a Model or an array [nx, ny, nz]")
        parts = []
        for name, reg in (regions or {}).items():  # (region_points' order)
            if isinstance(reg, tuple):
                raise ValueError("region %r: free points need a Model as the truth" % (name,))
            parts.append(tn.transpose(2, 1, 0)[np.broadcast_to(np.asarray(reg, dtype=bool), tn.shape).transpose(2, 1, 0)])
        tp = np.concatenate(parts + [tn.transpose(2, 1, 0).ravel()])
    models, lens = _chains(model_hist)
    if _on_device(models):
        r = ctx.recovery_history(models, px, py, pz, tp, off, w, True, probs, bins, convergence)
    else:
        r = ctx.recovery([m.cells() for m in models], px, py, pz, tp, off, w, True, probs, bins,
                         lens if convergence else None)
    M = sum(lens)

    def grid(a):  # the last nq listed points -> [nx, ny, nz]
        return a[-nq:].reshape(shape).transpose(2, 1, 0).copy()

    pit_p = (r["below"] + 0.5 * r["equal"]) / np.float64(M)  # per listed point
    inside_p = (band[0] <= pit_p) & (pit_p <= band[1])
    wp = w if w is not None else np.ones(len(px))
    out = {"x": xv, "y": yv, "z": zv, "names": names, "truth": grid(tp), "bias": grid(r["dmean"]), "std": grid(r["dstd"]),
           "below": grid(r["below"]), "equal": grid(r["equal"]), "above": grid(r["above"]), "pit": grid(pit_p),
           "inside": grid(inside_p), "weight": r["weight"][:R], "msd": r["series"][:, :R].copy()}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["zscore"] = out["bias"] / out["std"]
        out["pit_hist"] = np.histogram(out["pit"], bins=10, range=(0.0, 1.0))[0]
        out["coverage"] = np.array([np.sum(wp[a:b] * inside_p[a:b]) / np.sum(wp[a:b]) for a, b in zip(off[:R], off[1:R + 1])])
        out["mean_model_rms"] = np.sqrt(np.array([np.sum(wp[a:b] * r["dmean"][a:b] ** 2) / np.sum(wp[a:b])
                                                  for a, b in zip(off[:R], off[1:R + 1])]))
        out["rms"] = np.sqrt(out["msd"])
        out["rms_mean"], out["rms_std"] = out["rms"].mean(axis=0), out["rms"].std(axis=0, ddof=1) if M > 1 else np.full(R, np.nan)
        if len(np.ravel(probs)):
            out["rms_quantiles"] = np.quantile(out["rms"], np.ravel(probs), axis=0)
    out["msd_mean"], out["msd_std"] = r["mean"][:R], r["std"][:R]
    if r["quantiles"] is not None:
        out["msd_quantiles"] = r["quantiles"][:, :R]
    if r["hist"] is not None:
        out["msd_hist"] = r["hist"][:R]
    if convergence:
        rhat, ess, lags = r["rhat"][:R], r["ess"][:R], r["lags"][:R]
        out.update(rhat=rhat, ess=ess, lags=lags, summary=_conv_summary(rhat, ess, lags, lens))
    return out


def info_gain_bits(hist_a, hist_b, MA, MB):
    """The Kullback-Leibler divergence of side A's histogram from side B's, in bits, per row of ``hist_a``, ``hist_b``
    [..., nbins + 3] (``marginals``' slots: below lo, the bins, at or above hi, NaN) of ``MA`` and ``MB`` samples:
    sum over the slots s of pA_s log2(pA_s / pB_s) with p_s = (c_s + 0.5) / (M + 0.5 (nbins + 3)), the add-a-half
    estimate, which keeps an empty slot's term finite.  Formed on the host from the integer counts."""
    ha, hb = np.asarray(hist_a, dtype=np.float64), np.asarray(hist_b, dtype=np.float64)
    slots = ha.shape[-1]
    pa = (ha + 0.5) / (np.float64(MA) + 0.5 * slots)
    pb = (hb + 0.5) / (np.float64(MB) + 0.5 * slots)
    return np.sum(pa * np.log2(pa / pb), axis=-1)


def compare_summary(r, MA, MB):
    """What ``posterior_compare`` derives from the integer outputs ``r`` of ``TdContext.compare`` (any shape) for sides
    of ``MA`` and ``MB`` models -> dict: ``prob_greater`` = (greater + 0.5 equal) / (MA MB), ``prob_exceed`` = exceed /
    (MA MB), ``ks`` = max(ks_plus, ks_minus) / (MA MB), ``ks_sign`` (+1 where ks_plus is the larger: A's CDF lies
    above B's, A is the smaller; -1 where ks_minus is; 0 where they are equal), ``mean_diff`` = mean_a - mean_b and,
    with histograms, ``info_gain_bits`` (``info_gain_bits``).  Entries whose inputs are None are left out."""
    pairs = np.float64(MA) * np.float64(MB)
    out = {}
    if r.get("greater") is not None:
        out["prob_greater"] = (r["greater"] + 0.5 * r["equal"]) / pairs
    if r.get("exceed") is not None:
        out["prob_exceed"] = r["exceed"] / pairs
    if r.get("ks_plus") is not None:
        out["ks"] = np.maximum(r["ks_plus"], r["ks_minus"]) / pairs
        out["ks_sign"] = np.sign(r["ks_plus"] - r["ks_minus"]).astype(np.int8)
    if r.get("mean_a") is not None:
        out["mean_diff"] = r["mean_a"] - r["mean_b"]
    if r.get("hist_a") is not None:
        out["info_gain_bits"] = info_gain_bits(r["hist_a"], r["hist_b"], MA, MB)
    return out


def posterior_compare(model_hist_a, model_hist_b, dataStruct, TD_parameters, exceed=((1.0, 0.0),), probs=None, bins=None,
                      xs=None, ys=None, zs=None):
    """One ensemble against another, node by node: the posterior against a ``debug_prior=1`` ensemble (how far did the
    data move the marginal?), a run against a run with other data or another prior, zeta_S against zeta_P.  Each
    side as ``posterior_volume`` takes it (Models, nested lists, a ``History`` or a list of them, recorded on any
    context of the device; where only one side is on the device its samples are read back), independent samples, at
    most 16384 a side.  With a_i, b_j the two sides' values at a node, on the lattice ``xs`` x ``ys`` x ``zs``
    (default dataStruct.xVec / yVec / zVec) -> dict of [nx, ny, nz] arrays: the exact pair counts ``less``, ``equal``,
    ``greater`` (a_i <, ==, > b_j), ``exceed`` [npairs, ...] (a_i > s b_j + t for ``exceed`` = [(s, t)]: with zeta =
    1000 / Q, (r, 0) asks for Q_B / Q_A > r), ``ks_plus``, ``ks_minus``; ``prob_greater`` = (greater + 0.5 equal) /
    (MA MB), the probability of superiority (Mann-Whitney's U over MA MB); ``prob_exceed`` = exceed / (MA MB); ``ks`` =
    max(ks_plus, ks_minus) / (MA MB), the two-sample Kolmogorov-Smirnov distance, ``ks_sign`` (+1: A's CDF lies
    above, A is the smaller) and ``ks_at``, the smallest value at which it is reached (NaN where the two samples
    have one CDF); ``mean_a``, ``std_a``, ``mean_b``, ``std_b`` (``posterior_volume``'s of each side, bit for bit)
    and ``mean_diff``; with ``probs`` ``quantiles_a``, ``quantiles_b`` [nprob, ...]; with ``bins`` = (nbins, lo, hi)
    ``hist_a``, ``hist_b`` [..., nbins + 3] and ``info_gain_bits`` = sum over the nbins + 3 slots s of pA_s log2(pA_s /
    pB_s) with p_s = (c_s + 0.5) / (M + 0.5 (nbins + 3)), formed on the host from the integer histograms; ``x``,
    ``y``, ``z``, ``MA``, ``MB``.  A p-value needs the effective sample sizes (``posterior_volume(convergence=True)``
    per side) and is the caller's.  Computed on the device as one ensemble of MA + MB models, slab by slab
    (td_rasterize_compare / td_history_compare)."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    probs = () if probs is None else probs
    (ma, la), (mb, lb) = _chains(model_hist_a), _chains(model_hist_b)
    MA, MB = sum(la), sum(lb)
    if _on_device(ma) and _on_device(mb):
        r = ctx.compare_history(ma, mb, qx, qy, qz, exceed, probs, bins)
    else:
        ma, mb = ([m for h in s for m in h.read()] if _on_device(s) else s for s in (ma, mb))
        r = ctx.compare([m.cells() for m in ma], [m.cells() for m in mb], qx, qy, qz, exceed, probs, bins)
    out = {"x": xv, "y": yv, "z": zv, "MA": MA, "MB": MB}
    r.update(compare_summary(r, MA, MB))
    for f, a in r.items():
        if a is None:
            continue
        if f in ("hist_a", "hist_b"):
            out[f] = a.reshape(shape + (a.shape[1],)).transpose(2, 1, 0, 3).copy()
        else:
            out[f] = _grid(a, shape)
    return out


def _node_weights(weights, xv, yv, zv, shape):
    """``weights`` of the ensemble calls on a lattice as the device reads them (x fastest), or None: "volume" ->
    ``voxel_weights``; None; an array [nx, ny, nz]."""
    if isinstance(weights, str):
        if weights != "volume":
            raise ValueError("weights: 'volume', None or an array [nx, ny, nz]")
        weights = voxel_weights(xv, yv, zv)
    if weights is None:
        return None
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != shape[::-1]:
        raise ValueError("weights must be [nx, ny, nz] = %s; got %s" % (shape[::-1], w.shape))
    return w.transpose(2, 1, 0).ravel()


def _thinned(model_hist, thin):
    """``_chains`` with every ``thin``-th sample of each chain kept (the first one included).  Histories are swept
    where they lie and cannot be read with a stride: ``thin`` > 1 is refused for them."""
    thin = int(thin)
    if thin < 1:
        raise ValueError("thin must be >= 1")
    models, lens = _chains(model_hist)
    if thin == 1:
        return models, lens
    if _on_device(models):
        raise ValueError("thin > 1 on device histories: a History is swept where it lies, every sample of it; record "
                         "thinner (keep_each, or run_recorded's `every`) or pass the Models read back")
    kept, klens, pos = [], [], 0
    for n in lens:
        part = models[pos:pos + n:thin]
        kept += part
        klens.append(len(part))
        pos += n
    return kept, klens


def distance_summary(dist2, wsum, lens):
    """``ensemble_distances``' numbers from the matrix of squared distances dist2 [M, M], the weights' sum and the
    chains' lengths (pure numpy).  -> dict: ``dist`` = sqrt(dist2 / wsum); ``row_mean`` [M], a sample's mean distance
    to the OTHER samples (0 for a single sample); ``medoid``, the argmin of the row sums of dist, the first index on
    ties (a row whose sum is NaN never wins); ``chain_of`` [M]; ``chain_distance`` [C, C], the mean of dist over a in
    chain c and b in chain d with a != b (NaN within a chain of one sample)."""
    d2 = np.asarray(dist2, dtype=np.float64)
    M = len(d2)
    lens = [int(n) for n in lens]
    if sum(lens) != M:
        raise ValueError("the chains' lengths must sum to the samples (%d); got %s" % (M, lens))
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.sqrt(d2 / np.float64(wsum))
    rows = dist.sum(axis=1)
    medoid = int(np.argmin(np.where(np.isnan(rows), np.inf, rows)))
    chain_of = np.repeat(np.arange(len(lens)), lens)
    edges = np.concatenate(([0], np.cumsum(lens)))
    C = len(lens)
    cd = np.full((C, C), np.nan)
    for c in range(C):
        for d in range(C):
            blk = dist[edges[c]:edges[c + 1], edges[d]:edges[d + 1]]
            if c != d:
                pairs, total = blk.size, blk.sum()
            else:
                pairs, total = blk.size - len(blk), blk.sum() - np.trace(blk)
            if pairs > 0:
                cd[c, d] = total / pairs
    return {"dist": dist, "medoid": medoid, "row_mean": rows / (M - 1) if M > 1 else np.zeros(M), "chain_of": chain_of,
            "chain_distance": cd}


def ensemble_distances(model_hist, dataStruct, TD_parameters, weights="volume", thin=1, xs=None, ys=None, zs=None):
    """Which sample represents the ensemble, and do the chains sample the same part of model space?  The mean of
    Voronoi models is not a Voronoi model: what can be published is a member, the medoid.  On the lattice ``xs`` x
    ``ys`` x ``zs`` (default: dataStruct.xVec / yVec / zVec) with a node's weight its voxel's volume
    (``weights="volume"``; None: every node 1; or an array [nx, ny, nz] >= 0) -> dict: ``dist`` [M, M], the RMS
    difference of two samples' volumes in zeta units, sqrt(dist2 / sum(w)); ``medoid``, the index of the sample with
    the smallest summed distance to the others (the first on ties); ``row_mean`` [M]; ``chain_distance`` [C, C], the
    mean distance between samples of chain c and chain d (a != b) -- chains that mix have off-diagonal entries like
    the diagonal's; ``chain_of`` [M]; ``weight_sum``; ``mean``, ``std`` [nx, ny, nz] (``posterior_volume``'s).
    ``thin`` keeps every thin-th sample of each chain (Model lists only; histories are swept whole).  Same inputs as
    ``posterior_volume``; the M x M matrix is formed on the device slab by slab (td_rasterize_gram / td_history_gram)
    and M is at most 11585."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    w = _node_weights(weights, xv, yv, zv, shape)
    models, lens = _thinned(model_hist, thin)
    if _on_device(models):
        r = ctx.gram_history(models, qx, qy, qz, w, want=("dist2",))
    else:
        r = ctx.gram([m.cells() for m in models], qx, qy, qz, w, want=("dist2",))
    out = distance_summary(r["dist2"], r["wsum"], lens)
    out.update(weight_sum=r["wsum"], x=xv, y=yv, z=zv, mean=_grid(r["mean"], shape), std=_grid(r["std"], shape))
    return out


def pattern_summary(gram, k=8):
    """``posterior_patterns``' eigen step on the Gram matrix [M, M] of the centred samples (pure numpy,
    numpy.linalg.eigh).  -> dict: ``eigenvalues`` [k] (the largest first, k at most M), ``vectors`` [M, k] with each
    eigenvector's component of largest magnitude positive (the first such index on ties), ``scores`` [M, k] = vectors
    * sqrt(max(eigenvalue, 0)), ``explained`` = eigenvalues / trace(gram), ``participation`` = (sum lambda)^2 / sum
    lambda^2 over all M eigenvalues: the number of patterns that carry the variance."""
    G = np.asarray(gram, dtype=np.float64)
    M = len(G)
    k = max(0, min(int(k), M))
    lam, U = np.linalg.eigh(G)
    lam, U = lam[::-1], U[:, ::-1]
    Uk = U[:, :k].copy()
    for j in range(k):
        if Uk[int(np.argmax(np.abs(Uk[:, j]))), j] < 0:
            Uk[:, j] = -Uk[:, j]
    with np.errstate(invalid="ignore", divide="ignore"):
        explained = lam[:k] / np.trace(G)
        participation = float(np.sum(lam) ** 2 / np.sum(lam * lam))
    return {"eigenvalues": lam[:k].copy(), "vectors": Uk, "scores": Uk * np.sqrt(np.maximum(lam[:k], 0.0)),
            "explained": explained, "participation": participation}


def posterior_patterns(model_hist, dataStruct, TD_parameters, k=8, weights="volume", thin=1, xs=None, ys=None, zs=None):
    """Which whole-volume patterns does the data leave undetermined -- the wedge trading against the slab, a depth
    smear?  The principal components of the ensemble on the lattice ``xs`` x ``ys`` x ``zs`` (default:
    dataStruct.xVec / yVec / zVec), a node weighing its voxel's volume (``weights`` as for ``ensemble_distances``).
    The M x M Gram matrix of the centred samples is formed on the device (td_rasterize_gram / td_history_gram); its
    eigen-decomposition is the host's (numpy.linalg.eigh: LAPACK's time, O(M^3), is not the device's -- 9.3 s at M = 10^4
    beside 0.45 s for the matrix where DESIGN 4.6o measured both).  -> dict: ``eigenvalues`` [k]; ``explained`` [k] =
    eigenvalue / trace; ``participation``; ``scores`` [M, k], one number per sample and pattern (unit eigenvector
    times sqrt(eigenvalue), signs fixed as in ``pattern_summary``), shaped for ``posterior_covariance(series=...)``;
    ``patterns`` [k, nx, ny, nz], the regression of zeta at every node on a score, cov / std(score): zeta per sigma of
    the score; ``corr`` [k, nx, ny, nz]; ``score_std`` [k]; ``mean``, ``std`` [nx, ny, nz]; where every chain
    holds at least 4 samples ``rhat``, ``ess``, ``lags`` [k], each score's split R-hat and effective
    sample size (td_convergence_values): model-space mixing in k numbers; ``chain_of`` [M]; ``x``, ``y``, ``z``.
    ``thin`` as for ``ensemble_distances``.  The maps come from the existing covariance call with ``series=scores``."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature; the lattice decides everything here)
    xv, yv, zv, shape, qx, qy, qz = _lattice(dataStruct, xs, ys, zs)
    w = _node_weights(weights, xv, yv, zv, shape)
    models, lens = _thinned(model_hist, thin)
    if _on_device(models):
        r = ctx.gram_history(models, qx, qy, qz, w, want=("gram",))
    else:
        r = ctx.gram([m.cells() for m in models], qx, qy, qz, w, want=("gram",))
    out = pattern_summary(r["gram"], k)
    del out["vectors"]
    cov = posterior_covariance(models, dataStruct, TD_parameters, None, series=out["scores"], xs=xv, ys=yv, zs=zv)
    sd = cov["target_std"]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["patterns"] = cov["cov"] / sd[:, None, None, None]
    out.update(corr=cov["corr"], score_std=sd, mean=cov["mean"], std=cov["std"], x=xv, y=yv, z=zv,
               chain_of=np.repeat(np.arange(len(lens)), lens), weight_sum=r["wsum"])
    if out["scores"].shape[1] > 0 and min(lens) >= 4:
        c = ctx.convergence(out["scores"], lens)
        out.update(rhat=c["rhat"], ess=c["ess"], lags=c["lags"])
    return out


def posterior_predictive(model_hist, dataStruct, TD_parameters, probs=(0.05, 0.5, 0.95), bins=None, convergence=False,
                         values=False, max_lag=0):
    """Does the ensemble fit the data, ray by ray, and does it predict data it was not fitted to?  Every
    model's forward t* on the rays of ``dataStruct`` -- which may differ from the one the ensemble was
    sampled with: held-out rays, re-picked data, another allSig -- in one sweep on the device
    (td_rasterize_predict / td_history_predict).  Same inputs as ``posterior_volume`` (Models, nested lists, a
    ``History`` or a list of them, recorded on any context of the device).  -> dict: ``phi`` [nmodels], each
    model's chi^2 against dataStruct.tS / allSig; ``mean``, ``std`` [n] of the predicted t* over the models;
    ``quantiles`` [nprob, n]; ``hist`` [n, nbins + 3] with ``bins`` = (nbins, lo, hi); with ``convergence``
    ``rhat``, ``ess``, ``lags`` [n] and ``summary`` as in ``convergence_maps``; with ``values`` ``ptS``
    [nmodels, n]; ``residual`` = (mean - tS) / allSig; and, with at least two ``probs``, ``coverage``: the
    share of rays whose observed tS lies within the outermost pair of quantiles."""
    ctx = context_for(dataStruct)  # (TD_parameters: the siblings' signature)
    models, lens = _chains(model_hist)
    if _on_device(models):
        r = ctx.predict_history(models, probs, bins, convergence, max_lag, values)
    else:
        r = ctx.predict([m.cells() for m in models], probs, bins, lens if convergence else None, max_lag, values)
    tS = np.asarray(dataStruct.tS, dtype=np.float64).ravel()
    sig = np.asarray(dataStruct.allSig, dtype=np.float64).ravel()
    out = {"phi": r["phi"], "mean": r["mean"], "std": r["std"], "residual": (r["mean"] - tS) / sig}
    q = r["quantiles"]
    if q is not None:
        out["quantiles"] = q
        if len(q) >= 2:
            lo, hi = q[int(np.argmin(np.ravel(probs)))], q[int(np.argmax(np.ravel(probs)))]
            out["coverage"] = float(np.mean((tS >= lo) & (tS <= hi))) if len(tS) else float("nan")
    if r["hist"] is not None:
        out["hist"] = r["hist"]
    if values:
        out["ptS"] = r["ptS"]
    if convergence:
        out.update(rhat=r["rhat"], ess=r["ess"], lags=r["lags"],
                   summary=_conv_summary(r["rhat"], r["ess"], r["lags"], lens))
    return out


def trace_diagnostics(histories, max_lag=0):
    """R-hat / ESS / lags of the two scalar traces of a ``History`` or a list of them (one chain each):
    {"phi": {rhat, ess, lags}, "ncells": {...}}, through td_convergence_values with two columns."""
    if hasattr(histories, "read_arrays"):
        histories = [histories]
    histories = [h for h in histories if len(h) > 0]
    traces = [h.traces() for h in histories]
    r = histories[0].ctx.convergence(np.concatenate(traces), [len(t) for t in traces], max_lag)
    return {name: {f: r[f][k].item() for f in ("rhat", "ess", "lags")} for k, name in enumerate(("phi", "ncells"))}
