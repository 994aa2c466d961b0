"""tstar-mi355x: MI355X-native forward model for the rj-MCMC Voronoi t* tomography
of Geronimorz/MCMC-in-Tonga.

The directory name contains dashes, so it is imported under the module name
``mcmc_in_tonga_amd`` by ``tonga.py`` at the repository root:

    import tonga; tt = tonga.load()
    ds = tt.load_data_Tonga(); prm = tt.define_TDstructrure()
    model, ds, valid = tt.evaluate(tt.random_model(1000, 2), ds, prm)

Layers: L1 types/config (defstruct, config), L2 data (data),
L3 forward model over the C ABI (forward -> libtdstar.so), L4 chain (chain).
"""
from ._lib import TD_ENGINE_DEVICE, TD_ENGINE_DROPIN, TD_ENGINE_HOST, TdError, lib  # noqa: F401
from .chain import (MAX_LAUNCH_ITERS, Chain, History, Rounds, TD_inversion_function, build_starting,  # noqa: F401
                    chain_params, main_inversion, run_batch, run_batch_recorded, run_chains, thinning)
from .config import define_TDstructrure, parameters  # noqa: F401
from .data import (CONFIGS, ak135_slowness, box, interp1, load_data_Tonga, lonlat2xy, pad_rays,  # noqa: F401
                   random_model, segments, synthetic_rays)
from .defstruct import DataStruct, Model, Ray  # noqa: F401
from .forward import Interpolation, TdContext, context_for, evaluate, v_nearest  # noqa: F401
from .tempering import Exchange, NativeComm, TemperingLadder, decide_swaps, geometric_ladder  # noqa: F401
from .posterior import (box_region, checkerboard_model, compare_summary, convergence_maps, credible_maps,  # noqa: F401
                        depth_layers, distance_summary, ensemble_distances, info_gain_bits, model_distributions,
                        pattern_summary, plot_model_hist, posterior_compare, posterior_covariance, posterior_interfaces,
                        posterior_patterns, posterior_predictive, posterior_recovery, posterior_regions, posterior_resolution,
                        posterior_support, posterior_volume, ray_density, region_points, resolution_offsets, section,
                        support_weights, synthetic_data, trace_diagnostics, voxel_weights)
from .sharded import RayShardedContext, ray_points, shard_rays, sub_datastruct  # noqa: F401
from . import jld  # noqa: F401  (save/load model.jld, main_inversion.jl:18)
