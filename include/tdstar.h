/*
 * tdstar.h -- C ABI of the MI355X-native t* forward model (libtdstar.so).
 *
 * Drop-in boundary for the per-proposal hot path of the rj-MCMC Voronoi t*
 * tomography in Geronimorz/MCMC-in-Tonga (Julia).  Each entry point names the
 * reference interface it replaces (file:line in the reference tree).  The
 * signatures use plain pointers and sizes only, so a Julia `ccall`, a Python
 * `ctypes` binding or a C/C++ host can call them unchanged.
 *
 * Conventions
 *  - All arrays are FP64 unless noted; ray arrays keep the reference's
 *    DataStruct layout: rayX/rayY/rayZ are m x n COLUMN-MAJOR (ray i = column
 *    i), tail-padded with NaN; rayL/rayU are (m-1) x n (DefStruct.jl:24-28).
 *  - Cell indices crossing the ABI are 0-based (Julia adds 1); -1 = "no cell
 *    closer than the 1e9 sentinel" (MCsub.jl:249-250: v_nearest returns 0.0).
 *  - Every call returns a td_status; on error the message is available from
 *    td_last_error(ctx) (td_last_error(NULL) for td_create failures, per
 *    thread).  No C++ exception crosses the ABI.
 *  - A context is bound to one device, owns one HIP stream, is NOT thread-
 *    safe (one context per Julia worker process, main_inversion.jl:15), and
 *    every call is synchronous: outputs are valid on return.
 *  - Host buffers are owned by the caller and only read/written during the
 *    call.  Ray geometry is copied to device memory once, at td_create.
 */
#ifndef TDSTAR_H
#define TDSTAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: td_info gained num_cus (its size changed) */
#define TDSTAR_ABI_VERSION 2

typedef struct td_ctx td_ctx;
typedef struct td_chain td_chain;

typedef enum td_status {
    TD_OK = 0,
    TD_ERR_ARG = 1,    /* bad pointer / size / option */
    TD_ERR_LAYOUT = 2, /* NaN padding of rayX and rayL disagree (Julia: DimensionMismatch) */
    TD_ERR_HIP = 3,    /* HIP runtime error (message names the call) */
    TD_ERR_NOMEM = 4,
    TD_ERR_BOUNDS = 5  /* Y/Z shorter than npoints (Julia: BoundsError) */
} td_status;

/* ------------------------------------------------------------------------
 * Context: device-resident copy of DataStruct's hot fields.
 * Replaces the device half of load_data_Tonga.jl:59-81 (rayX/Y/Z, rayL/U,
 * tS, allSig).  Validates the NaN layout: for every ray, the number of
 * leading non-NaN entries of rayL must equal max(npoints-1, 0) where npoints
 * is the number of leading non-NaN entries of rayX (MCsub.jl:150,312-316).
 * n may be 0.  device < 0 selects the current HIP device.
 * ------------------------------------------------------------------------ */
int td_create(td_ctx **out, int device, const double *rayX, const double *rayY, const double *rayZ,
              const double *rayL, const double *rayU, int64_t m, int64_t n, const double *tS,
              const double *allSig);
int td_destroy(td_ctx *ctx);
const char *td_last_error(const td_ctx *ctx);

typedef struct td_info {
    int32_t abi_version;
    int32_t device;
    int64_t m, n;         /* DataStruct.rayX size */
    int64_t npoints;      /* P: valid ray points over all rays */
    int64_t nsegments;    /* S = P - (rays with >= 1 point) */
    double likelihood;    /* the MCsub.jl:179 constant for the current allSig */
    char arch[32];        /* e.g. "gfx950" */
    int32_t num_cus;      /* compute units: td_chain_run_batch packs two chains per CU beyond this many */
} td_info;
int td_get_info(const td_ctx *ctx, td_info *info);

/* Per-kernel device timing with HIP events recorded on the context's stream
 * around every launch (off by default; used by bench.py for the roofline).
 * Kernel names: "nn_partial", "nn_merge", "ray_sums", "chi2", "chain_run",
 * "history_pack" (a recorded ladder's slots packed, td_rounds_*_recorded).
 * td_timing_get waits for the recorded events and returns the launch count
 * and summed duration since the last reset. */
int td_timing_enable(td_ctx *ctx, int enable);
int td_timing_reset(td_ctx *ctx);
int td_timing_get(td_ctx *ctx, const char *kernel, int64_t *launches, double *total_ms);

/* Replaces DataStruct.allSig (DefStruct.jl:10) for action 5
 * (TD_inversion_function.jl:252-261); n values. */
int td_set_sigma(td_ctx *ctx, const double *allSig);

/* td_evaluate's incremental path (below): 2 (default) = a resident kernel
 * answers every call through a mailbox in pinned host memory; 1 = one launch
 * per call; 0 = every call a full evaluate.  A resident kernel occupies its
 * stream's hardware queue, so one kept alive while the caller runs other GPU
 * work (another context, a collective on another stream) can hold that work
 * back until its 200 ms idle watchdog.  The library stops this thread's
 * resident kernels before any call that launches other work; a caller that
 * interleaves its OWN GPU work with td_evaluate calls (e.g. an allgather
 * between evaluates: a ray-sharded run) should select mode 1. */
int td_set_incremental(td_ctx *ctx, int mode);

/* ------------------------------------------------------------------------
 * evaluate -- replaces MCsub.jl:123-185 `evaluate(model, dataStruct,
 * TD_parameters)` (interp_style 1, MCsub.jl:326-327).
 *   cells: Model.xCell/yCell/zCell/zeta (DefStruct.jl:34-37), nCells long,
 *          in Julia order (tie-breaks follow it).
 *   debug_prior == 1: phi = likelihood = 1, nothing else written
 *          (MCsub.jl:134-136).
 *   ptS_out[n]   -> Model.ptS (MCsub.jl:174)         (nullable)
 *   phi_out      -> Model.phi (MCsub.jl:169-173)     (nullable)
 *   likelihood_out -> Model.likelihood (MCsub.jl:179-182) (nullable)
 *   nearest_out[P] -> 0-based cell chosen for every valid ray point, ray-major
 *          (what v_nearest computes but never returns)  (nullable)
 * phi is the sequential chi^2 of MCsub.jl:170-172 and ptS uses Julia's sum
 * association (oracle/README.md), so both are bit-exact to the CPU oracle.
 * Incremental path: when the cells are the previous call's model (or the model
 * before it) plus ONE reference-shaped edit -- an appended cell (birth,
 * TD_inversion_function.jl:85-88), a deleted one (death, :132-135), one new
 * zeta (change, :189) or one new site (move, :234-236) -- and nearest_out is
 * NULL, the context evaluates only what the edit changes on a device-resident
 * copy of the chain state (the DEVICE engine's algorithm); the results are
 * bit-identical to the full evaluate.  Other calls evaluate in full.
 * ------------------------------------------------------------------------ */
int td_evaluate(td_ctx *ctx, const double *xCell, const double *yCell, const double *zCell,
                const double *zeta, int64_t nCells, int debug_prior, double *ptS_out, double *phi_out,
                double *likelihood_out, int32_t *nearest_out);

/* The chi^2 and likelihood of MCsub.jl:169-182 for a caller-given ptS of n
 * rays (tS, allSig: the n data and errors): phi = the sequential
 * sum_k ((ptS-tS)[k]^2 * 1.0) / allSig[k]^2, computed on the device exactly as
 * td_evaluate's (bit for bit), and likelihood = the a5 constant in Julia's
 * sum association.  The reduction step of a ray-sharded evaluate: every rank
 * td_evaluate's a context over its own ray subset, the ptS are gathered in
 * ray order (one allgather), and phi is this call on the whole vector
 * (mcmc-in-tonga_amd/sharded.py).  tS / allSig are re-uploaded only when
 * they change between calls. */
int td_misfit(td_ctx *ctx, int64_t n, const double *ptS, const double *tS, const double *allSig, double *phi_out,
              double *likelihood_out);

/* Several models at once (independent chains / tempering replicas on one
 * GPU): model k's cells are [cell_off[k], cell_off[k+1]) of the cell arrays.
 * ptS_out is nmodels x n (row k = model k), phi_out/likelihood_out nmodels. */
int td_evaluate_batch(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                      const double *yCell, const double *zCell, const double *zeta, double *ptS_out,
                      double *phi_out, double *likelihood_out);

/* ------------------------------------------------------------------------
 * Interpolation -- replaces MCsub.jl:306-336 (interp_style 1), as called for
 * the birth/death 1-point queries (TD_inversion_function.jl:81,146) and on
 * grids (MCsub.jl:766-768,800-802).  npoints = leading non-NaN entries of X
 * (MCsub.jl:312-316); ny == 1 / nz == 1 broadcast (MCsub.jl:317-322);
 * otherwise ny, nz must be >= npoints (TD_ERR_BOUNDS).  Writes npoints
 * values to zeta_out (capacity nx) and, if non-NULL, nearest cells to
 * nearest_out and npoints to *npoints_out.
 * ------------------------------------------------------------------------ */
int td_interpolate(td_ctx *ctx, const double *xCell, const double *yCell, const double *zCell,
                   const double *zeta, int64_t nCells, const double *X, int64_t nx, const double *Y,
                   int64_t ny, const double *Z, int64_t nz, double *zeta_out, int32_t *nearest_out,
                   int64_t *npoints_out);

/* Slowness of ray points from a gridded 3-D model: pre_process_data.jl:34
 * `itp.(ix, iy, iz)` with load_3Dvel.jl:32 `interpolate((x, y, z), sn,
 * Gridded(Linear()))`.  Knots strictly increasing (>= 2 per
 * axis); values column-major nx x ny x nz (x fastest, Julia's sn[1,:,:,:]).
 * A point outside the grid (Interpolations.jl: BoundsError) gets NaN and is
 * counted in *n_outside.  Context-free (no ray geometry needed): runs on
 * `device`, synchronous.  td_last_error(NULL) on failure. */
int td_trilinear(int device, const double *xs, int64_t nx, const double *ys, int64_t ny, const double *zs,
                 int64_t nz, const double *values, const double *px, const double *py, const double *pz,
                 int64_t npts, double *out, int64_t *n_outside);

/* ------------------------------------------------------------------------
 * Posterior maps -- the numbers of plot_model_hist (MCsub.jl:753-825), not the
 * plots.  For nq query points (a cross-section: MCsub.jl:765-768 xz at y =
 * ySlice, :799-802 xy at z = zSlice) and nmodels saved models (model k's cells
 * are [cell_off[k], cell_off[k+1]) of the cell arrays, in model_hist order,
 * chain by chain, MCsub.jl:761-763):
 *   values_out[k*nq + q] = v_nearest of model k at point q   (nullable)
 *   mean_out[q] = Statistics.mean over the models            (MCsub.jl:774)
 *   std_out[q]  = Statistics.std (corrected) over the models (MCsub.jl:775)
 * with Julia's sum association for a Vector of matrices (raster.hip).
 * ------------------------------------------------------------------------ */
int td_rasterize(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                 const double *yCell, const double *zCell, const double *zeta, const double *qx,
                 const double *qy, const double *qz, int64_t nq, double *mean_out, double *std_out,
                 double *values_out);

/* ------------------------------------------------------------------------
 * rj-MCMC chain -- replaces TD_inversion_function.jl:7-305 (one chain) for
 * the three priors of define_TDstructure.jl:15 (1 uniform, the default; 2
 * normal; 3 exponential: TD_inversion_function.jl:91-119, 150-172, 194-212,
 * MCsub.jl:97-108).  The chain
 * state (cells, per-point nearest-cell cache, ptS, phi) lives in device
 * memory; proposals are evaluated incrementally (birth: one new cell vs the
 * cache; death/move: re-search only the points whose cell changed; change:
 * no search) and are bit-identical to a full evaluate of the proposed model.
 * RNG: counter-based Philox4x32-10 keyed by (seed, chain), so runs are
 * reproducible (the reference seeds from the wall clock, :13).
 * ------------------------------------------------------------------------ */
typedef struct td_chain_params {
    /* define_TDstructure.jl:1-44 fields that reach the chain */
    int32_t debug_prior;   /* 1: sample the prior (evaluate returns phi = 1) */
    int32_t sig;           /* percent (10) */
    int32_t zeta_scale;    /* 50 */
    int32_t max_cells;     /* 100 */
    int32_t min_cells;     /* 5 */
    int32_t prior;         /* 1 uniform, 2 normal, 3 exponential (TD_ERR_ARG otherwise) */
    double n_iter, burn_in, keep_each;
    /* xVec/yVec/zVec extents (DataStruct.xVec etc., min(xVec...), max(xVec...)) */
    double xmin, xmax, ymin, ymax, zmin, zmax;
    uint64_t seed;
    int32_t chain;          /* chain id (TD_inversion_function.jl:10) */
    double temperature;     /* tempering: acceptance uses phi / temperature (1 = reference) */
    int32_t engine;         /* TD_ENGINE_DEVICE (default) or TD_ENGINE_HOST */
    int64_t start_iter;     /* first iteration index (resume from a checkpoint); <= 0 means 1 */
} td_chain_params;

/* Engines: DEVICE runs the whole loop (proposal, incremental forward model,
 * accept/reject) inside one persistent GPU workgroup per td_chain_run call;
 * HOST is the reference's structure -- every proposal is a full td_evaluate
 * of the proposed model (TD_inversion_function.jl:93,141,191,238) -- kept as
 * the parity reference for the DEVICE engine. */
#define TD_ENGINE_DEVICE 0
#define TD_ENGINE_HOST 1
/* DROPIN: the host loop of HOST, calling the PUBLIC td_evaluate /
 * td_interpolate exactly as the unchanged Julia host would (td_evaluate's
 * incremental path then follows the chain on the device).  Measures the
 * drop-in boundary; same trajectory as the other two. */
#define TD_ENGINE_DROPIN 2

typedef struct td_chain_stats {
    int64_t iterations;        /* proposals drawn so far */
    int64_t evaluations;       /* forward-model evaluations performed */
    int64_t accepted[5];       /* per action 1..4 (index 0 unused) */
    int64_t proposed[5];
    double phi;                /* current model */
    int64_t ncells;
    int64_t bytes;             /* DEVICE engine: algorithmic global-memory bytes read by the proposals */
    int32_t last_action;       /* Model.action of the last iteration: the drawn action 1..4 (:72-73), 0 before any */
    int32_t last_accept;       /* Model.accept of the last iteration: 1 if its proposal was accepted (:74,123,...) */
} td_chain_stats;

/* Start a chain from the given model (cells may be NULL/0 to draw a starting
 * model as build_starting, MCsub.jl:76-121). */
int td_chain_create(td_chain **out, td_ctx *ctx, const td_chain_params *params, const double *xCell,
                    const double *yCell, const double *zCell, const double *zeta, int64_t nCells);
int td_chain_destroy(td_chain *ch);
/* Run `iterations` proposals (TD_inversion_function.jl:70-274 loop body). */
int td_chain_run(td_chain *ch, int64_t iterations);
/* Run `iterations` proposals on each of `nchains` chains of ONE context in a
 * single launch, one workgroup per chain (independent chains / tempering
 * replicas sharing a GPU: main_inversion.jl:15 pmap over chains).  Device
 * engine: one kernel; host engine: the chains run one after the other.  Each
 * chain's result is identical to td_chain_run(chain, iterations). */
int td_chain_run_batch(td_chain *const *chains, int64_t nchains, int64_t iterations);
int td_chain_stats_get(const td_chain *ch, td_chain_stats *st);
/* Copy the current model out (cells arrays capacity `cap`; *nCells receives
 * the count; ptS_out[n] nullable). */
int td_chain_get_model(const td_chain *ch, double *xCell, double *yCell, double *zCell, double *zeta,
                       int64_t cap, int64_t *nCells, double *phi, double *ptS_out);
/* Tempering: change the temperature between runs (swap step). */
int td_chain_set_temperature(td_chain *ch, double temperature);

/* ------------------------------------------------------------------------
 * Sample history -- the thinned model_hist of TD_inversion_function.jl:275-288
 * (every keep_each-th model from burn_in on), recorded in DEVICE memory while
 * the chain runs, so a whole thinned run is one launch instead of one launch
 * and one td_chain_get_model per saved model.
 *   Layout: the cells of the samples packed one after the other in four SoA
 * component arrays (x, y, z, zeta) of one stride = max_cells_total, each
 * sample's cells in Julia order; a device-resident prefix off[max_samples + 1]
 * (off[0] = 0) holds the samples' cell offsets -- the (cell_off, cells,
 * stride) form the posterior kernels take.  Per sample a header: the absolute
 * iteration index (the value ChainScalars::iter counts: a chain started at
 * start_iter = 1 saves the model after its i-th iteration with iteration i),
 * the exact phi, ncells and Model.action / Model.accept of that iteration
 * (TD_inversion_function.jl:73-74); with_ptS != 0 also ptS, [max_samples][n].
 * The per-action counters are not part of a sample: when the DEVICE engine
 * takes it the next proposal is already drawn and counted.
 *   td_history_create checks its arguments before any HIP call: max_samples
 * < 1, max_cells_total < 1 or a NULL context give TD_ERR_ARG and a message
 * (td_last_error(NULL) without a context).  td_history_clear empties the
 * history (its capacity stays).  A history belongs to its context and must be
 * destroyed before it.
 *   td_history_read: ONE bulk read of samples [first, first + count): off_out
 * [count + 1] rebased to 0; x / y / z / zeta of capacity cell_cap (TD_ERR_ARG
 * when the samples hold more cells); phi, iter, action, accept [count];
 * ptS_out [count x n] (nullable; TD_ERR_ARG if the history has no ptS).  Any
 * output may be NULL.
 * ------------------------------------------------------------------------ */
typedef struct td_history td_history;
int td_history_create(td_history **out, td_ctx *ctx, int64_t max_samples, int64_t max_cells_total, int with_ptS);
int td_history_destroy(td_history *h);
int td_history_clear(td_history *h);
int td_history_count(const td_history *h, int64_t *samples, int64_t *cells_used);
int td_history_read(td_history *h, int64_t first, int64_t count, int64_t *off_out, double *x, double *y, double *z,
                    double *zeta, int64_t cell_cap, double *phi, int64_t *iter, int32_t *action, int32_t *accept,
                    double *ptS_out);
/* td_chain_run(ch, iterations), with the model after the call's iterations
 * number first, first + every, ... (1-based; first >= 1, every >= 1; those
 * <= iterations) appended to h: the DEVICE engine's kernel writes them as it
 * goes (one launch, no host in the loop); HOST and DROPIN append from their
 * host loop (the parity twins).  The chain's trajectory, stats and end state
 * are those of the unrecorded run, and a run split over several calls (first
 * carried over) leaves the same history as one call.
 *   Capacity is checked on the host BEFORE anything runs: with new = the
 * number of samples the call takes, samples + new <= max_samples and
 * cells_used + new * (the chain's max_cells) <= max_cells_total; otherwise
 * TD_ERR_ARG with a message, nothing has run, chain and history are unchanged.
 * Nothing is ever truncated.  A history accumulates across calls (and across
 * chains of its context, one after the other).
 *   td_chain_run_batch_recorded: td_chain_run_batch with one history per chain
 * (hs[k] for chains[k]), in one launch -- the packed two-chains-per-CU kernels
 * included; a history listed twice is TD_ERR_ARG.
 *   A chain held by a running td_rounds launch is stopped first, as by every
 * other call.  A tempering ladder records the replica at ladder level 0 through
 * td_rounds_temper_recorded / td_rounds_exchange_recorded (below, with the
 * rounds); recording inside td_rounds_run, in a ladder spread over several
 * ranks and in td_evaluate's resident server is not provided. */
int td_chain_run_recorded(td_chain *ch, int64_t iterations, int64_t first, int64_t every, td_history *h);
int td_chain_run_batch_recorded(td_chain *const *chains, int64_t nchains, int64_t iterations, int64_t first,
                                int64_t every, td_history *const *hs);
/* td_rasterize on the concatenation of the histories' samples, history by
 * history in sample order (model_hist order, MCsub.jl:761-763), bit-identical
 * to td_rasterize on the models read back.  The cells reach the kernels by
 * device-to-device copies; only the offsets come from the histories' host
 * mirror.  (Where td_rasterize would take its per-model search, whose
 * bounding boxes are computed on the host, the cells are fetched and that
 * path runs.)  Every history must belong to ctx and hold >= 1 sample in all. */
int td_history_rasterize(td_ctx *ctx, td_history *const *hs, int64_t nh, const double *qx, const double *qy,
                         const double *qz, int64_t nq, double *mean_out, double *std_out, double *values_out);

/* ------------------------------------------------------------------------
 * Posterior marginals -- what a trans-dimensional ensemble is read by beyond
 * plot_model_hist's mean and std: per-node quantiles (median, credible
 * interval), per-node histograms, and the ensemble distributions of
 * plot_distribution.jl:66-80.  V[k][q] is td_rasterize's value matrix (model k
 * at point q), M = nmodels; nothing but the results leaves the device.
 *   quant_out[p*nq + q] = Statistics.quantile(V[:, q], probs[p]), Julia's
 * default (alpha = beta = 1): with v = V[:, q] sorted ascending (isless:
 * -0.0 before 0.0),
 *     aleph = M*p + (1 - p);  j = clamp(trunc(aleph), 1, max(M-1, 1));
 *     g = clamp(aleph - j, 0, 1);  a = v[j];  b = M == 1 ? v[1] : v[j+1]
 *     quantile = a + g*(b - a)                      (1-based, unfused FP64)
 * j and g are computed on the host; the device selects a and b exactly.  A
 * column that holds a NaN gives NaN at every probability (Julia throws).
 *   hist_out[q*(nbins+3) + s], with w = (hi - lo)/nbins (host, FP64), counts
 * the models whose value at q falls in slot s:
 *     0: v < lo;  1 + min((int)floor((v - lo)/w), nbins-1): lo <= v < hi;
 *     nbins+1: v >= hi;  nbins+2: NaN            -- every row sums to M.
 *   nprob 0..64 (0: no quantiles), nbins 0..4096 (0: no histogram); both 0
 * returns mean and std only.  TD_ERR_ARG, before any HIP call: want NULL, a
 * count out of range, a probability outside [0, 1] or NaN, lo/hi non-finite or
 * lo >= hi with nbins > 0, a NULL array for a non-zero count.  hi - lo must be
 * finite too (nbins > 0): (-1e308, 1e308) is refused, its w would be +inf.
 *   mean_out / std_out are td_rasterize's, bit for bit.  Columns of up to
 * 16384 models are sorted in LDS; longer ones take an exact radix select over
 * the value matrix in device memory (csrc/marginals.hip); same results.
 *   td_history_marginals is to td_rasterize_marginals what
 * td_history_rasterize is to td_rasterize.
 *   td_history_zeta_hist: the pooled histogram (same slots, nbins 1..4096) of
 * every zeta of every sample the histories hold, counted where the samples
 * lie, and, if ncells_out is non-NULL, each sample's number of cells, history
 * by history (from the histories' host mirror of the offsets).
 * ------------------------------------------------------------------------ */
typedef struct td_marginals {
    int64_t nprob; const double *probs; double *quant_out;   /* [nprob][nq]; nprob 0..64 */
    int64_t nbins; double lo, hi;       int64_t *hist_out;   /* [nq][nbins+3]; nbins 0..4096 */
} td_marginals;
int td_rasterize_marginals(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                           const double *yCell, const double *zCell, const double *zeta, const double *qx,
                           const double *qy, const double *qz, int64_t nq, double *mean_out, double *std_out,
                           const td_marginals *want);
int td_history_marginals(td_ctx *ctx, td_history *const *hs, int64_t nh, const double *qx, const double *qy,
                         const double *qz, int64_t nq, double *mean_out, double *std_out, const td_marginals *want);
int td_history_zeta_hist(td_ctx *ctx, td_history *const *hs, int64_t nh, int64_t nbins, double lo, double hi,
                         int64_t *hist_out /* nbins+3 */, int64_t *ncells_out /* one per sample, nullable */);

/* ------------------------------------------------------------------------
 * Convergence diagnostics -- whether the chains an ensemble pools sample the
 * same distribution (split Gelman-Rubin R-hat) and how many independent
 * samples a node's statistics rest on (effective sample size, Geyer's initial
 * monotone positive sequence), per column of a value matrix V[M][ncol]
 * (model-major, td_rasterize's: model k at point q), where it lies.
 *   Chains: nchains chains of lengths L_c >= 4, sum L_c = M; chain c is rows
 * [P_c, P_c + L_c).  With N = min L_c and n = N / 2 (integer), every chain
 * gives its LAST 2n rows as two sequences of n rows: sequence 2c is rows
 * [P_c + L_c - 2n, P_c + L_c - n), sequence 2c+1 the n rows after it;
 * m = 2 nchains.  T = n - 1 for max_lag 0, else min(n - 1, max_lag).
 * tau_floor = 1 / log10((double)(m n)), computed on the host.
 *   All FP64, IEEE, unfused; every sum starts at 0.0 and is sequential in the
 * stated order.  Per column and sequence s with rows x_1..x_n:
 *     mean_s = (x_1 + x_2 + ..., i ascending) / n;   d_i = x_i - mean_s
 *     var_s  = (sum_i d_i d_i, i ascending) / (n - 1)
 *     acov_s(t) = (sum_{i=1}^{n-t} d_i d_{i+t}, i ascending) / n      (t >= 1)
 * per column:
 *     W  = (sum_s var_s, s ascending) / m;     mu = (sum_s mean_s) / m
 *     Bn = (sum_s (mean_s - mu)^2) / (m - 1)
 *     vp = ((double)(n - 1) / (double)n) W + Bn
 *     rhat = sqrt(vp / W)          (plain IEEE: 0/0 NaN, x/0 +inf)
 *     A(t) = (sum_s acov_s(t), s ascending) / m;  rho(t) = 1 - (W - A(t)) / vp
 *     Pprev = 1 + rho(1); S = Pprev; last = 1; capped = true
 *     for k = 1, 2, ... while 2k + 1 <= T:
 *         P = rho(2k) + rho(2k+1)
 *         if not (P > 0): capped = false; break          (a NaN stops too)
 *         if P > Pprev: P = Pprev
 *         S = S + P; Pprev = P; last = 2k + 1
 *     tau = -1 + 2 S; if tau < tau_floor: tau = tau_floor   (NaN stays NaN)
 *     ess = (double)(m n) / tau
 *     lags = capped ? -last : last
 * A negative lags says that the cap or n ended the sum: tau is a lower bound.
 * A constant column and a column that holds a NaN give NaN, NaN.
 *   Each of rhat_out, ess_out, lags_out may be NULL; with ess_out and lags_out
 * both NULL no autocovariance is computed.  TD_ERR_ARG, before any HIP call
 * (the message, which names the entry point, through td_last_error(NULL)
 * without a context): want NULL, max_lag < 0, the three outputs all NULL,
 * nchains < 1, chain_len NULL, a length < 4, lengths that do not sum to M /
 * nmodels, m n > INT32_MAX.
 *   td_convergence_values: a host matrix (scalar traces such as phi or the
 * number of cells), uploaded through the pinned staging block.
 * td_rasterize_convergence: td_rasterize's models, the value matrix never
 * leaving the device; mean_out / std_out are td_rasterize's, bit for bit.
 * td_history_convergence is to it what td_history_rasterize is to
 * td_rasterize: one history is one chain, a history without samples is
 * skipped.  (csrc/convergence.hip; the lags are computed in rounds until
 * every column has stopped, the results do not depend on the rounds.)
 * ------------------------------------------------------------------------ */
typedef struct td_convergence {
    int64_t max_lag;                 /* >= 0; 0: up to n - 1 */
    double *rhat_out, *ess_out;      /* [ncol], each nullable */
    int32_t *lags_out;               /* [ncol], nullable */
} td_convergence;
int td_convergence_values(td_ctx *ctx, const double *values /* host [M][ncol] */, int64_t M, int64_t ncol,
                          int64_t nchains, const int64_t *chain_len, const td_convergence *want);
int td_rasterize_convergence(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                             const double *yCell, const double *zCell, const double *zeta, const double *qx,
                             const double *qy, const double *qz, int64_t nq, int64_t nchains,
                             const int64_t *chain_len, double *mean_out, double *std_out,
                             const td_convergence *want);
int td_history_convergence(td_ctx *ctx, td_history *const *hs, int64_t nh, const double *qx, const double *qy,
                           const double *qz, int64_t nq, double *mean_out, double *std_out,
                           const td_convergence *want);

/* ------------------------------------------------------------------------
 * Posterior volumes -- the numbers above at every node of a lattice
 * xVec x yVec x zVec (or of any node list), whatever its size: what the
 * posterior of a 3-D tomography is read, exported and compared as.
 *   td_rasterize_volume takes td_rasterize's models (nchains / chain_len are
 * read only with conv), td_history_volume the samples of the histories,
 * history by history, where they lie (one history with samples = one chain;
 * one without samples is skipped).  A lattice is sent x fastest.
 *   Contract.  Every output at node q equals, bit for bit, what td_rasterize /
 * td_rasterize_marginals / td_rasterize_convergence (or the td_history_*
 * forms) return for the same models and that node: the nearest cell is the
 * lexicographic minimum of (FP64 squared distance, cell index) below the 1e9
 * sentinel, a NaN never wins, a model that answers nothing gives 0.0, and the
 * statistics are those entry points' own kernels'.  values_out (nullable:
 * small volumes, tests) is td_rasterize's value matrix [nmodels][nq]; marg
 * (nullable) and conv (nullable) are td_marginals / td_convergence with
 * quant_out [nprob][nq], hist_out [nq][nbins+3] and outputs [nq].
 *   nq is 64-bit and no product nq x nmodels is formed in 32 bits; the only
 * limit is memory (the outputs, the models and one slab).  One search
 * structure is built for all models -- per model a bucket grid of about
 * nCells / 2 buckets over the cells' box, the cells counting-sorted into one
 * compact array of 32 B per cell -- and the nodes are swept in slabs of the
 * largest multiple of 64 nodes whose value matrix fits 1 GiB (at least 64), so
 * the value matrix never exists whole.  The results do not depend on the slab
 * size, on the order the sort leaves inside a bucket, or on which sweep runs
 * (models of few cells are swept by td_rasterize's brute-force kernel).
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context): vol NULL, nq < 0, a
 * NULL qx / qy / qz / mean_out / std_out for nq > 0, what td_marginals and
 * td_convergence reject (above), chain lengths that do not fit the models.
 * nq == 0 returns TD_OK.  (csrc/volume.hip)
 * ------------------------------------------------------------------------ */
typedef struct td_volume {
    const double *qx, *qy, *qz; int64_t nq;   /* any node list; a lattice is sent x fastest */
    double *mean_out, *std_out;               /* [nq] */
    double *values_out;                       /* [nmodels][nq], nullable (small volumes, tests) */
    const td_marginals *marg;                 /* nullable; quant_out [nprob][nq], hist_out [nq][nbins+3] */
    const td_convergence *conv;               /* nullable; outputs [nq] */
} td_volume;
int td_rasterize_volume(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                        const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                        const int64_t *chain_len /* used with conv */, const td_volume *vol);
int td_history_volume(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_volume *vol);

/* ------------------------------------------------------------------------
 * Posterior predictive data -- whether an ensemble fits the data, ray by ray,
 * and predicts data it was not fitted to: every model's predicted t* on the
 * rays of ctx, its chi^2 against ctx's tS / allSig, and the statistics of the
 * matrix ptS[nmodels][n] over the models, in one sweep on the device.
 *   td_rasterize_predict takes td_rasterize's models (nchains / chain_len are
 * read only with conv), td_history_predict the samples of the histories,
 * history by history, where they lie (one history with samples = one chain;
 * one without samples is skipped).  The context names the rays -- they may be
 * a held-out set, re-picked data or another allSig -- and the histories name
 * the ensemble: a history need NOT belong to ctx, it must only live on ctx's
 * device (else TD_ERR_ARG); only its cell buffers and offsets are read.
 *   Contract.  Row k of ptS_out and phi_out[k] equal td_evaluate of model k on
 * ctx, bit for bit: the nearest cell of a ray point is the lexicographic
 * minimum of (FP64 squared distance, cell index) below the 1e9 sentinel, a NaN
 * never wins, a point with no answer takes zeta = 0; a ray's segment terms and
 * their sum are td_evaluate's (Julia's Base.sum association, every length
 * class); chi^2 is the sequential sum in ray order (MCsub.jl:170-172, see
 * td_misfit; td_set_sigma is honoured).  A model of 0 cells and a context of
 * 0 rays give what td_evaluate_batch gives.  mean_out / std_out, marg and conv
 * are td_rasterize's, td_marginals' and td_convergence's own kernels on the
 * matrix ptS[nmodels][n] as a value matrix (column = ray): their numbers are
 * what td_convergence_values and the section calls return for that matrix.
 *   No product of models x points or models x rays is formed in 32 bits; a ray
 * of more than 2^18 points is TD_ERR_ARG; the only other limit is memory (the
 * models, ptS[nmodels][n] and one slab).  The search structure is the posterior
 * volumes' (one bucket grid per model, built once; tdt_set_volume_method is
 * honoured), the queries are ctx's ray points, already on the device, swept in
 * slabs of whole rays and, where the budget asks for it, in chunks of models.
 * The results depend on neither.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: out
 * NULL; nothing asked for (every output NULL, no marg, no conv); only one of
 * mean_out / std_out; what td_marginals and td_convergence reject (above);
 * offsets not monotone; chain lengths that do not fit the models; no model or
 * no sample in all; ctx NULL.  (csrc/predict.hip)
 * ------------------------------------------------------------------------ */
typedef struct td_predict {
    double *ptS_out;              /* [nmodels][n], nullable: every model's predicted t* (row k = model k)       */
    double *phi_out;              /* [nmodels], nullable: every model's sequential chi^2 against the context's  */
                                  /*            tS / allSig (td_set_sigma is honoured)                          */
    double *mean_out, *std_out;   /* [n], nullable (both or neither): over the models, per ray                  */
    const td_marginals *marg;     /* nullable; quant_out [nprob][n], hist_out [n][nbins+3]                      */
    const td_convergence *conv;   /* nullable; outputs [n] (R-hat / ESS of each ray's predicted t*)             */
} td_predict;
int td_rasterize_predict(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                         const double *yCell, const double *zCell, const double *zeta, int64_t nchains,
                         const int64_t *chain_len /* used with conv */, const td_predict *out);
int td_history_predict(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_predict *out);

/* ------------------------------------------------------------------------
 * Posterior covariance -- what trades off against what: the covariance and
 * the correlation, over the models of an ensemble, between zeta at a few
 * targets and zeta at every node of a lattice (or of any node list).  It is
 * the ensemble's own point-spread function: when zeta at the target goes up
 * across the samples, where does it go down, and how far does that reach.
 *   td_rasterize_covariance takes td_rasterize's models, td_history_covariance
 * the samples of the histories, history by history, where they lie (one
 * without samples is skipped; a history need not belong to ctx, it must only
 * live on ctx's device).  A lattice is sent x fastest.
 *   Contract (M = the number of models).  v_q[k] is model k's nearest-cell
 * zeta at node q, td_rasterize's value under td_rasterize's rules: the
 * lexicographic minimum of (FP64 squared distance, cell index) below the 1e9
 * sentinel, a NaN never wins, no answer gives 0.0.  a_t[k] is the series of
 * target t: for a target point (tx, ty, tz) the nearest-cell value there, by
 * the same sweep; else column t of series[M][nseries] (row = model: the
 * layout of ptS_out and values_out, so a ray's predicted t*, the phi trace or
 * the nCells trace can be handed in as it is).  m_q, s_q, m_t, s_t are
 * td_rasterize's mean and sigma of those columns, from the same kernel
 * (mean_out / std_out equal td_rasterize_volume's).  Then
 *   cov[t][q]  = S / (M - 1), S = the sum over k of (v_q[k] - m_q)(a_t[k] - m_t)
 * in td_rasterize's association (M < 16: left to right; else pairwise halves
 * at mid = (lo + hi) >> 1 down to blocks of at most 1024, each block left to
 * right), without FMA: each difference and each product is rounded once; and
 *   corr[t][q] = cov[t][q] / (s_q * s_t), the product formed first, nothing
 * clamped (a value 1 ulp beyond +-1 stays as it is).  M = 1 gives NaN, as
 * sigma does; a zero sigma gives what the division gives; a NaN in a series
 * gives a NaN row.  Output rows: the points first, then the series.
 *   nq is 64-bit and no product with nmodels or nt + nseries is formed in 32
 * bits; more than 2^25 models are TD_ERR_ARG.  The search structure and the
 * slabs are the posterior volumes' (the value matrix never exists whole;
 * tdt_set_volume_slab_nodes, _method and _counting are honoured) and the
 * results depend on none of them.
 *   TD_ERR_ARG, before any HIP call (the message, which names the entry
 * point, through td_last_error(NULL) without a context), in this order: cov
 * NULL; nq, nt or nseries < 0; nt + nseries == 0; cov_out and corr_out both
 * NULL; a NULL coordinate array for a positive count; series NULL with
 * nseries > 0; only one of mean_out / std_out or of tmean_out / tstd_out;
 * offsets not monotone; no model or no sample in all; a history on another
 * device; ctx NULL.  nq == 0 returns TD_OK (tmean_out / tstd_out are still
 * written).  (csrc/covariance.hip)
 * ------------------------------------------------------------------------ */
typedef struct td_covariance {
    const double *qx, *qy, *qz; int64_t nq;     /* any node list; a lattice is sent x fastest          */
    const double *tx, *ty, *tz; int64_t nt;     /* target points, nullable when nt == 0                */
    const double *series;       int64_t nseries;/* host [nmodels][nseries], nullable when nseries == 0 */
    double *cov_out, *corr_out;                 /* [nt + nseries][nq]; each nullable, not both         */
    double *mean_out, *std_out;                 /* [nq], nullable (both or neither)                    */
    double *tmean_out, *tstd_out;               /* [nt + nseries], nullable (both or neither)          */
} td_covariance;
int td_rasterize_covariance(td_ctx *ctx, int64_t nmodels, const int64_t *cell_off, const double *xCell,
                            const double *yCell, const double *zCell, const double *zeta, const td_covariance *cov);
int td_history_covariance(td_ctx *ctx, td_history *const *hs, int64_t nh, const td_covariance *cov);

/* ------------------------------------------------------------------------
 * Resident tempering rounds (parallel tempering; the reference's
 * chains are independent pmap workers, main_inversion.jl:15, so this is a new
 * capability): DEVICE chains of one context run in ONE launch that stays
 * resident across swap rounds.  td_rounds_run posts a round -- K proposals on
 * every chain at the given temperatures -- and returns each chain's phi after
 * it; the caller gathers the phis (across ranks: an allgather), decides the
 * swaps and passes the new temperatures to the next td_rounds_run.  No
 * launch per round; the launch returns by itself after 200 ms without a
 * round (and is started again by the next one, with identical results).
 * Every chain's trajectory equals td_chain_run of K proposals per round with
 * td_chain_set_temperature between rounds.  Any other call on these chains
 * (or any GPU work of this thread through this library) first ends the
 * launch; td_chain_stats_get's accepted/proposed counts are current after
 * that, phi and iterations after every round. */
typedef struct td_rounds td_rounds;
int td_rounds_create(td_rounds **out, td_chain *const *chains, int64_t nchains);
int td_rounds_run(td_rounds *r, int64_t K, const double *temps, double *phi_out);
int td_rounds_destroy(td_rounds *r);

/* The swap step of parallel tempering (replaces mcmc-in-tonga_amd/tempering.py
 * decide_swaps, the same decision bit for bit): R replicas, phis[g] and
 * levels[g] of replica g (gathered over all ranks), temps[l] the ladder.  In
 * round rnd the level pairs (l, l+1), l = rnd mod 2, 2 + rnd mod 2, ... are
 * tried with u = a SplitMix64 hash of (seed, rnd, l) and accepted when
 * log alpha = (phi_a - phi_b)(1/(2T_l) - 1/(2T_l+1)) >= 0 or log u < log alpha
 * (a at level l, b at l+1).  new_levels[R]; tried/accepted[R-1] are added to
 * (per level pair).  Host-only (no GPU). */
int td_swap_decide(int64_t R, const double *phis, const int64_t *levels, const double *temps, int64_t rnd,
                   uint64_t seed, int64_t *new_levels, int64_t *tried, int64_t *accepted);
/* M rounds of a resident tempering launch whose replicas are all its chains
 * (one process, one GPU: the gather is the identity), the swaps decided
 * between rounds by td_swap_decide -- no return to the caller per round.
 * Round j: K proposals on every chain at temps[levels[k]] (chain k = replica
 * k), then the swap step of round rnd0 + j.  levels[nchains] in/out;
 * phis_out[M x nchains] the phis of each round, levels_out[M x nchains] the
 * levels after it (both nullable); tried/accepted[nchains - 1] added to. */
int td_rounds_temper(td_rounds *r, int64_t M, int64_t K, const double *temps, int64_t *levels, int64_t rnd0,
                     uint64_t seed, double *phis_out, int64_t *levels_out, int64_t *tried, int64_t *accepted);

/* td_rounds_temper, with the T = 1 ensemble of the ladder recorded in h: the
 * sample of round j is the state of the replica that RAN the round at ladder
 * level 0 (levels[k] == 0 when the round was posted -- the level, not a compare
 * of temperatures), after the round's K-th proposal and before its swap step,
 * laid out as td_chain_run_recorded's samples are (cells in Julia order, the
 * chain's absolute iteration, the exact phi, ncells, action and accept of the
 * round's last iteration, ptS when h keeps it).  Thinning counts ROUNDS: the
 * call's rounds number first, first + every, ... (1-based; first >= 1, every
 * >= 1) are sampled, and M rounds split over several calls with `first`
 * carried over leave the history of one call.  Everything else -- every
 * replica's trajectory, stats and end state, phis_out, levels, tried /
 * accepted -- is td_rounds_temper's.
 *   Temperatures move, not models, so the recorder is another workgroup from
 * round to round: the kernel writes each sample into a slot of its own, and
 * the call ends its resident launch before it packs the slots (one small
 * kernel) and returns -- one relaunch per call, not per round.  On return h
 * holds every sample of the call; td_history_count / _read and every
 * td_history_* consumer work on it unchanged.
 *   Capacity is checked on the host BEFORE anything runs, as for
 * td_chain_run_recorded: with new = the samples the call takes and cells_each =
 * the largest of the chains' max(max_cells, cells now), samples + new <=
 * max_samples and cells_used + new * cells_each <= max_cells_total; otherwise
 * TD_ERR_ARG with a message, and the ladder, the chains and h are unchanged.
 * Also TD_ERR_ARG with a message: h NULL, h of another context, first < 1,
 * every < 1. */
int td_rounds_temper_recorded(td_rounds *r, int64_t M, int64_t K, const double *temps, int64_t *levels, int64_t rnd0,
                              uint64_t seed, double *phis_out, int64_t *levels_out, int64_t *tried, int64_t *accepted,
                              int64_t first, int64_t every, td_history *h);

/* ------------------------------------------------------------------------
 * The exchange across GPUs (one replica per GPU, an RCCL allgather
 * over xGMI for the swap step).  A td_comm is an RCCL communicator of the
 * job's ranks: rank 0 makes the id (td_comm_unique_id) and the caller ships
 * it to every rank (e.g. torch.distributed); td_comm_create blocks until all
 * ranks joined.  td_comm_allgather: count doubles from every rank, host
 * buffers (out[nranks * count], rank order). */
#define TD_COMM_ID_BYTES 128
typedef struct td_comm td_comm;
int td_comm_unique_id(uint8_t *id /* TD_COMM_ID_BYTES */);
int td_comm_create(td_comm **out, int device, int nranks, int rank, const uint8_t *id);
int td_comm_allgather(td_comm *c, const double *in, int64_t count, double *out);
int td_comm_destroy(td_comm *c);
/* M rounds of parallel tempering with no host in the loop: the chains of r
 * (this rank's replicas, replica g = rank * nchains + k; every rank holds as
 * many) run in ONE launch; after every K proposals each publishes its exact
 * phi to device memory, an allgather on the communicator's stream (issued
 * ahead, each waiting on a flag the kernel raises: hipStreamWaitValue64)
 * brings every replica's phi, and every workgroup decides the round's swaps
 * itself (td_swap_decide's rule) and takes its chain's new temperature.
 * comm NULL: one rank holds every replica (the phis meet in device memory, no
 * collective).  Same trace as td_rounds_temper over the same replicas: the
 * host replays every decision on the logged phis and fails (TD_ERR_HIP) if
 * the device's differ.  levels[R] in/out, phis_out / levels_out [M x R],
 * tried / accepted [R-1] added to (all nullable but levels); R <= 64.
 * timing_out[7] (nullable, s): the call, launch issued, exchanges enqueued;
 * per round (means, workgroup 0's wall clock): the exchange (this rank's phis
 * all in -> every phi gathered), the proposals (gathered -> its next phi),
 * the wait for the rank's slowest replica (its phi -> the rank's last); the
 * kernel's span from its first publish to its last gather. */
int td_rounds_exchange(td_rounds *r, td_comm *comm, int64_t M, int64_t K, const double *temps, int64_t *levels,
                       int64_t rnd0, uint64_t seed, double *phis_out, int64_t *levels_out, int64_t *tried,
                       int64_t *accepted, double *timing_out);

/* td_rounds_exchange with the ladder's T = 1 ensemble recorded in h, as
 * td_rounds_temper_recorded records it (same samples, same checks): the
 * workgroup that holds level 0 in a sampled round takes the sample itself.
 * ONE rank only -- comm NULL, or a communicator of one rank; several ranks give
 * TD_ERR_ARG with a message (the cold replica would wander between GPUs, which
 * needs a merged history). */
int td_rounds_exchange_recorded(td_rounds *r, td_comm *comm, int64_t M, int64_t K, const double *temps,
                                int64_t *levels, int64_t rnd0, uint64_t seed, double *phis_out, int64_t *levels_out,
                                int64_t *tried, int64_t *accepted, double *timing_out, int64_t first, int64_t every,
                                td_history *h);

#ifdef __cplusplus
}
#endif
#endif /* TDSTAR_H */
