/*
 * tdstar_testing.h -- host-only hooks of libtdstar.so that expose the chain's
 * RNG, deterministic math and proposal/acceptance logic (csrc/chain_logic.h)
 * so the CPU test suite can check them without a GPU.  They compute exactly
 * what the device kernel computes (same source, __host__ __device__).
 * Not part of the drop-in boundary; no reference interface is replaced.
 */
#ifndef TDSTAR_TESTING_H
#define TDSTAR_TESTING_H
#include <stdint.h>

#include "tdstar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Philox4x32-10 block (Salmon et al. 2011; Random123 known-answer vectors). */
void tdt_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double tdt_det_log(double x);
double tdt_det_exp(double x);
/* Wichura AS241 standard-normal quantile. */
double tdt_normal_quantile(double p);
/* The 7 uniforms of one iteration: action, accept, a, b, c, zeta, index. */
void tdt_draws(uint64_t seed, uint32_t chain, uint64_t iter, double out[7]);
/* Proposal of iteration `iter` for the given model (TD_inversion_function.jl:72-236):
 * out = {action, active, valid, index, x, y, z, zeta}; czeta_birth is the
 * Interpolation value at the birth site (needed to draw zetanew). */
int tdt_propose(const td_chain_params *prm, uint64_t iter, int64_t ncells, const double *cx, const double *cy,
                const double *cz, const double *czeta, double czeta_birth, double out[8]);
/* Diagnostic: turn the DEVICE engine's per-phase s_memtime stamps on/off and
 * read the accumulated shader cycles: [0..6] phases A..G of k_chain_run
 * (draw, tiles + birth/death query, points, orphans, ray sums, chi^2 +
 * accept, commit), [8..11] whole proposals by action (birth, death, change,
 * move), [12..13] commit / next proposal, [14] proven early rejections, [15]
 * grid searches that fell back to a full scan, [16 + 10 (action-1) + j] the
 * phases split by action (j: A..F, commit, next proposal, final barrier),
 * [56 + w] phase F of wave w, [64] chi^2 tail terms, [65] chi^2 scan rounds;
 * [35] / [45] deaths / changes taken on the short road (the cell owned no ray
 * point), [55] guessed proposals adopted with the barren flag up, [25] those
 * whose flag was cleared at adoption.  Never enabled in measured runs. */
int tdt_chain_profile(td_chain *ch, int enable, int64_t out[80]);
/* LDS plan of a device chain: [0] bytes of the LDS layout (tiles, rays and
 * order mirrored), [1] bytes of the HBM layout, [2] 1 if the HBM layout holds
 * its super-tiles in LDS, [3] 1 if a free-running launch of this chain alone
 * takes the LDS layout (it fits and the chain's lds_mode is 0). */
int tdt_chain_lds(td_chain *ch, int64_t out[4]);
/* The DEVICE engine's per-slot point counts (csrc/chain_dev.h DevChain::own) against a recount of the cached
 * nearest slots: both arrays are copied back, and the number of slots whose count differs (plus the points
 * with no valid owner) is returned -- 0 when the invariant own[s] == #{q : best_s[q] == s} holds.  A negative
 * value is minus a td_status.  Needs a GPU. */
int tdt_chain_own_check(td_chain *ch);
/* The k_chain_run instance and dynamic LDS size a launch takes (csrc/chain_variant.h; host only, no
 * context).  in: [0..3] the chains' largest LDS plans small, big, half, hyb; [4..7] force_hbm, packed,
 * tiles_ok, all_auto (over the chains' lds_mode); [8] scripted, [9] some chain records, [10] exchange
 * rounds, [11] resident tempering rounds; [12] nchains, [13] num_cus, [14] the LDS budget.
 * out: [0..5] SMALL, SCRIPT, NTH, RLDS, ROUNDS, REC; [6] LDS bytes; [7] the instance's index in the
 * launcher's table, -1 if it has none (the launch would fail).  These 15 inputs reach positions 0..11. */
int tdt_chain_variant(const int64_t in[15], int64_t out[8]);
/* The same choice with the one fact tdt_chain_variant's inputs leave false: rounds_rec != 0 = the launch is a
 * recorded ladder's (td_rounds_temper_recorded / td_rounds_exchange_recorded; it counts with in[10] or in[11]
 * set).  Its instances sit at table positions >= 12. */
int tdt_chain_variant_rounds(const int64_t in[15], int rounds_rec, int64_t out[8]);
/* Launches of each k_chain_run instance by this process since it started: out[i] for table position i,
 * *n = the table's length (out has room for 32).  Host only. */
int tdt_chain_launch_counts(int64_t out[32], int *n);
/* Launches of k_draws (the draws of a whole launch precomputed ahead of k_chain_run) by this process since it
 * started.  A launch that draws inside the kernel instead -- a resident or round launch, one whose draws
 * would exceed the budget, every launch under TD_PRE_DRAWS=0 -- adds none.  Host only. */
int tdt_chain_draws_launches(int64_t *n);
/* The pack kernel of a recorded ladder (csrc/history_pack.hip) on caller-given slots: cells = host [4][stride]
 * (x, y, z, zeta rows), `count` slots of slot_cells cells from cell slot0 of every row, ncells[count] the cells
 * each slot holds (0 .. slot_cells).  On return the samples lie packed from slot0 on in every row (the cells
 * beyond them are unspecified) and off_out[0 .. count] are their offsets (off_out[0] = slot0).  The kernel
 * moves tdt_history_pack_chunk() cells per round of its block.  TD_ERR_ARG before any HIP call for slots that
 * do not fit the stride or a count outside its slot.  Needs a GPU. */
int tdt_history_pack(int device, double *cells, int64_t stride, int64_t slot0, int64_t slot_cells,
                     const int32_t *ncells, int64_t count, int64_t *off_out);
int tdt_history_pack_chunk(void);
/* Cycles of nq back-to-back nearest-cell queries through the chain's bucket grid by one wave
 * (pts: nq x {x, y, z}); mode 0: the whole query, 1: its loads only, 2: its arithmetic only.
 * out[0] = cycles, out[1] = unproven queries (full scans). */
int tdt_chain_query_lat(td_chain *ch, const double *pts, int nq, int mode, int64_t out[4]);
/* The chain's phase-B tile filter on caller boxes (FP32, SoA: x of every tile, then y, then z), FP64 tile
 * maxima and FP64 queries (x, y, z each): hit[q * nt + t] = 1 if tile t passes for query q.  mode 0: the
 * filter of the HBM layout's super-tiles; 1: the LDS layout's tile pass (tile_may_hit2). */
int tdt_tile_filter(const float *lo, const float *hi, const double *maxd, int nt, const double *queries, int nq,
                    int mode, uint8_t *hit);
/* Each query's answer from the chain's grid search (mode 0: the LDS grid copy with the global first
 * bound; 6: the descriptor-reading form): squared distance, the winning cell's value, proven (1) or
 * left to the full scan (0). */
int tdt_chain_query_answers(td_chain *ch, const double *pts, int nq, int mode, double *dist, double *value,
                            int32_t *proven);
/* The same queries with a killed and a moved cell, as a death's, a move's and the drop-in path's queries run:
 * kill[i] / moved[i] = 0-based Julia positions (-1: none), mapped to slots through the chain's order as
 * k_chain_run maps them; slot moved is taken at msite[3 i .. 3 i + 2] with the value czeta[moved].  mode 0 and 6
 * as above, 7: wave_nearest (the grid search, then the full scan of every slot if unproven).  pos[i] = the
 * winner's 0-based Julia position (-1: no cell below the 1e9 sentinel; -2: a slot no position names).
 * info = {nslots, cap, ncells, the grid's overflow flag}.  TD_ERR_ARG before any launch for a position
 * outside [-1, ncells).  Needs a GPU. */
int tdt_chain_nearest(td_chain *ch, const double *pts, const int32_t *kill, const int32_t *moved, const double *msite,
                      int nq, int mode, double *dist, double *value, int32_t *proven, int32_t *pos, int64_t info[4]);
/* The DEVICE engine's bucket grid (csrc/chain_dev.h bucket_count / buckets / bslot) against its cell arrays,
 * all copied back.  out[0] live slots found in no bucket, [1] live slots found in more than one, [2] entries
 * whose (x, y, z, zeta) differ bitwise from cx / cy / cz / czeta[slot], [3] entries in a bucket other than
 * grid_bucket(site), [4] entries that name a free slot or a slot >= nslots (plus buckets whose count is
 * outside 0 .. 32), [5] the overflow flag, [6] the largest bucket count, [7] nslots.  [0..4] are 0 while the
 * flag is clear; once it is set (a bucket was full: the chain scans every slot from then on) cells may be
 * missing from the grid, so [0] alone may be non-zero.  Needs a GPU. */
int tdt_chain_grid_check(td_chain *ch, int64_t out[8]);
/* The cross-lane primitives of csrc/wave_ops.h, one wave per row: row r of in[nrows][64] holds lane l's 64-bit
 * word at [r][l]; out[r][l] = what lane l gets back.  op 0 wave_min_u64, 1 wave_min_u64_2p, 2 wave_min_u32 of
 * the low words (zero-extended), 3 wave_xor_u64, 4 row_max_u64 (specified in lanes 15, 31, 47, 63 only),
 * 5 wave_scan_f64, 6 wave_sum_f64, 7 readlane_f64 of lane arg[r] (5..7: the words are doubles' bits).  arg is
 * read for op 7 only: TD_ERR_ARG before any HIP call unless every arg[r] is in 0 .. 63.  1 <= nrows <= 65536.
 * Needs a GPU. */
int tdt_wave_ops(int device, int op, const uint64_t *in, const int32_t *arg, int64_t nrows, uint64_t *out);
/* The chain's exact scan of every slot (csrc/chain_search.h wave_full_scan) on caller-given slot arrays
 * (stamp[cap]: < 0 = a free slot; cx, cy, cz, czeta[cap]), one wave answering nq queries q[nq][3] one after
 * another: the lexicographic minimum of (squared distance, stamp) over the slots s < nslots with stamp[s] >= 0
 * and s != skip[i], slot moved[i] taken at msite[i][0..2] (-1: none of either); a cell wins only below the 1e9
 * sentinel, else the answer is (1e9, -1, 0.0).  TD_ERR_ARG before any HIP call if nslots > cap or a skip /
 * moved lies outside [-1, cap).  Needs a GPU. */
int tdt_nearest_scan(int device, const int64_t *stamp, const double *cx, const double *cy, const double *cz,
                     const double *czeta, int64_t cap, int64_t nslots, const double *q, const int32_t *skip,
                     const int32_t *moved, const double *msite, int64_t nq, double *out_d, int32_t *out_slot,
                     double *out_z);
/* Metropolis-Hastings decision, eqs. 14-17 (:96-97, :151-152, :196, :241). */
int tdt_accept(const td_chain_params *prm, int action, double u_accept, double zeta_new, int64_t ncells, double phi,
               double phi_n, double czeta, double zeta_killed, double zetanew_death);
/* The device chain's decision pre-filter on a bracket of (phi, phi_n) (chain_logic.h decide_sure):
 * 1 = accepted at every point of [phi_lo, phi_hi] x [phin_lo, phin_hi], -1 = rejected at every point,
 * 0 = undecided (the kernel then evaluates the corners with the acceptance rule itself). */
int tdt_decide_sure(const td_chain_params *prm, int action, double u_accept, double zeta_new, int64_t ncells,
                    double phi_lo, double phi_hi, double phin_lo, double phin_hi, double czeta, double zeta_killed,
                    double zetanew_death);
/* Device engine layout: 0 (default) mirrors tiles, rays and the Julia order
 * in LDS when they fit (the 381-ray configs); 1 keeps them in HBM, the path
 * larger geometries take; 2 runs the 4-wave kernel that puts two chains on a
 * CU (td_chain_run_batch of more chains than CUs): the tiles in LDS when they
 * fit in 80 KB, else everything in HBM; 3 (testing) that kernel with
 * everything in HBM.  Same results either way. */
int tdt_chain_set_lds_mode(td_chain *ch, int mode);
/* Device engine, decisions on bounds (DESIGN.md 4.2 phase F): k > 0 takes every
 * k-th decision of a launch on the exact chi^2 sums, as a decision falling
 * inside the brackets would (the committed partial sums made exact again from
 * where accepted proposals left them, with the proposal's terms in place);
 * 0 (default) only where the brackets require it.  Same results either way. */
int tdt_chain_set_exact_every(td_chain *ch, int k);
/* td_evaluate's resident server (incremental.cpp): sleep `ms` between the
 * host's alive check and the post of every command, so the kernel's 200 ms
 * idle watchdog can fire first (the race of a descheduled host thread).  The
 * command must then be re-issued to a new launch with the same results.  0 = off. */
int tdt_set_server_post_delay(int ms);
/* The resident launches registered to the calling thread: td_evaluate's shadow servers and the launches of
 * td_rounds_*, i.e. what "the library stops this thread's resident kernels" (include/tdstar.h,
 * td_set_incremental) would stop.  0 on return from every entry point that issues other GPU work; 1 after
 * the calls documented to keep their server (td_evaluate's incremental path, the one-point td_interpolate,
 * a DROPIN chain's run) and after a round of td_rounds_run / _temper.  A launch that returned by its own
 * idle watchdog stays registered until the next call notices.  Host only. */
int tdt_resident_count(int64_t *n);
/* Resident tempering rounds (td_rounds_*): at the next launch the workgroups of
 * the listed chains return at their first wait, before the host posts the
 * round, while the others run it -- the race of a workgroup's idle watchdog
 * firing just as a round is posted.  td_rounds_run must then re-post the round
 * to a new launch in which the chains that ran it only report phi: every chain
 * runs each round once, with the results of an undisturbed launch.  One-shot;
 * ends the running launch. */
int tdt_rounds_force_exit(td_rounds *r, const int32_t *slots, int64_t nslots);
/* Testing: the drop-in path's one-point Interpolation on the host (host_nn.h: MCsub.jl:247-263 over a
 * bucket grid of the committed model).  Builds the grid from the n cells, applies edits[0..nedits) as
 * committed (6 doubles each: action 1 birth / 2 death / 3 change / 4 move, 0-based Julia index, x, y, z,
 * zeta), then answers nq points on that model plus `pending` (6 doubles, or NULL): val_out[k] and, if
 * pos_out, the winner's 0-based Julia position (-1: no cell below the 1e9 sentinel).  Host only. */
int tdt_host_nn_query(const double *x, const double *y, const double *z, const double *zeta, int64_t n,
                      const double *edits, int64_t nedits, const double *pending, const double *qx,
                      const double *qy, const double *qz, int64_t nq, double *val_out, int64_t *pos_out);

/* Testing: the bucket grid's lower bound on the host (csrc/internal.h grid_axis / grid_block_lb, the code
 * the evaluate grid, the chain's grid query and the volume sweep prove their answers with).  Makes the
 * grid of make_cell_grid(lo, hi, target, max_dim, max_buckets) and, for each of npts points, writes its
 * bucket ijk[3 p .. 3 p + 2] = (i, j, k) and lb[p] = grid_block_lb(G, x, y, z, R): a strict lower bound
 * of the FP64 squared distance to every cell whose bucket lies outside the point's (2R+1)^3 block.
 * dims, h, e (each nullable, 3 entries): the grid's buckets, bucket edges and face allowances per axis.
 * Host only. */
int tdt_grid_lb(const double lo[3], const double hi[3], double target, int max_dim, int64_t max_buckets,
                const double *px, const double *py, const double *pz, int64_t npts, int R, int32_t *ijk, double *lb,
                int32_t dims[3], double h[3], double e[3]);

/* Diagnostic: the drop-in path's wall time per stage, ns, accumulated on the
 * context (then zeroed if reset): [0] td_evaluate, [1] its model
 * classification (which state the caller's cells are an edit of), [2] its
 * resident server's round trip (post -> answer), [3] td_interpolate of one
 * point, [4] its classification, [5] its server round trip, [6] td_evaluate
 * calls, [7] 1-point td_interpolate calls, [8] full evaluates, [9] a DROPIN
 * chain's modeln copies (the host loop's deepcopy), [10] its iterations'
 * time, [11] its iterations; the full evaluate's host side: [12] cells
 * packed into pinned memory, [13] kernels issued, [14] the wait for them,
 * [15] chi^2 and copy-out; [16] the resident server's busy time by its own
 * clock (command seen -> answered), evaluate commands, [17] queries. */
int tdt_dropin_timing(td_ctx *ctx, int reset, int64_t out[18]);
/* The block-wide exact sequential sum (exact_sum.h, used for chi^2 over long
 * ray lists): prefix[k] = C0 + term[0] + ... + term[k] added strictly left to
 * right in FP64 (MCsub.jl:170-172).  *fast = 1 when the parallel path proved
 * its result (else prefix/C_end are untouched and the kernels take the
 * one-lane loop).  Needs a GPU. */
int tdt_exact_sum(int device, const double *term, int64_t cnt, double C0, double *prefix, double *C_end, int *fast);
/* The one-wave exact sequential sum (exact_sum.h wave_seq_sum, the chain's
 * chi^2 tail): same contract as tdt_exact_sum, always exact; *fallbacks =
 * 256-term chunks that needed the slower binade-by-binade path.  Needs a GPU. */
int tdt_wave_seq_sum(int device, const double *term, int64_t cnt, double C0, double *prefix, double *C_end,
                     int *fallbacks);
/* The one-wave sum after a few terms changed (exact_sum.h wave_delta_sum, the
 * chain's chi^2): prefix[k] = C0 + term[0] + ... + term[k] left to right,
 * given old_prefix (the same sums over the old terms) and changed[k] != 0
 * where term[k] differs from the old term.  Needs a GPU. */
int tdt_wave_delta_sum(int device, const double *term, const double *old_prefix, const int *changed, int64_t cnt,
                       double C0, double *prefix, double *C_end);
/* The chain's chi^2 walk (exact_sum.h delta_marks / delta_walk / delta_remark /
 * delta_commit, one 512-thread workgroup): old_prefix[0..n) are the partial
 * sums of term_old (C_{-1} = 0), term[k0..n) the new terms, changed[k] != 0
 * where they differ; prefix = the new partial sums (old ones before k0), C_end
 * = prefix[n-1], events = the terms the walk added one by one, mask_ok = the
 * event words kept across the proposal equal those of the new state.
 * n <= 65536. */
int tdt_block_delta_sum(int device, const double *term, const double *term_old, const double *old_prefix,
                        const int *changed, int64_t k0, int64_t n, double *prefix, double *C_end, int64_t *events,
                        int *mask_ok);

/* chi^2 (MCsub.jl:169-172) of a caller-given ptS[n] against the context's tS
 * and allSig, through the code that computes it in the product: path 0
 * td_evaluate's (the host adds the terms in k order where the kernel put
 * ptS), 1 the block-wide exact scan of td_misfit (k_chi2), 2 the device
 * chain's starting-state prefix sums (k_chi2_prefix), 3 the chain's
 * proposal-time one-wave scan (from k0 = 0 -> out[0], and restarted at
 * k0 = n/2 on path 2's prefix -> out[1]).  Lets the tests pin the HIP code to
 * the reference's own model.jld phi values.  1 <= n <= 4096.  Needs a GPU. */
int tdt_chi2(td_ctx *ctx, const double *ptS, int path, double out[2]);

/* td_evaluate's incremental path: 0 off (every call a full evaluate), 1 one
 * k_chain_run launch per call, 2 (default) a resident launch fed through a
 * pinned-memory mailbox (it returns by itself after 200 ms without a call).
 * Changing the mode releases the shadow chain. */
int tdt_set_incremental(td_ctx *ctx, int on);

/* Diagnostic of the resident server (mode 2): out = {shader cycles, 100 MHz
 * wall ticks} of its last evaluation (command receipt to answer), the polls of
 * the mailbox before that command arrived, 0. */
int tdt_shadow_diag(td_ctx *ctx, int64_t out[4]);
/* Diagnostic: stop the resident server and read its chain's phase stamps (as
 * tdt_chain_profile; stamps are on only with TD_SHADOW_PROFILE set). */
int tdt_shadow_profile(td_ctx *ctx, int64_t out[80]);

/* Nearest-cell method of td_evaluate / td_interpolate: 0 auto (bucket grid
 * from 256 cells on), 1 brute force (every point x every cell: the one-launch
 * tile search where the points fit a lane each per CU, else the split search),
 * 2 bucket grid, 3 brute force through the split search (k_nn_partial +
 * k_nn_merge) always.  All give the same answer (the lexicographic
 * (distance, index) minimum). */
int tdt_set_nn_method(td_ctx *ctx, int method);

/* Posterior marginals (td_rasterize_marginals).  tdt_quantile_rank: the host's part of a quantile of M
 * values at probability p, the 1-based j and the weight g of v[j+1] (include/tdstar.h); needs no GPU.
 * tdt_set_marginals_method: the regime that selects the order statistics, 0 auto (resident up to
 * tdt_marginals_resident_max models), 1 resident (columns sorted in LDS; a later call with more models
 * than it holds returns TD_ERR_ARG), 2 streaming (radix select over device memory).  Same results.
 * tdt_marginals_plan: the quantile kernel's launch for M models x nq nodes on num_cus compute units
 * (td_info.num_cus) under that method with nprob probabilities, out = {resident (0 / 1), Mp, W, threads,
 * dynamic LDS bytes}; pure host code.  Resident: a workgroup sorts a tile of W nodes x Mp keys (M rounded
 * up to a power of two) in LDS: W = min(64, 16384 / Mp), halved while W > 8 and ceil(nq / W) < 2 num_cus;
 * threads = Mp W / 2 within 64 .. 1024; 8 Mp W bytes.  Streaming: {0, 0, 1, 512, 2048 nprob} (a workgroup
 * per node).  TD_ERR_ARG where a call would refuse (method 1 beyond tdt_marginals_resident_max) and for
 * M < 1, nq < 1, num_cus < 0, nprob outside 0 .. 64. */
int tdt_quantile_rank(int64_t M, double p, int64_t *j, double *g);
int tdt_set_marginals_method(td_ctx *ctx, int method);
int tdt_marginals_resident_max(td_ctx *ctx, int64_t *M);
int tdt_marginals_plan(int64_t M, int64_t nq, int num_cus, int method, int nprob, int64_t out[5]);

/* Convergence diagnostics (td_convergence_values).  tdt_convergence_plan: what the chain lengths and
 * max_lag decide (include/tdstar.h), out = {n, m, T, first row of sequence 0}, seq_start [m] (nullable)
 * every sequence's first row, *tau_floor (nullable); pure host code, TD_ERR_ARG as the entry points.
 * tdt_set_convergence_round: the lags computed per round, 0 auto, else even and >= 2 (shrunk, not
 * below 2, while the autocovariance scratch would exceed its budget).  tdt_set_convergence_lag_block:
 * the lags one wave accumulates, 0 auto, 8 or 16.  Same results whatever either is. */
int tdt_convergence_plan(int64_t nchains, const int64_t *chain_len, int64_t max_lag, int64_t out[4],
                         int64_t *seq_start, double *tau_floor);
int tdt_set_convergence_round(td_ctx *ctx, int64_t R);
int tdt_set_convergence_lag_block(td_ctx *ctx, int LB);

/* Posterior volumes (td_rasterize_volume).  tdt_volume_plan: what (nmodels, nq), the budget in bytes of a
 * slab's value matrix (0: the default, 1 GiB) and a forced slab size (0: none) decide, out = {nodes per
 * slab, slabs}: nodes = the largest multiple of 64 with 8 nmodels nodes <= budget (forced: rounded down to
 * a multiple of 64), at least 64, at most 2^18 and 128 floor((2^31 - 1) / (8 ceil(nmodels / 8))) (one
 * launch's blocks); pure host code.  tdt_set_volume_slab_nodes: force the slab size of later calls (0:
 * auto).  tdt_set_volume_method: the sweep, 0 auto (bucket grids from a mean of 140 cells per model on),
 * 1 bucket grids, 2 td_rasterize's brute-force kernel.  Same results whatever either is.
 * tdt_volume_counters: the (model, node) pairs of the last call decided by the 3x3x3 block, by the 5x5x5
 * block, by a full scan of the model, and by the brute-force kernel.  The three grid paths are counted by
 * a second instance of the search kernel, which tdt_set_volume_counting(ctx, 1) selects for later calls
 * (same values; its atomics on three shared words take longer than the search itself): a grid sweep
 * without it reports -1, -1, -1. */
int tdt_volume_plan(int64_t nmodels, int64_t nq, int64_t budget, int64_t forced, int64_t out[2]);
int tdt_set_volume_slab_nodes(td_ctx *ctx, int64_t n);
int tdt_set_volume_method(td_ctx *ctx, int method);
int tdt_volume_counters(td_ctx *ctx, int64_t out[4]);
int tdt_set_volume_counting(td_ctx *ctx, int on);

/* Posterior predictive data (td_rasterize_predict).  tdt_predict_plan: what nmodels, the n rays' point
 * counts ray_points[n], the budget in bytes of a slab's value matrix (0: the default, 1 GiB) and the forced
 * sizes (0: none) decide; pure host code.  out = {points, chunk, slabs}: a slab is a run of whole
 * consecutive rays of at most `points` points in all and at most 2^20 rays, filled greedily ray after ray;
 * points = the largest multiple of 64 with 8 nmodels points <= budget (forced_points: rounded down to a
 * multiple of 64), at least 64, raised to the longest ray rounded up to 64, at most 2^18; the models are
 * swept `chunk` at a time: forced_chunk, else max(1, budget / (8 points)); at most nmodels and 2^19.
 * edges (nullable, room for n + 1): edges[k] .. edges[k + 1] are slab k's rays ({0} without rays).
 * TD_ERR_ARG for a ray of more than 2^18 points.  tdt_set_predict_plan: force both for later calls (0:
 * auto).  tdt_set_predict_placement: 1 runs the workgroups of model m of the ray-sum kernel on XCD m % 8
 * (0, the default: a model's workgroups follow each other).  Same results whatever any of them is.
 * tdt_volume_counters also reports a predictive call's sweeps. */
int tdt_predict_plan(int64_t nmodels, int64_t n, const int64_t *ray_points, int64_t budget, int64_t forced_points,
                     int64_t forced_chunk, int64_t out[3], int64_t *edges);
int tdt_set_predict_plan(td_ctx *ctx, int64_t slab_points, int64_t model_chunk);
int tdt_set_predict_placement(td_ctx *ctx, int xcd);

/* Posterior covariance (td_rasterize_covariance).  tdt_covariance_group: G, the targets k_cov_targets
 * keeps in registers at a time (a slab's value matrix is read once per G targets; a target count that is
 * no multiple of G gets a tail group); pure host code.  The volume hooks above (slab nodes, method,
 * counting, counters) also act on and report a covariance call's sweeps. */
int tdt_covariance_group(void);

/* Diagnostic: the nearest-cell search alone, `reps` back-to-back launches over
 * the context's ray points on the given cells (method as tdt_set_nn_method,
 * 1..3), timed by two HIP events; *us_out = microseconds per search. */
int tdt_nn_bench(td_ctx *ctx, const double *x, const double *y, const double *z, const double *zeta, int64_t ncells,
                 int method, int reps, double *us_out);

#ifdef __cplusplus
}
#endif
#endif
