// chain_resident.h -- what a resident launch of the chain kernel talks to the host with (wave 0):
// system-scope mailbox access, the server's command wait (server_wait) and its answer (server_report),
// and the two tempering-round protocols (round_wait: the host swaps; round_exchange: the kernel does).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "chain_search.h"
#include "chain_shared.h"
#include "wave_ops.h"

namespace tdstar {

namespace {

// System-scope access to the mailbox (pinned host memory, the host polls it)
__device__ __forceinline__ long long mb_load(const long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void mb_store(long long *p, long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Server mode, wave 0: wait for the next EVAL or QUIT command, answering
// QUERY commands (one-point Interpolation on the committed model or the model
// plus one edit -- the state here is the committed one, a pending proposal
// lives only in the candidate overlay) meanwhile.  EVAL: its steps into
// sh.srv_*, the pending proposal's fate into sh.gs.accept; QUIT or silence:
// sh.srv_quit (and undo).
__device__ void server_wait(Mailbox *mb, const DevChain &d, const Views &v, Shared &sh, int lane) {
    constexpr int kWords = (int)(offsetof(Mailbox, done) / sizeof(long long));
    static_assert(kWords <= 64 && kWords <= (int)(sizeof(sh.mbox) / sizeof(long long)), "mailbox payload");
    long long seen = sh.srv_seq;
    long long t0 = (long long)wall_clock64();
    if (lane == 0 && sh.srv_busy_c) {  // diagnostic: the busy interval that ends here (clock rate)
        mb_store(&mb->diag[0], clock64() - sh.srv_busy_c);
        mb_store(&mb->diag[1], t0 - sh.srv_busy_w);
    }
    static_assert(kMailboxCheckWord == kWords - 1, "the check is the command's last word");
    long long polls = 0;
    while (true) {
        // every poll reads the whole command, one word per lane (as cheap as seq alone: one round
        // trip); a new seq is taken only with a matching check -- the poll may have caught the
        // host between its words (then the next poll reads them again)
        // (no system-scope acquire: the command is read through system-scope atomics, and one
        // would invalidate this XCD's L2, the chain's working set, at every call)
        const long long w = lane < kWords ? mb_load(reinterpret_cast<const long long *>(mb) + lane) : 0;
        const long long sq = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(w >> 32), 0) << 32) |
                                         (unsigned)__builtin_amdgcn_readlane((int)w, 0));
        ++polls;
        bool fresh = sq != seen;
        if (fresh) {  // (a torn read: not yet -- the next poll reads the words again)
            const unsigned long long h =
                wave_xor_u64(lane >= 1 && lane < kWords - 1 ? mailbox_word_mix((unsigned long long)w, lane, sq) : 0ull);
            const unsigned long long chk =
                ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(w >> 32), kWords - 1) << 32) |
                (unsigned)__builtin_amdgcn_readlane((int)w, kWords - 1);
            fresh = h == chk;
        }
        if (fresh) {
            seen = sq;
            if (lane == 0) {
                sh.srv_busy_c = clock64();
                sh.srv_busy_w = (long long)wall_clock64();
                mb_store(&mb->diag[2], polls);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (lane < kWords) sh.mbox[lane] = w;
            wave_sync_lds();
            const Mailbox &c = *reinterpret_cast<const Mailbox *>(sh.mbox);
            if (c.type == kCmdQuery) {
                const double x = c.q[0], y = c.q[1], z = c.q[2];
                const bool has_edit = c.has_edit != 0;
                const ScriptStep e = c.qedit;
                int skip = -1, moved = -1, slot_k = -1;
                if (has_edit && e.action != tdchain::kBirth) slot_k = v.ord[e.index];
                if (has_edit && e.action == tdchain::kDeath) skip = slot_k;  // the reduced model (:132-135)
                if (has_edit && e.action == tdchain::kMove) moved = slot_k;  // the cell at its new site
                const Nearest r = wave_nearest(d, v, sh, lane, x, y, z, skip, moved, e.x, e.y, e.z,
                                               moved >= 0 ? d.czeta[moved] : 0.0);
                double val = r.z;
                if (has_edit && e.action == tdchain::kChange && r.s == slot_k) val = e.zeta;
                if (has_edit && e.action == tdchain::kBirth) {  // the appended cell wins only strictly (last position)
                    const double dd = dist2(e.x, e.y, e.z, x, y, z);
                    if (dd < r.d && dd < kSentinel) val = e.zeta;
                }
                if (lane == 0) {
                    mb_store(reinterpret_cast<long long *>(&mb->qval), __double_as_longlong(val));
                    __builtin_amdgcn_s_waitcnt(0);  // the answer acknowledged before done (no L2 write-back)
                    mb_store(&mb->done, sq);
                }
                wave_sync_lds();
                t0 = (long long)wall_clock64();
                continue;
            }
            if (lane == 0) {
                sh.srv_seq = sq;
                if (c.type == kCmdEval) {
                    const int ns = min(max(c.nsteps, 1), kMaxScript);
                    for (int k = 0; k < ns; ++k) sh.srv_step[k] = c.step[k];
                    sh.srv_n = ns;
                    sh.srv_k = 0;
                    sh.gs.accept = c.decision != 0 ? 1 : 0;
                    sh.srv_quit = 0;
                } else {  // quit: the pending proposal (if any) is undone
                    sh.gs.accept = 0;
                    sh.srv_quit = 1;
                }
            }
            wave_sync_lds();
            return;
        }
        if ((long long)wall_clock64() - t0 > kServerIdleTicks) {  // no host: undo and return
            if (lane == 0) {
                sh.gs.accept = 0;
                sh.srv_quit = 1;
            }
            wave_sync_lds();
            return;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// Resident tempering rounds, wave 0 at a round boundary: publish the chain's
// phi for the round just finished (done = its seq), then wait for the next
// command: RUN (K proposals at the slot's new temperature) or QUIT; silence
// past the idle watchdog is a QUIT (the state is consistent between rounds).
// Results in sh.rK / sh.rT / sh.rinv2t / sh.srv_quit.
// A RUN posted with the slot's `skip` set (the chain ran that round in a launch
// the host lost, chain.cpp td_rounds_run) is answered with phi at once and
// waited past: the chain runs each round exactly once.  `phi` = the chain's
// exact phi (the launch's first wait: its stored one).
__device__ void round_wait(RoundBox *rb, int b, Shared &sh, int lane, bool publish, double phi) {
    RoundSlot *slot = &rb->slot[b];
    // The mailbox is coherent pinned host memory and every access to it is a system-scope atomic,
    // so no system-scope fence is needed -- one would write back (release) or invalidate (acquire)
    // this XCD's whole L2, the chain's working set, at every round.  phi is acknowledged before
    // done is written (the host reads done, then phi).
    if (publish && lane == 0) {
        mb_store(reinterpret_cast<long long *>(&slot->phi), __double_as_longlong(phi));
        __builtin_amdgcn_s_waitcnt(0);
        mb_store(&slot->done, sh.rseq);
    }
    long long seen = sh.rseq;
    long long idle = kServerIdleTicks;
    if (!publish) {  // a launch's first wait: the testing override of the watchdog
        const long long o = mb_load(&slot->idle);
        if (o > 0) idle = o;
    }
    long long t0 = (long long)wall_clock64();
    while (true) {
        const long long sq = mb_load(&rb->seq);
        if (sq != seen) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (lane == 0) {
                // (the host wrote them before seq: four loads in flight together)
                const long long w = mb_load(reinterpret_cast<const long long *>(rb) + 1);  // cmd | K << 32
                const long long tb = mb_load(reinterpret_cast<const long long *>(&slot->T));
                const long long ib = mb_load(reinterpret_cast<const long long *>(&slot->inv_2t));
                const long long sk = mb_load(&slot->skip);
                const int cmd = (int)(w & 0xffffffffll), K = (int)(w >> 32);
                sh.rseq = sq;
                sh.rskip = 0;
                if (cmd == kRoundRun && K > 0 && sk) {  // ran already: report it again
                    mb_store(reinterpret_cast<long long *>(&slot->phi), __double_as_longlong(phi));
                    __builtin_amdgcn_s_waitcnt(0);
                    mb_store(&slot->done, sq);
                    sh.rskip = 1;
                } else if (cmd == kRoundRun && K > 0) {
                    sh.rK = K;
                    sh.rT = __longlong_as_double(tb);
                    sh.rinv2t = __longlong_as_double(ib);
                    sh.srv_quit = 0;
                } else {
                    sh.srv_quit = 1;
                }
            }
            wave_sync_lds();
            if (sh.rskip) {
                seen = sq;
                t0 = (long long)wall_clock64();
                continue;
            }
            return;
        }
        if ((long long)wall_clock64() - t0 > idle) {
            if (lane == 0) sh.srv_quit = 1;
            wave_sync_lds();
            return;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// Exchange rounds (chain_dev.h RoundX), wave 0 at the end of round j with the
// chain's exact phi: publish it, wait for every replica's phi of the round,
// make the round's swap decisions (all of them, the same in every workgroup
// of every rank: chain_logic.h swap_accept on the gathered vector) and take
// this chain's new temperature (sh.rT, sh.rinv2t).  sh.srv_quit = 1 when an
// exchange never came (x.err set).  R <= 64: lane g holds replica g.
__device__ void round_exchange(const RoundX &x, int b, long long j, Shared &sh, int lane, double phi) {
    const int R = x.R;
    const unsigned long long tag = x.ready_base + (unsigned long long)j + 1ull;
    if (b == 0 && lane == 0) x.log_t[3 * j] = (long long)wall_clock64();
    if (lane == 0) {  // phi acknowledged before the flag (the readers load the flag, then phi)
        mb_store(reinterpret_cast<long long *>(&x.xin[(j & 1) * x.local + b]), __double_as_longlong(phi));
        __builtin_amdgcn_s_waitcnt(0);
        mb_store(reinterpret_cast<long long *>(&x.rdy[b]), (long long)tag);
    }
    const bool one = x.gdone == nullptr;  // one rank: xout is xin, every replica's flag is local
    const int nflags = one ? R : x.local;
    bool ok = true;
    if (one || b == 0) {  // wait for the flags (lane g reads flag g)
        const long long t0 = (long long)wall_clock64();
        while (true) {
            const unsigned long long f =
                lane < nflags ? (unsigned long long)mb_load(reinterpret_cast<const long long *>(&x.rdy[lane])) : tag;
            if (__all(f >= tag)) break;
            if ((long long)wall_clock64() - t0 > kExchangeTicks) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!one && ok && lane == 0)  // this rank's phis are in: the exchange stream may gather
            mb_store(reinterpret_cast<long long *>(x.ready), (long long)tag);
        if (b == 0 && lane == 0) x.log_t[3 * j + 1] = (long long)wall_clock64();
    }
    if (!one && ok) {  // the allgather of round j done (the exchange stream's write)
        const unsigned long long want = x.gdone_base + (unsigned long long)j + 1ull;
        const long long t0 = (long long)wall_clock64();
        while ((unsigned long long)mb_load(reinterpret_cast<const long long *>(x.gdone)) < want) {
            if ((long long)wall_clock64() - t0 > kExchangeTicks) {
                ok = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    if (!ok) {
        if (lane == 0) {
            mb_store(x.err, 1ll);
            sh.srv_quit = 1;
        }
        wave_sync_lds();
        return;
    }
    if (b == 0 && lane == 0) x.log_t[3 * j + 2] = (long long)wall_clock64();
    // every replica's phi and level (system-scope loads: the gathered vector bypasses the L2s)
    const bool in = lane < R;
    const double ph =
        in ? __longlong_as_double(mb_load(reinterpret_cast<const long long *>(&x.xout[(j & 1) * R + lane]))) : 0.0;
    const int lv = in ? x.lev[b * R + lane] : lane;
    // owner of level l (lane l): the replica at that level -- a forward permute of the levels
    const int owner = __builtin_amdgcn_ds_permute(lv * 4, lane);
    const unsigned long long rnd = (unsigned long long)(x.rnd0 + j);
    const int par = (int)(rnd & 1ull);
    // pair leaders l = par, par + 2, ... < R - 1 decide the disjoint pairs (l, l + 1)
    const bool leader = lane >= par && ((lane - par) & 1) == 0 && lane + 1 < R;
    const int owner_hi = __shfl(owner, (lane + 1) & 63);
    const double pa = __shfl(ph, owner & 63), pb = __shfl(ph, owner_hi & 63);
    bool acc = false;
    if (leader) acc = tdchain::swap_accept(pa, pb, x.temps[lane], x.temps[lane + 1], x.seed, rnd, (uint64_t)lane);
    // every replica: its pair (led by its level, or by the level below) and that pair's fate
    int lead = -1;
    if (in) {
        if (lv >= par && ((lv - par) & 1) == 0 && lv + 1 < R) lead = lv;
        else if (lv - 1 >= par && ((lv - 1 - par) & 1) == 0) lead = lv - 1;
    }
    const int acc_i = __shfl((int)acc, lead < 0 ? 0 : lead);
    const int nl = (lead >= 0 && acc_i) ? (lv == lead ? lead + 1 : lead) : lv;
    if (in) {
        x.lev[b * R + lane] = nl;
        if (b == 0) {
            x.log_phi[j * R + lane] = ph;
            x.log_lev[j * R + lane] = nl;
        }
    }
    const int me = x.rank * x.local + b;
    const int my_level = __shfl(nl, me);
    if (lane == 0) {
        const double T = x.temps[my_level];
        sh.rT = T;
        sh.rinv2t = 1.0 / (2.0 * T);  // = params_derived's inv_2t
    }
    wave_sync_lds();
}

// A scripted step's answer in the pinned output (wave 0; system-scope stores): [phi, k, (ray, ptS) x k],
// the changed rays' new t* (the caller holds the model's ptS); k = -1: the whole proposed ptS follows.
// phi: NaN when the answer goes out before phase F (a server's step: the host forms phi_n itself).
__device__ void server_report(double *outp, const Views &v, const Shared &sh, int n, int lane, double phi) {
    long long *out = reinterpret_cast<long long *>(outp);
    auto put = [&](int i, double x) { mb_store(out + i, __double_as_longlong(x)); };
    const int nr = sh.n_rays;
    const bool few = 2 * nr + 2 <= n + 1;
    if (few) {
        for (int i = lane; i < nr; i += 64) {
            const int r = v.ray_at(i);
            put(2 + 2 * i, (double)r);
            put(3 + 2 * i, v.cptS[r]);
        }
    } else {
        for (int r = lane; r < n; r += 64) put(2 + r, v.rflag[r] ? v.cptS[r] : v.ptS[r]);
    }
    if (lane == 0) {
        put(0, phi);
        put(1, few ? (double)nr : -1.0);
    }
}

}  // namespace

}  // namespace tdstar
