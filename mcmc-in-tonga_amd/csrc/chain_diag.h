// chain_diag.h -- k_chain_run's diagnostics macros (they name its locals: sh, tid, lane, wv, it, kWv,
// prof_on, action): the phase stamps, and the wave-skew (-DTD_CHAIN_SKEW) and phase-B probe
// (-DTD_B_PROBE) testing builds.  chain_kernels.hip is the only unit that uses them, so the only one a
// testing build compiles again.
#pragma once

// Diagnostic phase stamp (lane 0 of wave 0, right after a barrier): cycles
// since the previous stamp are charged to phase k.  Off unless d.profile.
#define STAMP(k)                                   \
    do {                                           \
        if (prof_on && tid == 0) {                 \
            const long long t_ = clock64();        \
            sh.prof[k] += t_ - sh.t_last;          \
            sh.prof[16 + 10 * (action - 1) +       \
                    ((k) <= 5 ? (k) : (k) == 12 ? 6 : (k) == 13 ? 7 : 8)] += t_ - sh.t_last; \
            sh.t_last = t_;                        \
        }                                          \
    } while (0)

// Wave-skew testing build (-DTD_CHAIN_SKEW, tools/build_skew.sh): after every block barrier and every
// barrier-free phase end of the chain loop, one wave -- rotating with the iteration and the site --
// sleeps 8k-16k cycles (a whole phase or more), so any shared word read without a synchronisation
// that orders it shows up as a wrong answer in the chain parity tests.  Off in the product build.
#ifdef TD_CHAIN_SKEW
#define SKEW(site)                                                                      \
    do {                                                                                \
        if (lane == 0) sh.dbg_site[wv] = (int)((it << 8) | (site));                     \
        if (wv == (int)(((unsigned long long)it * 5ull + (site)) % (unsigned)kWv)) {    \
            __builtin_amdgcn_s_sleep(127);                                              \
            if (((it + (site)) & 1) != 0) __builtin_amdgcn_s_sleep(127);                \
        }                                                                               \
    } while (0)
#else
#define SKEW(site) \
    do {           \
    } while (0)
#endif
// The chain's spin waits (a wave waiting for other waves' counts in LDS).  In the skew build each gives up
// after ~0.5 s, adds `site` to the diagnostic slot prof[79] (tdt_chain_profile) and goes on, so a wait that
// can never end shows up as a wrong answer and a nonzero slot instead of a hung launch.
#ifdef TD_CHAIN_SKEW
// (the first time one gives up, prof[56 + w] holds wave w's last skew site, as it << 8 | site, and
// prof[64] the iteration << 8 | the giving-up wave)
#define SPIN_WAIT(cond, site)                                                                        \
    do {                                                                                             \
        long long n_ = 0;                                                                            \
        while (cond) {                                                                               \
            __builtin_amdgcn_s_sleep(1);                                                             \
            if (++n_ > (1ll << 23)) {                                                                \
                if (lane == 0) {                                                                     \
                    if (atomicAdd((unsigned long long *)&sh.prof[79], (unsigned long long)(site)) == 0ull) { \
                        for (int w_ = 0; w_ < kWv; ++w_) sh.prof[56 + w_] = sh.dbg_site[w_];       \
                        sh.prof[64] = (it << 8) | wv;                                                \
                    }                                                                                \
                }                                                                                    \
                break;                                                                               \
            }                                                                                        \
        }                                                                                            \
    } while (0)
#else
#define SPIN_WAIT(cond, site)                      \
    do {                                           \
        while (cond) __builtin_amdgcn_s_sleep(1);  \
    } while (0)
#endif

// Phase-B probe build (-DTD_B_PROBE, diagnostics only): tid 0's cycles from the phase's start (STAMP(0)) to
// points inside phase B, summed into prof[72 + k] (those slots' preamble use is off in that build).
#ifdef TD_B_PROBE
#define BPROBE(k)                                                       \
    do {                                                                \
        if (prof_on && tid == 0) sh.prof[72 + (k)] += clock64() - sh.t_last; \
    } while (0)
#else
#define BPROBE(k) \
    do {          \
    } while (0)
#endif
