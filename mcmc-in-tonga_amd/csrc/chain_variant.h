// chain_variant.h -- which k_chain_run instance a launch takes (host only, no HIP types).
//
// chain_run (chain_kernels.hip) folds its chains' LDS plans and lds_modes into the facts below, asks
// choose_chain_variant() and launches the table entry it names; chain_lds_sizes (chain_state.hip)
// asks it for one free-running chain; tests/test_chain_variant.py holds it, through
// tdt_chain_variant, against the if-chain it replaced, and tests/test_chain_variant_rounds.py, through
// tdt_chain_variant_rounds, holds what a ladder's recording adds.
#pragma once

#include <cstddef>

namespace tdstar {

constexpr int kVariantThreads = 512;  // == kChainThreads (chain_dev.h; asserted in chain_kernels.hip)

// k_chain_run's template arguments, in its order
struct ChainVariant {
    bool small, script;
    int nth;
    bool rlds, rounds, rec;
};
inline bool operator==(const ChainVariant &a, const ChainVariant &b) {
    return a.small == b.small && a.script == b.script && a.nth == b.nth && a.rlds == b.rlds &&
           a.rounds == b.rounds && a.rec == b.rec;
}

struct ChainLaunchFacts {
    // the largest lds_plan total of any chain: tiles, rays and order in LDS (8 waves); all in HBM (8
    // waves); all in HBM (4 waves); the tiles in LDS (4 waves)
    size_t small, big, half, hyb;
    // over the chains' lds_mode: any >= 1; all >= 2 (two chains per CU asked for); all == 2 (the tiles
    // in LDS when they fit; 3, testing: the all-in-HBM 4-wave kernel); all == 0
    bool force_hbm, packed, tiles_ok, all_auto;
    bool scripted;  // host-given proposals (scripted steps, the resident server)
    bool rec;       // some chain records (RecDesc::every > 0)
    bool rx, rb;    // exchange rounds; resident tempering rounds
    int nchains, num_cus;
    size_t budget;  // kLdsBudget
    // a ladder's recording (td_rounds_temper_recorded / td_rounds_exchange_recorded; with rb or rx): the
    // launch samples the replica at ladder level 0.  Last, and absent from tdt_chain_variant's 15 inputs:
    // `rec` with rb or rx alone still names a non-recording instance.
    bool rounds_rec;
};

struct ChainChoice {
    ChainVariant v;
    size_t lds;  // dynamic LDS of the launch: one size for the whole grid
};

inline ChainChoice choose_chain_variant(ChainLaunchFacts f) {
    const int T = kVariantThreads;
    // a recorded launch: the instances that carry the sampling (free-running, outside tempering rounds)
    const bool rec = f.rec && !f.scripted && !f.rb && !f.rx;
    // More chains than CUs: one chain per CU would run them in rounds of num_cus workgroups; two
    // 4-wave chains per CU run them all at once (1.35x the 8-wave kernel's rate at 512 config-3
    // chains) -- the tiles-in-LDS kernel when it fits, else the all-in-HBM one
    if (f.all_auto && f.num_cus > 0 && f.nchains > f.num_cus && !f.scripted && !f.rb && !f.rx &&
        (f.hyb <= f.budget / 2 || f.half <= f.budget / 2)) {
        f.packed = true;
        f.tiles_ok = f.hyb <= f.budget / 2;
        f.force_hbm = true;
    }
    if (f.rounds_rec && (f.rx || f.rb)) {  // a recorded ladder, either round protocol: one 8-wave chain per CU
        if (f.small <= f.budget && f.all_auto) return {{true, false, T, true, true, true}, f.small};
        return {{false, false, T, false, true, true}, f.big};
    }
    if (f.rx) {  // exchange rounds: one 8-wave chain per CU
        if (f.small <= f.budget && f.all_auto) return {{true, false, T, true, true, false}, f.small};
        return {{false, false, T, false, true, false}, f.big};
    }
    // the small (LDS-mirrored) variant only if every chain fits
    if (f.small <= f.budget && !f.force_hbm) return {{true, f.scripted, T, true, false, rec}, f.small};
    // two chains resident per CU (4 waves, <= half the budget of LDS each): the tiles in LDS, the rays
    // and the order in HBM
    if (f.packed && !f.scripted && f.tiles_ok && f.hyb <= f.budget / 2)
        return {{true, false, T / 2, false, false, rec}, f.hyb};
    // rays in HBM, 4 waves: two chains resident per CU
    if (f.packed && !f.scripted && f.half <= f.budget / 2) return {{false, false, T / 2, false, false, rec}, f.half};
    return {{false, f.scripted, T, false, false, rec}, f.big};
}

}  // namespace tdstar
