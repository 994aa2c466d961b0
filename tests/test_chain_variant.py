"""Which k_chain_run instance a launch takes (csrc/chain_variant.h choose_chain_variant, through
tdt_chain_variant; no GPU): held against the if-chain the launcher had before the choice became a
function, over every combination of its inputs around every limit."""
import ctypes
import itertools

BUDGET = 160 * 1024
T = 512

# k_chain_run<SMALL, SCRIPT, NTH, RLDS, ROUNDS, REC>: the 12 instances the launcher's table holds
INSTANCES = {
    (1, 0, T, 1, 0, 0), (1, 1, T, 1, 0, 0), (0, 0, T, 0, 0, 0), (0, 1, T, 0, 0, 0),
    (0, 0, T // 2, 0, 0, 0), (1, 0, T // 2, 0, 0, 0), (1, 0, T, 1, 1, 0), (0, 0, T, 0, 1, 0),
    (1, 0, T, 1, 0, 1), (0, 0, T, 0, 0, 1), (0, 0, T // 2, 0, 0, 1), (1, 0, T // 2, 0, 0, 1),
}


def parent_choice(small, big, half, hyb, force_hbm, packed, tiles_ok, all_auto, scripted, rec, rx, rb, nchains,
                  num_cus, budget):
    """chain_run's launch code before the split, statement for statement: its launch sites as
    (SMALL, SCRIPT, NTH, RLDS, ROUNDS, REC) with the template's defaults (RLDS = SMALL, ROUNDS = REC = false)
    written out, and the LDS size each passes."""
    rec = rec and not scripted and not rb and not rx
    if (all_auto and num_cus > 0 and nchains > num_cus and not scripted and not rb and not rx and
            (hyb <= budget // 2 or half <= budget // 2)):
        packed = True
        tiles_ok = hyb <= budget // 2
        force_hbm = True

    def launch_free(sm, nth, rlds, lds):
        return (sm, 0, nth, rlds, 0, 1 if rec else 0), lds

    if rx:
        if small <= budget and all_auto:
            return (1, 0, T, 1, 1, 0), small
        return (0, 0, T, 0, 1, 0), big
    if small <= budget and not force_hbm:
        if scripted:
            return (1, 1, T, 1, 0, 0), small
        return launch_free(1, T, 1, small)
    if packed and not scripted and tiles_ok and hyb <= budget // 2:
        return launch_free(1, T // 2, 0, hyb)
    if packed and not scripted and half <= budget // 2:
        return launch_free(0, T // 2, 0, half)
    if scripted:
        return (0, 1, T, 0, 0, 0), big
    return launch_free(0, T, 0, big)


def test_choice_matches_the_launchers_former_if_chain(tt):
    f = tt.lib().tdt_chain_variant
    inp, out = (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 8)()
    pin, pout = ctypes.addressof(inp), ctypes.addressof(out)
    around = lambda lim: (lim - 16, lim, lim + 16)
    num_cus = 256
    reached, indices = set(), {}
    for sizes in itertools.product(around(BUDGET), around(BUDGET), around(BUDGET // 2), around(BUDGET // 2)):
        for flags in itertools.product((0, 1), repeat=8):
            for nchains in (num_cus - 1, num_cus + 1):
                inp[:] = sizes + flags + (nchains, num_cus, BUDGET)
                assert f(pin, pout) == 0
                got, lds, at = tuple(out[0:6]), out[6], out[7]
                want, want_lds = parent_choice(*sizes, *flags, nchains, num_cus, BUDGET)
                assert (got, lds) == (want, want_lds), (sizes, flags, nchains)
                assert got in INSTANCES and 0 <= at < 12, (got, at)
                assert indices.setdefault(got, at) == at
                reached.add(got)
    assert reached == INSTANCES
    assert sorted(indices.values()) == list(range(12))
    # no CU count known (a single chain's launch): never packed by itself
    inp[:] = (BUDGET + 16, BUDGET, BUDGET // 2, BUDGET // 2, 0, 0, 0, 1, 0, 0, 0, 0, 1000, 0, BUDGET)
    assert f(pin, pout) == 0 and tuple(out[0:6]) == (0, 0, T, 0, 0, 0) and out[6] == BUDGET


def test_null_arguments(tt):
    out = (ctypes.c_int64 * 8)()
    assert tt.lib().tdt_chain_variant(None, ctypes.addressof(out)) == 1  # TD_ERR_ARG
