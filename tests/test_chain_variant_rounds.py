"""Which k_chain_run instance a recorded ladder's launch takes (csrc/chain_variant.h, through
tdt_chain_variant_rounds; no GPU).  The fact "this launch records a ladder" is not among
tdt_chain_variant's 15 inputs: absent it is false, and the choice is the one tests/test_chain_variant.py
holds; present, with either round protocol, it names the two instances added behind the launcher's first
twelve."""
import ctypes
import itertools

BUDGET = 160 * 1024
T = 512
ROUNDS_REC = {(1, 0, T, 1, 1, 1), (0, 0, T, 0, 1, 1)}  # LDS layout; all in HBM


def inputs():
    """Every input of tests/test_chain_variant.py's sweep."""
    around = lambda lim: (lim - 16, lim, lim + 16)  # noqa: E731
    num_cus = 256
    for sizes in itertools.product(around(BUDGET), around(BUDGET), around(BUDGET // 2), around(BUDGET // 2)):
        for flags in itertools.product((0, 1), repeat=8):
            for nchains in (num_cus - 1, num_cus + 1):
                yield sizes + flags + (nchains, num_cus, BUDGET)
    yield (BUDGET + 16, BUDGET, BUDGET // 2, BUDGET // 2, 0, 0, 0, 1, 0, 0, 0, 0, 1000, 0, BUDGET)


def test_absent_fact_is_the_existing_choice(tt):
    f, g = tt.lib().tdt_chain_variant, tt.lib().tdt_chain_variant_rounds
    inp, a, b = (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
    for row in inputs():
        inp[:] = row
        assert f(ctypes.addressof(inp), ctypes.addressof(a)) == 0
        assert g(ctypes.addressof(inp), 0, ctypes.addressof(b)) == 0
        assert list(a) == list(b), row
        assert 0 <= a[7] < 12 and tuple(a[0:6]) not in ROUNDS_REC, row


def test_recorded_ladder_names_the_new_instances(tt):
    g = tt.lib().tdt_chain_variant_rounds
    inp, out, plain = (ctypes.c_int64 * 15)(), (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
    reached, indices = set(), {}
    for row in inputs():
        small, big = row[0], row[1]
        all_auto, rx, rb = row[7], row[10], row[11]
        inp[:] = row
        assert g(ctypes.addressof(inp), 1, ctypes.addressof(out)) == 0
        assert g(ctypes.addressof(inp), 0, ctypes.addressof(plain)) == 0
        got, lds, at = tuple(out[0:6]), out[6], out[7]
        if not (rx or rb):  # the fact counts only with a round protocol
            assert list(out) == list(plain), row
            continue
        # one 8-wave chain per CU, the layout by the exchange rounds' rule: in LDS when every chain
        # fits and none asks for another layout
        want = ((1, 0, T, 1, 1, 1), small) if small <= BUDGET and all_auto else ((0, 0, T, 0, 1, 1), big)
        assert (got, lds) == want, row
        assert at >= 12, (row, at)
        assert indices.setdefault(got, at) == at
        reached.add(got)
    assert reached == ROUNDS_REC
    assert sorted(indices.values()) == [12, 13]


def test_null_arguments(tt):
    out = (ctypes.c_int64 * 8)()
    assert tt.lib().tdt_chain_variant_rounds(None, 1, ctypes.addressof(out)) == 1  # TD_ERR_ARG
