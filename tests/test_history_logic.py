"""The host-side logic of the device sample history that needs no GPU: the thinning arithmetic of a
recorded stretch (chain.thinning) against a brute-force replay of TD_inversion_function.jl:275-288, and
td_history_create's argument errors (checked before any HIP call)."""
import ctypes

import numpy as np


def replay(start, stop, burn_in, keep_each, model_num):
    """TD_inversion_function.jl:275-288, literally: the saved iterations of start..stop, and model_num after."""
    saved = []
    for it in range(start, stop + 1):
        if it >= burn_in:
            model_num += 1
            if model_num % keep_each == 0:
                saved.append(it)
    return saved, model_num


def stretch_samples(tt, it, count, burn_in, keep_each, model_num):
    first, every, ns = tt.thinning(it, count, burn_in, keep_each, model_num)
    assert first >= 1 and every >= 1 and ns >= 0
    s = [it + first - 1 + k * every for k in range(ns)]
    assert all(it <= x <= it + count - 1 for x in s)
    # the C ABI's count for (iterations, first, every) is the same: with no sample, `first` lies past the stretch
    assert (0 if first > count else (count - first) // every + 1) == ns
    return s


def cases():
    rng = np.random.default_rng(20)
    out = [(300, 100.0, 20, 1, 0), (300, 100.0, 1, 1, 0), (50, 50.0, 10, 1, 0), (50, 50.0, 1, 1, 0),
           (200, 60.5, 7, 1, 0), (200, 60.5, 1, 1, 0), (120, 0.0, 10, 1, 0), (400, 399.5, 3, 1, 0)]
    for _ in range(300):
        n_iter = int(rng.integers(1, 401))
        burn = float(rng.integers(0, n_iter + 1))
        if rng.random() < 0.3:
            burn = float(rng.uniform(0, n_iter))  # a non-integer burn_in
        if rng.random() < 0.1:
            burn = float(n_iter)
        keep = int(rng.choice([1, 2, 3, 7, 10, 20, 50]))
        start = int(rng.integers(1, n_iter + 1))
        # a resume: model_num as the interrupted run left it, or anything (model_num % keep_each != 0 too)
        model_num = replay(1, start - 1, burn, keep, 0)[1] if rng.random() < 0.5 else int(rng.integers(0, 500))
        out.append((n_iter, burn, keep, start, model_num))
    return out


def test_thinning_matches_reference_replay(tt):
    seen_resume = 0
    for n_iter, burn, keep, start, model_num in cases():
        want, _ = replay(start, n_iter, burn, keep, model_num)
        got = stretch_samples(tt, start, n_iter - start + 1, burn, keep, model_num)
        assert got == want, (n_iter, burn, keep, start, model_num)
        seen_resume += model_num % keep != 0
    assert seen_resume > 20


def test_thinning_is_invariant_to_cuts(tt):
    rng = np.random.default_rng(21)
    for n_iter, burn, keep, start, model_num in cases():
        want, _ = replay(start, n_iter, burn, keep, model_num)
        cuts = sorted(set(int(c) for c in rng.integers(start, n_iter + 1, int(rng.integers(0, 6)))))
        got, it, mn = [], start, model_num
        for end in cuts + [n_iter]:
            if end < it:
                continue
            got += stretch_samples(tt, it, end - it + 1, burn, keep, mn)
            mn = replay(it, end, burn, keep, mn)[1]
            it = end + 1
        assert got == want, (n_iter, burn, keep, start, model_num, cuts)


def test_thinning_empty_stretches(tt):
    assert tt.thinning(1, 0, 0.0, 10, 0) == (10, 10, 0)
    assert tt.thinning(1, 99, 100.0, 1, 0) == (100, 1, 0)  # all before burn-in: the first sample would be the 100th
    assert tt.thinning(1, 5, 0.0, 0, 0)[2] == 0 and tt.thinning(1, 5, 0.0, 0, 0)[0] > 5  # keep_each 0: never
    assert tt.thinning(1, 100, 100.0, 1, 0) == (100, 1, 1)  # iter >= burn_in: the burn_in-th iteration counts
    assert tt.thinning(100, 1, 100.0, 10, 9) == (1, 10, 1)


def test_history_create_argument_errors_without_gpu(tt):
    L = tt.lib()
    h = ctypes.c_void_p(1)
    for args, text in (((None, 0, 10, 0), b"max_samples >= 1"), ((None, -3, 10, 1), b"max_samples >= 1"),
                       ((None, 4, 0, 0), b"max_cells_total >= 1"), ((None, 4, 10, 1), b"ctx is NULL")):
        rc = L.td_history_create(ctypes.byref(h), *args)
        assert rc == 1  # TD_ERR_ARG, before any HIP call
        assert text in L.td_last_error(None), (args, L.td_last_error(None))
        assert not h.value  # no handle comes back
        h = ctypes.c_void_p(1)
