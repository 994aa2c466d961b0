"""CPU: what the fourteen posterior entry points answer to a refused call without a context -- the status and
the text of td_last_error(NULL), byte for byte as recorded in tests/posterior_refusals.json.  Every row
combines a request (valid, NULL, or invalid in one field its check function names), an ensemble (valid,
nmodels = 0, cell_off NULL, cell_off[0] = 1, a descending offset at the second model, arrays NULL with cells;
or no history list, an empty one, a NULL history) and chain lengths (valid or nchains = 0), so the recorded
message shows which check runs first.  The file is written by record() below from a build of the commit whose
answers are to be kept, never by pytest."""
import ctypes
import itertools
import json
import os
from importlib import import_module

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "posterior_refusals.json")


def rows(tt):
    """([(name, call)], what the calls point into): call() -> the status."""
    L = tt.lib()
    B = import_module("mcmc_in_tonga_amd._lib")
    P = B.ptr
    nq = 4
    q = [np.zeros(nq) for _ in range(3)]
    mean, std = np.zeros(nq), np.zeros(nq)
    c = [np.zeros(8) for _ in range(4)]
    quant, hist = np.zeros((1, nq)), np.zeros((nq, 5), dtype=np.int64)
    rhat = np.zeros(nq)
    keep = []

    def hold(x):
        keep.append(x)
        return x

    def marg(nprob=1, p=True, qo=True, nbins=2, lo=0.0, hi=1.0, ho=True, prob=0.5):
        pr = hold(np.array([prob]))
        return hold(B.TdMarginals(nprob, P(pr) if p else None, P(quant) if qo else None, nbins, lo, hi,
                                  P(hist) if ho else None))

    def conv(max_lag=0, r=True):
        return hold(B.TdConvergence(max_lag, P(rhat) if r else None, None, None))

    def ref(s):
        return ctypes.byref(s) if s is not None else None

    def adr(s):
        return ctypes.addressof(s) if s is not None else None

    MARG = {"ok": marg(), "NULL": None, "nprob<0": marg(nprob=-1), "nprob>64": marg(nprob=65),
            "probs NULL": marg(p=False), "quant_out NULL": marg(qo=False), "prob>1": marg(prob=1.5),
            "nbins<0": marg(nbins=-1), "nbins>4096": marg(nbins=4097), "lo>=hi": marg(lo=1.0, hi=1.0),
            "hist_out NULL": marg(ho=False)}
    CONV = {"ok": conv(), "NULL": None, "max_lag<0": conv(max_lag=-1), "no output": conv(r=False)}
    # the section entry points' own request: (nq, qx given, mean_out given)
    SECTION = {"ok": (nq, True, True), "nq<0": (-1, True, True), "qx NULL": (nq, False, True),
               "mean_out NULL": (nq, True, False), "nq=0": (0, False, False)}

    def vol(n=nq, qx=True, mo=True, m=None, cv=None):
        return hold(B.TdVolume(P(q[0]) if qx else None, P(q[1]), P(q[2]), n, P(mean) if mo else None, P(std), None,
                               adr(m), adr(cv)))

    VOL = {"ok": vol(), "ok conv": vol(cv=CONV["ok"]), "nq=0": vol(n=0), "NULL": None, "nq<0": vol(n=-1),
           "qx NULL": vol(qx=False), "mean_out NULL": vol(mo=False), "marg nprob<0": vol(m=MARG["nprob<0"]),
           "conv max_lag<0": vol(cv=CONV["max_lag<0"]), "conv no output": vol(cv=CONV["no output"])}
    phi = np.zeros(2)

    def pred(ph=True, mo=False, so=False, m=None, cv=None):
        return hold(B.TdPredict(None, P(phi) if ph else None, P(mean) if mo else None, P(std) if so else None, adr(m),
                                adr(cv)))

    PRED = {"ok": pred(), "ok conv": pred(cv=CONV["ok"]), "NULL": None, "nothing asked": pred(ph=False),
            "mean without std": pred(mo=True), "std without mean": pred(so=True), "marg nprob<0": pred(m=MARG["nprob<0"]),
            "conv max_lag<0": pred(cv=CONV["max_lag<0"])}
    t3, series, covo = [np.zeros(2) for _ in range(3)], np.zeros((2, 1)), np.zeros((3, nq))
    tm = np.zeros(3)

    def cov(n=nq, nt=2, ns=1, qx=True, tx=True, se=True, co=True, mo=True, so=True, tmo=True, tso=True):
        return hold(B.TdCovariance(P(q[0]) if qx else None, P(q[1]), P(q[2]), n, P(t3[0]) if tx else None, P(t3[1]),
                                   P(t3[2]), nt, P(series) if se else None, ns, P(covo) if co else None, None,
                                   P(mean) if mo else None, P(std) if so else None, P(tm) if tmo else None,
                                   P(tm) if tso else None))

    COV = {"ok": cov(), "NULL": None, "nq<0": cov(n=-1), "nt<0": cov(nt=-1), "nseries<0": cov(ns=-1),
           "no target": cov(nt=0, ns=0), "no output": cov(co=False), "qx NULL": cov(qx=False), "tx NULL": cov(tx=False),
           "series NULL": cov(se=False), "mean without std": cov(so=False), "tmean without tstd": cov(tso=False)}

    def off(*v):
        return hold(np.array(v, dtype=np.int64))

    cells = tuple(P(a) for a in c)
    # (nmodels, cell_off, the four arrays): eight models of one cell, so that two chains of four rows fit
    good = P(off(*range(9)))
    ENS = {"ok": (8, good, cells), "nmodels=0": (0, good, cells), "cell_off NULL": (8, None, cells),
           "cell_off[0]=1": (8, P(off(1, 1, 2, 3, 4, 5, 6, 7, 8)), cells),
           "descending": (8, P(off(0, 8, 5, 6, 7, 8, 8, 8, 8)), cells), "arrays NULL": (8, good, (None,) * 4),
           "negative total": (8, P(off(0, 1, 2, 3, 4, 5, 6, 7, -1)), cells)}
    CHAINS = {"ok": (2, P(off(4, 4))), "nchains=0": (0, P(off(4, 4))), "chain_len NULL": (1, None)}
    HS = {"hs NULL": (None, 1), "nh=0": (hold((ctypes.c_void_p * 1)(None)), 0),
          "a NULL history": (hold((ctypes.c_void_p * 1)(None)), 1)}
    out = []

    def add(name, parts, fn, *args):
        out.append(("%s | %s" % (name, " | ".join(parts)), lambda: fn(None, *args)))

    for (rn, (n, qx, mo)), (en, (nm, po, ca)) in itertools.product(SECTION.items(), ENS.items()):
        sec = (P(q[0]) if qx else None, P(q[1]), P(q[2]), n, P(mean) if mo else None, P(std))
        add("td_rasterize", (rn, en), L.td_rasterize, nm, po, *ca, *sec, None)
        for mn, m in MARG.items():
            if rn == "ok" or mn in ("ok", "NULL", "nprob<0"):
                add("td_rasterize_marginals", (mn, rn, en), L.td_rasterize_marginals, nm, po, *ca, *sec, ref(m))
        for (cn, cv), (hn, (nch, pl)) in itertools.product(CONV.items(), CHAINS.items()):
            if rn == "ok" or cn in ("ok", "NULL"):
                add("td_rasterize_convergence", (cn, hn, rn, en), L.td_rasterize_convergence, nm, po, *ca, *sec[:4], nch,
                    pl, *sec[4:], ref(cv))
    for (rn, (n, qx, mo)), (hn, (hs, nh)) in itertools.product(SECTION.items(), HS.items()):
        sec = (P(q[0]) if qx else None, P(q[1]), P(q[2]), n, P(mean) if mo else None, P(std))
        add("td_history_rasterize", (rn, hn), L.td_history_rasterize, hs, nh, *sec, None)
        for mn, m in MARG.items():
            add("td_history_marginals", (mn, rn, hn), L.td_history_marginals, hs, nh, *sec, ref(m))
        for cn, cv in CONV.items():
            add("td_history_convergence", (cn, rn, hn), L.td_history_convergence, hs, nh, *sec, ref(cv))
    for (en, (nm, po, ca)), (hn, (nch, pl)) in itertools.product(ENS.items(), CHAINS.items()):
        for rn, r in VOL.items():
            add("td_rasterize_volume", (rn, hn, en), L.td_rasterize_volume, nm, po, *ca, nch, pl, ref(r))
        for rn, r in PRED.items():
            add("td_rasterize_predict", (rn, hn, en), L.td_rasterize_predict, nm, po, *ca, nch, pl, ref(r))
    for (en, (nm, po, ca)), (rn, r) in itertools.product(ENS.items(), COV.items()):
        add("td_rasterize_covariance", (rn, en), L.td_rasterize_covariance, nm, po, *ca, ref(r))
    for hn, (hs, nh) in HS.items():
        for rn, r in VOL.items():
            add("td_history_volume", (rn, hn), L.td_history_volume, hs, nh, ref(r))
        for rn, r in PRED.items():
            add("td_history_predict", (rn, hn), L.td_history_predict, hs, nh, ref(r))
        for rn, r in COV.items():
            add("td_history_covariance", (rn, hn), L.td_history_covariance, hs, nh, ref(r))
        h23 = hold(np.zeros(23, dtype=np.int64))
        for bn, (nb, lo, hi, ho) in {"ok": (20, 0.0, 1.0, True), "nbins<0": (-1, 0.0, 1.0, True),
                                     "nbins>4096": (4097, 0.0, 1.0, True), "lo>=hi": (20, 1.0, 1.0, True),
                                     "nbins=0": (0, 0.0, 1.0, True), "hist_out NULL": (20, 0.0, 1.0, False)}.items():
            add("td_history_zeta_hist", (bn, hn), L.td_history_zeta_hist, hs, nh, nb, lo, hi, P(h23) if ho else None, None)
    vals = hold(np.zeros((8, nq)))
    for (cn, cv), (hn, (nch, pl)), (vn, (pv, ncol)) in itertools.product(
            CONV.items(), CHAINS.items(), {"ok": (P(vals), nq), "ncol<0": (P(vals), -1), "values NULL": (None, nq),
                                           "ncol=0": (None, 0)}.items()):
        add("td_convergence_values", (cn, hn, vn), L.td_convergence_values, pv, 8, ncol, nch, pl, ref(cv))
    return out, keep + [q, mean, std, c, quant, hist, rhat, phi, t3, series, covo, tm]


def answers(tt):
    L = tt.lib()
    got = {}
    table, alive = rows(tt)
    for name, call in table:
        assert name not in got, name
        status = call()
        got[name] = [status, L.td_last_error(None).decode()]
    del alive
    return got


def record(tt, path=RECORDED):
    """Run once, by hand, on the build whose refusals are to be kept: python -c "import tonga,
    test_posterior_refusals_host as t; t.record(tonga.load())" with tests/ on sys.path."""
    with open(path, "w") as f:
        json.dump(answers(tt), f, indent=0, sort_keys=True)
        f.write("\n")


def test_every_refusal_is_the_recorded_one(tt):
    want = json.load(open(RECORDED))
    got = answers(tt)
    assert sorted(got) == sorted(want)
    entry_points = {name.split(" | ")[0] for name in got}
    assert len(entry_points) == 14, entry_points
    assert all(status != 0 for status, _ in got.values())  # every row is a refused call
    wrong = {name: (got[name], want[name]) for name in got if got[name] != want[name]}
    assert not wrong, wrong
