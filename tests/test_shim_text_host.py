"""CPU: the Julia binding that INTEGRATION.md prints, held to the header and to its transliteration.  No GPU.

The suite has no Julia, so the printed `ccall`s cannot run.  What can be checked without running them:
  * every `ccall((:name, LIB), Ret, (types...), args...)` of every Julia block names a symbol of _lib.SIGNATURES
    (which tests/test_data_and_abi.py ties to include/tdstar.h), with a return type and a type tuple that map onto
    its ctypes prototype, as many arguments as types, and a library constant that the document defines;
  * tests/shim_replay.py claims every statement line of section 2's functions, in the block's order: the block
    cannot change without the transliteration (which tests/test_gpu_shim_replay.py runs) changing with it;
  * the two orderings whose absence broke `debug_prior = 1` and a resumed chain: `evaluate` makes the context
    before the debug_prior return, and `Interpolation` has no error( of its own;
  * the restatement's `resume=` (oracle/chain_ref.py) continues an uninterrupted run with ==, and
    chain_cases.steps_diff, the GPU replay's whole judgement, reports every kind of difference."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import chain_cases as cc
import shim_replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT = open(os.path.join(ROOT, "INTEGRATION.md")).read()

PD, PI32, PI64, VP = (ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                      ctypes.c_void_p)
JULIA_TYPES = {
    "Cint": ctypes.c_int, "Int64": ctypes.c_int64, "UInt64": ctypes.c_uint64,
    "Ptr{Float64}": PD, "Ref{Float64}": PD, "Ptr{Int32}": PI32, "Ptr{Int64}": PI64, "Ref{Int64}": PI64,
    "Ptr{UInt8}": ctypes.c_char_p, "Cstring": ctypes.c_char_p, "Ptr{Cvoid}": VP,
    "Ptr{Ptr{Cvoid}}": ctypes.POINTER(VP), "Ref{Ptr{Cvoid}}": ctypes.POINTER(VP),
}


def julia_blocks(text=TEXT):
    return re.findall(r"```julia\n(.*?)```", text, flags=re.S)


def aliases(text=TEXT):
    """`const NAME = Ptr{Cvoid}` of the blocks: NAME -> c_void_p, Ref{NAME} and Ptr{NAME} -> POINTER(c_void_p)"""
    out = {}
    for block in julia_blocks(text):
        for name in re.findall(r"^const (\w+) = Ptr\{Cvoid\}\s*$", block, flags=re.M):
            out[name] = VP
            out["Ref{%s}" % name] = out["Ptr{%s}" % name] = ctypes.POINTER(VP)
    return out


def split_top(s):
    """The comma-separated parts of s at nesting depth 0 of () [] {} (strings skipped), stripped."""
    parts, depth, start, quote = [], 0, 0, False
    for i, ch in enumerate(s):
        if ch == '"':
            quote = not quote
        elif quote:
            continue
        elif ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        elif ch == "," and depth == 0:
            parts.append(s[start:i].strip())
            start = i + 1
    parts.append(s[start:].strip())
    return parts


def ccalls(block):
    """[(name, library constant, return type, [types], [arguments])] of a block's ccall(...)s"""
    out = []
    for m in re.finditer(r"\bccall\(", block):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(block[i], 0)
            i += 1
        parts = split_top(block[m.end():i - 1])
        head = re.fullmatch(r"\(:(\w+),\s*(\w+)\)", parts[0])
        assert head and re.fullmatch(r"\(.*\)", parts[2], flags=re.S), parts[:3]
        types = [t for t in split_top(parts[2][1:-1]) if t]  # (T,) has a trailing comma
        out.append((head.group(1), head.group(2), parts[1], types, parts[3:]))
    return out


def test_the_ccall_reader_reads():
    got = ccalls('x = f(ccall((:td_a, LIB), Cint, (Ptr{Cvoid},), ctx)) + ccall((:td_b, L2), Cstring,\n'
                 '   (Ref{R_}, Ptr{Ptr{Cvoid}}, Int64), r, g(a, b), length(chains))')
    assert got == [("td_a", "LIB", "Cint", ["Ptr{Cvoid}"], ["ctx"]),
                   ("td_b", "L2", "Cstring", ["Ref{R_}", "Ptr{Ptr{Cvoid}}", "Int64"],
                    ["r", "g(a, b)", "length(chains)"])]
    assert aliases("```julia\nconst R_ = Ptr{Cvoid}\n```")["Ref{R_}"] is JULIA_TYPES["Ref{Ptr{Cvoid}}"]


def test_every_printed_ccall_matches_the_ctypes_prototype(tt):
    from importlib import import_module

    signatures = import_module("mcmc_in_tonga_amd._lib").SIGNATURES
    types = dict(JULIA_TYPES, **aliases())
    seen = []
    for block in julia_blocks():
        for name, libname, ret, argtypes, args in ccalls(block):
            where = "ccall of %s" % name
            assert name in signatures, where
            restype, proto = signatures[name]
            assert ret in types and types[ret] is restype, (where, ret, restype)
            assert all(t in types for t in argtypes), (where, [t for t in argtypes if t not in types])
            assert [types[t] for t in argtypes] == list(proto), (where, argtypes, proto)
            assert len(args) == len(argtypes), (where, len(args), len(argtypes))
            assert re.search(r"^const %s\s*=" % libname, TEXT, flags=re.M), (where, libname)
            seen.append(name)
    # the reader found the calls it is there for: section 2's four and section 3's
    assert {"td_last_error", "td_create", "td_evaluate", "td_interpolate", "td_rounds_create", "td_rounds_temper",
            "td_rounds_destroy", "td_comm_unique_id", "td_comm_create", "td_rounds_exchange",
            "td_comm_destroy"} == set(seen), sorted(seen)
    assert seen.count("td_create") == 2  # the worker's context and the ray-less one


def shim_block():
    blocks = [b for b in julia_blocks() if "function evaluate(" in b]
    assert len(blocks) == 1
    return blocks[0]


def statement_lines(block):
    """name -> the statement lines of each `function name(...) ... end` of the block (stripped, trailing comments
    cut, blank and comment lines and lone `end`s left out), and of each one-line `name(args) = ...` definition."""
    out, name = {}, None
    for raw in block.splitlines():
        line = re.sub(r"\s+#(?![^\"]*\"[^\"]*$).*$", "", raw).strip()
        m = re.match(r"function (\w+)\(", raw)
        if m:
            name = m.group(1)
            out[name] = []
        elif raw.startswith("end"):
            name = None
        elif name is not None:
            if line and not line.startswith("#") and line != "end":
                out[name].append(line)
        elif re.match(r"\w+\([\w, ]*\) = ", raw):
            out[raw.split("(")[0]] = [line]
    return out


def test_the_transliteration_claims_every_statement_of_the_shim():
    block = shim_block()
    lines = statement_lines(block)
    assert set(lines) == {"tdcheck", "tdctx", "tdctx0", "evaluate", "Interpolation"}
    assert set(shim_replay.STATEMENTS) == set(lines)
    for name, claimed in shim_replay.STATEMENTS.items():
        at = block.index("function %s(" % name if name != "tdcheck" else "tdcheck(rc, ctx) =")
        for k, s in enumerate(claimed):  # each occurs in the block, in this order
            at = block.find(s, at)
            assert at >= 0, (name, k, s)
            at += len(s)
        assert claimed == lines[name], (name, [s for s in lines[name] if s not in claimed])  # none left unclaimed
        assert callable(getattr(shim_replay.Shim, name))
    for const in ("TDCTX", "TDCTX0"):
        assert "const %s = Ref{Ptr{Cvoid}}(C_NULL)" % const in block


def test_the_shim_makes_its_context_whatever_the_call_order():
    lines = statement_lines(shim_block())
    ev = lines["evaluate"]
    made = [k for k, s in enumerate(ev) if "tdctx(" in s]
    returned = [k for k, s in enumerate(ev) if re.search(r"debug_prior == 1 && return", s)]
    assert len(made) == 1 and len(returned) == 1 and made[0] < returned[0], ev
    assert not any("error(" in s for s in lines["Interpolation"]), lines["Interpolation"]
    # the ray-less context is never the worker's: TDCTX is assigned in tdctx alone, and from td_create's out
    assigned = [(name, s) for name, body in lines.items() for s in body if re.match(r"TDCTX\[\] =", s)]
    assert assigned == [("tdctx", "TDCTX[] = out[]")]
    assert "tdctx0()" in " ".join(lines["Interpolation"]) and "TDCTX[]" in " ".join(lines["Interpolation"])
    assert "happens naturally\" " not in TEXT and "so this happens naturally" not in TEXT


@pytest.fixture(scope="module")
def reference(tt, orc):
    return cc.reference(tt, "A-p1-T1")


def first_entered(steps, action, k0=100):
    """The first k >= k0 whose iteration k + 1 (steps[k]) has this action and is not skipped."""
    from oracle import chain_ref

    return next(k for k in range(k0, len(steps)) if steps[k].action == action and steps[k].outcome != chain_ref.SKIPPED)


def test_a_resumed_restatement_continues_the_uninterrupted_one(tt, orc, reference):
    """run(..., resume=(phi_k, ptS_k), start_iter=k + 1) from the cells of steps[k - 1] gives steps[k:] with ==,
    evaluating no starting model (:41-67)."""
    name = "A-p1-T1"
    steps = reference["steps"]
    k = first_entered(steps, 1)
    assert steps[k].iter == k + 1
    ds = cc.rays(tt, cc.CASES[name][0])
    n = len(steps) - k
    got = cc.restate(tt, ds, cc.chain_params(tt, name), steps[k - 1].cells, n, start_iter=k + 1,
                     resume=(steps[k - 1].phi, steps[k - 1].ptS))
    assert cc.steps_diff(got, cc.window(steps, k, n)) is None
    assert [s.margin for s in got["steps"]] == [s.margin for s in steps[k:]]
    assert got["start"][1] is steps[k - 1].ptS
    # no starting evaluate: the two parts' evaluations add up to the whole run's (whose first k iterations, run
    # by themselves, count the starting model's)
    head = cc.restate(tt, ds, cc.chain_params(tt, name), cc.start_model(tt, 8, 1, cc.CASES[name][7]), k)
    assert cc.steps_diff(head, dict(reference, steps=steps[:k], **dict(zip(("accepted", "proposed"),
                                                                          cc.counts(steps[:k]))))) is None
    assert head["evaluations"] + got["evaluations"] == reference["evaluations"]


def test_forward_calls_take_the_oracles_place(tt, orc, reference):
    """run(forward=(ev, interp)) calls them where it called the oracle, in the same order, and still counts."""
    import oracle

    name = "A-p1-T1"
    ds = cc.rays(tt, cc.CASES[name][0])
    log = []

    def ev(c):
        log.append("e")
        r = oracle.evaluate(ds.rayX, ds.rayY, ds.rayZ, ds.rayL, ds.rayU, ds.tS, ds.allSig, c)
        return r["phi"], r["ptS"], 1

    def interp(c, x, y, z):
        log.append("i")
        return float(oracle.interpolation(c, [x], [y], [z])[0][0])

    n = 200
    got = cc.restate(tt, ds, cc.chain_params(tt, name), cc.start_model(tt, 8, 1, cc.CASES[name][7]), n,
                     forward=(ev, interp))
    want = dict(reference, steps=reference["steps"][:n])
    want["accepted"], want["proposed"] = cc.counts(want["steps"])
    assert cc.steps_diff(got, want) is None
    assert got["evaluations"] == log.count("e") > n // 2
    assert log[0] == "e" and log.count("i") == got["proposed"][0] + got["proposed"][1]


@pytest.mark.parametrize("name", ["B-p2"])
def test_no_death_of_the_replayed_cases_queries_a_tie(tt, orc, name):
    """From the reference's steps and draws alone: no death the loop entered interpolates (:146) at a point that
    lies on a site of the reduced model or at equal distance from its two nearest cells -- the sites are
    continuous draws.  That is why tests/test_gpu_shim_replay.py scripts such queries
    (test_one_point_queries_that_tie) instead of finding them in the case's replay."""
    from oracle import chain_ref

    _, ncells, _, _, _, prior, _, seed = cc.CASES[name]
    draws = cc.draws_of(tt, seed, cc.CHAIN)
    cells = cc.start_model(tt, ncells, prior, seed).cells()
    deaths = 0
    for s in cc.reference(tt, name)["steps"]:
        if s.action == 2 and s.outcome != chain_ref.SKIPPED:
            x, y, z, _ = (np.asarray(a, dtype=np.float64) for a in cells)
            kill = int(np.floor(draws(s.iter)[6] * len(x)))  # :128
            if s.accept:
                assert all(np.array_equal(np.delete(a, kill), b) for a, b in zip((x, y, z), s.cells))
            d = np.sort((np.delete(x, kill) - x[kill]) ** 2 + (np.delete(y, kill) - y[kill]) ** 2 +
                        (np.delete(z, kill) - z[kill]) ** 2)
            assert d[0] > 0.0 and d[0] != d[1], s.iter
            deaths += 1
        cells = s.cells
    assert deaths >= 20


def test_steps_diff_can_fail(tt, orc, reference):
    steps = reference["steps"][:300]
    want = cc.window(reference["steps"], 1, 299)
    assert want["steps"] == steps[1:] and want["start"][0] == steps[0].phi

    def changed(k, **fields):
        got = dict(want, steps=list(want["steps"]))
        s = copy.copy(got["steps"][k])
        for key, v in fields.items():
            setattr(s, key, v)
        got["steps"][k] = s
        return got

    assert cc.steps_diff(dict(want), want) is None
    s = want["steps"][150]
    up = lambda a, j=0: np.concatenate([a[:j], [np.nextafter(a[j], np.inf)], a[j + 1:]])
    for word, fields in (("iter", dict(iter=s.iter + 1)), ("action", dict(action=s.action % 4 + 1)),
                         ("accept", dict(accept=1 - s.accept)), ("outcome", dict(outcome="other")),
                         ("ncells", dict(ncells=s.ncells + 1)), ("phi", dict(phi=np.nextafter(s.phi, 0.0))),
                         ("ptS", dict(ptS=up(s.ptS, 3))), ("ptS", dict(ptS=None)),
                         ("xCell", dict(cells=(up(s.cells[0]),) + s.cells[1:])),
                         ("yCell", dict(cells=s.cells[:1] + (up(s.cells[1]),) + s.cells[2:])),
                         ("zCell", dict(cells=s.cells[:2] + (up(s.cells[2]),) + s.cells[3:])),
                         ("zetaCell", dict(cells=s.cells[:3] + (up(s.cells[3], s.ncells - 1),)))):
        bad = cc.steps_diff(changed(150, **fields), want)
        assert bad is not None and word in bad and "iteration %d" % s.iter in bad, (word, bad)
    assert cc.steps_diff(changed(150, ptS=None), want, with_ptS=False) is None
    assert "steps" in cc.steps_diff(dict(want, steps=want["steps"][:-1]), want)
    assert "accepted" in cc.steps_diff(dict(want, accepted=want["proposed"]), want)
    assert "proposed" in cc.steps_diff(dict(want, proposed=want["accepted"]), want)
    assert "starting model's phi" in cc.steps_diff(dict(want, start=(np.nextafter(want["start"][0], 0.0),
                                                                      want["start"][1])), want)
    assert "starting model's ptS" in cc.steps_diff(dict(want, start=(want["start"][0], up(want["start"][1]))), want)
    assert "starting model's ptS" in cc.steps_diff(dict(want, start=(want["start"][0], None)), want)
