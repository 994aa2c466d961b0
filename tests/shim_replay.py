"""The Julia shim of INTEGRATION.md section 2 (`tdstar.jl`), transliterated: what an unchanged Julia host's
`evaluate` and `Interpolation` send to libtdstar.so, as ctypes statements on tt.lib() in the shim's order with the
shim's arguments.  The suite has no Julia to run the printed binding with; this is the
next best thing, and tests/test_gpu_shim_replay.py drives it with the restatement of the reference's loop
(oracle/chain_ref.py) in the place of the Julia host.

STATEMENTS lists, per function of the block, the Julia statements this module restates, line by line (a
statement that spans lines is listed line by line; trailing comments and lone `end`s are left out).
tests/test_shim_text_host.py asserts that they are the block's lines, all of them and in that order, so the text
cannot change without this module failing a CPU test.  In the methods below the number in brackets is the index of
the statement in its function's list.

What stands for what:
  * `const TDCTX`, `const TDCTX0` (Ref{Ptr{Cvoid}}(C_NULL)) are the attributes TDCTX and TDCTX0, c_void_p(None);
  * `d` (DataStruct) is any object with rayX, rayY, rayZ, rayL, rayU (m x n and (m - 1) x n as numpy holds them),
    tS and allSig.  Julia's arrays are column-major, so the pointer ccall passes sees the C-order transpose;
  * `model` is the tuple of the four cell arrays; `evaluate` returns (model.phi, model.ptS, 1) -- model.ptS is
    None where the shim leaves the field as it was (debug_prior = 1);
  * `GC.@preserve` keeps Julia's arrays alive during the ccall: here the locals do;
  * Julia converts `m`, `n`, `length(.)` to Int64 and `-1`, `0` to Cint by the ccall's type tuple: the ctypes
    prototypes of _lib.SIGNATURES (which tt.lib() applies, and tests/test_shim_text_host.py ties to the type
    tuples printed in the block) do the same here;
  * `error("tdstar: ", text)` is ShimError("tdstar: " + text).

Not used, on purpose: TdContext, context_for and forward._scratch_context.  They are what the Julia side lacks."""
import ctypes

import numpy as np

STATEMENTS = {
    "tdcheck": [
        'tdcheck(rc, ctx) = rc == 0 || error("tdstar: ", unsafe_string(ccall((:td_last_error, LIBTD), Cstring, '
        '(Ptr{Cvoid},), ctx)))',
    ],
    "tdctx": [
        "if TDCTX[] == C_NULL",
        "m, n = size(d.rayX)",
        "out = Ref{Ptr{Cvoid}}(C_NULL)",
        "GC.@preserve d begin",
        "rc = ccall((:td_create, LIBTD), Cint,",
        "(Ptr{Ptr{Cvoid}}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},",
        "Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),",
        "out, -1, d.rayX, d.rayY, d.rayZ, d.rayL, d.rayU, m, n, d.tS, d.allSig)",
        "tdcheck(rc, C_NULL)",
        "TDCTX[] = out[]",
        "return TDCTX[]",
    ],
    "tdctx0": [
        "if TDCTX0[] == C_NULL",
        "out = Ref{Ptr{Cvoid}}(C_NULL)",
        "rc = ccall((:td_create, LIBTD), Cint,",
        "(Ptr{Ptr{Cvoid}}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},",
        "Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),",
        "out, -1, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 1, 0, C_NULL, C_NULL)",
        "tdcheck(rc, C_NULL)",
        "TDCTX0[] = out[]",
        "return TDCTX0[]",
    ],
    "evaluate": [
        "ctx = tdctx(dataStruct)",
        "model.phi = 1; model.likelihood = 1",
        "TD_parameters.debug_prior == 1 && return model, dataStruct, 1",
        "n = size(dataStruct.rayX, 2)",
        "ptS = zeros(n); phi = Ref(0.0); lik = Ref(0.0)",
        "GC.@preserve model begin",
        "rc = ccall((:td_evaluate, LIBTD), Cint,",
        "(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Cint,",
        "Ptr{Float64}, Ref{Float64}, Ref{Float64}, Ptr{Int32}),",
        "ctx, model.xCell, model.yCell, model.zCell, model.zeta, length(model.xCell), 0,",
        "ptS, phi, lik, C_NULL)",
        "tdcheck(rc, ctx)",
        "model.phi = phi[]; model.ptS = ptS; model.tS = dataStruct.tS; model.likelihood = lik[]",
        "return model, dataStruct, 1",
    ],
    "Interpolation": [
        'TD_parameters.interp_style == 1 || throw(ArgumentError("tdstar: only interp_style 1 (MCsub.jl:326)"))',
        "X = collect(Float64, X); Y = collect(Float64, Y); Z = collect(Float64, Z)",
        "zeta = zeros(length(X)); np = Ref{Int64}(0)",
        "ctx = TDCTX[] == C_NULL ? tdctx0() : TDCTX[]",
        "GC.@preserve model X Y Z begin",
        "rc = ccall((:td_interpolate, LIBTD), Cint,",
        "(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,",
        "Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,",
        "Ptr{Float64}, Ptr{Int32}, Ref{Int64}),",
        "ctx, model.xCell, model.yCell, model.zCell, model.zeta, length(model.xCell),",
        "X, length(X), Y, length(Y), Z, length(Z), zeta, C_NULL, np)",
        "tdcheck(rc, ctx)",
        "return zeta[1:np[]]",
    ],
}

C_NULL = None
_pd = ctypes.POINTER(ctypes.c_double)


class ShimError(RuntimeError):
    """Julia's ErrorException out of the shim's own error(...)"""


def _vec(a):
    """A Julia Vector{Float64}: the array itself where it already is one (no copy, as ccall passes it)."""
    return np.ascontiguousarray(a, dtype=np.float64)


def _colmajor(a):
    """A Julia Matrix{Float64} as ccall's Ptr{Float64} sees it: column by column."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).T)


def _p(a):
    return a.ctypes.data_as(_pd)


class Shim:
    """One worker process's tdstar.jl: the module's two constants and its functions."""

    def __init__(self, tt, interp_style=1):
        self.L = tt.lib()
        self.TDCTX = ctypes.c_void_p(C_NULL)  # const TDCTX = Ref{Ptr{Cvoid}}(C_NULL)
        self.TDCTX0 = ctypes.c_void_p(C_NULL)  # const TDCTX0 = Ref{Ptr{Cvoid}}(C_NULL)
        self.interp_style = interp_style  # TD_parameters.interp_style
        self.calls = {"td_create": 0, "td_evaluate": 0, "td_interpolate": 0}

    def tdcheck(self, rc, ctx):
        if rc == 0:  # tdcheck [0]
            return True
        text = self.L.td_last_error(ctx)
        raise ShimError("tdstar: " + (text.decode() if text else ""))

    def tdctx(self, d):
        if self.TDCTX.value is None:  # [0]
            m, n = np.asarray(d.rayX).shape  # [1]
            out = ctypes.c_void_p(C_NULL)  # [2]
            rayX, rayY, rayZ, rayL, rayU = (_colmajor(a) for a in (d.rayX, d.rayY, d.rayZ, d.rayL, d.rayU))  # [3]
            tS, allSig = _vec(d.tS), _vec(d.allSig)
            self.calls["td_create"] += 1
            rc = self.L.td_create(ctypes.byref(out), -1, _p(rayX), _p(rayY), _p(rayZ), _p(rayL), _p(rayU), m, n,
                                  _p(tS), _p(allSig))  # [4]-[7]
            self.tdcheck(rc, C_NULL)  # [8]
            self.TDCTX.value = out.value  # [9]
        return self.TDCTX  # [10]

    def tdctx0(self):
        if self.TDCTX0.value is None:  # [0]
            out = ctypes.c_void_p(C_NULL)  # [1]
            self.calls["td_create"] += 1
            rc = self.L.td_create(ctypes.byref(out), -1, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 1, 0, C_NULL,
                                  C_NULL)  # [2]-[5]
            self.tdcheck(rc, C_NULL)  # [6]
            self.TDCTX0.value = out.value  # [7]
        return self.TDCTX0  # [8]

    def evaluate(self, model, dataStruct, debug_prior):
        """-> (model.phi, model.ptS, 1)"""
        ctx = self.tdctx(dataStruct)  # [0]
        model_phi, model_ptS = 1.0, None  # [1] (phi is a Float64 field; ptS is not touched)
        if debug_prior == 1:  # [2]
            return model_phi, model_ptS, 1
        n = np.asarray(dataStruct.rayX).shape[1]  # [3]
        ptS, phi, lik = np.zeros(n), ctypes.c_double(0.0), ctypes.c_double(0.0)  # [4]
        xCell, yCell, zCell, zeta = (_vec(a) for a in model)  # [5]
        self.calls["td_evaluate"] += 1
        rc = self.L.td_evaluate(ctx, _p(xCell), _p(yCell), _p(zCell), _p(zeta), len(xCell), 0,
                                _p(ptS), ctypes.byref(phi), ctypes.byref(lik), C_NULL)  # [6]-[10]
        self.tdcheck(rc, ctx)  # [11]
        model_phi, model_ptS = phi.value, ptS  # [12]
        return model_phi, model_ptS, 1  # [13]

    def Interpolation(self, model, X, Y, Z):  # noqa: N802 -- the reference's name
        if self.interp_style != 1:  # [0]
            raise ValueError("tdstar: only interp_style 1 (MCsub.jl:326)")
        X, Y, Z = (np.array(a, dtype=np.float64).reshape(-1) for a in (X, Y, Z))  # [1] (collect copies)
        zeta, np_ = np.zeros(len(X)), ctypes.c_int64(0)  # [2]
        ctx = self.tdctx0() if self.TDCTX.value is None else self.TDCTX  # [3]
        xCell, yCell, zCell, mzeta = (_vec(a) for a in model)  # [4]
        self.calls["td_interpolate"] += 1
        rc = self.L.td_interpolate(ctx, _p(xCell), _p(yCell), _p(zCell), _p(mzeta), len(xCell),
                                   _p(X), len(X), _p(Y), len(Y), _p(Z), len(Z), _p(zeta), C_NULL,
                                   ctypes.byref(np_))  # [5]-[10]
        self.tdcheck(rc, ctx)  # [11]
        return zeta[:np_.value]  # [12]

    # ---- not the shim's: what a test needs around it
    def forward(self, dataStruct, debug_prior=0):
        """The pair oracle.chain_ref.run(forward=...) takes: the host's two calls, evaluate(modeln, dataStruct,
        TD_parameters) and Interpolation(TD_parameters, model, [x], [y], [z])[1]."""
        return (lambda cells: self.evaluate(cells, dataStruct, debug_prior),
                lambda cells, x, y, z: float(self.Interpolation(cells, [x], [y], [z])[0]))

    def close(self):
        """td_destroy of whatever contexts were made (Julia never calls it: they live as long as the worker)."""
        for ref in (self.TDCTX, self.TDCTX0):
            if ref.value is not None:
                self.L.td_destroy(ref)
                ref.value = None
