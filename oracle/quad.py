"""oracle/quad.py -- TEST INFRASTRUCTURE: ctypes view of celerite_quad.c (the quad-precision truth).

Built on first use (``make -C oracle liboracle_quad.so``); see oracle/celerite_quad.c for what is promoted from
float64 and what is formed in quad.  Every entry returns ``(lnL, lnL_lo, scale, status)``: lnL rounded to double,
the remainder of the quad value (lnL + lnL_lo is the truth to ~1e-32 relative), the error scale
S = 1/2 (sum |ln D_n| + sum z_n^2 / D_n + N ln 2 pi), and celerite's status (0 ok, 2 not positive definite, 3 not
finite).
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "liboracle_quad.so")
_lib = None

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("celerite_quad.c", "predict_sweep.h")]
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(map(os.path.getmtime, srcs)):
        subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle_quad.so"], stdout=subprocess.DEVNULL)
    return _SO


def lib():
    global _lib
    if _lib is None:
        build()
        h = ctypes.CDLL(_SO)
        h.oracle_quad_logprob_batch.restype = ctypes.c_int
        h.oracle_quad_logprob_batch.argtypes = [
            ctypes.c_long, ctypes.c_long, _dp, _dp, _dp, ctypes.c_int, _ip, _dp, ctypes.c_int, ctypes.c_int,
            ctypes.c_long, _dp, _ip, ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, _ip]
        h.oracle_quad_coeffs_batch.restype = ctypes.c_int
        h.oracle_quad_coeffs_batch.argtypes = [
            ctypes.c_long, ctypes.c_long, _dp, _dp, _dp, ctypes.c_long, ctypes.c_int, ctypes.c_int,
            _dp, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int, _dp, _ip, ctypes.c_int, ctypes.c_int,
            _dp, _dp, _dp, _ip]
        h.oracle_quad_build_coeffs.restype = ctypes.c_int
        h.oracle_quad_build_coeffs.argtypes = [
            ctypes.c_int, _ip, _dp, _dp, _ip, _dp, _dp, _ip, _dp, _dp, _dp, _dp, _dp]
        _lib = h
    return _lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def default_threads():
    """OMP_NUM_THREADS when set, else the CPUs this process may run on (not the machine's count)."""
    env = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    if env.isdigit() and int(env) > 0:
        return int(env)
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except AttributeError:
        return os.cpu_count() or 1


def _threads(nthreads):
    return int(nthreads) if nthreads else default_threads()


def _series(t, y, dy):
    t = _d(t)
    y, dy = np.atleast_2d(_d(y)), np.atleast_2d(_d(dy))
    L, N = y.shape
    assert t.shape == (N,) and dy.shape == (L, N)
    return t, y, dy, L, N


def _lc(lc_index, B, L):
    if lc_index is None:
        return None, None
    lc = np.ascontiguousarray(lc_index, dtype=np.int32)
    assert lc.shape == (B,) and lc.min() >= 0 and lc.max() < L
    return lc, lc.ctypes.data_as(_ip)


def loglike(t, y, dy, kinds, params_full, lc_index=None, mean_kind=0, extra=None, reverse=False, nthreads=None):
    """lnL(theta) in quad.  params_full: [B][PF] (kernel parameters, then the mean's: 1 constant or (slope, intercept));
    dy as given to the reference (yerr = fl64(dy + 1e-12) is formed inside)."""
    t, y, dy, L, N = _series(t, y, dy)
    params = np.atleast_2d(_d(params_full))
    B, PF = params.shape
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    extra = _d(np.full(len(kinds), 0.01) if extra is None else extra)
    lc, lp = _lc(lc_index, B, L)
    hi, lo, scale = np.empty(B), np.empty(B), np.empty(B)
    status = np.zeros(B, dtype=np.int32)
    rc = lib().oracle_quad_logprob_batch(N, L, _p(t), _p(y), _p(dy), len(kinds), kinds.ctypes.data_as(_ip), _p(extra),
                                         int(mean_kind), PF, B, _p(params), lp, int(bool(reverse)), _threads(nthreads),
                                         _p(hi), _p(lo), _p(scale), status.ctypes.data_as(_ip))
    if rc != 0:
        raise RuntimeError("oracle_quad_logprob_batch failed (unknown term kind or J > 32)")
    return hi, lo, scale, status


def loglike_coeffs(t, y, dy, a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter=None, mean_kind=0,
                   mean_params=None, lc_index=None, reverse=False, nthreads=None):
    """The raw-coefficient entry: float64 coefficients [B][jr] / [B][jc] promoted exactly (Engine.loglike_coeffs)."""
    t, y, dy, L, N = _series(t, y, dy)
    ar, cr = np.atleast_2d(_d(a_real)), np.atleast_2d(_d(c_real))
    ac, bc = np.atleast_2d(_d(a_comp)), np.atleast_2d(_d(b_comp))
    cc, dc = np.atleast_2d(_d(c_comp)), np.atleast_2d(_d(d_comp))
    B = max(ar.shape[0], ac.shape[0])
    jr = ar.shape[1] if ar.size else 0
    jc = ac.shape[1] if ac.size else 0
    for a, j in ((ar, jr), (cr, jr), (ac, jc), (bc, jc), (cc, jc), (dc, jc)):
        assert a.size == 0 and j == 0 or a.shape == (B, j)
    nm = 2 if mean_kind == 1 else 1
    mp = np.zeros((B, nm)) if mean_params is None else _d(np.broadcast_to(np.asarray(mean_params, dtype=np.float64)
                                                                          .reshape(-1, nm), (B, nm)))
    jit = None if jitter is None else _d(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (B,)))
    lc, lp = _lc(lc_index, B, L)
    hi, lo, scale = np.empty(B), np.empty(B), np.empty(B)
    status = np.zeros(B, dtype=np.int32)
    rc = lib().oracle_quad_coeffs_batch(N, L, _p(t), _p(y), _p(dy), B, jr, jc, _p(ar if jr else None),
                                        _p(cr if jr else None), _p(ac if jc else None), _p(bc if jc else None),
                                        _p(cc if jc else None), _p(dc if jc else None), _p(jit), int(mean_kind), _p(mp),
                                        lp, int(bool(reverse)), _threads(nthreads), _p(hi), _p(lo), _p(scale),
                                        status.ctypes.data_as(_ip))
    if rc != 0:
        raise RuntimeError("oracle_quad_coeffs_batch failed (J > 32)")
    return hi, lo, scale, status


def build_coeffs(kinds, params, extra=None):
    """The quad builders rounded to double: (ar, cr, ac, bc, cc, dc, jitter) as oracle.dense.build_coeffs returns them."""
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    p = _d(params)
    extra = _d(np.full(len(kinds), 0.01) if extra is None else extra)
    n = 2 * len(kinds) + 2
    ar, cr, ac, bc, cc, dc = (np.zeros(n) for _ in range(6))
    jr, jc, jit = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0.0)
    rc = lib().oracle_quad_build_coeffs(len(kinds), kinds.ctypes.data_as(_ip), _p(extra), _p(p), ctypes.byref(jr),
                                        _p(ar), _p(cr), ctypes.byref(jc), _p(ac), _p(bc), _p(cc), _p(dc),
                                        ctypes.byref(jit))
    if rc != 0:
        raise ValueError("unknown term kind")
    r, c = jr.value, jc.value
    return ar[:r], cr[:r], ac[:c], bc[:c], cc[:c], dc[:c], jit.value
