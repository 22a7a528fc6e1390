"""oracle/predict.py -- TEST INFRASTRUCTURE: ctypes view of the prediction / solve entries of oracle/predict_sweep.h.

Each function runs in quad (oracle/celerite_quad.c, the truth) or, with ``c64=True``, in float64 with celerite's phase
at the absolute time (oracle/celerite_ref.c).  ``reverse`` sweeps the time-reversed series: K^-1 b and diag(K^-1) are
equivariant under reversal, so it is a second, independent rounding path to the same values.  Inputs follow
oracle/quad.py: dy as given to the reference (yerr = fl64(dy + 1e-12) is formed inside), full parameter vectors
(kernel parameters, then the mean's: 1 constant or (slope, intercept) under mean_kind 1).
"""
import ctypes
from types import SimpleNamespace

import numpy as np

from oracle import celerite as _c64
from oracle import quad as _quad

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_L, _I = ctypes.c_long, ctypes.c_int
_declared = {}


def _lib(c64):
    if c64 not in _declared:
        h = _c64.lib() if c64 else _quad.lib()
        pre = "oracle_" if c64 else "oracle_quad_"
        fns = {}
        for name, args in (
                ("predict_batch", [_L, _L, _dp, _dp, _dp, _I, _ip, _dp, _I, _I, _L, _dp, _ip, _I, _I,
                                   _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
                ("apply_inverse", [_L, _dp, _dp, _I, _ip, _dp, _dp, _L, _dp, _I, _I, _dp, _dp, _dp]),
                ("predict_at", [_L, _dp, _dp, _dp, _I, _ip, _dp, _I, _dp, _L, _dp, _I, _I,
                                _dp, _dp, _dp, _dp, _dp, _dp])):
            fn = getattr(h, pre + name)
            fn.restype, fn.argtypes = ctypes.c_int, args
            fns[name] = fn
        _declared[c64] = fns
    return _declared[c64]


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _kinds(kinds, extra):
    kinds = np.ascontiguousarray(kinds, dtype=np.int32)
    return kinds, _d(np.full(len(kinds), 0.01) if extra is None else extra)


def predict(t, y, dy, kinds, params_full, lc_index=None, mean_kind=0, extra=None, reverse=False, c64=False,
            nthreads=None):
    """Engine.predict's quantities for B rows -> namespace of mu, var, s_mu, s_var, mu_lo, var_lo (each [B][N]) and
    status [B].  mu leaves a constant mean out (the kernels see it as y_offset) and adds a linear one; var is
    noise-free; s_mu = |r| + d |K^-1 r| and s_var = d + d^2 (K^-1)_nn are the scales of the cancellations in mu and var
    (d = yerr^2 + jitter); mu + mu_lo, var + var_lo are the values to the arithmetic's resolution (lo = 0 for c64)."""
    t, y, dy, L, N = _quad._series(t, y, dy)
    params = np.atleast_2d(_d(params_full))
    B, PF = params.shape
    kinds, extra = _kinds(kinds, extra)
    lc, lp = _quad._lc(lc_index, B, L)
    outs = [np.empty((B, N)) for _ in range(6)]
    status = np.zeros(B, dtype=np.int32)
    rc = _lib(c64)["predict_batch"](N, L, _p(t), _p(y), _p(dy), len(kinds), kinds.ctypes.data_as(_ip), _p(extra),
                                    int(mean_kind), PF, B, _p(params), lp, int(bool(reverse)),
                                    _quad._threads(nthreads), *[_p(o) for o in outs], status.ctypes.data_as(_ip))
    if rc != 0:
        raise RuntimeError("predict_batch failed (unknown term kind)")
    return SimpleNamespace(status=status, **dict(zip(("mu", "var", "s_mu", "s_var", "mu_lo", "var_lo"), outs)))


def apply_inverse(t, dy, kinds, params_full, b, extra=None, reverse=False, c64=False, residual=False, nthreads=None):
    """K^-1 b for b [N] or [N][M] at one parameter vector -> namespace of x, x_lo, residual (None unless asked) and
    status.  residual: K x - b of the solution before it is rounded to double, with the semiseparable product in the
    same arithmetic."""
    t = _d(t)
    dy = _d(dy)
    N = len(t)
    b = _d(b)
    one = b.ndim == 1
    b = np.ascontiguousarray(b.reshape(N, -1))
    M = b.shape[1]
    kinds, extra = _kinds(kinds, extra)
    x, lo = np.empty_like(b), np.empty_like(b)
    res = np.empty_like(b) if residual else None
    st = _lib(c64)["apply_inverse"](N, _p(t), _p(dy), len(kinds), kinds.ctypes.data_as(_ip), _p(extra),
                                    _p(_d(params_full)), M, _p(b), int(bool(reverse)), _quad._threads(nthreads),
                                    _p(x), _p(lo), _p(res))
    if one:
        x, lo = x[:, 0], lo[:, 0]
        res = None if res is None else res[:, 0]
    return SimpleNamespace(x=x, x_lo=lo, residual=res, status=int(st))


def predict_at(t, y, dy, kinds, params_full, ts, mean_kind=0, extra=None, reverse=False, c64=False, nthreads=None):
    """GP.predict(y, t=ts, return_var=True) -> namespace of mu, var, s_mu, s_var, mu_lo, var_lo (each [Ns]) and
    status.  mu includes the whole mean; s_mu = |mean(ts)| + sum |k_* K^-1 r|, s_var = k(0) + |k_*^T K^-1 k_*|."""
    t, y, dy, ts = _d(t), _d(y), _d(dy), _d(np.atleast_1d(ts))
    N, Ns = len(t), len(ts)
    assert y.shape == (N,) and dy.shape == (N,)
    kinds, extra = _kinds(kinds, extra)
    outs = [np.empty(Ns) for _ in range(6)]
    st = _lib(c64)["predict_at"](N, _p(t), _p(y), _p(dy), len(kinds), kinds.ctypes.data_as(_ip), _p(extra),
                                 int(mean_kind), _p(_d(params_full)), Ns, _p(ts), int(bool(reverse)),
                                 _quad._threads(nthreads), *[_p(o) for o in outs])
    return SimpleNamespace(status=int(st), **dict(zip(("mu", "var", "s_mu", "s_var", "mu_lo", "var_lo"), outs)))
