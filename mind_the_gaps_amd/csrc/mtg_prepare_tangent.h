// mtg_prepare_tangent.h -- the derivative of every coefficient slot of MtgCoefLayout by ONE free parameter of one
// evaluation: the tangent of mtg_prepare.h's expansion, which it does not touch (the primal coefficients, the prior's
// verdict and the structure sig[e] of a row stay what mtg_prepare_kernel made them).  Every parameter is a logarithm,
// so most tangents ARE the primal coefficient, read back from the workspace; the rest (an SHO term's quality factor,
// Matern-3/2, the jitter) are formed from theta.  An SHO term is differentiated on the side of Q = 1/2 its primal
// expansion took: the same Q = exp(theta) is compared, so the slots counted here are those sig[e] counts.
// tests/loglike_grad_replay.py (coefficients) is the same in numpy.
#pragma once
#include "mtg_device.h"

#include <math.h>

// coef: the row's column of the coefficient workspace (a.coef + e, slot stride cs); th: the row's free parameters;
// p: the free parameter differentiated by; dc: this lane's column of the tangent workspace (slot stride ds).
// Every slot of the layout is written (zero where theta[p] does not reach).
__device__ __forceinline__ void mtg_prepare_tangent_one(const MtgModel &m, const double *th, const double *coef, int64_t cs,
                                                        int p, double *dc, int64_t ds)
{
#pragma clang fp contract(off)
    auto par = [th, &m](int k) -> double {
        const int s = m.src[k];
        return s >= 0 ? th[s] : m.defaults[k];
    };
    const MtgCoefLayout lay{m.nr_max, m.nc_max};
    for (int s = 0; s < lay.nslots(); ++s) dc[s * ds] = 0.0;
    int kf = -1;                                   // index of theta[p] in the full parameter vector
    for (int k = 0; k < m.PF; ++k)
        if (m.src[k] == p) kf = k;
    auto put = [dc, ds](int slot, double v) { dc[slot * ds] = v; };
    auto get = [coef, cs](int slot) -> double { return coef[slot * cs]; };

    int ir = 0, ic = 0;
    double dasum = 0.0;
    for (int i = 0; i < m.nterms; ++i) {
        const int o = m.poff[i], q = kf - o;       // q: which of the term's parameters, when it is this term's
        switch (m.kinds[i]) {
        case MTG_TERM_REAL:
        case MTG_TERM_DRW:
            if (q == 0) { const double av = get(lay.ar(ir)); put(lay.ar(ir), av); dasum += av; }
            if (q == 1) put(lay.cr(ir), get(lay.cr(ir)));
            ++ir;
            break;
        case MTG_TERM_COMPLEX3:
            if (q == 0) { const double av = get(lay.ac(ic)); put(lay.ac(ic), av); dasum += av; }
            if (q == 1) put(lay.cc(ic), get(lay.cc(ic)));
            if (q == 2) put(lay.dc(ic), get(lay.dc(ic)));
            ++ic;
            break;
        case MTG_TERM_COMPLEX4:
            if (q == 0) { const double av = get(lay.ac(ic)); put(lay.ac(ic), av); dasum += av; }
            if (q == 1) put(lay.bc(ic), get(lay.bc(ic)));
            if (q == 2) put(lay.cc(ic), get(lay.cc(ic)));
            if (q == 3) put(lay.dc(ic), get(lay.dc(ic)));
            ++ic;
            break;
        case MTG_TERM_SHO: {
            const double Q = exp(par(o + 1));
            if (Q < 0.5) {  // two real terms
                if (q >= 0 && q < 3) {
                    const double a1 = get(lay.ar(ir)), a2 = get(lay.ar(ir + 1));
                    const double c1 = get(lay.cr(ir)), c2 = get(lay.cr(ir + 1));
                    double da1 = a1, da2 = a2, dc1 = 0.0, dc2 = 0.0;          // ln S0: the amplitudes scale
                    if (q == 2) { dc1 = c1; dc2 = c2; }                        // ln w0: everything scales
                    if (q == 1) {
                        const double S0 = exp(par(o)), w0 = exp(par(o + 2));
                        const double f = sqrt(1.0 - 4.0 * Q * Q);
                        const double g = 4.0 * Q * Q / f;                      // -df / dlnQ; d(1/f) / dlnQ = g / f^2
                        const double h = 0.5 * S0 * w0 * Q;
                        da1 = a1 + h * g / (f * f); da2 = a2 - h * g / (f * f);
                        dc1 = -c1 + 0.5 * w0 / Q * g; dc2 = -c2 - 0.5 * w0 / Q * g;
                    }
                    put(lay.ar(ir), da1); put(lay.ar(ir + 1), da2);
                    put(lay.cr(ir), dc1); put(lay.cr(ir + 1), dc2);
                    dasum += da1; dasum += da2;
                }
                ir += 2;
            } else {
                if (q >= 0 && q < 3) {
                    const double av = get(lay.ac(ic)), bv = get(lay.bc(ic)), cv = get(lay.cc(ic)), dv = get(lay.dc(ic));
                    double db = bv, dcv = 0.0, dd = 0.0;
                    if (q == 2) { dcv = cv; dd = dv; }
                    if (q == 1) {
                        const double g = 4.0 * Q * Q / (4.0 * Q * Q - 1.0);    // dlnf / dlnQ, f = sqrt(4 Q^2 - 1)
                        db = bv * (1.0 - g); dcv = -cv; dd = dv * (g - 1.0);
                    }
                    put(lay.ac(ic), av); put(lay.bc(ic), db); put(lay.cc(ic), dcv); put(lay.dc(ic), dd);
                    dasum += av;
                }
                ++ic;
            }
            break;
        }
        case MTG_TERM_MATERN32:   // a = exp(2 ln sigma), b = w0 a / eps, c = w0 = sqrt(3) exp(-ln rho), d = eps
            if (q == 0) {
                const double av = 2.0 * get(lay.ac(ic));
                put(lay.ac(ic), av); put(lay.bc(ic), 2.0 * get(lay.bc(ic)));
                dasum += av;
            }
            if (q == 1) { put(lay.bc(ic), -get(lay.bc(ic))); put(lay.cc(ic), -get(lay.cc(ic))); }
            ++ic;
            break;
        case MTG_TERM_JITTER:
            if (q == 0) {
                const double jv = 2.0 * exp(2.0 * par(o));
                dasum += jv;
                put(lay.jit(), jv);
            }
            break;
        case MTG_TERM_LORENTZIAN:  // a = S0, b = 0, c = w0 / 2 Q, d = w0
            if (q == 0) { const double av = get(lay.ac(ic)); put(lay.ac(ic), av); dasum += av; }
            if (q == 1) put(lay.cc(ic), -get(lay.cc(ic)));
            if (q == 2) { put(lay.cc(ic), get(lay.cc(ic))); put(lay.dc(ic), get(lay.dc(ic))); }
            ++ic;
            break;
        case MTG_TERM_COSINUS:
            if (q == 0) { const double av = get(lay.ac(ic)); put(lay.ac(ic), av); dasum += av; }
            if (q == 1) put(lay.dc(ic), get(lay.dc(ic)));
            ++ic;
            break;
        case MTG_TERM_BPL:         // c = d = w0
            if (q == 0) { const double av = get(lay.ac(ic)); put(lay.ac(ic), av); dasum += av; }
            if (q == 1) put(lay.bc(ic), get(lay.bc(ic)));
            if (q == 2) { put(lay.cc(ic), get(lay.cc(ic))); put(lay.dc(ic), get(lay.dc(ic))); }
            ++ic;
            break;
        default:
            break;
        }
    }
    put(lay.asum(), dasum);
    // mean(t) = slope * t + intercept
    if (m.mean_kind == MTG_MEAN_LINEAR) {
        if (kf == m.nk) put(lay.mean(0), 1.0);
        if (kf == m.nk + 1) put(lay.mean(1), 1.0);
    } else if (kf == m.nk) {
        put(lay.mean(1), 1.0);
    }
}
