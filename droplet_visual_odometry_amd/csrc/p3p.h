// Track PnP (dvo.h dvo_stream_set_track_pnp): the sample generator and the perspective-three-point
// solver, for the host and the device.  tracks.hip compiles this text into track_pnp_kernel, api.cpp
// into dvo_track_pnp_samples_host and dvo_p3p_host, and tests/track_pnp_check.cpp into a host program.
//
// Every operation below is one of + - * / sqrt in double, rounded once (-ffp-contract=off), in the
// order written; comparisons, negation, |x| and max select exactly.  Every trip count is a constant.
#pragma once

#include <cstdint>

#include "mwc.h"

namespace dvo {

constexpr int kP3pDraws = 8;       // draws a sample may take
constexpr int kP3pBisect = 100;    // halvings of the resolvent's bracket
constexpr int kP3pNewton = 5;      // Newton steps on the three depths
constexpr uint64_t kP3pSeed = ~0ull;  // what seed 0 stands for: the E-RANSAC's

// Sample h of n correspondences: three distinct indices, or false (idx untouched) where 8 draws do
// not give three.  n >= 1.
__host__ __device__ inline bool p3p_sample(uint64_t seed, int h, int n, int* idx) {
    uint64_t s = mwc_jump_by(seed ? seed : kP3pSeed, 8ull * (uint64_t)h);
    int i0 = -1, i1 = -1, i2 = -1;
    for (int d = 0; d < kP3pDraws; ++d) {
        s = mwc_step(s);
        const int i = (int)((uint32_t)s % (uint32_t)n);
        if (i0 < 0)
            i0 = i;
        else if (i1 < 0) {
            if (i != i0) i1 = i;
        } else if (i2 < 0) {
            if (i != i0 && i != i1) i2 = i;
        }
    }
    if (i2 < 0) return false;
    idx[0] = i0, idx[1] = i1, idx[2] = i2;
    return true;
}

__host__ __device__ __forceinline__ bool p3p_finite(double x) { return x - x == 0.0; }

// The poses (R row by row, t: x' = R Y + t) that put the points Y[3 i ..] on the rays of (nu, nv) =
// nunv[2 i ..]: up to 4, in candidate order, into R[s][9], t[s][3].  Returns how many were kept.
__host__ __device__ inline int p3p_solve(const double* Y, const double* nunv, double (*Ro)[9], double (*to)[3]) {
    // the unit bearings, the cosines between them and the squared sides
    double f[3][3];
    for (int i = 0; i < 3; ++i) {
        const double nu = nunv[2 * i], nv = nunv[2 * i + 1];
        const double len = sqrt((nu * nu + nv * nv) + 1);
        f[i][0] = nu / len, f[i][1] = nv / len, f[i][2] = 1 / len;
    }
    const double c01 = (f[0][0] * f[1][0] + f[0][1] * f[1][1]) + f[0][2] * f[1][2];
    const double c02 = (f[0][0] * f[2][0] + f[0][1] * f[2][1]) + f[0][2] * f[2][2];
    const double c12 = (f[1][0] * f[2][0] + f[1][1] * f[2][1]) + f[1][2] * f[2][2];
    double e1[3], e2[3];  // Y1 - Y0, Y2 - Y0
    for (int j = 0; j < 3; ++j) e1[j] = Y[3 + j] - Y[j], e2[j] = Y[6 + j] - Y[j];
    const double a01 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double a02 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    double a12;
    {
        const double g0 = Y[6] - Y[3], g1 = Y[7] - Y[4], g2 = Y[8] - Y[5];
        a12 = (g0 * g0 + g1 * g1) + g2 * g2;
    }
    // With d1 = u d0 and d2 = v d0 the three side equations leave two quadratics in u,
    //   p2 u^2 + p1 u + P0(v) = 0,   q2 u^2 + Q1(v) u + Q0(v) = 0,
    // whose resultant G = A^2 - B C (A = p2 Q0 - P0 q2, B = p2 Q1 - p1 q2, C = p1 Q0 - P0 Q1) is a
    // quartic in v, and u = -A(v) / B(v).  Coefficients from the constant term up.
    const double p2 = a02, p1 = -((2 * a02) * c01), q2 = a12 - a01;
    const double P0[3] = {a02 - a01, (2 * a01) * c02, -a01};
    const double Q1[2] = {-((2 * a12) * c01), (2 * a01) * c12};
    const double Q0[3] = {a12, 0.0, -a01};
    double A[3], B[2], C[4], G[5];
    for (int k = 0; k < 3; ++k) A[k] = p2 * Q0[k] - P0[k] * q2;
    B[0] = p2 * Q1[0] - p1 * q2;
    B[1] = p2 * Q1[1];
    C[0] = p1 * Q0[0] - P0[0] * Q1[0];
    C[1] = p1 * Q0[1] - (P0[0] * Q1[1] + P0[1] * Q1[0]);
    C[2] = p1 * Q0[2] - (P0[1] * Q1[1] + P0[2] * Q1[0]);
    C[3] = -(P0[2] * Q1[1]);
    G[0] = A[0] * A[0] - B[0] * C[0];
    G[1] = 2 * (A[0] * A[1]) - (B[0] * C[1] + B[1] * C[0]);
    G[2] = (2 * (A[0] * A[2]) + A[1] * A[1]) - (B[0] * C[2] + B[1] * C[1]);
    G[3] = 2 * (A[1] * A[2]) - (B[0] * C[3] + B[1] * C[2]);
    G[4] = A[2] * A[2] - B[1] * C[3];
    // monic v^4 + b v^3 + c v^2 + d v + e, depressed by v = y - b / 4 to y^4 + p y^2 + q y + r
    const double b = G[3] / G[4], c = G[2] / G[4], d = G[1] / G[4], e = G[0] / G[4];
    const double b2 = b * b;
    const double p = c - 0.375 * b2;
    const double q = (d - 0.5 * (b * c)) + 0.125 * (b2 * b);
    const double r = ((e - 0.25 * (b * d)) + 0.0625 * (b2 * c)) - 0.01171875 * (b2 * b2);
    // Ferrari's resolvent g(m) = m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8: g(0) <= 0 and g > 0 at
    // Cauchy's bound, so kP3pBisect halvings of [0, bound] close on a root m >= 0; hi is taken
    const double k2 = p, k1 = 0.25 * (p * p) - r, k0 = -(0.125 * (q * q));
    double lo = 0.0, hi;
    {
        const double m2 = k2 < 0 ? -k2 : k2, m1 = k1 < 0 ? -k1 : k1, m0 = k0 < 0 ? -k0 : k0;
        const double mx = m2 > m1 ? m2 : m1;
        hi = 1 + (mx > m0 ? mx : m0);
    }
    for (int it = 0; it < kP3pBisect; ++it) {
        const double mid = 0.5 * (lo + hi);
        const double g = ((mid + k2) * mid + k1) * mid + k0;
        if (g > 0)
            hi = mid;
        else
            lo = mid;
    }
    const double m = hi;
    // y^2 + p / 2 + m = +- s (y - q / (4 m)), s = sqrt(2 m): two quadratics, y = (+-s +- sqrt(disc)) / 2
    const double s = sqrt(2 * m), hh = 0.5 * p + m, w = q / (2 * s);
    const double rt0 = sqrt(s * s - 4 * (hh + w)), rt1 = sqrt(s * s - 4 * (hh - w));
    const double ys[4] = {0.5 * (s + rt0), 0.5 * (s - rt0), 0.5 * (rt1 - s), 0.5 * (-s - rt1)};
    // the world triangle's frame: E1 along Y1 - Y0, E3 the normal, E2 = E3 x E1
    double E1[3], E2[3], E3[3];
    {
        const double l1 = sqrt(a01);
        for (int j = 0; j < 3; ++j) E1[j] = e1[j] / l1;
        const double n0 = E1[1] * e2[2] - E1[2] * e2[1], n1 = E1[2] * e2[0] - E1[0] * e2[2], n2 = E1[0] * e2[1] - E1[1] * e2[0];
        const double l3 = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        E3[0] = n0 / l3, E3[1] = n1 / l3, E3[2] = n2 / l3;
        E2[0] = E3[1] * E1[2] - E3[2] * E1[1];
        E2[1] = E3[2] * E1[0] - E3[0] * E1[2];
        E2[2] = E3[0] * E1[1] - E3[1] * E1[0];
    }
    int kept = 0;
    for (int cand = 0; cand < 4; ++cand) {
        const double v = ys[cand] - 0.25 * b;
        const double u = -(((A[2] * v + A[1]) * v + A[0]) / (B[1] * v + B[0]));
        double d0 = sqrt(a02 / ((1 + v * v) - (2 * v) * c02));
        double d1 = u * d0, d2 = v * d0;
        // Newton on the three side equations: J delta = residual by Cramer's rule
        for (int it = 0; it < kP3pNewton; ++it) {
            const double r0 = ((d0 * d0 + d1 * d1) - (2 * (d0 * d1)) * c01) - a01;
            const double r1 = ((d0 * d0 + d2 * d2) - (2 * (d0 * d2)) * c02) - a02;
            const double r2 = ((d1 * d1 + d2 * d2) - (2 * (d1 * d2)) * c12) - a12;
            const double j00 = 2 * (d0 - d1 * c01), j01 = 2 * (d1 - d0 * c01);
            const double j10 = 2 * (d0 - d2 * c02), j12 = 2 * (d2 - d0 * c02);
            const double j21 = 2 * (d1 - d2 * c12), j22 = 2 * (d2 - d1 * c12);
            const double det = -(j00 * (j12 * j21) + j01 * (j10 * j22));
            const double x = r1 * j22 - j12 * r2;
            const double n0 = -(r0 * (j12 * j21)) - j01 * x;
            const double n1 = j00 * x - r0 * (j10 * j22);
            const double n2 = (r0 * (j10 * j21) - j00 * (r1 * j21)) - j01 * (j10 * r2);
            d0 = d0 - n0 / det;
            d1 = d1 - n1 / det;
            d2 = d2 - n2 / det;
        }
        // the camera triangle's frame from X_i = d_i f_i, then R = sum F_k E_k^T, t = X0 - R Y0
        double X0[3], x1[3], x2[3], F1[3], F2[3], F3[3];
        for (int j = 0; j < 3; ++j) {
            X0[j] = d0 * f[0][j];
            x1[j] = d1 * f[1][j] - X0[j];
            x2[j] = d2 * f[2][j] - X0[j];
        }
        {
            const double l1 = sqrt((x1[0] * x1[0] + x1[1] * x1[1]) + x1[2] * x1[2]);
            for (int j = 0; j < 3; ++j) F1[j] = x1[j] / l1;
            const double n0 = F1[1] * x2[2] - F1[2] * x2[1], n1 = F1[2] * x2[0] - F1[0] * x2[2], n2 = F1[0] * x2[1] - F1[1] * x2[0];
            const double l3 = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            F3[0] = n0 / l3, F3[1] = n1 / l3, F3[2] = n2 / l3;
            F2[0] = F3[1] * F1[2] - F3[2] * F1[1];
            F2[1] = F3[2] * F1[0] - F3[0] * F1[2];
            F2[2] = F3[0] * F1[1] - F3[1] * F1[0];
        }
        double R[9], t[3];
        bool ok = d0 > 0 && d1 > 0 && d2 > 0;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                R[3 * i + j] = (F1[i] * E1[j] + F2[i] * E2[j]) + F3[i] * E3[j];
                ok = ok && p3p_finite(R[3 * i + j]);
            }
            t[i] = X0[i] - ((R[3 * i] * Y[0] + R[3 * i + 1] * Y[1]) + R[3 * i + 2] * Y[2]);
            ok = ok && p3p_finite(t[i]);
        }
        if (ok) {
            for (int i = 0; i < 9; ++i) Ro[kept][i] = R[i];
            for (int i = 0; i < 3; ++i) to[kept][i] = t[i];
            ++kept;
        }
    }
    return kept;
}

}  // namespace dvo
