// logit_newton_check.cpp -- csrc/logit_newton.h on the CPU: its own main, no HIP.  tests/test_logit_newton_host.py compiles and runs
// it; it may also be built with -fsanitize=address,undefined as it stands.
//   1. Cholesky on a known SPD system and on a singular matrix (refused); the identity damping rescues the singular one and keeps the
//      step orthogonal to the null direction.
//   2. The mode reductions against hand-computed values, ridge included.
//   3. The frozen-class mask and the active parameter lists.
//   4. A full fit, all three modes, on a 12-row K = 3 problem whose sums are computed right here: max|g| / N <= tol.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mermaid_classifier_amd/csrc/logit_newton.h"

namespace ln = logit_newton;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static bool close(double a, double b, double tol = 1e-12) { return std::fabs(a - b) <= tol * (1.0 + std::fabs(b)); }

static void test_cholesky()
{
    std::vector<double> A = {4, 2, 2, 3}, b = {2, 1}, x;
    CHECK(ln::cholesky_solve(2, A, b, x));
    CHECK(close(x[0], 0.5) && close(x[1], 0.0, 1e-15));
    std::vector<double> S = {1, -1, -1, 1}, g = {1, -1}, d;   // singular: null direction (1, 1); g is orthogonal to it
    std::vector<double> S2 = S;
    CHECK(!ln::cholesky_solve(2, S2, g, d));
    CHECK(ln::damped_step(2, S, g, 1e-3, d));   // tau = trace / 2 = 1: (S + 1e-3 I) d = -g -> d = -g / 2.001
    CHECK(close(d[0], -1.0 / 2.001) && close(d[1], 1.0 / 2.001));
    CHECK(std::fabs(d[0] + d[1]) <= 2001.0 * 4.0 * 2.3e-16);   // orthogonal to the null direction, to the system's condition number (2001) in ulps
    std::vector<double> Zero = {0, 0, 0, 0};
    CHECK(close(ln::damping_scale(2, Zero), 1.0));   // no positive trace: the scale falls back to 1
    CHECK(ln::damped_step(2, Zero, g, 0.5, d) && close(d[0], -2.0) && close(d[1], 2.0));
    std::vector<double> Neg = {-1, 0, 0, -1};
    CHECK(!ln::damped_step(2, Neg, g, 1e-3, d));
}

static void test_reductions()
{
    const int K = 2;
    const double g[4] = {1, 2, 3, 4};
    double H[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) H[i * 4 + j] = (i + 1) * (j + 1);
    const uint8_t none[2] = {0, 0}, second[2] = {0, 1};
    const double a1[2] = {1, 1}, c0[2] = {0, 0}, a15[2] = {1.5, 1.5}, c2[2] = {0.25, -0.5};
    std::vector<double> gr, Hr;
    ln::reduce(K, ln::TEMPERATURE, none, 0.0, a1, c0, g, H, gr, Hr);
    CHECK(gr.size() == 1 && close(gr[0], 3.0) && close(Hr[0], 9.0));
    ln::reduce(K, ln::TEMPERATURE, none, 0.5, a15, c0, g, H, gr, Hr);   // ridge: 0.5 (0.5 + 0.5) on g, 0.5 K on H
    CHECK(close(gr[0], 3.5) && close(Hr[0], 10.0));
    ln::reduce(K, ln::BIAS, none, 2.0, a1, c2, g, H, gr, Hr);
    CHECK(gr.size() == 2 && close(gr[0], 3.0 + 0.5) && close(gr[1], 4.0 - 1.0));
    CHECK(close(Hr[0], 9.0 + 2.0) && close(Hr[1], 12.0) && close(Hr[2], 12.0) && close(Hr[3], 16.0 + 2.0));
    ln::reduce(K, ln::VECTOR, second, 0.0, a1, c0, g, H, gr, Hr);   // class 1 frozen: a_0 and c_0 remain
    CHECK(gr.size() == 2 && close(gr[0], 1.0) && close(gr[1], 3.0));
    CHECK(close(Hr[0], 1.0) && close(Hr[1], 3.0) && close(Hr[2], 3.0) && close(Hr[3], 9.0));
    ln::reduce(K, ln::VECTOR, none, 0.0, a1, c0, g, nullptr, gr, Hr);   // gradient only
    CHECK(gr.size() == 4 && close(gr[3], 4.0));
    CHECK(close(ln::ridge_term(K, 2.0, a15, c2), 0.5 * 2.0 * (0.25 + 0.25 + 0.0625 + 0.25)));
    double a2[2], cc2[2];
    ln::apply_step(K, ln::TEMPERATURE, none, a15, c0, std::vector<double>{0.25}, a2, cc2);
    CHECK(close(a2[0], 1.75) && close(a2[1], 1.75) && cc2[0] == 0.0);
    ln::apply_step(K, ln::VECTOR, second, a1, c0, std::vector<double>{0.5, -0.25}, a2, cc2);
    CHECK(close(a2[0], 1.5) && a2[1] == 1.0 && close(cc2[0], -0.25) && cc2[1] == 0.0);
}

static void test_frozen()
{
    const int64_t counts[3] = {3, 0, 2};
    uint8_t fz[3];
    ln::frozen_mask(3, ln::BIAS, counts, fz);
    CHECK(fz[0] == 0 && fz[1] == 1 && fz[2] == 0);
    CHECK(ln::active_dim(3, ln::BIAS, fz) == 2 && ln::active_dim(3, ln::VECTOR, fz) == 4);
    const std::vector<int> idx = ln::active_index(3, ln::VECTOR, fz);
    CHECK(idx.size() == 4 && idx[0] == 0 && idx[1] == 2 && idx[2] == 3 && idx[3] == 5);
    ln::frozen_mask(3, ln::TEMPERATURE, counts, fz);
    CHECK(fz[0] == 0 && fz[1] == 0 && fz[2] == 0 && ln::active_dim(3, ln::TEMPERATURE, fz) == 1);
}

// the definition of include/mmc.h in plain C++ on a tiny problem
struct Problem {
    int N, K;
    std::vector<double> z;
    std::vector<int> y;
    int evals = 0;
    int operator()(const double* a, const double* c, bool want_hess, double* f, double* g, double* H)
    {
        ++evals;
        const int P = 2 * K;
        *f = 0.0;
        for (int i = 0; i < P; ++i) g[i] = 0.0;
        if (want_hess)
            for (int i = 0; i < P * P; ++i) H[i] = 0.0;
        std::vector<double> u(K), p(K), v(P);
        for (int n = 0; n < N; ++n) {
            double m = -INFINITY, s = 0.0;
            for (int k = 0; k < K; ++k) { u[k] = a[k] * z[n * K + k] + c[k]; m = std::fmax(m, u[k]); }
            for (int k = 0; k < K; ++k) { p[k] = std::exp(u[k] - m); s += p[k]; }
            *f += m + std::log(s) - u[y[n]];
            for (int k = 0; k < K; ++k) {
                p[k] /= s;
                const double zk = z[n * K + k], r = p[k] - (k == y[n] ? 1.0 : 0.0);
                g[k] += zk * r;
                g[K + k] += r;
                v[k] = zk * p[k];
                v[K + k] = p[k];
                if (want_hess) {
                    H[k * P + k] += zk * zk * p[k];
                    H[(K + k) * P + K + k] += p[k];
                    H[k * P + K + k] += zk * p[k];
                    H[(K + k) * P + k] += zk * p[k];
                }
            }
            if (want_hess)
                for (int i = 0; i < P; ++i)
                    for (int j = 0; j < P; ++j) H[i * P + j] -= v[i] * v[j];
        }
        return 0;
    }
};

static void test_fit()
{
    Problem pb;
    pb.N = 12;
    pb.K = 3;
    // over-confident scores with some rows on the wrong side
    const double z[12][3] = {{3.1, 0.2, -1.0}, {2.0, 2.4, 0.1}, {-0.5, 3.3, 0.4}, {0.3, 2.2, 2.9}, {1.9, -0.7, 2.5}, {2.8, 0.6, 0.2},
                             {0.1, 1.7, -2.0}, {-1.2, 0.4, 3.0}, {2.2, 2.1, 2.0}, {0.5, -0.3, 1.1}, {3.0, 1.0, 2.6}, {-0.4, 2.6, 1.5}};
    const int y[12] = {0, 0, 1, 1, 2, 1, 1, 2, 2, 0, 2, 1};
    for (int n = 0; n < 12; ++n) {
        for (int k = 0; k < 3; ++k) pb.z.push_back(z[n][k]);
        pb.y.push_back(y[n]);
    }
    const int64_t counts[3] = {3, 5, 4};
    const double tol = 1e-9;
    for (int mode = 0; mode < 3; ++mode) {
        for (double l2 : {0.0, 1e-2}) {
            uint8_t fz[3];
            ln::frozen_mask(3, mode, counts, fz);
            double a[3], c[3];
            ln::FitResult res;
            const int r = ln::fit(3, mode, l2, tol, 100, pb.N, fz, pb, a, c, &res);
            CHECK(r == 0 && res.converged == 1 && res.trials >= 1 && res.trials <= 100);
            CHECK(res.f_after <= res.f_before);
            double f, g[6];
            pb(a, c, false, &f, g, nullptr);
            CHECK(f == res.f_after);
            std::vector<double> gr, unused;
            ln::reduce(3, mode, fz, l2 * pb.N, a, c, g, nullptr, gr, unused);
            CHECK(ln::max_abs(gr) / pb.N <= tol);
            CHECK(std::fabs(c[0] + c[1] + c[2]) / 3.0 <= 1e-9);
            if (mode == ln::TEMPERATURE) CHECK(a[0] == a[1] && a[1] == a[2] && a[0] < 1.0 && c[0] == 0.0);
            if (mode == ln::BIAS) CHECK(a[0] == 1.0 && a[1] == 1.0 && a[2] == 1.0);
            std::printf("mode %d l2 %g: %d trials, F %.12g -> %.12g, max|g|/N %.3g, a = %.6f %.6f %.6f, c = %.6f %.6f %.6f\n", mode, l2,
                        res.trials, res.f_before, res.f_after, ln::max_abs(gr) / pb.N, a[0], a[1], a[2], c[0], c[1], c[2]);
        }
    }
    // a class nobody carries stays at the identity, and one trial is the cap that was asked for
    for (int n = 0; n < 12; ++n)
        if (pb.y[n] == 2) pb.y[n] = 0;
    const int64_t counts2[3] = {7, 5, 0};
    uint8_t fz[3];
    ln::frozen_mask(3, ln::VECTOR, counts2, fz);
    double a[3], c[3];
    ln::FitResult res;
    CHECK(ln::fit(3, ln::VECTOR, 0.0, tol, 100, pb.N, fz, pb, a, c, &res) == 0);
    CHECK(res.converged == 1 && fz[2] == 1 && a[2] == 1.0 && c[2] == 0.0 && a[0] != 1.0);
    CHECK(ln::fit(3, ln::VECTOR, 0.0, 1e-300, 1, pb.N, fz, pb, a, c, &res) == 0);
    CHECK(res.converged == 0 && res.trials == 1 && std::isfinite(a[0]) && std::isfinite(c[1]));
}

int main()
{
    test_cholesky();
    test_reductions();
    test_frozen();
    test_fit();
    if (failures) {
        std::printf("%d checks FAILED\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
