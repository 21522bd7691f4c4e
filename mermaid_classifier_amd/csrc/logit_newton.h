// logit_newton.h -- the host half of logit calibration (include/mmc.h, "logit calibration"): the damped Newton iteration over the
// affine map z' = a (.) z + c of stored logits.  Host only, no HIP: logit_scaling.hip feeds it the device sums, and
// tests/host/logit_newton_check.cpp compiles it alone.  Everything is float64.
//
// Parameters theta = (a, c) in R^2K; a mode picks the ACTIVE parameters, in this order:
//   TEMPERATURE   [s]                    a = s 1, c = 0
//   BIAS          [c_k : k live]         a = 1
//   VECTOR        [a_k : k live] then [c_k : k live]
// A class is live unless frozen (no stored row carries it); frozen classes stay at a_k = 1, c_k = 0 in BIAS and VECTOR.
// TEMPERATURE has one parameter whatever the counts are (every class moves with s, so an absent class cannot run away alone).
//
// Objective: F = data term + (l2 N / 2) (|a - 1|^2 + |c|^2).  reduce() adds the ridge to the full gradient / Hessian
// (l2 N (a - 1), l2 N c; l2 N on the diagonal) and then projects: TEMPERATURE sums the a-gradient and the a-a block, the other
// modes select rows and columns.
//
// Step: d solves (H + lambda tau I) d = -g by Cholesky, tau = trace(H) / dim (1 when the trace is not positive).  The damping is
// a multiple of the IDENTITY: with nothing frozen the shift c -> c + t 1 is a null direction of H, g is orthogonal to it, and so
// is every d -- c keeps mean zero from the start c = 0.  A factorisation that meets a non-positive pivot fails; the caller
// raises lambda and tries again.
//
// Rule (fit()): lambda = 1e-3.  Evaluate F, g, H at the start.  Repeat until max|g_active| / N <= tol or `max_trials` trial points
// have been evaluated: solve for d (lambda <- 8 lambda while the factorisation fails, at most 60 times); evaluate F at theta + d (a
// trial point, without the Hessian); accept iff F_trial is finite and F_trial <= F, then lambda <- max(lambda / 8, 1e-12) and g, H
// are taken at the new point; otherwise lambda <- 8 lambda.  The result is the last accepted point -- finite by construction.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace logit_newton {

enum { TEMPERATURE = 0, BIAS = 1, VECTOR = 2 };

constexpr double kLambdaStart = 1e-3, kLambdaFactor = 8.0, kLambdaMin = 1e-12;
constexpr int kMaxRaises = 60;   // 8^60: past every finite trace ratio

inline int live_classes(int K, const uint8_t* frozen)
{
    int n = 0;
    for (int k = 0; k < K; ++k) n += frozen[k] ? 0 : 1;
    return n;
}

inline int active_dim(int K, int mode, const uint8_t* frozen)
{
    if (mode == TEMPERATURE) return 1;
    const int live = live_classes(K, frozen);
    return mode == BIAS ? live : 2 * live;
}

// frozen[k] = 1 where no row carries class k (BIAS / VECTOR); TEMPERATURE freezes nothing
inline void frozen_mask(int K, int mode, const int64_t* counts, uint8_t* frozen)
{
    for (int k = 0; k < K; ++k) frozen[k] = mode != TEMPERATURE && counts[k] == 0 ? 1 : 0;
}

// index into theta = (a[0..K), c[0..K)) of every active parameter of BIAS / VECTOR, in active order
inline std::vector<int> active_index(int K, int mode, const uint8_t* frozen)
{
    std::vector<int> idx;
    if (mode == VECTOR)
        for (int k = 0; k < K; ++k)
            if (!frozen[k]) idx.push_back(k);
    if (mode == BIAS || mode == VECTOR)
        for (int k = 0; k < K; ++k)
            if (!frozen[k]) idx.push_back(K + k);
    return idx;
}

inline double ridge_term(int K, double l2N, const double* a, const double* c)
{
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += (a[k] - 1.0) * (a[k] - 1.0) + c[k] * c[k];
    return 0.5 * l2N * s;
}

// data-term gradient g (2K) and Hessian H (2K x 2K row-major, may be null) at (a, c) -> the active gradient gr (dim) and Hessian
// Hr (dim x dim, only when H is given), ridge included.
inline void reduce(int K, int mode, const uint8_t* frozen, double l2N, const double* a, const double* c, const double* g, const double* H,
                   std::vector<double>& gr, std::vector<double>& Hr)
{
    const int P = 2 * K;
    if (mode == TEMPERATURE) {
        double gs = 0.0, hs = 0.0;
        for (int k = 0; k < K; ++k) gs += g[k] + l2N * (a[k] - 1.0);
        gr.assign(1, gs);
        if (H) {
            for (int k = 0; k < K; ++k)
                for (int l = 0; l < K; ++l) hs += H[(size_t)k * P + l];
            Hr.assign(1, hs + l2N * K);
        }
        return;
    }
    const std::vector<int> idx = active_index(K, mode, frozen);
    const int n = (int)idx.size();
    gr.resize(n);
    for (int i = 0; i < n; ++i) {
        const int p = idx[i];
        gr[i] = g[p] + l2N * (p < K ? a[p] - 1.0 : c[p - K]);
    }
    if (H) {
        Hr.resize((size_t)n * n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) Hr[(size_t)i * n + j] = H[(size_t)idx[i] * P + idx[j]] + (i == j ? l2N : 0.0);
    }
}

// In-place Cholesky A = L L^T of the symmetric n x n matrix (lower triangle written), then x = A^-1 b.  false when a pivot is not
// positive and finite: A is not (numerically) positive definite.
inline bool cholesky_solve(int n, std::vector<double>& A, const std::vector<double>& b, std::vector<double>& x)
{
    for (int j = 0; j < n; ++j) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double l = std::sqrt(d);
        A[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; ++i) {
            double s = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = s / l;
        }
    }
    x.assign(n, 0.0);
    for (int i = 0; i < n; ++i) {   // L y = b
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= A[(size_t)i * n + k] * x[k];
        x[i] = s / A[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {   // L^T x = y
        double s = x[i];
        for (int k = i + 1; k < n; ++k) s -= A[(size_t)k * n + i] * x[k];
        x[i] = s / A[(size_t)i * n + i];
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return false;
    return true;
}

inline double damping_scale(int n, const std::vector<double>& Hr)
{
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += Hr[(size_t)i * n + i];
    const double tau = tr / n;
    return tau > 0.0 && std::isfinite(tau) ? tau : 1.0;
}

// d = -(Hr + lambda tau I)^-1 gr; false when the damped matrix is not positive definite
inline bool damped_step(int n, const std::vector<double>& Hr, const std::vector<double>& gr, double lambda, std::vector<double>& d)
{
    std::vector<double> A = Hr, rhs(n);
    const double shift = lambda * damping_scale(n, Hr);
    for (int i = 0; i < n; ++i) {
        A[(size_t)i * n + i] += shift;
        rhs[i] = -gr[i];
    }
    return cholesky_solve(n, A, rhs, d);
}

// (a, c) + the active step d -> (a2, c2)
inline void apply_step(int K, int mode, const uint8_t* frozen, const double* a, const double* c, const std::vector<double>& d, double* a2,
                       double* c2)
{
    for (int k = 0; k < K; ++k) { a2[k] = a[k]; c2[k] = c[k]; }
    if (mode == TEMPERATURE) {
        for (int k = 0; k < K; ++k) a2[k] = a[0] + d[0];
        return;
    }
    const std::vector<int> idx = active_index(K, mode, frozen);
    for (size_t i = 0; i < idx.size(); ++i) {
        const int p = idx[i];
        if (p < K) a2[p] += d[i];
        else c2[p - K] += d[i];
    }
}

inline double max_abs(const std::vector<double>& v)
{
    double m = 0.0;
    for (double x : v) m = std::fmax(m, std::fabs(x));
    return m;
}

struct FitResult {
    double f_before = 0.0, f_after = 0.0;   // data term at the start and at the returned point (sums, not means)
    int trials = 0, converged = 0;
};

// The rule in the header comment.  eval(a, c, want_hess, &data_term, g[2K], H[2K x 2K]) -> 0, or an error code that fit() hands
// back; H is only written when want_hess.  a / c (K each) are outputs: the start is the identity.  Returns 0, an eval error, or
// -1 when the data term at the identity is not finite.
template <typename Eval>
int fit(int K, int mode, double l2, double tol, int max_trials, int64_t N, const uint8_t* frozen, Eval&& eval, double* a, double* c,
        FitResult* out)
{
    const int P = 2 * K, n = active_dim(K, mode, frozen);
    const double l2N = l2 * (double)N;
    for (int k = 0; k < K; ++k) { a[k] = 1.0; c[k] = 0.0; }
    std::vector<double> g(P), H((size_t)P * P), gt(P), gr, Hr, d, unused;
    std::vector<double> a2(K), c2(K);
    double fd = 0.0;
    int r = eval(a, c, true, &fd, g.data(), H.data());
    if (r) return r;
    if (!std::isfinite(fd)) return -1;
    out->f_before = out->f_after = fd;
    out->trials = 0;
    out->converged = 0;
    if (n == 0) {   // every class frozen: nothing to fit
        out->converged = 1;
        return 0;
    }
    double F = fd + ridge_term(K, l2N, a, c);
    reduce(K, mode, frozen, l2N, a, c, g.data(), H.data(), gr, Hr);
    double lambda = kLambdaStart;
    while (true) {
        if (max_abs(gr) / (double)N <= tol) { out->converged = 1; break; }
        if (out->trials >= max_trials) break;
        int raises = 0;
        while (!damped_step(n, Hr, gr, lambda, d) && raises < kMaxRaises) { lambda *= kLambdaFactor; ++raises; }
        if (raises >= kMaxRaises) break;
        apply_step(K, mode, frozen, a, c, d, a2.data(), c2.data());
        double ft = 0.0;
        r = eval(a2.data(), c2.data(), false, &ft, gt.data(), nullptr);
        if (r) return r;
        ++out->trials;
        const double Ft = ft + ridge_term(K, l2N, a2.data(), c2.data());
        if (std::isfinite(Ft) && Ft <= F) {
            for (int k = 0; k < K; ++k) { a[k] = a2[k]; c[k] = c2[k]; }
            F = Ft;
            out->f_after = ft;
            lambda = std::fmax(lambda / kLambdaFactor, kLambdaMin);
            reduce(K, mode, frozen, l2N, a, c, gt.data(), nullptr, gr, unused);
            if (max_abs(gr) / (double)N <= tol) { out->converged = 1; break; }
            r = eval(a, c, true, &fd, g.data(), H.data());   // the Hessian at the accepted point (same data term and gradient)
            if (r) return r;
            reduce(K, mode, frozen, l2N, a, c, g.data(), H.data(), gr, Hr);
        } else {
            lambda *= kLambdaFactor;
        }
    }
    return 0;
}

}  // namespace logit_newton
