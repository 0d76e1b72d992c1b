// sym_eigen.cpp — kgwas_sym_eigen: the symmetric fp64 eigendecomposition K = U diag(d) U^T behind lmm_lrt (lmm.cpp).
//
// Householder tridiagonalisation, implicit QL with Wilkinson shifts on the tridiagonal (d, e), and the eigenvectors from the
// recorded plane rotations and reflectors. Written here: libkgwas.so links no ROCm library (Makefile), and the work is one
// decomposition per run. The steps:
//   1. reflectors H_0 .. H_{n-3}, H_k = I - v_k v_k^T / h_k acting on rows and columns k+1 .. n-1, one at a time on the full
//      symmetric matrix (p = A v / h, q = p - (v.p / 2h) v, A -= v q^T + q v^T);
//   2. QL on (d, e) alone; every rotation (i, c, s) is appended to a list;
//   3. Z = I, then every rotation on columns i, i+1 of Z. Z is held transposed (a column is contiguous) and the threads own
//      disjoint slices of the rows: element-wise work, so the result does not depend on the number of threads;
//   4. U = H_0 .. H_{n-3} Z: the reflectors in reverse order on every eigenvector, eigenvectors split over the threads, each dot
//      product in index order;
//   5. eigenvalues ascending (a stable sort, so equal ones keep the order QL left them in), U's columns with them.
// Steps 1 and 2 run on the calling thread. -ffp-contract=off (Makefile) keeps vectorised and scalar loop bodies identical.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "common.h"

using namespace kgwas;

namespace {

struct Rot {
    uint32_t i;
    double c, s;
};

// A (n x n, both triangles, destroyed) -> diagonal d[n], sub-diagonal e[n] (e[k] couples k and k+1; e[n-1] = 0), reflector
// vectors in V (row k: v_k in entries k+1 .. n-1) and hs[k] (0: no reflector).
void tridiagonalise(uint64_t n, double* A, double* d, double* e, double* V, double* hs) {
    std::vector<double> p(n), q(n);
    for (uint64_t k = 0; k + 2 < n; k++) {
        double* v = V + k * n;
        double scale = 0;
        for (uint64_t i = k + 1; i < n; i++) scale = std::max(scale, std::fabs(A[i * n + k]));
        double tail = 0;  // anything below the sub-diagonal?
        for (uint64_t i = k + 2; i < n; i++) tail = std::max(tail, std::fabs(A[i * n + k]));
        hs[k] = 0;
        if (tail == 0) {
            e[k] = A[(k + 1) * n + k];
            continue;
        }
        double ss = 0;
        for (uint64_t i = k + 1; i < n; i++) {
            v[i] = A[i * n + k] / scale;
            ss += v[i] * v[i];
        }
        const double norm = std::sqrt(ss);
        const double alpha = v[k + 1] > 0 ? -norm : norm;
        const double h = ss - v[k + 1] * alpha;  // v.v / 2 after v[k+1] -= alpha
        v[k + 1] -= alpha;
        hs[k] = h;
        e[k] = alpha * scale;
        // p = A22 v / h
        for (uint64_t i = k + 1; i < n; i++) {
            const double* a = A + i * n;
            double s = 0;
            for (uint64_t j = k + 1; j < n; j++) s += a[j] * v[j];
            p[i] = s / h;
        }
        double vp = 0;
        for (uint64_t i = k + 1; i < n; i++) vp += v[i] * p[i];
        const double kc = vp / (2 * h);
        for (uint64_t i = k + 1; i < n; i++) q[i] = p[i] - kc * v[i];
        for (uint64_t i = k + 1; i < n; i++) {
            double* a = A + i * n;
            const double vi = v[i], qi = q[i];
            for (uint64_t j = k + 1; j < n; j++) a[j] -= vi * q[j] + qi * v[j];
        }
    }
    for (uint64_t k = 0; k < n; k++) d[k] = A[k * n + k];
    if (n >= 2) e[n - 2] = A[(n - 1) * n + (n - 2)];
    e[n - 1] = 0;
}

// Implicit QL with Wilkinson shifts; d becomes the eigenvalues, the rotations go to rots in the order they are applied.
void ql_implicit(uint64_t n, double* d, double* e, std::vector<Rot>& rots) {
    const double eps = 2.220446049250313e-16;
    // an off-diagonal entry is negligible against its neighbours or against the matrix: the second test is what ends the
    // iteration inside a cluster of zero eigenvalues (a kinship matrix of duplicated individuals or of rank below n)
    double anorm = 0;
    for (uint64_t i = 0; i < n; i++) anorm = std::max(anorm, std::fabs(d[i]) + std::fabs(e[i]));
    for (uint64_t l = 0; l < n; l++) {
        for (int iter = 0;; iter++) {
            uint64_t m = l;
            for (; m + 1 < n; m++) {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= eps * dd || std::fabs(e[m]) <= eps * anorm) break;
            }
            if (m == l) break;
            if (iter == 300) throw Error(KGWAS_ERR_STATE, "kgwas_sym_eigen: QL did not converge");
            double g = (d[l + 1] - d[l]) / (2 * e[l]);
            double r = std::hypot(g, 1.0);
            g = d[m] - d[l] + e[l] / (g + (g >= 0 ? std::fabs(r) : -std::fabs(r)));
            double s = 1, c = 1, p = 0;
            uint64_t i = m;
            bool underflow = false;
            while (i-- > l) {
                double f = s * e[i];
                const double b = c * e[i];
                r = std::hypot(f, g);
                e[i + 1] = r;
                if (r == 0) {
                    d[i + 1] -= p;
                    e[m] = 0;
                    underflow = true;
                    break;
                }
                s = f / r;
                c = g / r;
                g = d[i + 1] - p;
                r = (d[i] - g) * s + 2 * c * b;
                p = s * r;
                d[i + 1] = g + p;
                g = c * r - b;
                rots.push_back({(uint32_t)i, c, s});
            }
            if (underflow) continue;
            d[l] -= p;
            e[l] = g;
            e[m] = 0;
        }
    }
}

}  // namespace

extern "C" int kgwas_sym_eigen(uint64_t n, const double* K, double* d, double* U, uint32_t threads) {
    return guarded([&] {
        if (!n || !K || !d || !U) throw Error(KGWAS_ERR_ARG, "kgwas_sym_eigen: null or empty argument");
        if (n >= (1ull << 16)) throw Error(KGWAS_ERR_ARG, "kgwas_sym_eigen: more than 65535 rows");
        for (uint64_t i = 0; i < n * n; i++)
            if (!std::isfinite(K[i])) throw Error(KGWAS_ERR_FORMAT, "kgwas_sym_eigen: the matrix holds a value that is not finite");
        if (!threads) threads = kgwas_host_cpu_quota();
        threads = std::max<uint32_t>(1, std::min<uint32_t>(threads, 256));
        // the symmetric part, so that both triangles agree
        std::vector<double> A(n * n), V(n * n, 0.0), hs(n, 0.0), e(n, 0.0), dd(n);
        for (uint64_t i = 0; i < n; i++)
            for (uint64_t j = 0; j <= i; j++) A[i * n + j] = A[j * n + i] = 0.5 * (K[i * n + j] + K[j * n + i]);
        tridiagonalise(n, A.data(), dd.data(), e.data(), V.data(), hs.data());
        std::vector<double>().swap(A);
        std::vector<Rot> rots;
        rots.reserve(2 * n * n);
        ql_implicit(n, dd.data(), e.data(), rots);
        // Zt[i * n + k] = Z[k][i]
        std::vector<double> Zt(n * n, 0.0);
        for (uint64_t i = 0; i < n; i++) Zt[i * n + i] = 1;
        const uint64_t slice = 64;  // rows of Z per work item
        {
            std::atomic<uint64_t> next{0};
            kgwas_run_on_threads(threads, "kgwas-eig-rot", [&] {
                for (uint64_t k0; (k0 = next.fetch_add(slice)) < n;) {
                    const uint64_t k1 = std::min(n, k0 + slice);
                    for (const Rot& r : rots) {
                        double* z0 = Zt.data() + (uint64_t)r.i * n;
                        double* z1 = z0 + n;
                        const double c = r.c, s = r.s;
                        for (uint64_t k = k0; k < k1; k++) {
                            const double f = z1[k];
                            z1[k] = s * z0[k] + c * f;
                            z0[k] = c * z0[k] - s * f;
                        }
                    }
                }
            });
        }
        std::vector<Rot>().swap(rots);
        {
            std::atomic<uint64_t> next{0};
            kgwas_run_on_threads(threads, "kgwas-eig-refl", [&] {
                for (uint64_t i; (i = next.fetch_add(1)) < n;) {
                    double* z = Zt.data() + i * n;
                    for (uint64_t k = n < 2 ? 0 : n - 2; k-- > 0;) {
                        if (hs[k] == 0) continue;
                        const double* v = V.data() + k * n;
                        double s = 0;
                        for (uint64_t j = k + 1; j < n; j++) s += v[j] * z[j];
                        s /= hs[k];
                        for (uint64_t j = k + 1; j < n; j++) z[j] -= s * v[j];
                    }
                }
            });
        }
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return dd[a] < dd[b]; });
        for (uint64_t c = 0; c < n; c++) {
            d[c] = dd[order[c]];
            const double* z = Zt.data() + (uint64_t)order[c] * n;
            for (uint64_t k = 0; k < n; k++) U[k * n + c] = z[k];
        }
    });
}
