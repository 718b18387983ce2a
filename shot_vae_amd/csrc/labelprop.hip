// Label spreading and label propagation on a CSR graph in three entry points (declared, with the exact definitions, in
// include/shotvae_hip.h):
//   sv_lp_normalize    the degrees of the rows (double, eight lanes per row as sv_tsne_attract) and the iteration matrix: D^-1/2 W D^-1/2
//                      or D^-1 W, every entry formed in double and rounded once
//   sv_lp_step         one iteration f_out = epilogue(S f_in): a CSR gather with the lanes along the classes, the additions of a row in
//                      segment order in double, then the clamp of the variant; the blocks' shares of sum / max |f_out - f_in| and a
//                      one-block merge
//   sv_lp_finish       the rows normalised to distributions, the first maximum, its probability and the counts of decided / unreached rows
// Plain HIP C++; each takes a stream and allocates nothing: capturable.  Every floating-point sum is taken in a fixed order that depends
// only on the call's arguments and there is no atomic of any kind: a repeated call sequence gives the same bits.  A segment is clamped to
// [0, nnz] and a column outside the matrix is skipped: nothing is read outside the arrays whatever rowptr and col hold.
#include "common.h"
#include <math.h>

constexpr int LP_LANES = 8;           // sv_lp_normalize: lanes per row
constexpr int LP_KMAX = 1024;
constexpr int LP_AHEAD = 8;           // sv_lp_step: gathers in flight per lane

__device__ __forceinline__ int64_t lp_clamp(int64_t q, int64_t nnz) { return q < 0 ? 0 : q > nnz ? nnz : q; }

// NaN-keeping maximum of two non-negative values
__device__ __forceinline__ double lp_max(double a, double b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }

// ------------------------------------------------------------------------------------------ sv_lp_normalize
// lane s of a row adds the valid entries s, s + 8, .. of its segment in order; the eight lane sums meet in a butterfly (xor 4, 2, 1)
__global__ __launch_bounds__(256) void lp_degree_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                        const float* __restrict__ val, int N, int64_t nnz, double* __restrict__ deg) {
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LP_LANES;
    const int s = threadIdx.x & (LP_LANES - 1);
    const bool live = row < N;
    double d = 0.0;
    if (live) {
        const int64_t end = lp_clamp(rowptr[row + 1], nnz);
        for (int64_t q = lp_clamp(rowptr[row], nnz) + s; q < end; q += LP_LANES) {
            const int64_t j = col[q];
            if (j < 0 || j >= N) continue;
            d += (double)val[q];
        }
    }
#pragma unroll
    for (int off = LP_LANES / 2; off > 0; off >>= 1) d += __shfl_xor(d, off);
    if (live && s == 0) deg[row] = d;
}

__global__ __launch_bounds__(256) void lp_scale_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ col,
                                                       const float* __restrict__ val, int N, int64_t nnz, int mode,
                                                       const double* __restrict__ deg, float* __restrict__ sval) {
#pragma clang fp contract(off)                         // the header's operations, one rounding each
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LP_LANES;
    const int s = threadIdx.x & (LP_LANES - 1);
    if (row >= N) return;
    const double di = deg[row];
    const int64_t end = lp_clamp(rowptr[row + 1], nnz);
    for (int64_t q = lp_clamp(rowptr[row], nnz) + s; q < end; q += LP_LANES) {
        const int64_t j = col[q];
        float out = 0.f;
        if (j >= 0 && j < N) {
            const double w = (double)val[q];
            if (mode == SV_LP_SYM) {
                const double dd = di * deg[j];
                const double root = sqrt(dd);
                out = dd == 0.0 ? 0.f : (float)(w / root);
            } else {
                out = di == 0.0 ? 0.f : (float)(w / di);
            }
        }
        sval[q] = out;
    }
}

int sv_lp_normalize(const int64_t* rowptr, const int64_t* col, const float* val, int N, int64_t nnz, int mode, double* deg, float* sval,
                    void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(rowptr, SV_E_ARG, "sv_lp_normalize: rowptr is NULL");
    SV_REQUIRE(N > 0 && nnz >= 0, SV_E_ARG, "sv_lp_normalize: bad size (N=%d, nnz=%lld)", N, (long long)nnz);
    SV_REQUIRE(nnz == 0 || (col && val && sval), SV_E_ARG, "sv_lp_normalize: col, val or sval is NULL with nnz=%lld", (long long)nnz);
    SV_REQUIRE(deg, SV_E_ARG, "sv_lp_normalize: deg is NULL");
    SV_REQUIRE(mode == SV_LP_SYM || mode == SV_LP_ROW, SV_E_ARG, "sv_lp_normalize: unknown mode %d", mode);
    const dim3 grid((unsigned)(((int64_t)N * LP_LANES - 1) / 256 + 1));
    hipLaunchKernelGGL(lp_degree_kernel, grid, dim3(256), 0, (hipStream_t)stream, rowptr, col, val, N, nnz, deg);
    if (nnz > 0) hipLaunchKernelGGL(lp_scale_kernel, grid, dim3(256), 0, (hipStream_t)stream, rowptr, col, val, N, nnz, mode, deg, sval);
    return sv_check_launch("sv_lp_normalize");
}

// ------------------------------------------------------------------------------------------ sv_lp_step
// LPR lanes per row (16 for K <= 16, else 64), 256 / LPR rows per block; lane l owns the classes l, l + LPR, ..  The lanes of a row
// read the same (col, sval) entry -- one broadcast load -- and gather LPR consecutive floats of the row it names; LP_AHEAD entries are
// loaded before the first is added, and they are added in segment order.  The propagation variant keeps the row's accumulators in LDS
// (double [rows][K], dynamic) so that every lane can add them in class order; the block's shares of the statistics meet in a binary
// tree in LDS, the same pairs whatever the values.
template <int LPR>
__global__ __launch_bounds__(256) void lp_step_kernel(const float* __restrict__ f_in, int M, const int64_t* __restrict__ rowptr,
                                                      const int64_t* __restrict__ col, const float* __restrict__ sval, int64_t nnz, int N,
                                                      int K, const int64_t* __restrict__ label, int variant, double alpha,
                                                      double one_minus_alpha, float* __restrict__ f_out, double* __restrict__ scratch) {
#pragma clang fp contract(off)                         // the header's operations, one rounding each
    extern __shared__ double lp_lds[];                 // [rows][K] under propagation, then [2][256] with statistics
    constexpr int ROWS = 256 / LPR;
    const int tid = threadIdx.x, r = tid / LPR, lane = tid % LPR;
    const int64_t row = (int64_t)blockIdx.x * ROWS + r;
    const bool live = row < N;
    const bool prop = variant == SV_LP_PROPAGATION;
    double* mine = lp_lds + (int64_t)r * K;
    int64_t beg = 0, end = 0, lab = -1;
    if (live) {
        beg = lp_clamp(rowptr[row], nnz);
        end = lp_clamp(rowptr[row + 1], nnz);
        if (label) lab = label[row];
    }
    const bool labelled = lab >= 0 && lab < K;
    double dsum = 0.0, dmax = 0.0;

    for (int c0 = 0; c0 < K; c0 += LPR) {
        const int c = c0 + lane;
        const bool has = live && c < K;
        double acc = 0.0;
        if (has && !(prop && labelled)) {
            for (int64_t q = beg; q < end; q += LP_AHEAD) {
                int64_t j[LP_AHEAD];
                float w[LP_AHEAD], v[LP_AHEAD];
#pragma unroll
                for (int u = 0; u < LP_AHEAD; ++u) {
                    const bool in = q + u < end;
                    j[u] = in ? col[q + u] : -1;
                    w[u] = in ? sval[q + u] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < LP_AHEAD; ++u) {
                    const bool ok = j[u] >= 0 && j[u] < M;                 // (never read outside f_in)
                    v[u] = ok ? f_in[j[u] * K + c] : 0.f;
                    if (!ok) w[u] = 0.f;                                   // no edge: + 0.0, which changes no bit of acc
                }
#pragma unroll
                for (int u = 0; u < LP_AHEAD; ++u) {
                    const double prod = (double)w[u] * (double)v[u];       // exact
                    acc = acc + prod;
                }
            }
        }
        if (prop) {
            if (has) mine[c] = acc;
        } else if (has) {
            float out;
            if (variant == SV_LP_SPREADING) {
                const double t = alpha * acc;
                out = (float)(t + (c == lab ? one_minus_alpha : 0.0));
            } else {
                out = (float)acc;
            }
            f_out[row * K + c] = out;
            if (scratch) {
                const double d = fabs((double)out - (double)f_in[row * K + c]);
                dsum = dsum + d;
                dmax = lp_max(dmax, d);
            }
        }
    }
    if (prop) {
        __syncthreads();
        double s = 0.0;
        if (live && !labelled)
            for (int c = 0; c < K; ++c) s = s + mine[c];                   // class order; every lane of the row forms the same bits
        if (s == 0.0) s = 1.0;
        if (live) {
            for (int c = lane; c < K; c += LPR) {
                const float out = labelled ? (c == lab ? 1.f : 0.f) : (float)(mine[c] / s);
                f_out[row * K + c] = out;
                if (scratch) {
                    const double d = fabs((double)out - (double)f_in[row * K + c]);
                    dsum = dsum + d;
                    dmax = lp_max(dmax, d);
                }
            }
        }
    }
    if (scratch) {
        double* sh_s = lp_lds + (prop ? (int64_t)ROWS * K : 0);
        double* sh_m = sh_s + 256;
        sh_s[tid] = dsum;
        sh_m[tid] = dmax;
        __syncthreads();
#pragma unroll
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) {
                sh_s[tid] = sh_s[tid] + sh_s[tid + h];
                sh_m[tid] = lp_max(sh_m[tid], sh_m[tid + h]);
            }
            __syncthreads();
        }
        if (tid == 0) {
            scratch[2 * (int64_t)blockIdx.x] = sh_s[0];
            scratch[2 * (int64_t)blockIdx.x + 1] = sh_m[0];
        }
    }
}

// one block: thread t merges the blocks t, t + 256, .. in block order, then the 256 shares meet in the same binary tree
__global__ __launch_bounds__(256) void lp_merge_kernel(const double* __restrict__ scratch, int64_t nblocks, double* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double sh_s[256];
    __shared__ double sh_m[256];
    const int tid = threadIdx.x;
    double dsum = 0.0, dmax = 0.0;
    for (int64_t b = tid; b < nblocks; b += 256) {
        dsum = dsum + scratch[2 * b];
        dmax = lp_max(dmax, scratch[2 * b + 1]);
    }
    sh_s[tid] = dsum;
    sh_m[tid] = dmax;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            sh_s[tid] = sh_s[tid] + sh_s[tid + h];
            sh_m[tid] = lp_max(sh_m[tid], sh_m[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[0] = sh_s[0];
        stats[1] = sh_m[0];
    }
}

int sv_lp_step(const float* f_in, int M, const int64_t* rowptr, const int64_t* col, const float* sval, int64_t nnz, int N, int K,
               const int64_t* label, int variant, double alpha, double one_minus_alpha, float* f_out, double* scratch, double* stats,
               void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(f_in && f_out && rowptr, SV_E_ARG, "sv_lp_step: f_in, f_out or rowptr is NULL");
    SV_REQUIRE(N > 0 && M > 0 && nnz >= 0, SV_E_ARG, "sv_lp_step: bad size (N=%d, M=%d, nnz=%lld)", N, M, (long long)nnz);
    SV_REQUIRE(K >= 1 && K <= LP_KMAX, SV_E_ARG, "sv_lp_step: K=%d outside [1, %d]", K, LP_KMAX);
    SV_REQUIRE(nnz == 0 || (col && sval), SV_E_ARG, "sv_lp_step: col or sval is NULL with nnz=%lld", (long long)nnz);
    SV_REQUIRE(variant == SV_LP_SPREADING || variant == SV_LP_PROPAGATION || variant == SV_LP_PRODUCT, SV_E_ARG,
               "sv_lp_step: unknown variant %d", variant);
    SV_REQUIRE(label || variant == SV_LP_PRODUCT, SV_E_ARG, "sv_lp_step: label is NULL (only the product variant runs without)");
    SV_REQUIRE(variant != SV_LP_SPREADING || (isfinite(alpha) && isfinite(one_minus_alpha)), SV_E_ARG,
               "sv_lp_step: alpha=%g or one_minus_alpha=%g is not finite", alpha, one_minus_alpha);
    {   // an output that overlaps the input would be read while it is written
        const uintptr_t in0 = (uintptr_t)f_in, in1 = in0 + (uintptr_t)M * K * sizeof(float);
        const uintptr_t out0 = (uintptr_t)f_out, out1 = out0 + (uintptr_t)N * K * sizeof(float);
        SV_REQUIRE(out1 <= in0 || in1 <= out0, SV_E_ARG, "sv_lp_step: f_out aliases f_in");
    }
    SV_REQUIRE(!stats || (scratch && M == N), SV_E_ARG, "sv_lp_step: stats needs scratch and M == N (M=%d, N=%d)", M, N);
    const int lpr = K <= 16 ? 16 : 64, rows = 256 / lpr;
    const int64_t nblocks = ((int64_t)N - 1) / rows + 1;
    double* sc = stats ? scratch : nullptr;
    const size_t lds = ((variant == SV_LP_PROPAGATION ? (size_t)rows * K : 0) + (sc ? 512 : 0)) * sizeof(double);
    if (lpr == 16)
        hipLaunchKernelGGL(lp_step_kernel<16>, dim3((unsigned)nblocks), dim3(256), lds, (hipStream_t)stream, f_in, M, rowptr, col, sval, nnz,
                           N, K, label, variant, alpha, one_minus_alpha, f_out, sc);
    else
        hipLaunchKernelGGL(lp_step_kernel<64>, dim3((unsigned)nblocks), dim3(256), lds, (hipStream_t)stream, f_in, M, rowptr, col, sval, nnz,
                           N, K, label, variant, alpha, one_minus_alpha, f_out, sc);
    if (stats) hipLaunchKernelGGL(lp_merge_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sc, nblocks, stats);
    return sv_check_launch("sv_lp_step");
}

// ------------------------------------------------------------------------------------------ sv_lp_finish
// One thread per row: the sum in class order in double, the first maximum, a NaN anywhere.  The counting launch (one block) scans the
// rows again with the same function, so that the counts do not depend on which outputs were asked for.
struct LpRow {
    double s;
    int best;
    bool nan;
};

__device__ __forceinline__ LpRow lp_row_scan(const float* __restrict__ frow, int K) {
    LpRow o;
    o.s = 0.0;
    o.best = 0;
    o.nan = false;
    float top = frow[0];
    for (int c = 0; c < K; ++c) {
        const float v = frow[c];
        o.s = o.s + (double)v;
        if (v != v) o.nan = true;
        if (v > top) { top = v; o.best = c; }
    }
    return o;
}

__global__ __launch_bounds__(256) void lp_finish_kernel(const float* __restrict__ f, int N, int K, float* __restrict__ proba,
                                                        int64_t* __restrict__ pred, float* __restrict__ conf) {
#pragma clang fp contract(off)
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    const float* frow = f + row * K;
    const LpRow o = lp_row_scan(frow, K);
    const double s = o.s == 0.0 ? 1.0 : o.s;
    if (proba)
        for (int c = 0; c < K; ++c) proba[row * K + c] = (float)((double)frow[c] / s);
    if (pred) pred[row] = (o.nan || o.s == 0.0) ? -1 : o.best;
    if (conf) conf[row] = (float)((double)frow[o.best] / s);
}

__global__ __launch_bounds__(1024) void lp_count_kernel(const float* __restrict__ f, int N, int K, int64_t* __restrict__ counts) {
    __shared__ int64_t sh_d[1024];
    __shared__ int64_t sh_u[1024];
    const int tid = threadIdx.x;
    int64_t decided = 0, unreached = 0;
    for (int64_t row = tid; row < N; row += 1024) {
        const LpRow o = lp_row_scan(f + row * K, K);
        if (!o.nan && o.s == 0.0) ++unreached;
        else if (!o.nan) ++decided;
    }
    sh_d[tid] = decided;
    sh_u[tid] = unreached;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if (tid < h) { sh_d[tid] += sh_d[tid + h]; sh_u[tid] += sh_u[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) { counts[0] = sh_d[0]; counts[1] = sh_u[0]; }
}

int sv_lp_finish(const float* f, int N, int K, float* proba, int64_t* pred, float* conf, int64_t* counts, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(f, SV_E_ARG, "sv_lp_finish: f is NULL");
    SV_REQUIRE(N > 0, SV_E_ARG, "sv_lp_finish: non-positive size (N=%d)", N);
    SV_REQUIRE(K >= 1 && K <= LP_KMAX, SV_E_ARG, "sv_lp_finish: K=%d outside [1, %d]", K, LP_KMAX);
    SV_REQUIRE(proba || pred || conf || counts, SV_E_ARG, "sv_lp_finish: every output (proba, pred, conf, counts) is NULL");
    SV_REQUIRE((const void*)proba != (const void*)f, SV_E_ARG, "sv_lp_finish: proba aliases f");
    if (proba || pred || conf)
        hipLaunchKernelGGL(lp_finish_kernel, dim3((unsigned)((N - 1) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, f, N, K, proba, pred, conf);
    if (counts) hipLaunchKernelGGL(lp_count_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, f, N, K, counts);
    return sv_check_launch("sv_lp_finish");
}
