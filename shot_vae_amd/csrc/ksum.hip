// Kernel two-sample statistics in latent space: weighted row sums of a positive-definite kernel over all pairs of two row sets -- the
// quantity behind the MMD, the KID, the witness function and the permutation test (declared, with the exact definitions, in
// include/shotvae_hip.h):
//   sv_ksum_scan     part[s][p][i] = sum_j w_j k(q_i, g_j) over the gallery tiles p, p + P, .. of the call, in double, for S problems
//   sv_ksum_finish   row_sum[s][i] (=, +=) sum_p part[s][p][i];  total[s] = sum_i q_w[i] row_sum[s][i]
// knn_kernel's tile (64 queries x 64 gallery rows, 16 dimensions per staged chunk, the next chunk's global loads in flight while this
// one is multiplied) with a kernel function where the merge is: no key tile, no list, two barriers per chunk and none per tile.  The
// pair value is sv_pairdist's SV_DIST_EUCLID value bit for bit (ball_scan_kernel's operations, one for one); the polynomial kernel takes
// the dot product by the same 16-block rule.  The state is a double sum per query row: it lives in registers over all tiles of a block,
// the 16 shares of a row meet in kn_aux_reduce's butterfly, and a block WRITES its slot of `part` -- no atomic of any kind, no workspace
// of its own, and which pairs meet in which order is a function of the arguments alone.  Plain HIP C++; both take a stream and
// allocate nothing: capturable.
#include "common.h"
#include <math.h>

constexpr int KS_PMAX = 64;           // partial states
constexpr int KS_SCALES = 8;          // scales of an RBF / IMQ mixture
constexpr int KS_DEGREE = 8;          // degree of the polynomial kernel
constexpr int KS_SMAX = 65535;        // problems of a launch (blockIdx.z)

// Block (x, p, s): query tile x of problem s, the gallery tiles p, p + P, ... of the call.  Thread (ty, tx) owns rows 4 ty .., columns
// 4 tx .. of every tile; the four weights of its columns are staged once per tile (prefetched with the tile's first chunk), as
// ball_scan_kernel stages its radii.  A row beyond Q, a column beyond N and the self pair are left out by predicate.
template <int KIND>
__global__ __launch_bounds__(KN_THREADS, 2) void ksum_scan_kernel(const double* __restrict__ kparam, int n_scale, int degree,
                                                                  const float* __restrict__ q, int Q, int64_t q_stride,
                                                                  const float* __restrict__ g, const float* __restrict__ g_w, int N,
                                                                  int64_t g_stride, int64_t w_stride, int D, int64_t col0, int64_t self0,
                                                                  int P, double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int MQ = 4, TQ = 16 * MQ, LDQ = TQ + 4, LDG = KN_TG + 4;
    constexpr int ST = SV_DIST_EUCLID;                 // the staging role: one operand array, zeros beyond the end
    constexpr bool POLY = KIND == SV_KSUM_POLY;
    __shared__ __attribute__((aligned(16))) float sm[KN_DC * (LDQ + LDG)];
    __shared__ __attribute__((aligned(16))) float sw[KN_TG];
    __shared__ double kp[2 * KS_SCALES];               // the kernel's parameters (a_s, b_s): one broadcast read per use
    float* Aq = sm;
    float* Ag = Aq + KN_DC * LDQ;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, p = blockIdx.y;
    const int64_t prob = blockIdx.z;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int64_t step = (int64_t)P * KN_TG;
    q += prob * q_stride;
    g += prob * g_stride;
    if (g_w) g_w += prob * w_stride;

    if (tid < 2 * n_scale) kp[tid] = kparam[tid];     // (read behind the first tile's barriers)

    double sum[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) sum[m] = 0.0;

    float pq[MQ], pg[4], unused[4], pw = 0.f;
    kn_load<ST, TQ>(q, nullptr, q0, Q, 0, D, pq, unused);
    kn_load<ST, KN_TG>(g, nullptr, (int64_t)p * KN_TG, N, 0, D, pg, unused);
    if (tid < KN_TG && (int64_t)p * KN_TG + tid < N) pw = g_w ? g_w[(int64_t)p * KN_TG + tid] : 1.f;
    for (int64_t g0 = (int64_t)p * KN_TG; g0 < N; g0 += step) {
        double acc[MQ][4];
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;

        for (int d0 = 0; d0 < D; d0 += KN_DC) {
            __syncthreads();                           // the previous chunk's products and the previous tile's weights are read
            kn_store<ST, TQ, false>(pq, unused, q0, Q, d0, D, Aq, nullptr, nullptr);
            kn_store<ST, KN_TG, true>(pg, unused, g0, N, d0, D, Ag, nullptr, nullptr);
            if (d0 == 0 && tid < KN_TG) sw[tid] = pw;  // (a column beyond the end: 0, and never read into a sum)
            __syncthreads();
            {
                const bool last = d0 + KN_DC >= D;
                const int nd0 = last ? 0 : d0 + KN_DC;
                kn_load<ST, TQ>(q, nullptr, q0, Q, nd0, D, pq, unused);
                kn_load<ST, KN_TG>(g, nullptr, last ? g0 + step : g0, N, nd0, D, pg, unused);
                if (last && tid < KN_TG) pw = g0 + step + tid < N ? (g_w ? g_w[g0 + step + tid] : 1.f) : 0.f;
            }
            float part4[MQ][4];
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) part4[m][n] = 0.f;
#pragma unroll 4
            for (int dd = 0; dd < KN_DC; ++dd) {
                float qa[MQ];
                const f32x4 ga = *reinterpret_cast<const f32x4*>(&Ag[dd * LDG + 4 * tx]);
#pragma unroll
                for (int m = 0; m < MQ; ++m) qa[m] = Aq[dd * LDQ + MQ * ty + m];
#pragma unroll
                for (int m = 0; m < MQ; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        // knn_kernel's operations, one for one: the value of a pair is sv_pairdist's (POLY: the cosine's numerator)
                        if (POLY) {
                            part4[m][n] = fmaf(qa[m], ga[n], part4[m][n]);
                        } else {
                            const float dm = qa[m] - ga[n];
                            part4[m][n] = fmaf(dm, dm, part4[m][n]);
                        }
                    }
            }
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += (double)part4[m][n];
        }

        // (sw was written before this tile's last barrier; the next write is behind the next tile's first)
        const f32x4 w = *reinterpret_cast<const f32x4*>(&sw[4 * tx]);
        // k of the 16 pairs from their fp32 values (v for RBF / IMQ, u for POLY), in double, every operation rounded once; the scales
        // in order, each pair's k from 0.0.  (All 16, whatever the predicate below says: a value that does not count is not added.)
        double kv[MQ][4];
        if (POLY) {
            const double a = kp[0], c = kp[1];
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const double t = a * (double)(float)acc[m][n];
                    acc[m][n] = t + c;
                    kv[m][n] = acc[m][n];
                }
            for (int e = 1; e < degree; ++e) {
#pragma unroll
                for (int m = 0; m < MQ; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) kv[m][n] = kv[m][n] * acc[m][n];
            }
        } else {
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    acc[m][n] = (double)(float)acc[m][n];
                    kv[m][n] = 0.0;
                }
            for (int s = 0; s < n_scale; ++s) {
                const double a = kp[2 * s], b = kp[2 * s + 1];
#pragma unroll
                for (int m = 0; m < MQ; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const double t = a * acc[m][n];
                        double term;
                        if (KIND == SV_KSUM_RBF) {
                            term = b * exp(-t);
                        } else {
                            const double den = 1.0 + t;
                            term = b / den;
                        }
                        kv[m][n] = kv[m][n] + term;
                    }
            }
        }
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int row = MQ * ty + m, col = 4 * tx + n;
                const int64_t gi = col0 + g0 + col;
                const bool in = q0 + row < Q && g0 + col < N && !(self0 >= 0 && gi == self0 + q0 + row);
                const double term = (double)w[n] * kv[m][n];
                if (in) sum[m] = sum[m] + term;
            }
    }

#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        const double t = kn_aux_reduce(sum[m]);
        const int64_t row = q0 + MQ * ty + m;
        if (tx == 0 && row < Q) part[(prob * P + p) * (int64_t)Q + row] = t;
    }
}

int sv_ksum_scan(int kind, const double* kparam, int n_scale, int degree, const float* q, int Q, int64_t q_stride, const float* g,
                 const float* g_w, int N, int64_t g_stride, int64_t w_stride, int D, int S, int64_t col0, int64_t self0, int P,
                 double* part, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(kind >= SV_KSUM_RBF && kind <= SV_KSUM_POLY, SV_E_ARG, "sv_ksum_scan: bad kind %d", kind);
    SV_REQUIRE(n_scale >= 1 && n_scale <= (kind == SV_KSUM_POLY ? 1 : KS_SCALES), SV_E_ARG, "sv_ksum_scan: n_scale=%d outside [1, %d]",
               n_scale, kind == SV_KSUM_POLY ? 1 : KS_SCALES);
    SV_REQUIRE(kind != SV_KSUM_POLY || (degree >= 1 && degree <= KS_DEGREE), SV_E_ARG, "sv_ksum_scan: degree=%d outside [1, %d]", degree,
               KS_DEGREE);
    SV_REQUIRE(kparam && q && g && part, SV_E_ARG, "sv_ksum_scan: kparam, q, g or part is NULL");
    SV_REQUIRE(Q > 0 && N > 0 && D > 0, SV_E_ARG, "sv_ksum_scan: non-positive size (Q=%d N=%d D=%d)", Q, N, D);
    SV_REQUIRE(S >= 1 && S <= KS_SMAX, SV_E_ARG, "sv_ksum_scan: S=%d outside [1, %d]", S, KS_SMAX);
    SV_REQUIRE(P >= 1 && P <= KS_PMAX, SV_E_ARG, "sv_ksum_scan: P=%d outside [1, %d]", P, KS_PMAX);
    SV_REQUIRE(q_stride == 0 || q_stride >= (int64_t)Q * D, SV_E_SHAPE, "sv_ksum_scan: q_stride=%lld is neither 0 nor >= Q * D",
               (long long)q_stride);
    SV_REQUIRE(g_stride == 0 || g_stride >= (int64_t)N * D, SV_E_SHAPE, "sv_ksum_scan: g_stride=%lld is neither 0 nor >= N * D",
               (long long)g_stride);
    SV_REQUIRE(w_stride == 0 || w_stride >= N, SV_E_SHAPE, "sv_ksum_scan: w_stride=%lld is neither 0 nor >= N", (long long)w_stride);
    SV_REQUIRE(col0 >= 0 && self0 >= -1, SV_E_ARG, "sv_ksum_scan: col0=%lld must be >= 0 and self0=%lld >= -1", (long long)col0,
               (long long)self0);
    SV_REQUIRE(col0 <= INT64_MAX - N - 64 && self0 <= INT64_MAX - Q - 64, SV_E_SHAPE,
               "sv_ksum_scan: col0=%lld + N or self0=%lld + Q overflows the index", (long long)col0, (long long)self0);
    const int64_t lim = INT64_MAX / 8 / S;
    SV_REQUIRE(q_stride <= lim && g_stride <= lim && w_stride <= lim, SV_E_SHAPE, "sv_ksum_scan: S=%d strides overflow the index", S);
    const dim3 grid((Q + 63) / 64, P, S);
#define KS_GO(K)                                                                                                                \
    hipLaunchKernelGGL(ksum_scan_kernel<K>, grid, dim3(KN_THREADS), 0, (hipStream_t)stream, kparam, n_scale, degree, q, Q, q_stride, g, \
                       g_w, N, g_stride, w_stride, D, col0, self0, P, part)
    switch (kind) {
        case SV_KSUM_RBF: KS_GO(SV_KSUM_RBF); break;
        case SV_KSUM_IMQ: KS_GO(SV_KSUM_IMQ); break;
        default: KS_GO(SV_KSUM_POLY); break;
    }
#undef KS_GO
    return sv_check_launch("sv_ksum_scan");
}

// ------------------------------------------------------------------------------------------ sv_ksum_finish
// one thread per (problem, row): the partial states in the order of p
__global__ __launch_bounds__(256) void ksum_rows_kernel(const double* __restrict__ part, int64_t S, int P, int64_t Q, int accumulate,
                                                        double* __restrict__ row_sum) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= S * Q) return;
    const int64_t s = r / Q, i = r - s * Q;
    double t = part[s * P * Q + i];
    for (int p = 1; p < P; ++p) t = t + part[(s * P + p) * Q + i];
    row_sum[r] = accumulate ? row_sum[r] + t : t;
}

// one block per problem: sv_lp_step's merge order -- thread t takes the rows t, t + 256, .. in order, then the 256 shares meet in a
// binary tree, the same pairs whatever the values
__global__ __launch_bounds__(256) void ksum_total_kernel(const double* __restrict__ row_sum, int64_t Q, const float* __restrict__ q_w,
                                                         int64_t w_stride, double* __restrict__ total) {
#pragma clang fp contract(off)
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    double t = 0.0;
    for (int64_t i = tid; i < Q; i += 256) {
        const double v = row_sum[s * Q + i];
        const double term = q_w ? (double)q_w[s * w_stride + i] * v : v;
        t = t + term;
    }
    sh[tid] = t;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) sh[tid] = sh[tid] + sh[tid + h];
        __syncthreads();
    }
    if (tid == 0) total[s] = sh[0];
}

int sv_ksum_finish(const double* part, int S, int P, int Q, int accumulate, double* row_sum, const float* q_w, int64_t w_stride,
                   double* total, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(part && row_sum, SV_E_ARG, "sv_ksum_finish: part or row_sum is NULL");
    SV_REQUIRE(Q > 0, SV_E_ARG, "sv_ksum_finish: non-positive size (Q=%d)", Q);
    SV_REQUIRE(S >= 1 && S <= KS_SMAX, SV_E_ARG, "sv_ksum_finish: S=%d outside [1, %d]", S, KS_SMAX);
    SV_REQUIRE(P >= 1 && P <= KS_PMAX, SV_E_ARG, "sv_ksum_finish: P=%d outside [1, %d]", P, KS_PMAX);
    SV_REQUIRE(total || !q_w, SV_E_ARG, "sv_ksum_finish: q_w without total");
    SV_REQUIRE(w_stride == 0 || w_stride >= Q, SV_E_SHAPE, "sv_ksum_finish: w_stride=%lld is neither 0 nor >= Q", (long long)w_stride);
    SV_REQUIRE(w_stride <= INT64_MAX / 8 / S, SV_E_SHAPE, "sv_ksum_finish: S=%d strides overflow the index", S);
    const int64_t rows = (int64_t)S * Q;
    hipLaunchKernelGGL(ksum_rows_kernel, dim3((unsigned)((rows - 1) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, part, (int64_t)S, P,
                       (int64_t)Q, accumulate, row_sum);
    if (total)
        hipLaunchKernelGGL(ksum_total_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, row_sum, (int64_t)Q, q_w, w_stride, total);
    return sv_check_launch("sv_ksum_finish");
}
