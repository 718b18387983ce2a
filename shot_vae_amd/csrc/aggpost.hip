// The aggregate posterior q(z) = 1/N sum_j q(z | x_j) of a gallery of encoded images (declared, with the exact definitions, in
// include/shotvae_hip.h):
//   sv_aggpost_sample  z ~ q(z | x_i) from sv_latent_sweep's stream, with log q(z_i | x_i) and log p(z_i)
//   sv_aggpost_scan    the joint density: a streaming log-sum-exp over the gallery of log N(z_i; mu_j, sigma_j^2) -- knn.hip's tiles
//                      with an online (maximum, sum) state where the neighbour lists are; the [Q][N] matrix never leaves the chip
//   sv_aggpost_dims    the per-dimension marginals: one log-sum-exp per (query, dimension), no sum over the dimensions
//   sv_aggpost_finish  merges the P partial states of a row and subtracts log(count)
// Plain HIP C++; each takes a stream and allocates nothing: capturable.  A pair's value is ONE fixed sequence of operations (sv_pairdist's
// rule: 16 dimensions in fp32 with explicit fmaf, the 16-blocks in double); the terms enter a state in a fixed order that depends only
// on the call's arguments, the partial states meet in index order, and there is no atomic: a repeated call sequence gives the same bits.
#include "common.h"
#include <math.h>

constexpr double AP_HALF_LOG_2PI = 0.91893853320467274178;
constexpr int AP_PMAX = 64;

// state += exp(v): one exponential per term.  The rules of score_lse_merge: -inf has weight 0, +inf is absorbing, a NaN is kept.
__device__ __forceinline__ void ap_lse_add(ScoreLse& p, double v) {
    if (v != v || p.m != p.m) { p.m = NAN; p.a = 0.0; return; }
    if (v == -INFINITY || p.m == INFINITY) return;
    if (v == INFINITY) { p.m = INFINITY; p.a = 1.0; return; }
    if (v <= p.m) {
        p.a += exp(v - p.m);
    } else {
        p.a = p.a * exp(p.m - v) + 1.0;                // (the empty state: 0 * exp(-inf) + 1)
        p.m = v;
    }
}

// ------------------------------------------------------------------------------------------ sv_aggpost_sample
constexpr int AS_THREADS = 64, AS_CHUNK = 4 * AS_THREADS;

// one wave per row; 256 dimensions at a time: every thread writes the terms of its four columns to LDS, thread 0 adds them in index
// order in double
__global__ __launch_bounds__(AS_THREADS) void aggpost_sample_kernel(const float* mu, const float* ls, const int64_t* key, int64_t row0,
                                                                    int s, int D, float* z, float* lqx, float* lpz) {
    __shared__ float tq[AS_CHUNK], tp[AS_CHUNK];
    const int tid = threadIdx.x;
    const int64_t i = blockIdx.x;
    const uint64_t kv = key ? (uint64_t)key[0] : 0u;
    const uint64_t row = (uint64_t)(row0 + i);
    double aq = 0.0, ap = 0.0;
    for (int c0 = 0; c0 < D; c0 += AS_CHUNK) {
        const int j = (c0 >> 2) + tid;                 // the generator call of columns 4 j .. 4 j + 3
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (key && 4 * j < D) sv_normals4(kv, row, ((uint32_t)s << 16) | (uint32_t)j, SV_SCORE_PHILOX_TAG, n);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * j + q;
            if (d < D) {
                const float m = mu[i * D + d], l = ls[i * D + d];
                const float v = key ? m + expf(l) * n[q] : m;
                z[i * D + d] = v;
                tq[4 * tid + q] = -0.5f * n[q] * n[q] - l;
                tp[4 * tid + q] = -0.5f * v * v;
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int nd = D - c0 < AS_CHUNK ? D - c0 : AS_CHUNK;
            for (int d = 0; d < nd; ++d) {
                aq += (double)tq[d];
                ap += (double)tp[d];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        lqx[i] = (float)(aq - (double)D * AP_HALF_LOG_2PI);
        lpz[i] = (float)(ap - (double)D * AP_HALF_LOG_2PI);
    }
}

int sv_aggpost_sample(const float* mu, const float* ls, const int64_t* key, int64_t row0, int s, int Q, int D, float* z, float* lqx,
                      float* lpz, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(mu && ls, SV_E_ARG, "sv_aggpost_sample: mu or ls is NULL");
    SV_REQUIRE(z && lqx && lpz, SV_E_ARG, "sv_aggpost_sample: an output (z, lqx, lpz) is NULL");
    SV_REQUIRE(Q > 0 && D > 0, SV_E_ARG, "sv_aggpost_sample: non-positive size (Q=%d D=%d)", Q, D);
    SV_REQUIRE(row0 >= 0, SV_E_ARG, "sv_aggpost_sample: row0=%lld must be >= 0", (long long)row0);
    SV_REQUIRE(s >= 0, SV_E_ARG, "sv_aggpost_sample: s=%d must be >= 0", s);
    SV_REQUIRE(s < 65536 && D <= (1 << 18), SV_E_SHAPE, "sv_aggpost_sample: s=%d >= 65536 or D=%d > 2^18 (the counter's fields)", s, D);
    hipLaunchKernelGGL(aggpost_sample_kernel, dim3(Q), dim3(AS_THREADS), 0, (hipStream_t)stream, mu, ls, key, row0, s, D, z, lqx, lpz);
    return sv_check_launch("sv_aggpost_sample");
}

// ------------------------------------------------------------------------------------------ sv_aggpost_scan
// knn_kernel's tile: 64 queries x 64 gallery rows, 16 dimensions per staged chunk, the next chunk's global loads in flight while this
// one is multiplied.  Block (x, p) takes the gallery tiles p, p + P, ... of the call; thread (ty, tx) keeps one state per row of its
// own (rows 4 ty .., the columns 4 tx .. of every tile, in tile and column order); the 16 states of a row meet in a butterfly at the
// end and are merged into (or, with init, replace) partial state p.
__global__ __launch_bounds__(KN_THREADS, 2) void aggpost_scan_kernel(const float* __restrict__ z, int Q, const float* __restrict__ g_mu,
                                                                     const float* __restrict__ g_ls, int N, int D, int64_t col0,
                                                                     int64_t self0, double* sm_, double* ss_, int P, int init) {
    constexpr int MQ = 4, TQ = 16 * MQ, LDQ = TQ + 4, LDG = KN_TG + 4;
    __shared__ __attribute__((aligned(16))) float sm[KN_DC * (LDQ + 2 * LDG)];
    __shared__ double auxg[KN_TG];
    float* Aq = sm;
    float* Ag = Aq + KN_DC * LDQ;
    float* Bg = Ag + KN_DC * LDG;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, p = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int64_t step = (int64_t)P * KN_TG;
    const double cst = (double)D * AP_HALF_LOG_2PI;

    ScoreLse st[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) st[m] = ScoreLse{-INFINITY, 0.0};

    float pqm[MQ], pql[MQ], pgm[4], pgl[4];
    kn_load<SV_DIST_EUCLID, TQ>(z, nullptr, q0, Q, 0, D, pqm, pql);
    kn_load<SV_DIST_KL, KN_TG>(g_mu, g_ls, (int64_t)p * KN_TG, N, 0, D, pgm, pgl);
    for (int64_t g0 = (int64_t)p * KN_TG; g0 < N; g0 += step) {
        double acc[MQ][4], ag[4];
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;
#pragma unroll
        for (int n = 0; n < 4; ++n) ag[n] = 0.0;

        for (int d0 = 0; d0 < D; d0 += KN_DC) {
            __syncthreads();                           // the previous chunk's products are read
            kn_store<SV_DIST_EUCLID, TQ, false>(pqm, pql, q0, Q, d0, D, Aq, nullptr, nullptr);
            kn_store<SV_DIST_KL, KN_TG, true>(pgm, pgl, g0, N, d0, D, Ag, Bg, ag);          // Bg = 1 / sigma^2, ag += ls
            __syncthreads();
            {
                const bool last = d0 + KN_DC >= D;
                const int nd0 = last ? 0 : d0 + KN_DC;
                kn_load<SV_DIST_EUCLID, TQ>(z, nullptr, q0, Q, nd0, D, pqm, pql);
                kn_load<SV_DIST_KL, KN_TG>(g_mu, g_ls, last ? g0 + step : g0, N, nd0, D, pgm, pgl);
            }
            float part[MQ][4];
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) part[m][n] = 0.f;
#pragma unroll 4
            for (int dd = 0; dd < KN_DC; ++dd) {
                const f32x4 ga = *reinterpret_cast<const f32x4*>(&Ag[dd * LDG + 4 * tx]);
                const f32x4 gb = *reinterpret_cast<const f32x4*>(&Bg[dd * LDG + 4 * tx]);
                float qa[MQ];
#pragma unroll
                for (int m = 0; m < MQ; ++m) qa[m] = Aq[dd * LDQ + MQ * ty + m];
#pragma unroll
                for (int m = 0; m < MQ; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const float dm = qa[m] - ga[n];
                        part[m][n] = fmaf(dm * dm, gb[n], part[m][n]);         // (z - mu)^2 / sigma^2
                    }
            }
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += (double)part[m][n];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {                  // (tx, ty = the dimension and row index of the staging role)
            const double t = kn_aux_reduce(ag[i]);
            if (tx == 0) auxg[ty + 16 * i] = t;
        }
        __syncthreads();                               // the row scalars are visible

#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int row = MQ * ty + m, col = 4 * tx + n;
                const int64_t gi = col0 + g0 + col;
                if (g0 + col >= N || (self0 >= 0 && gi == self0 + q0 + row)) continue;
                ap_lse_add(st[m], fma(-0.5, acc[m][n], -auxg[col]) - cst);
            }
    }

#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        ScoreLse t = st[m];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const ScoreLse o{__shfl_xor(t.m, off), __shfl_xor(t.a, off)};
            t = score_lse_merge(t, o);
        }
        const int64_t row = q0 + MQ * ty + m;
        if (tx == 0 && row < Q) {
            const int64_t at = (int64_t)p * Q + row;
            if (!init) t = score_lse_merge(ScoreLse{sm_[at], ss_[at]}, t);
            sm_[at] = t.m;
            ss_[at] = t.a;
        }
    }
}

#define AP_REQUIRE_COMMON(who)                                                                                                         \
    SV_REQUIRE(z && g_mu && g_ls, SV_E_ARG, who ": a pointer (z, g_mu, g_ls) is NULL");                                                \
    SV_REQUIRE(m && s, SV_E_ARG, who ": a state (m, s) is NULL");                                                                      \
    SV_REQUIRE(Q > 0 && N > 0 && D > 0, SV_E_ARG, who ": non-positive size (Q=%d N=%d D=%d)", Q, N, D);                                 \
    SV_REQUIRE(P >= 1 && P <= AP_PMAX, SV_E_ARG, who ": P=%d outside [1, %d]", P, AP_PMAX);                                             \
    SV_REQUIRE(col0 >= 0 && self0 >= -1, SV_E_ARG, who ": col0=%lld must be >= 0 and self0=%lld >= -1", (long long)col0,               \
               (long long)self0);                                                                                                      \
    SV_REQUIRE(col0 <= INT64_MAX - N - 64, SV_E_SHAPE, who ": col0=%lld + N overflows the index", (long long)col0)

int sv_aggpost_scan(const float* z, int Q, const float* g_mu, const float* g_ls, int N, int D, int64_t col0, int64_t self0, double* m,
                    double* s, int P, int init, void* stream) {
    SvProfScope prof_scope(stream);
    AP_REQUIRE_COMMON("sv_aggpost_scan");
    hipLaunchKernelGGL(aggpost_scan_kernel, dim3((Q + 63) / 64, P), dim3(KN_THREADS), 0, (hipStream_t)stream, z, Q, g_mu, g_ls, N, D, col0,
                       self0, m, s, P, init);
    return sv_check_launch("sv_aggpost_scan");
}

// ------------------------------------------------------------------------------------------ sv_aggpost_dims
// Q N D exponentials and nothing to sum over d: VALU and transcendental work.  Lane = dimension, wave w of the block = query rows
// 8 w .. 8 w + 7 of its 32, all held in registers: a gallery element (mu, ls) is loaded once per wave -- 64 consecutive floats --,
// turned into (-1 / (2 sigma^2), -ls - log(2 pi) / 2) once and serves the 8 rows.  No LDS, no barrier.  The state of a (row, dimension)
// is (m fp32 -- the terms are fp32 values, their maximum is exact --, s double); a term costs ONE exponential, exp(-|v - m|): it is
// the new term's weight when v <= m and the old sum's scale when v > m.  Block (x, y, p): 32 rows, 64 dimensions, gallery tiles of 64
// rows p, p + P, ..., rows in index order.
constexpr int AD_RQ = 8, AD_THREADS = 256, AD_ROWS = AD_RQ * (AD_THREADS / 64);

template <bool LOO>
__global__ __launch_bounds__(AD_THREADS) void aggpost_dims_kernel(const float* __restrict__ z, int Q, const float* __restrict__ g_mu,
                                                                  const float* __restrict__ g_ls, int N, int D, int64_t col0,
                                                                  int64_t self0, double* sm_, double* ss_, int P, int init) {
    const int d = blockIdx.y * 64 + (threadIdx.x & 63), p = blockIdx.z;
    const int64_t q0 = (int64_t)blockIdx.x * AD_ROWS + (threadIdx.x >> 6) * AD_RQ;
    if (d >= D) return;                                // (no barrier below)
    float zr[AD_RQ], m[AD_RQ];
    double s[AD_RQ];
    int64_t skip[AD_RQ];
#pragma unroll
    for (int r = 0; r < AD_RQ; ++r) {
        zr[r] = q0 + r < Q ? z[(q0 + r) * D + d] : 0.f;
        m[r] = -INFINITY;
        s[r] = 0.0;
        skip[r] = LOO ? self0 + q0 + r - col0 : -1;    // the gallery row of this call that is query row r itself
    }
    const int64_t step = (int64_t)P * KN_TG;
    for (int64_t j0 = (int64_t)p * KN_TG; j0 < N; j0 += step) {
        const int64_t j1 = j0 + KN_TG < N ? j0 + KN_TG : N;
#pragma unroll 2
        for (int64_t j = j0; j < j1; ++j) {
            const float gm = g_mu[j * D + d], gl = g_ls[j * D + d];
            const float nhb = -0.5f * expf(-2.f * gl), c = -gl - (float)AP_HALF_LOG_2PI;
#pragma unroll
            for (int r = 0; r < AD_RQ; ++r) {
                const float dm = zr[r] - gm;
                float v = fmaf(dm * dm, nhb, c);
                if (LOO && j == skip[r]) v = -INFINITY;
                const float dl = v == m[r] ? 0.f : v - m[r];           // (-inf - -inf and inf - inf: equal, not NaN)
                const float e = __expf(-fabsf(dl));                    // NaN for a NaN term: s becomes, and stays, NaN
                if (v > m[r]) {
                    s[r] = fma(s[r], (double)e, 1.0);
                    m[r] = v;
                } else {
                    s[r] += (double)e;                                 // (while m = -inf this counts -inf terms: the sum is rescaled
                }                                                      //  by exp(-inf) = 0 at the first finite term, or never read)
            }
        }
    }
#pragma unroll
    for (int r = 0; r < AD_RQ; ++r) {
        if (q0 + r >= Q) continue;
        ScoreLse t{(double)m[r], s[r]};
        if (s[r] != s[r]) t = ScoreLse{NAN, 0.0};
        else if (m[r] == -INFINITY) t.a = 0.0;
        else if (m[r] == INFINITY) t.a = 1.0;
        const int64_t at = ((int64_t)p * Q + q0 + r) * D + d;
        if (!init) t = score_lse_merge(ScoreLse{sm_[at], ss_[at]}, t);
        sm_[at] = t.m;
        ss_[at] = t.a;
    }
}

int sv_aggpost_dims(const float* z, int Q, const float* g_mu, const float* g_ls, int N, int D, int64_t col0, int64_t self0, double* m,
                    double* s, int P, int init, void* stream) {
    SvProfScope prof_scope(stream);
    AP_REQUIRE_COMMON("sv_aggpost_dims");
    SV_REQUIRE(D <= (1 << 22), SV_E_SHAPE, "sv_aggpost_dims: D=%d > 2^22 (the grid's second dimension)", D);
    const dim3 grid((Q + AD_ROWS - 1) / AD_ROWS, (D + 63) / 64, P);
    if (self0 >= 0)
        hipLaunchKernelGGL((aggpost_dims_kernel<true>), grid, dim3(AD_THREADS), 0, (hipStream_t)stream, z, Q, g_mu, g_ls, N, D, col0, self0,
                           m, s, P, init);
    else
        hipLaunchKernelGGL((aggpost_dims_kernel<false>), grid, dim3(AD_THREADS), 0, (hipStream_t)stream, z, Q, g_mu, g_ls, N, D, col0, self0,
                           m, s, P, init);
    return sv_check_launch("sv_aggpost_dims");
}

// ------------------------------------------------------------------------------------------ sv_aggpost_finish
__global__ __launch_bounds__(256) void aggpost_finish_kernel(const double* sm_, const double* ss_, int P, int64_t R, double log_count,
                                                             float* out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    double M = -INFINITY, sum = 0.0;
    bool nan = false;
    for (int p = 0; p < P; ++p) {
        const double mp = sm_[(int64_t)p * R + r], sp = ss_[(int64_t)p * R + r];
        nan = nan || mp != mp || sp != sp;
        M = fmax(M, mp);
    }
    if (nan) { out[r] = NAN; return; }
    if (!(M > -INFINITY) || M == INFINITY) { out[r] = (float)M; return; }       // every partial is empty, or a term was +inf
    for (int p = 0; p < P; ++p) {
        const double mp = sm_[(int64_t)p * R + r];
        if (mp > -INFINITY) sum += ss_[(int64_t)p * R + r] * exp(mp - M);
    }
    out[r] = (float)(M + log(sum) - log_count);
}

int sv_aggpost_finish(const double* m, const double* s, int P, int64_t R, int64_t count, float* out, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(m && s && out, SV_E_ARG, "sv_aggpost_finish: a pointer (m, s, out) is NULL");
    SV_REQUIRE(P >= 1 && P <= AP_PMAX, SV_E_ARG, "sv_aggpost_finish: P=%d outside [1, %d]", P, AP_PMAX);
    SV_REQUIRE(R > 0, SV_E_ARG, "sv_aggpost_finish: non-positive size (R=%lld)", (long long)R);
    SV_REQUIRE(count >= 1, SV_E_ARG, "sv_aggpost_finish: count=%lld must be >= 1", (long long)count);
    SV_REQUIRE(R <= (int64_t)INT32_MAX * 256, SV_E_SHAPE, "sv_aggpost_finish: R=%lld exceeds the grid", (long long)R);
    hipLaunchKernelGGL(aggpost_finish_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, s, P, R,
                       log((double)count), out);
    return sv_check_launch("sv_aggpost_finish");
}
