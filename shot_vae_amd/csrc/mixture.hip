// Diagonal Gaussian mixtures on the latent space: one EM iteration in three entry points, the derived table and the sampler (declared,
// with the exact definitions, in include/shotvae_hip.h):
//   sv_gmm_prepare  (logw, mean, var) -> the table the scans read: ivar = 1 / var, cst, cdf
//   sv_gmm_estep    log sum_k exp v(i, k) per row -- knn.hip's tiles with an online (maximum fp32, sum double) state per row where the
//                   neighbour lists are --, the first maximum, and on request the responsibilities; the [N][K] matrix exists only then
//   sv_gmm_accum    r = expf(v - lse) recomputed per tile and added, with r x and r x^2, into P partial states (sv_kmeans_accum's rule:
//                   tile t of 64 rows to state t mod P), the accumulators in registers
//   sv_gmm_finish   scikit-learn's M-step for diagonal covariances in double over the merged states, then the table
//   sv_gmm_sample   z = mean_c + sqrt(var_c) n from sv_latent_draw's stream under SV_GMM_PHILOX_TAG, c from the table's cdf
// Plain HIP C++, fp32 / fp64 VALU; each takes a stream and allocates nothing: capturable.  v(i, k) is ONE sequence of operations
// (gm_tile, used by both scans); every floating-point sum is taken in a fixed order that depends only on the call's arguments; there is
// no atomic of any kind.  A repeated call sequence gives the same bits.
#include "common.h"
#include <float.h>
#include <math.h>

constexpr int GM_PMAX = 64;
constexpr int GM_SLICE = 32;                       // sv_gmm_accum: the dimensions a block owns
constexpr int GM_DMAX = 1 << 20;                   // ... its grid's second dimension: D / 32 <= 65535 blocks
constexpr int GM_LD = KN_TG + 4;
constexpr int GM_STAGE = 3 * KN_DC * GM_LD;        // floats of LDS gm_tile stages through: x, mean, ivar chunks
constexpr double GM_LOG_2PI = 1.83787706640934548356;

// ------------------------------------------------------------------------------------------ v(i, k)
// The values of rows q0 .. q0 + 63 against components g0 .. g0 + 16 NC - 1: thread (ty, tx) gets rows 4 ty + m, components g0 + NC tx + n
// (NC = 4: knn_kernel's 64 x 64 tile; NC = 1: 64 x 16, a quarter of the work, for K <= 16 -- a pair's operations are the same).
// sv_pairdist's summation rule on knn_kernel's tile: 16 dimensions per staged chunk in fp32 with explicit fmaf in index order, the chunks
// in double in index order; the next chunk's global loads are in flight while this one is multiplied.  Rows, components and dimensions
// beyond the end are staged as zeros (ivar = 0: no term).
//   v = NaN                                        the sum is NaN or infinite (a row with a NaN or infinite entry)
//     = -inf                                       cst_k = -inf (a component of weight 0), or a component beyond K
//     = (float) fma(-0.5, sum, (double) cst_k)     otherwise
// Starts with a barrier (the stage may still be read) and is called by every thread of the block.
template <int NC>
__device__ __forceinline__ void gm_tile(const float* __restrict__ x, int N, int64_t q0, const float* __restrict__ mean,
                                        const float* __restrict__ ivar, const float* __restrict__ cst, int K, int64_t g0, int D, float* sm,
                                        float v[4][NC]) {
    constexpr int TG = 16 * NC, LDG = TG + 4;
    float* Aq = sm;
    float* Ag = Aq + KN_DC * GM_LD;
    float* Bg = Ag + KN_DC * LDG;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][NC];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NC; ++n) acc[m][n] = 0.0;
    float pq[4], pm[NC], pi[NC], none[4];
    kn_load<SV_DIST_EUCLID, 64>(x, nullptr, q0, N, 0, D, pq, none);
    kn_load<SV_DIST_KL, TG>(mean, ivar, g0, K, 0, D, pm, pi);                // (the KL staging loads two arrays; nothing is transformed)
    for (int d0 = 0; d0 < D; d0 += KN_DC) {
        __syncthreads();                               // the previous chunk's products are read
        kn_store<SV_DIST_EUCLID, 64, false>(pq, none, q0, N, d0, D, Aq, nullptr, nullptr);
        kn_store<SV_DIST_EUCLID, TG, true>(pm, none, g0, K, d0, D, Ag, nullptr, nullptr);
        kn_store<SV_DIST_EUCLID, TG, true>(pi, none, g0, K, d0, D, Bg, nullptr, nullptr);
        __syncthreads();
        if (d0 + KN_DC < D) {
            kn_load<SV_DIST_EUCLID, 64>(x, nullptr, q0, N, d0 + KN_DC, D, pq, none);
            kn_load<SV_DIST_KL, TG>(mean, ivar, g0, K, d0 + KN_DC, D, pm, pi);
        }
        float part[4][NC];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) part[m][n] = 0.f;
#pragma unroll 4
        for (int dd = 0; dd < KN_DC; ++dd) {
            float ga[NC], gb[NC], qa[4];
            if constexpr (NC == 4) {
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(&Ag[dd * LDG + 4 * tx]);
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(&Bg[dd * LDG + 4 * tx]);
#pragma unroll
                for (int n = 0; n < 4; ++n) { ga[n] = a4[n]; gb[n] = b4[n]; }
            } else {
#pragma unroll
                for (int n = 0; n < NC; ++n) { ga[n] = Ag[dd * LDG + NC * tx + n]; gb[n] = Bg[dd * LDG + NC * tx + n]; }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) qa[m] = Aq[dd * GM_LD + 4 * ty + m];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < NC; ++n) {
                    const float dm = qa[m] - ga[n];
                    part[m][n] = fmaf(dm * dm, gb[n], part[m][n]);         // (x - mean)^2 / var
                }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) acc[m][n] += (double)part[m][n];
    }
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        const int64_t col = g0 + NC * tx + n;
        const float c = col < K ? cst[col] : -INFINITY;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const double a = acc[m][n];
            v[m][n] = col >= K ? -INFINITY : !(a < (double)INFINITY) ? NAN : c == -INFINITY ? -INFINITY : (float)fma(-0.5, a, (double)c);
        }
    }
}

// the online log-sum-exp state of a row: the maximum in fp32 (the terms are fp32 values: exact), the sum in double, expf on fp32
// differences.  Terms are finite or -inf (weight 0); the empty state is (-inf, 0).
struct GmLse { float m; double s; };
__device__ __forceinline__ void gm_lse_add(GmLse& p, float v) {
    if (v == -INFINITY) return;
    if (v <= p.m) {
        p.s += (double)expf(v - p.m);
    } else {
        p.s = p.s * (double)expf(p.m - v) + 1.0;       // (the empty state: 0 * expf(-inf) + 1)
        p.m = v;
    }
}
__device__ __forceinline__ GmLse gm_lse_merge(GmLse p, GmLse q) {
    if (q.m == -INFINITY) return p;
    if (p.m == -INFINITY) return q;
    const float m = fmaxf(p.m, q.m);
    return GmLse{m, p.s * (double)expf(p.m - m) + q.s * (double)expf(q.m - m)};
}

// ------------------------------------------------------------------------------------------ sv_gmm_estep
// One block per 64 rows; the component tiles in index order.  Thread (ty, tx) keeps one state, one (value, index) maximum and one NaN
// flag per row of its own over its columns 4 tx .. of every tile; the 16 of a row meet in a butterfly, and lane tx = 0's result is the
// row's.  With resp the tiles are computed a second time against the finished lse.  NC = 1 (tiles of 16 components) serves K <= 16.
template <int NC>
__global__ __launch_bounds__(KN_THREADS, 2) void gmm_estep_kernel(const float* __restrict__ x, int N, const float* __restrict__ ivar,
                                                                  const float* __restrict__ mean, const float* __restrict__ cst, int K, int D,
                                                                  float* lse, int64_t* assign, float* resp) {
    __shared__ __attribute__((aligned(16))) float sm[GM_STAGE];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * 64;
    GmLse st[4];
    float bv[4];
    int64_t bi[4];
    int bad[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) { st[m] = GmLse{-INFINITY, 0.0}; bv[m] = -INFINITY; bi[m] = INT64_MAX; bad[m] = 0; }
    float v[4][NC];
    for (int64_t g0 = 0; g0 < K; g0 += 16 * NC) {
        gm_tile<NC>(x, N, q0, mean, ivar, cst, K, g0, D, sm, v);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int64_t col = g0 + NC * tx + n;
                const float f = v[m][n];
                if (col >= K) continue;
                if (f != f) { bad[m] = 1; continue; }
                gm_lse_add(st[m], f);
                if (f > bv[m]) { bv[m] = f; bi[m] = col; }             // (columns ascend: the first maximum)
            }
    }
    float row_lse[4];
    int row_bad[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        GmLse t = st[m];
        float fv = bv[m];
        int64_t fi = bi[m];
        int b = bad[m];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const GmLse o{__shfl_xor(t.m, off), __shfl_xor(t.s, off)};
            const float ov = __shfl_xor(fv, off);
            const int64_t oi = __shfl_xor(fi, off);
            b |= __shfl_xor(b, off);
            t = (tx & off) ? gm_lse_merge(o, t) : gm_lse_merge(t, o);          // the lower lanes' state first, on both sides
            if (ov > fv || (ov == fv && oi < fi)) { fv = ov; fi = oi; }
        }
        // -inf when every component has weight 0
        float l = b ? NAN : t.m == -INFINITY ? -INFINITY : (float)((double)t.m + log(t.s));
        l = __shfl(l, (threadIdx.x & 63) & ~15);                               // lane tx = 0's bits for the whole row
        row_lse[m] = l;
        row_bad[m] = b;
        const int64_t row = q0 + 4 * ty + m;
        if (tx == 0 && row < N) {
            lse[row] = l;
            if (assign) assign[row] = (b || fi == INT64_MAX) ? -1 : fi;
        }
    }
    if (!resp) return;
    for (int64_t g0 = 0; g0 < K; g0 += 16 * NC) {
        gm_tile<NC>(x, N, q0, mean, ivar, cst, K, g0, D, sm, v);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int64_t col = g0 + NC * tx + n, row = q0 + 4 * ty + m;
                if (col < K && row < N) resp[row * K + col] = row_bad[m] ? NAN : expf(v[m][n] - row_lse[m]);
            }
    }
}

int sv_gmm_estep(const float* x, int N, const float* ivar, const float* mean, const float* cst, int K, int D, float* lse, int64_t* assign,
                 float* resp, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && ivar && mean && cst, SV_E_ARG, "sv_gmm_estep: a pointer (x, ivar, mean, cst) is NULL");
    SV_REQUIRE(lse, SV_E_ARG, "sv_gmm_estep: lse is NULL");
    SV_REQUIRE(N > 0 && K > 0 && D > 0, SV_E_ARG, "sv_gmm_estep: non-positive size (N=%d K=%d D=%d)", N, K, D);
    if (K <= 16)
        hipLaunchKernelGGL((gmm_estep_kernel<1>), dim3((N - 1) / 64 + 1), dim3(KN_THREADS), 0, (hipStream_t)stream, x, N, ivar, mean, cst, K, D,
                           lse, assign, resp);
    else
        hipLaunchKernelGGL((gmm_estep_kernel<4>), dim3((N - 1) / 64 + 1), dim3(KN_THREADS), 0, (hipStream_t)stream, x, N, ivar, mean, cst, K, D,
                           lse, assign, resp);
    return sv_check_launch("sv_gmm_estep");
}

// ------------------------------------------------------------------------------------------ sv_gmm_accum
// Block (kt, s, p): the KT components from kt KT, the S = 32 dimensions from S s, partial state p.  It walks the row tiles p, p + P, ... of
// the call: gm_tile gives the tile's v (over ALL dimensions: every slice recomputes it -- the trade of DESIGN.md 4k), r = expf(v - lse)
// goes to LDS once together with the tile's 64 x S slice of x, and then thread (component c = tid % KT, dimension group g = tid / KT)
// streams the 64 rows in index order through its 1 + 2 J accumulators IN REGISTERS: r, and r x, (r x) x of its J = S KT / 256
// dimensions -- a [KT x 64] . [64 x S] product in double with a fixed order and no dependent LDS chain.  A row that is skipped (lse not
// finite) or beyond the end enters as r = 0, x = 0: adding +0 changes no accumulator bit.  KT = 16 serves K <= 16 (a 64-wide tile
// would leave three quarters of the block idle), KT = 64 everything else.  Block (0, 0, p) also counts the rows and adds the lse's.
// S = 32 dimensions: every slice recomputes v, but S = 64 with half the blocks measured SLOWER (0.566 against 0.537 ms at 50 000 x 128,
// K = 100, P = 64: 256 blocks leave one block of four waves per compute unit, and the walk is bound by latency, not by the VALU).
template <int KT>
__global__ __launch_bounds__(KN_THREADS, 2) void gmm_accum_kernel(const float* __restrict__ x, const float* __restrict__ lse, int N,
                                                                  const float* __restrict__ ivar, const float* __restrict__ mean,
                                                                  const float* __restrict__ cst, int K, int D, double* sums, int64_t* counts,
                                                                  int P, int init) {
    constexpr int S = GM_SLICE, NC = KT / 16, G = KN_THREADS / KT, J = S / G, LDX = S + 1;
    __shared__ __attribute__((aligned(16))) float sm[GM_STAGE];
    __shared__ float R[64 * KT];
    __shared__ float X[64 * LDX];
    __shared__ float sl[64];
    __shared__ int ok[64];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c = tid % KT, g = tid / KT, p = blockIdx.z;
    const int64_t k0 = (int64_t)blockIdx.x * KT, k = k0 + c;
    const int d0 = blockIdx.y * S + g * J;
    const int64_t stride = (int64_t)K * (2 * D + 1) + 1;
    double* state = sums + (int64_t)p * stride;
    double* mine = state + k * (2 * D + 1);
    const bool tally = blockIdx.x == 0 && blockIdx.y == 0 && tid == 0;

    double a0 = 0.0, a1[J], a2[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { a1[j] = 0.0; a2[j] = 0.0; }
    int64_t nfin = 0, nskip = 0;
    double lsum = 0.0;
    if (!init) {
        if (k < K) {
            a0 = mine[0];
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (d0 + j < D) { a1[j] = mine[1 + d0 + j]; a2[j] = mine[1 + D + d0 + j]; }
        }
        if (tally) { nfin = counts[2 * p]; nskip = counts[2 * p + 1]; lsum = state[stride - 1]; }
    }

    const int64_t ntiles = ((int64_t)N + 63) / 64;
    float v[4][NC];
    for (int64_t t = p; t < ntiles; t += P) {
        const int64_t q0 = t * 64;
        gm_tile<NC>(x, N, q0, mean, ivar, cst, K, k0, D, sm, v);          // (its barriers: the previous tile's R, X, sl are read)
        if (tid < 64) {
            const float l = q0 + tid < N ? lse[q0 + tid] : NAN;
            sl[tid] = l;
            ok[tid] = l - l == 0.f;                                    // finite
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int row = 4 * ty + m, col = NC * tx + n;
                R[row * KT + col] = ok[row] ? expf(v[m][n] - sl[row]) : 0.f;
            }
        for (int i = tid; i < 64 * S; i += KN_THREADS) {
            const int row = i / S, dd = i % S, d = blockIdx.y * S + dd;
            X[row * LDX + dd] = (ok[row] && d < D) ? x[(q0 + row) * D + d] : 0.f;          // (ok: the row is inside the call)
        }
        __syncthreads();
        for (int i = 0; i < 64; ++i) {
#pragma clang fp contract(off)                         // the header's order: the product rounded, THEN added.  (The operators are spelt
                                                       // out: __dmul_rn / __dadd_rn are inline functions whose own operations may still fuse.)
            const double r = (double)R[i * KT + c];
            a0 = a0 + r;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double xd = (double)X[i * LDX + g * J + j];
                const double rx = r * xd;                              // exact: 24 x 24 bits
                const double rxx = rx * xd;                            // rounded
                a1[j] = a1[j] + rx;
                a2[j] = a2[j] + rxx;
            }
        }
        if (tally)
            for (int i = 0; i < 64 && q0 + i < N; ++i) {
                if (ok[i]) { ++nfin; lsum = __dadd_rn(lsum, (double)sl[i]); }
                else ++nskip;
            }
    }

    if (k < K) {
        if (blockIdx.y == 0 && g == 0) mine[0] = a0;
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (d0 + j < D) { mine[1 + d0 + j] = a1[j]; mine[1 + D + d0 + j] = a2[j]; }
    }
    if (tally) { counts[2 * p] = nfin; counts[2 * p + 1] = nskip; state[stride - 1] = lsum; }
}

int sv_gmm_accum(const float* x, const float* lse, int N, const float* ivar, const float* mean, const float* cst, int K, int D, double* sums,
                 int64_t* counts, int P, int init, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && lse, SV_E_ARG, "sv_gmm_accum: x or lse is NULL");
    SV_REQUIRE(ivar && mean && cst, SV_E_ARG, "sv_gmm_accum: a table pointer (ivar, mean, cst) is NULL");
    SV_REQUIRE(sums && counts, SV_E_ARG, "sv_gmm_accum: a state (sums, counts) is NULL");
    SV_REQUIRE(N > 0 && K > 0 && D > 0, SV_E_ARG, "sv_gmm_accum: non-positive size (N=%d K=%d D=%d)", N, K, D);
    SV_REQUIRE(P >= 1 && P <= GM_PMAX, SV_E_ARG, "sv_gmm_accum: P=%d outside [1, %d]", P, GM_PMAX);
    SV_REQUIRE(D <= GM_DMAX, SV_E_SHAPE, "sv_gmm_accum: D=%d > 2^20 (the grid's second dimension)", D);
    SV_REQUIRE((int64_t)K * (2 * (int64_t)D + 1) < INT32_MAX, SV_E_SHAPE, "sv_gmm_accum: K (2 D + 1) = %lld does not fit 31 bits",
               (long long)K * (2 * (long long)D + 1));
    const int slices = (D + GM_SLICE - 1) / GM_SLICE;
    if (K <= 16)
        hipLaunchKernelGGL((gmm_accum_kernel<16>), dim3(1, slices, P), dim3(KN_THREADS), 0, (hipStream_t)stream, x, lse, N, ivar, mean, cst,
                           K, D, sums, counts, P, init);
    else
        hipLaunchKernelGGL((gmm_accum_kernel<64>), dim3((K + 63) / 64, slices, P), dim3(KN_THREADS), 0, (hipStream_t)stream, x, lse, N, ivar,
                           mean, cst, K, D, sums, counts, P, init);
    return sv_check_launch("sv_gmm_accum");
}

// ------------------------------------------------------------------------------------------ sv_gmm_prepare, sv_gmm_finish
// Two launches each, and the second is the same kernel.
// gmm_rows_kernel, one block per component, 256 dimensions at a time.  With states (the M-step): every thread merges the P sums of its
// dimension in index order and writes mean and var -- an empty component (its r-sums add up to exactly 0) keeps both.  Always: ivar =
// 1 / var of the fp32 var, and log var in double meets in LDS, where thread 0 adds it in index order.  That sum travels to the second launch
// in (cst[k], cdf[k]) -- the two halves of a double in the two fp32 slots: the entry points allocate nothing.
__global__ __launch_bounds__(256) void gmm_rows_kernel(const double* sums, int P, int K, int D, double reg_covar, float* mean, float* var,
                                                       float* ivar, float* cst, float* cdf) {
#pragma clang fp contract(off)                                 // scikit-learn's operations, one rounding each
    __shared__ double lv[256];
    const int tid = threadIdx.x, k = blockIdx.x;
    const int64_t stride = (int64_t)K * (2 * D + 1) + 1, at = (int64_t)k * (2 * D + 1);
    double nk = 0.0;
    if (sums)
        for (int p = 0; p < P; ++p) nk += sums[p * stride + at];
    const bool update = sums && nk != 0.0;
    nk += 10.0 * DBL_EPSILON;
    double slv = 0.0;
    for (int d0 = 0; d0 < D; d0 += 256) {
        const int d = d0 + tid;
        double t = 0.0;
        if (d < D) {
            float vf = var[(int64_t)k * D + d];
            if (update) {
                double s1 = 0.0, s2 = 0.0;
                for (int p = 0; p < P; ++p) {
                    s1 += sums[p * stride + at + 1 + d];
                    s2 += sums[p * stride + at + 1 + D + d];
                }
                const double mu = s1 / nk;
                const double sq = mu * mu;
                vf = (float)((s2 / nk - sq) + reg_covar);
                mean[(int64_t)k * D + d] = (float)mu;
                var[(int64_t)k * D + d] = vf;
            }
            ivar[(int64_t)k * D + d] = 1.f / vf;
            t = log((double)vf);
        }
        lv[tid] = t;
        __syncthreads();
        if (tid == 0) {
            const int nd = D - d0 < 256 ? D - d0 : 256;
            for (int i = 0; i < nd; ++i) slv += lv[i];
        }
        __syncthreads();
    }
    if (tid == 0) {
        cst[k] = __int_as_float(__double2loint(slv));
        cdf[k] = __int_as_float(__double2hiint(slv));
    }
}

// gmm_table_kernel, one block.  With states: n_k again (P adds), their total in index order, logw, and the statistics.  Then the table
// from the fp32 logw: cst, and the cdf in two passes over K (the total of exp(logw), then the running sum), 1024 components at a time
// through LDS with thread 0 adding in index order.
__global__ __launch_bounds__(1024) void gmm_table_kernel(const double* sums, const int64_t* counts, int P, int K, int D, float* logw,
                                                         const float* var, float* cst, float* cdf, float* stats) {
    __shared__ double sh[1024];
    __shared__ double bc;
    const int tid = threadIdx.x;
    const int64_t stride = (int64_t)K * (2 * D + 1) + 1;
    if (sums) {
        double total = 0.0;
        for (int k0 = 0; k0 < K; k0 += 1024) {
            const int k = k0 + tid;
            double nk = 0.0;
            if (k < K) {
                for (int p = 0; p < P; ++p) nk += sums[p * stride + (int64_t)k * (2 * D + 1)];
                nk = nk != 0.0 ? nk + 10.0 * DBL_EPSILON : 0.0;        // (an empty component has no share)
            }
            sh[tid] = nk;
            __syncthreads();
            if (tid == 0) {
                const int nk_ = K - k0 < 1024 ? K - k0 : 1024;
                for (int i = 0; i < nk_; ++i) total += sh[i];
            }
            __syncthreads();
        }
        if (tid == 0) bc = total;
        __syncthreads();
        const double tot = bc;
        // logw, and the smallest var written: over the components that were updated
        double least = INFINITY;
        for (int k0 = 0; k0 < K; k0 += 1024) {
            const int k = k0 + tid;
            double nk = 0.0;
            if (k < K) {
                for (int p = 0; p < P; ++p) nk += sums[p * stride + (int64_t)k * (2 * D + 1)];
                logw[k] = nk != 0.0 ? (float)log((nk + 10.0 * DBL_EPSILON) / tot) : -INFINITY;
            }
            sh[tid] = nk;
            __syncthreads();
            const int nk_ = K - k0 < 1024 ? K - k0 : 1024;
            for (int i = 0; i < nk_; ++i)
                if (sh[i] != 0.0)
                    for (int d = tid; d < D; d += 1024) least = fmin(least, (double)var[(int64_t)(k0 + i) * D + d]);
            __syncthreads();
        }
        sh[tid] = least;
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < 1024; ++i) least = fmin(least, sh[i]);
            int64_t nfin = 0, nskip = 0;
            double lsum = 0.0;
            for (int p = 0; p < P; ++p) {
                nfin += counts[2 * p];
                nskip += counts[2 * p + 1];
                lsum += sums[p * stride + stride - 1];
            }
            stats[0] = (float)(lsum / (double)nfin);                    // (no finite row: NaN)
            stats[1] = (float)nfin;
            stats[2] = (float)nskip;
            stats[3] = (float)least;
        }
        __syncthreads();                                                // logw is written
    }
    const double base = (double)D * GM_LOG_2PI;
    double total = 0.0, run = 0.0;
    int last = -1;
    for (int pass = 0; pass < 2; ++pass)
        for (int k0 = 0; k0 < K; k0 += 1024) {
            const int k = k0 + tid;
            if (k < K) {
                const float lw = logw[k];
                sh[tid] = exp((double)lw);
                if (pass == 0) {
                    const double slv = __hiloint2double(__float_as_int(cdf[k]), __float_as_int(cst[k]));
                    cst[k] = (float)((double)lw - 0.5 * (base + slv));
                }
            }
            __syncthreads();
            if (tid == 0) {
                const int nk_ = K - k0 < 1024 ? K - k0 : 1024;
                for (int i = 0; i < nk_; ++i) {
                    if (pass == 0) {
                        total += sh[i];
                    } else {
                        run += sh[i];
                        cdf[k0 + i] = (float)(run / total);
                        if (sh[i] > 0.0) last = k0 + i;
                    }
                }
            }
            __syncthreads();
        }
    if (tid == 0 && last >= 0) cdf[last] = 1.f;
}

int sv_gmm_prepare(const float* logw, const float* mean, const float* var, int K, int D, float* ivar, float* cst, float* cdf, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(logw && mean && var, SV_E_ARG, "sv_gmm_prepare: a model pointer (logw, mean, var) is NULL");
    SV_REQUIRE(ivar && cst && cdf, SV_E_ARG, "sv_gmm_prepare: a table pointer (ivar, cst, cdf) is NULL");
    SV_REQUIRE(K > 0 && D > 0, SV_E_ARG, "sv_gmm_prepare: non-positive size (K=%d D=%d)", K, D);
    hipLaunchKernelGGL(gmm_rows_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, (const double*)nullptr, 0, K, D, 0.0,
                       const_cast<float*>(mean), const_cast<float*>(var), ivar, cst, cdf);          // (without states nothing of the model is written)
    hipLaunchKernelGGL(gmm_table_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)nullptr, (const int64_t*)nullptr, 0, K,
                       D, const_cast<float*>(logw), var, cst, cdf, (float*)nullptr);
    return sv_check_launch("sv_gmm_prepare");
}

int sv_gmm_finish(const double* sums, const int64_t* counts, int P, int K, int D, double reg_covar, float* logw, float* mean, float* var,
                  float* ivar, float* cst, float* cdf, float* stats, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(sums && counts, SV_E_ARG, "sv_gmm_finish: a state (sums, counts) is NULL");
    SV_REQUIRE(logw && mean && var, SV_E_ARG, "sv_gmm_finish: a model pointer (logw, mean, var) is NULL");
    SV_REQUIRE(ivar && cst && cdf, SV_E_ARG, "sv_gmm_finish: a table pointer (ivar, cst, cdf) is NULL");
    SV_REQUIRE(stats, SV_E_ARG, "sv_gmm_finish: stats is NULL");
    SV_REQUIRE(K > 0 && D > 0, SV_E_ARG, "sv_gmm_finish: non-positive size (K=%d D=%d)", K, D);
    SV_REQUIRE(P >= 1 && P <= GM_PMAX, SV_E_ARG, "sv_gmm_finish: P=%d outside [1, %d]", P, GM_PMAX);
    SV_REQUIRE(reg_covar >= 0.0 && reg_covar <= DBL_MAX, SV_E_ARG, "sv_gmm_finish: reg_covar=%g must be finite and >= 0", reg_covar);
    SV_REQUIRE((int64_t)K * (2 * (int64_t)D + 1) < INT32_MAX, SV_E_SHAPE, "sv_gmm_finish: K (2 D + 1) = %lld does not fit 31 bits",
               (long long)K * (2 * (long long)D + 1));
    hipLaunchKernelGGL(gmm_rows_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, sums, P, K, D, reg_covar, mean, var, ivar, cst, cdf);
    hipLaunchKernelGGL(gmm_table_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sums, counts, P, K, D, logw, var, cst, cdf, stats);
    return sv_check_launch("sv_gmm_finish");
}

// ------------------------------------------------------------------------------------------ sv_gmm_sample
// One wave per row: every lane forms the row's u from the generator call whose third counter word is 0xFFFFFFFF, finds the first
// component with cdf > u by bisection (the cdf does not decrease), and writes its columns 4 j .. 4 j + 3 from generator call j.
constexpr int GS_THREADS = 64;
__global__ __launch_bounds__(GS_THREADS) void gmm_sample_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                                                                const float* __restrict__ cdf, int K, int D, const int64_t* key, int64_t row0,
                                                                float* z, int64_t* comp) {
    const int64_t b = blockIdx.x;
    const uint64_t kv = (uint64_t)key[0], row = (uint64_t)(row0 + b);
    const sv_u32x4 r = sv_philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), 0xFFFFFFFFu, SV_GMM_PHILOX_TAG, (uint32_t)kv, (uint32_t)(kv >> 32));
    const float u = (float)(r.v[0] >> 8) * 0x1p-24f;
    int lo = 0, hi = K - 1;                            // the first k in [lo, hi] with cdf[k] > u; K - 1 if there is none (a NaN table)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    const int c = lo;
    if (comp && threadIdx.x == 0) comp[b] = c;
    for (int j = threadIdx.x; 4 * j < D; j += GS_THREADS) {
        float n[4];
        sv_normals4(kv, row, (uint32_t)j, SV_GMM_PHILOX_TAG, n);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * j + q;
            if (d < D) z[b * D + d] = fmaf(sqrtf(var[(int64_t)c * D + d]), n[q], mean[(int64_t)c * D + d]);
        }
    }
}

int sv_gmm_sample(const float* mean, const float* var, const float* cdf, int K, int D, const int64_t* key, int64_t row0, int B, float* z,
                  int64_t* comp, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(mean && var && cdf, SV_E_ARG, "sv_gmm_sample: a pointer (mean, var, cdf) is NULL");
    SV_REQUIRE(key, SV_E_ARG, "sv_gmm_sample: key is NULL");
    SV_REQUIRE(z, SV_E_ARG, "sv_gmm_sample: z is NULL");
    SV_REQUIRE(K > 0 && D > 0 && B > 0, SV_E_ARG, "sv_gmm_sample: non-positive size (K=%d D=%d B=%d)", K, D, B);
    SV_REQUIRE(row0 >= 0, SV_E_ARG, "sv_gmm_sample: row0=%lld must be >= 0", (long long)row0);
    // the third counter word of a column's call is d >> 2; 0xFFFFFFFF belongs to the component's call
    SV_REQUIRE(D <= (1 << 30), SV_E_SHAPE, "sv_gmm_sample: D=%d > 2^30 (the counter's third word)", D);
    hipLaunchKernelGGL(gmm_sample_kernel, dim3(B), dim3(GS_THREADS), 0, (hipStream_t)stream, mean, var, cdf, K, D, key, row0, z, comp);
    return sv_check_launch("sv_gmm_sample");
}
