// Linear probes on the latent space: one iteration of a multinomial logistic regression fitted by Nesterov's method, in three entry
// points (declared, with the exact definitions, in include/shotvae_hip.h):
//   sv_probe_rows    log sum_k exp v(i, k) per row -- knn.hip's tiles with an online (maximum fp32, sum double) state per row --, the
//                    row's loss lse - v(i, y_i), the first maximum, and on request the probabilities; the [N][K] matrix exists only then
//   sv_probe_accum   r = expf(v - lse) - [k = y_i] recomputed per tile and added, with r x, into P partial states (sv_kmeans_accum's
//                    rule: tile t of 64 rows to state t mod P), the accumulators in registers
//   sv_probe_update  the P states merged into the gradient at the look-ahead point, then one step of Nesterov's method in double and the
//                    fp32 (w, b) the scans read
// Plain HIP C++, fp32 / fp64 VALU; each takes a stream and allocates nothing: capturable.  v(i, k) is ONE sequence of operations
// (lp_tile, used by both scans); every floating-point sum is taken in a fixed order that depends only on the call's arguments; there is
// no atomic of any kind.  A repeated call sequence gives the same bits.
#include "common.h"
#include <float.h>
#include <math.h>

constexpr int LP_PMAX = 64;
constexpr int LP_SLICE = 32;                       // sv_probe_accum: the dimensions a block owns
constexpr int LP_DMAX = 1 << 20;                   // ... its grid's second dimension: D / 32 <= 65535 blocks
constexpr int LP_LD = KN_TG + 4;
constexpr int LP_STAGE = 2 * KN_DC * LP_LD;        // floats of LDS lp_tile stages through: x and w chunks

// ------------------------------------------------------------------------------------------ v(i, k)
// The scores of rows q0 .. q0 + 63 against classes g0 .. g0 + 16 NC - 1: thread (ty, tx) gets rows 4 ty + m, classes g0 + NC tx + n
// (NC = 4: knn_kernel's 64 x 64 tile; NC = 1: 64 x 16, a quarter of the work, for K <= 16 -- a pair's operations are the same).
// sv_pairdist's summation rule on knn_kernel's tile: 16 dimensions per staged chunk in fp32 with explicit fmaf in index order, the chunks
// in double in index order, b_k added in double; the next chunk's global loads are in flight while this one is multiplied.  Rows,
// classes and dimensions beyond the end are staged as zeros.
//   v = -inf                                       a class beyond K
//     = NaN                                        the sum is NaN or infinite (a row with a NaN or infinite entry)
//     = (float)(sum + (double) b_k)                otherwise
// Starts with a barrier (the stage may still be read) and is called by every thread of the block.
template <int NC>
__device__ __forceinline__ void lp_tile(const float* __restrict__ x, int N, int64_t q0, const float* __restrict__ w,
                                        const float* __restrict__ b, int K, int64_t g0, int D, float* sm, float v[4][NC]) {
    constexpr int TG = 16 * NC, LDG = TG + 4;
    float* Aq = sm;
    float* Ag = Aq + KN_DC * LP_LD;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][NC];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < NC; ++n) acc[m][n] = 0.0;
    float pq[4], pw[NC], none[4];
    kn_load<SV_DIST_EUCLID, 64>(x, nullptr, q0, N, 0, D, pq, none);
    kn_load<SV_DIST_EUCLID, TG>(w, nullptr, g0, K, 0, D, pw, none);
    for (int d0 = 0; d0 < D; d0 += KN_DC) {
        __syncthreads();                               // the previous chunk's products are read
        kn_store<SV_DIST_EUCLID, 64, false>(pq, none, q0, N, d0, D, Aq, nullptr, nullptr);
        kn_store<SV_DIST_EUCLID, TG, true>(pw, none, g0, K, d0, D, Ag, nullptr, nullptr);
        __syncthreads();
        if (d0 + KN_DC < D) {
            kn_load<SV_DIST_EUCLID, 64>(x, nullptr, q0, N, d0 + KN_DC, D, pq, none);
            kn_load<SV_DIST_EUCLID, TG>(w, nullptr, g0, K, d0 + KN_DC, D, pw, none);
        }
        float part[4][NC];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) part[m][n] = 0.f;
#pragma unroll 4
        for (int dd = 0; dd < KN_DC; ++dd) {
            float ga[NC], qa[4];
            if constexpr (NC == 4) {
                const f32x4 a4 = *reinterpret_cast<const f32x4*>(&Ag[dd * LDG + 4 * tx]);
#pragma unroll
                for (int n = 0; n < 4; ++n) ga[n] = a4[n];
            } else {
#pragma unroll
                for (int n = 0; n < NC; ++n) ga[n] = Ag[dd * LDG + NC * tx + n];
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) qa[m] = Aq[dd * LP_LD + 4 * ty + m];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < NC; ++n) part[m][n] = fmaf(qa[m], ga[n], part[m][n]);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) acc[m][n] += (double)part[m][n];
    }
#pragma unroll
    for (int n = 0; n < NC; ++n) {
        const int64_t col = g0 + NC * tx + n;
        const double bk = col < K ? (double)b[col] : 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const double s = acc[m][n] + bk;
            v[m][n] = col >= K ? -INFINITY : !(fabs(s) < (double)INFINITY) ? NAN : (float)s;
        }
    }
}

// the online log-sum-exp state of a row (mixture.hip's GmLse rule): the maximum in fp32 (the terms are fp32 values: exact), the sum in
// double, expf on fp32 differences.  Terms are finite; the empty state is (-inf, 0).
struct LpLse { float m; double s; };
__device__ __forceinline__ void lp_lse_add(LpLse& p, float v) {
    if (v <= p.m) {
        p.s += (double)expf(v - p.m);
    } else {
        p.s = p.s * (double)expf(p.m - v) + 1.0;       // (the empty state: 0 * expf(-inf) + 1)
        p.m = v;
    }
}
__device__ __forceinline__ LpLse lp_lse_merge(LpLse p, LpLse q) {
    if (q.m == -INFINITY) return p;
    if (p.m == -INFINITY) return q;
    const float m = fmaxf(p.m, q.m);
    return LpLse{m, p.s * (double)expf(p.m - m) + q.s * (double)expf(q.m - m)};
}

// ------------------------------------------------------------------------------------------ sv_probe_rows
// One block per 64 rows; the class tiles in index order.  Thread (ty, tx) keeps one state, one (value, index) maximum, the score of the
// row's own class and one NaN flag per row of its own over its columns of every tile; the 16 of a row meet in a butterfly, the lower
// lanes' state first, and lane tx = 0's result is the row's.  With proba the tiles are computed a second time against the finished
// lse.  NC = 1 (tiles of 16 classes) serves K <= 16.
template <int NC>
__global__ __launch_bounds__(KN_THREADS, 2) void probe_rows_kernel(const float* __restrict__ x, int N, const float* __restrict__ w,
                                                                   const float* __restrict__ b, int K, int D,
                                                                   const int64_t* __restrict__ label, float* lse, float* loss, int64_t* pred,
                                                                   float* proba) {
    __shared__ __attribute__((aligned(16))) float sm[LP_STAGE];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * 64;
    LpLse st[4];
    float bv[4], vy[4];
    int64_t bi[4], lab[4];
    int bad[4], has[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int64_t row = q0 + 4 * ty + m;
        st[m] = LpLse{-INFINITY, 0.0};
        bv[m] = -INFINITY;
        bi[m] = INT64_MAX;
        bad[m] = 0;
        has[m] = 0;
        vy[m] = 0.f;
        lab[m] = (label && row < N) ? label[row] : -1;
    }
    float v[4][NC];
    for (int64_t g0 = 0; g0 < K; g0 += 16 * NC) {
        lp_tile<NC>(x, N, q0, w, b, K, g0, D, sm, v);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int64_t col = g0 + NC * tx + n;
                const float f = v[m][n];
                if (col >= K) continue;
                if (f != f) { bad[m] = 1; continue; }
                lp_lse_add(st[m], f);
                if (f > bv[m]) { bv[m] = f; bi[m] = col; }             // (columns ascend: the first maximum)
                if (col == lab[m]) { vy[m] = f; has[m] = 1; }
            }
    }
    float row_lse[4];
    int row_bad[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        LpLse t = st[m];
        float fv = bv[m], fy = vy[m];
        int64_t fi = bi[m];
        int bb = bad[m], hh = has[m];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const LpLse o{__shfl_xor(t.m, off), __shfl_xor(t.s, off)};
            const float ov = __shfl_xor(fv, off), oy = __shfl_xor(fy, off);
            const int64_t oi = __shfl_xor(fi, off);
            const int oh = __shfl_xor(hh, off);
            bb |= __shfl_xor(bb, off);
            t = (tx & off) ? lp_lse_merge(o, t) : lp_lse_merge(t, o);          // the lower lanes' state first, on both sides
            if (ov > fv || (ov == fv && oi < fi)) { fv = ov; fi = oi; }
            if (oh) { fy = oy; hh = 1; }                                       // (one lane of the 16 holds the class's score)
        }
        float l = (bb || t.m == -INFINITY) ? NAN : (float)((double)t.m + log(t.s));
        l = __shfl(l, (threadIdx.x & 63) & ~15);                               // lane tx = 0's bits for the whole row
        row_lse[m] = l;
        row_bad[m] = bb;
        const int64_t row = q0 + 4 * ty + m;
        if (tx == 0 && row < N) {
            lse[row] = l;
            if (loss) loss[row] = (bb || !hh) ? NAN : l - fy;
            if (pred) pred[row] = (bb || fi == INT64_MAX) ? -1 : fi;
        }
    }
    if (!proba) return;
    for (int64_t g0 = 0; g0 < K; g0 += 16 * NC) {
        lp_tile<NC>(x, N, q0, w, b, K, g0, D, sm, v);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int64_t col = g0 + NC * tx + n, row = q0 + 4 * ty + m;
                if (col < K && row < N) proba[row * K + col] = row_bad[m] ? NAN : expf(v[m][n] - row_lse[m]);
            }
    }
}

int sv_probe_rows(const float* x, int N, const float* w, const float* b, int K, int D, const int64_t* label, float* lse, float* loss,
                  int64_t* pred, float* proba, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && w && b, SV_E_ARG, "sv_probe_rows: a pointer (x, w, b) is NULL");
    SV_REQUIRE(lse, SV_E_ARG, "sv_probe_rows: lse is NULL");
    SV_REQUIRE(!loss || label, SV_E_ARG, "sv_probe_rows: loss without label");
    SV_REQUIRE(N > 0 && D > 0, SV_E_ARG, "sv_probe_rows: non-positive size (N=%d D=%d)", N, D);
    SV_REQUIRE(K >= 2, SV_E_ARG, "sv_probe_rows: K=%d classes (K >= 2)", K);
    if (K <= 16)
        hipLaunchKernelGGL((probe_rows_kernel<1>), dim3((N - 1) / 64 + 1), dim3(KN_THREADS), 0, (hipStream_t)stream, x, N, w, b, K, D, label,
                           lse, loss, pred, proba);
    else
        hipLaunchKernelGGL((probe_rows_kernel<4>), dim3((N - 1) / 64 + 1), dim3(KN_THREADS), 0, (hipStream_t)stream, x, N, w, b, K, D, label,
                           lse, loss, pred, proba);
    return sv_check_launch("sv_probe_rows");
}

// ------------------------------------------------------------------------------------------ sv_probe_accum
// Block (kt, s, p): the KT classes from kt KT, the S = 32 dimensions from S s, partial state p.  It walks the row tiles p, p + P, ... of
// the call: lp_tile gives the tile's v (over ALL dimensions: every slice recomputes it -- the trade of DESIGN.md 4l), r = expf(v - lse)
// - [k = y] goes to LDS once together with the tile's 64 x S slice of x, and then thread (class c = tid % KT, dimension group g = tid /
// KT) streams the 64 rows in index order through its 1 + J accumulators IN REGISTERS: r, and r x of its J = S KT / 256 dimensions -- a
// [KT x 64] . [64 x S] product in double with a fixed order and no dependent LDS chain.  A row that is skipped (lse not finite, or a
// label outside [0, K)) or beyond the end enters as r = 0, x = 0: adding +0 changes no accumulator bit.  KT = 16 serves K <= 16, KT = 64
// everything else.  Block (0, 0, p) also counts the rows and adds their losses.  S stays at 32 dimensions: the walk is bound by latency,
// and a grid that fills the device beat less recomputation (mixture.hip's measurement).
template <int KT>
__global__ __launch_bounds__(KN_THREADS, 2) void probe_accum_kernel(const float* __restrict__ x, const int64_t* __restrict__ label,
                                                                    const float* __restrict__ lse, const float* __restrict__ loss, int N,
                                                                    const float* __restrict__ w, const float* __restrict__ b, int K, int D,
                                                                    double* sums, int64_t* counts, int P, int init, float* resid) {
    constexpr int S = LP_SLICE, NC = KT / 16, G = KN_THREADS / KT, J = S / G, LDX = S + 1;
    __shared__ __attribute__((aligned(16))) float sm[LP_STAGE];
    __shared__ float R[64 * KT];
    __shared__ float X[64 * LDX];
    __shared__ float sl[64];
    __shared__ float so[64];
    __shared__ int yl[64];                             // the row's class, -1 for a row that is skipped or beyond the end
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c = tid % KT, g = tid / KT, p = blockIdx.z;
    const int64_t k0 = (int64_t)blockIdx.x * KT, k = k0 + c;
    const int d0 = blockIdx.y * S + g * J;
    const int64_t stride = (int64_t)K * (D + 1) + 1;
    double* state = sums + (int64_t)p * stride;
    double* mine = state + k * (D + 1);
    const bool tally = blockIdx.x == 0 && blockIdx.y == 0 && tid == 0;

    double a0 = 0.0, a1[J];
#pragma unroll
    for (int j = 0; j < J; ++j) a1[j] = 0.0;
    int64_t nused = 0, nskip = 0;
    double lsum = 0.0;
    if (!init) {
        if (k < K) {
            a0 = mine[0];
#pragma unroll
            for (int j = 0; j < J; ++j)
                if (d0 + j < D) a1[j] = mine[1 + d0 + j];
        }
        if (tally) { nused = counts[2 * p]; nskip = counts[2 * p + 1]; lsum = state[stride - 1]; }
    }

    const int64_t ntiles = ((int64_t)N + 63) / 64;
    float v[4][NC];
    for (int64_t t = p; t < ntiles; t += P) {
        const int64_t q0 = t * 64;
        lp_tile<NC>(x, N, q0, w, b, K, k0, D, sm, v);                  // (its barriers: the previous tile's R, X, sl, yl are read)
        if (tid < 64) {
            const bool in = q0 + tid < N;
            const float l = in ? lse[q0 + tid] : NAN;
            const int64_t y = in ? label[q0 + tid] : -1;
            const bool used = l - l == 0.f && y >= 0 && y < K;         // lse finite, the label a class
            sl[tid] = l;
            so[tid] = used ? loss[q0 + tid] : 0.f;
            yl[tid] = used ? (int)y : -1;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                const int row = 4 * ty + m, col = NC * tx + n;
                const int y = yl[row];
                const float r = y >= 0 ? expf(v[m][n] - sl[row]) - (k0 + col == y ? 1.f : 0.f) : 0.f;
                R[row * KT + col] = r;
                if (resid && blockIdx.y == 0 && q0 + row < N && k0 + col < K) resid[(q0 + row) * K + k0 + col] = r;
            }
        for (int i = tid; i < 64 * S; i += KN_THREADS) {
            const int row = i / S, dd = i % S, d = blockIdx.y * S + dd;
            X[row * LDX + dd] = (yl[row] >= 0 && d < D) ? x[(q0 + row) * D + d] : 0.f;          // (used: the row is inside the call)
        }
        __syncthreads();
#pragma unroll 8                                       // (fully unrolled, the 16-class form needed more than its 256 registers)
        for (int i = 0; i < 64; ++i) {
#pragma clang fp contract(off)                         // the header's order: the product rounded (it is exact), THEN added
            const double r = (double)R[i * KT + c];
            a0 = a0 + r;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double xd = (double)X[i * LDX + g * J + j];
                const double rx = r * xd;                              // exact: 24 x 24 bits
                a1[j] = a1[j] + rx;
            }
        }
        if (tally)
            for (int i = 0; i < 64 && q0 + i < N; ++i) {
                if (yl[i] >= 0) { ++nused; lsum = __dadd_rn(lsum, (double)so[i]); }
                else ++nskip;
            }
    }

    if (k < K) {
        if (blockIdx.y == 0 && g == 0) mine[0] = a0;
#pragma unroll
        for (int j = 0; j < J; ++j)
            if (d0 + j < D) mine[1 + d0 + j] = a1[j];
    }
    if (tally) { counts[2 * p] = nused; counts[2 * p + 1] = nskip; state[stride - 1] = lsum; }
}

int sv_probe_accum(const float* x, const int64_t* label, const float* lse, const float* loss, int N, const float* w, const float* b, int K,
                   int D, double* sums, int64_t* counts, int P, int init, float* resid, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && label && lse && loss, SV_E_ARG, "sv_probe_accum: a row pointer (x, label, lse, loss) is NULL");
    SV_REQUIRE(w && b, SV_E_ARG, "sv_probe_accum: a model pointer (w, b) is NULL");
    SV_REQUIRE(sums && counts, SV_E_ARG, "sv_probe_accum: a state (sums, counts) is NULL");
    SV_REQUIRE(N > 0 && D > 0, SV_E_ARG, "sv_probe_accum: non-positive size (N=%d D=%d)", N, D);
    SV_REQUIRE(K >= 2, SV_E_ARG, "sv_probe_accum: K=%d classes (K >= 2)", K);
    SV_REQUIRE(P >= 1 && P <= LP_PMAX, SV_E_ARG, "sv_probe_accum: P=%d outside [1, %d]", P, LP_PMAX);
    SV_REQUIRE(D <= LP_DMAX, SV_E_SHAPE, "sv_probe_accum: D=%d > 2^20 (the grid's second dimension)", D);
    SV_REQUIRE((int64_t)K * ((int64_t)D + 1) < INT32_MAX, SV_E_SHAPE, "sv_probe_accum: K (D + 1) = %lld does not fit 31 bits",
               (long long)K * ((long long)D + 1));
    const int slices = (D + LP_SLICE - 1) / LP_SLICE;
    if (K <= 16)
        hipLaunchKernelGGL((probe_accum_kernel<16>), dim3(1, slices, P), dim3(KN_THREADS), 0, (hipStream_t)stream, x, label, lse, loss, N, w,
                           b, K, D, sums, counts, P, init, resid);
    else
        hipLaunchKernelGGL((probe_accum_kernel<64>), dim3((K + 63) / 64, slices, P), dim3(KN_THREADS), 0, (hipStream_t)stream, x, label, lse,
                           loss, N, w, b, K, D, sums, counts, P, init, resid);
    return sv_check_launch("sv_probe_accum");
}

// ------------------------------------------------------------------------------------------ sv_probe_update
// probe_grad_kernel, one block per class, 256 elements of the class's row [intercept, D weights] at a time: every thread merges the P
// sums of its element in index order and writes the gradient at the look-ahead point INTO STATE 0 (the states are consumed).  Its share
// of sum look^2 (its elements in index order) and of max |g| meets in LDS, where thread 0 adds the 256 shares in index order; the class's
// two partials go to stats[4 + 2 k], stats[5 + 2 k]: the entry points allocate nothing.
__global__ __launch_bounds__(256) void probe_grad_kernel(double* sums, const int64_t* counts, int P, int K, int D, double lambda,
                                                         const double* look, double* stats) {
#pragma clang fp contract(off)                                 // the header's operations, one rounding each
    __shared__ double sq[256];
    __shared__ double mg[256];
    const int tid = threadIdx.x, k = blockIdx.x;
    const int64_t stride = (int64_t)K * (D + 1) + 1, at = (int64_t)k * (D + 1);
    int64_t n = 0;
    for (int p = 0; p < P; ++p) n += counts[2 * p];
    const double dn = (double)n;
    double q = 0.0, mx = 0.0;
    for (int e = tid; e <= D; e += 256) {
        double G = 0.0;
        for (int p = 0; p < P; ++p) G = G + sums[p * stride + at + e];
        double gr = G / dn;
        if (e > 0) {
            const double lk = look[at + e];
            const double pen = lambda * lk;
            gr = gr + pen;
            const double l2 = lk * lk;
            q = q + l2;
        }
        sums[at + e] = gr;
        mx = (gr != gr || mx != mx) ? NAN : fmax(mx, fabs(gr));
    }
    sq[tid] = q;
    mg[tid] = mx;
    __syncthreads();
    if (tid == 0) {
        double tq = 0.0, tm = 0.0;
        for (int i = 0; i < 256; ++i) {
            tq = tq + sq[i];
            tm = (mg[i] != mg[i] || tm != tm) ? NAN : fmax(tm, mg[i]);
        }
        stats[4 + 2 * k] = tm;
        stats[5 + 2 * k] = tq;
    }
}

// probe_step_kernel, one block: the counts and the loss sums of the P states in index order, the class partials in index order, the
// statistics, and the step itself over the K (D + 1) elements.  Without a used row nothing of the model is written.
__global__ __launch_bounds__(1024) void probe_step_kernel(const double* sums, const int64_t* counts, int P, int K, int D, double lambda,
                                                          double inv_L, double beta, double* theta, double* look, float* w, float* b,
                                                          double* stats) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int64_t stride = (int64_t)K * (D + 1) + 1, total = stride - 1;
    int64_t n = 0, nskip = 0;
    for (int p = 0; p < P; ++p) { n += counts[2 * p]; nskip += counts[2 * p + 1]; }
    if (tid == 0) {
        double lsum = 0.0, tq = 0.0, tm = 0.0;
        for (int p = 0; p < P; ++p) lsum = lsum + sums[p * stride + stride - 1];
        for (int k = 0; k < K; ++k) {
            const double m = stats[4 + 2 * k];
            tm = (m != m || tm != tm) ? NAN : fmax(tm, m);
            tq = tq + stats[5 + 2 * k];
        }
        const double mean = lsum / (double)n;
        const double pen = lambda * tq;
        const double half = 0.5 * pen;
        stats[0] = n ? mean + half : NAN;
        stats[1] = n ? tm : NAN;
        stats[2] = (double)n;
        stats[3] = (double)nskip;
    }
    if (n == 0) return;
    for (int64_t e = tid; e < total; e += 1024) {
        const double gr = sums[e], lk = look[e], th = theta[e];
        const double stp = inv_L * gr;
        const double tn = lk - stp;
        const double dif = tn - th;
        const double mom = beta * dif;
        const double ln = tn + mom;
        theta[e] = tn;
        look[e] = ln;
        const int64_t k = e / (D + 1), d = e % (D + 1);
        if (d == 0) b[k] = (float)ln;
        else w[k * D + d - 1] = (float)ln;
    }
}

int sv_probe_update(double* sums, const int64_t* counts, int P, int K, int D, double lambda, double inv_L, double beta, double* theta,
                    double* look, float* w, float* b, double* stats, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(sums && counts, SV_E_ARG, "sv_probe_update: a state (sums, counts) is NULL");
    SV_REQUIRE(theta && look, SV_E_ARG, "sv_probe_update: an iterate (theta, look) is NULL");
    SV_REQUIRE(w && b, SV_E_ARG, "sv_probe_update: a model pointer (w, b) is NULL");
    SV_REQUIRE(stats, SV_E_ARG, "sv_probe_update: stats is NULL");
    SV_REQUIRE(D > 0, SV_E_ARG, "sv_probe_update: non-positive size (D=%d)", D);
    SV_REQUIRE(K >= 2, SV_E_ARG, "sv_probe_update: K=%d classes (K >= 2)", K);
    SV_REQUIRE(P >= 1 && P <= LP_PMAX, SV_E_ARG, "sv_probe_update: P=%d outside [1, %d]", P, LP_PMAX);
    SV_REQUIRE(lambda > 0.0 && lambda <= DBL_MAX, SV_E_ARG, "sv_probe_update: lambda=%g must be finite and > 0", lambda);
    SV_REQUIRE(inv_L > 0.0 && inv_L <= DBL_MAX, SV_E_ARG, "sv_probe_update: inv_L=%g must be finite and > 0", inv_L);
    SV_REQUIRE(beta >= 0.0 && beta < 1.0, SV_E_ARG, "sv_probe_update: beta=%g outside [0, 1)", beta);
    SV_REQUIRE(D <= LP_DMAX, SV_E_SHAPE, "sv_probe_update: D=%d > 2^20", D);
    SV_REQUIRE((int64_t)K * ((int64_t)D + 1) < INT32_MAX, SV_E_SHAPE, "sv_probe_update: K (D + 1) = %lld does not fit 31 bits",
               (long long)K * ((long long)D + 1));
    hipLaunchKernelGGL(probe_grad_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, sums, counts, P, K, D, lambda, look, stats);
    hipLaunchKernelGGL(probe_step_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, sums, counts, P, K, D, lambda, inv_L, beta, theta, look,
                       w, b, stats);
    return sv_check_launch("sv_probe_update");
}
