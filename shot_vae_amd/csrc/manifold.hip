// Membership counts of k-th-neighbour balls in latent space: the question behind improved precision / recall and density / coverage
// (declared, with the exact definitions, in include/shotvae_hip.h):
//   sv_ball_scan   q_count[i] += #{j : v(i, j) <= g_r[j]},  g_count[j] += #{i : v(i, j) <= g_r[j]}  over the Q x N pairs of the call
// knn_kernel's tile (64 queries x 64 gallery rows, 16 dimensions per staged chunk, the next chunk's global loads in flight while this
// one is multiplied) with a compare where the merge is: no key tile, no list.  v(i, j) is sv_pairdist's value of the pair bit for bit
// (ONE fixed sequence of operations: 16 dimensions in fp32 with explicit fmaf, the 16-blocks in double, rounded once), so a count is a
// function of the pair set alone: the gallery cut into calls, the queries cut into calls and any P give the same integers.  The state is
// an integer: partial counts meet in registers and LDS and leave a block as integer atomics -- no workspace, no order-dependent sum,
// no float atomic.  Plain HIP C++; takes a stream and allocates nothing: capturable.
#include "common.h"
#include <math.h>

constexpr int BS_PMAX = 64;

// Block (x, p): query tile x, the gallery tiles p, p + P, ... of the call.  Thread (ty, tx) owns rows 4 ty .., columns 4 tx .. of every
// tile and compares its 4 x 4 values with the four radii of its columns (staged once per tile, prefetched with the tile's first chunk).
// Row counts stay in registers over all tiles and meet in a butterfly at the end: one atomic per row and block.  Column counts of a
// tile meet per wave in a butterfly, per block in cw (plain stores); the first 64 threads add them to g_count behind the NEXT tile's
// first barrier (or the one barrier after the last tile): one atomic per touched column and tile, and no barrier of their own.
template <int METRIC>
__global__ __launch_bounds__(KN_THREADS, 2) void ball_scan_kernel(const float* __restrict__ q_mu, const float* __restrict__ q_ls, int Q,
                                                                  const float* __restrict__ g_mu, const float* __restrict__ g_ls,
                                                                  const float* __restrict__ g_r, int N, int D, int64_t col0, int64_t self0,
                                                                  int P, unsigned long long* q_count, unsigned long long* g_count) {
    typedef KnTraits<METRIC> TR;
    constexpr int MQ = 4, TQ = 16 * MQ, LDQ = TQ + 4, LDG = KN_TG + 4;
    __shared__ __attribute__((aligned(16))) float sm[(TR::TWO ? 2 : 1) * KN_DC * (LDQ + LDG)];
    __shared__ __attribute__((aligned(16))) float sr[KN_TG];
    __shared__ __attribute__((aligned(16))) int cw[KN_THREADS / 64][KN_TG];
    float* Aq = sm;
    float* Ag = Aq + KN_DC * LDQ;
    float* Bq = TR::TWO ? Ag + KN_DC * LDG : nullptr;  // (W2 only: sigma)
    float* Bg = TR::TWO ? Bq + KN_DC * LDQ : nullptr;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6, p = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int64_t step = (int64_t)P * KN_TG;

    int rc[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) rc[m] = 0;
    bool pending = false;                              // cw holds the column counts of the tile at gprev
    int64_t gprev = 0;

    float pqm[MQ], pql[MQ], pgm[4], pgl[4], pr = NAN;
    kn_load<METRIC, TQ>(q_mu, q_ls, q0, Q, 0, D, pqm, pql);
    kn_load<METRIC, KN_TG>(g_mu, g_ls, (int64_t)p * KN_TG, N, 0, D, pgm, pgl);
    if (tid < KN_TG && (int64_t)p * KN_TG + tid < N) pr = g_r[(int64_t)p * KN_TG + tid];
    for (int64_t g0 = (int64_t)p * KN_TG; g0 < N; g0 += step) {
        double acc[MQ][4];
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;

        for (int d0 = 0; d0 < D; d0 += KN_DC) {
            __syncthreads();                           // the previous chunk's products, the previous tile's radii and cw are read
            kn_store<METRIC, TQ, false>(pqm, pql, q0, Q, d0, D, Aq, Bq, nullptr);
            kn_store<METRIC, KN_TG, true>(pgm, pgl, g0, N, d0, D, Ag, Bg, nullptr);
            if (d0 == 0 && tid < KN_TG) {
                sr[tid] = pr;                          // a column beyond the end: NaN, which contains nothing
                if (pending) {
                    const int c = cw[0][tid] + cw[1][tid] + cw[2][tid] + cw[3][tid];
                    if (c) atomicAdd(&g_count[gprev + tid], (unsigned long long)c);
                }
            }
            __syncthreads();
            {
                const bool last = d0 + KN_DC >= D;
                const int nd0 = last ? 0 : d0 + KN_DC;
                kn_load<METRIC, TQ>(q_mu, q_ls, q0, Q, nd0, D, pqm, pql);
                kn_load<METRIC, KN_TG>(g_mu, g_ls, last ? g0 + step : g0, N, nd0, D, pgm, pgl);
                if (last && tid < KN_TG) pr = g0 + step + tid < N ? g_r[g0 + step + tid] : NAN;
            }
            float part[MQ][4];
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) part[m][n] = 0.f;
#pragma unroll 4
            for (int dd = 0; dd < KN_DC; ++dd) {
                float qa[MQ], qb[MQ];
                const f32x4 ga = *reinterpret_cast<const f32x4*>(&Ag[dd * LDG + 4 * tx]);
                f32x4 gb = {0.f, 0.f, 0.f, 0.f};
                if (TR::TWO) gb = *reinterpret_cast<const f32x4*>(&Bg[dd * LDG + 4 * tx]);
#pragma unroll
                for (int m = 0; m < MQ; ++m) {
                    qa[m] = Aq[dd * LDQ + MQ * ty + m];
                    qb[m] = TR::TWO ? Bq[dd * LDQ + MQ * ty + m] : 0.f;
                }
#pragma unroll
                for (int m = 0; m < MQ; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        // knn_kernel's operations, one for one: the value of a pair is sv_pairdist's
                        const float dm = qa[m] - ga[n];
                        if (METRIC == SV_DIST_W2) {
                            const float ds = qb[m] - gb[n];
                            part[m][n] = fmaf(ds, ds, fmaf(dm, dm, part[m][n]));
                        } else {
                            part[m][n] = fmaf(dm, dm, part[m][n]);
                        }
                    }
            }
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += (double)part[m][n];
        }

        // (sr was written before this tile's last barrier; the next write is behind the next tile's first)
        const f32x4 r = *reinterpret_cast<const f32x4*>(&sr[4 * tx]);
        int cc[4] = {0, 0, 0, 0};
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int row = MQ * ty + m, col = 4 * tx + n;
                const float f = (float)acc[m][n];
                const int64_t gi = col0 + g0 + col;
                // f < +inf: false for a NaN and for +inf; f <= r: false for a NaN radius
                const bool in = q0 + row < Q && g0 + col < N && f < INFINITY && f <= r[n] && !(self0 >= 0 && gi == self0 + q0 + row);
                rc[m] += in;
                cc[n] += in;
            }
        if (g_count) {                                 // (a kernel argument: the whole block agrees)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                cc[n] += __shfl_xor(cc[n], 16);
                cc[n] += __shfl_xor(cc[n], 32);
            }
            if (lane < 16) {
#pragma unroll
                for (int n = 0; n < 4; ++n) cw[wave][4 * tx + n] = cc[n];
            }
            pending = true;
            gprev = g0;
        }
    }

    if (pending) {                                     // (the same for every thread of the block)
        __syncthreads();
        if (tid < KN_TG) {
            const int c = cw[0][tid] + cw[1][tid] + cw[2][tid] + cw[3][tid];
            if (c) atomicAdd(&g_count[gprev + tid], (unsigned long long)c);
        }
    }
    if (q_count) {
#pragma unroll
        for (int m = 0; m < MQ; ++m) {
            int t = rc[m];
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) t += __shfl_xor(t, off);
            const int64_t row = q0 + MQ * ty + m;
            if (tx == 0 && row < Q && t) atomicAdd(&q_count[row], (unsigned long long)t);
        }
    }
}

int sv_ball_scan(int metric, const float* q_mu, const float* q_ls, int Q, const float* g_mu, const float* g_ls, const float* g_r, int N,
                 int D, int64_t col0, int64_t self0, int P, int64_t* q_count, int64_t* g_count, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(metric == SV_DIST_W2 || metric == SV_DIST_EUCLID, SV_E_ARG,
               "sv_ball_scan: bad metric %d (a radius needs a symmetric distance: SV_DIST_W2 or SV_DIST_EUCLID)", metric);
    SV_REQUIRE(q_mu && g_mu && g_r, SV_E_ARG, "sv_ball_scan: q_mu, g_mu or g_r is NULL");
    SV_REQUIRE(metric != SV_DIST_W2 || (q_ls && g_ls), SV_E_ARG, "sv_ball_scan: metric %d reads ls: q_ls or g_ls is NULL", metric);
    SV_REQUIRE(q_count || g_count, SV_E_ARG, "sv_ball_scan: no output (q_count and g_count are both NULL)");
    SV_REQUIRE(Q > 0 && N > 0 && D > 0, SV_E_ARG, "sv_ball_scan: non-positive size (Q=%d N=%d D=%d)", Q, N, D);
    SV_REQUIRE(P >= 1 && P <= BS_PMAX, SV_E_ARG, "sv_ball_scan: P=%d outside [1, %d]", P, BS_PMAX);
    SV_REQUIRE(col0 >= 0 && self0 >= -1, SV_E_ARG, "sv_ball_scan: col0=%lld must be >= 0 and self0=%lld >= -1", (long long)col0,
               (long long)self0);
    SV_REQUIRE(col0 <= INT64_MAX - N - 64 && self0 <= INT64_MAX - Q - 64, SV_E_SHAPE,
               "sv_ball_scan: col0=%lld + N or self0=%lld + Q overflows the index", (long long)col0, (long long)self0);
    const dim3 grid((Q + 63) / 64, P);
    unsigned long long* qc = reinterpret_cast<unsigned long long*>(q_count);
    unsigned long long* gc = reinterpret_cast<unsigned long long*>(g_count);
    if (metric == SV_DIST_W2)
        hipLaunchKernelGGL(ball_scan_kernel<SV_DIST_W2>, grid, dim3(KN_THREADS), 0, (hipStream_t)stream, q_mu, q_ls, Q, g_mu, g_ls, g_r, N, D,
                           col0, self0, P, qc, gc);
    else
        hipLaunchKernelGGL(ball_scan_kernel<SV_DIST_EUCLID>, grid, dim3(KN_THREADS), 0, (hipStream_t)stream, q_mu, q_ls, Q, g_mu, g_ls, g_r, N,
                           D, col0, self0, P, qc, gc);
    return sv_check_launch("sv_ball_scan");
}
