// Posterior distance matrices and k-nearest-neighbour search in latent space (declared, with the exact definitions, in
// include/shotvae_hip.h):
//   sv_pairdist   the [Q][N] matrix of one of the four metrics of lib/utils/calculate_dist.py
//   sv_knn_scan   the same tiles, merged into running per-query k-lists: the matrix never leaves the chip
//   sv_knn_vote   class votes of the neighbours, the prediction and the integer counters of a test set
// Plain HIP C++, fp32 VALU in the direct-difference form (no |a|^2 + |b|^2 - 2ab expansion: the self-distance is exact).  Each takes
// a stream and allocates nothing: capturable.  A pair's distance is ONE fixed sequence of operations (16 dimensions summed in fp32 in
// index order, the 16-blocks summed in double in index order), whatever tile it falls in; a k-list is the k smallest (key, index)
// pairs under a strict total order.  So the lists do not depend on how a gallery is cut into calls, there is no float atomic, and
// deterministic mode is the only mode.
#include "common.h"
#include <math.h>

// (the tile constants KN_THREADS / KN_TG / KN_DC and the staging helpers kn_load / kn_store / kn_aux_reduce are in common.h: aggpost.hip
// stages its tiles with them too)

constexpr int KN_KMAX = 256;          // four list slots per lane of the merging wave
constexpr int64_t KN_NOIDX = INT64_MAX;      // an empty slot inside the kernel: (key = +inf, index = INT64_MAX) sorts last

__device__ __forceinline__ bool kn_before(float ka, int64_t ia, float kb, int64_t ib) { return ka < kb || (ka == kb && ia < ib); }

// PAIR: write the matrix.  Otherwise: merge every tile into the block's k-lists (LDS; dynamic: int64 index [TQ][k], then float key
// [TQ][k]).  key = the distance, or minus the similarity for the cosine: smaller is closer for every metric inside the kernel.
template <int METRIC, int MQ, bool PAIR>
__global__ __launch_bounds__(KN_THREADS, 2) void knn_kernel(const float* __restrict__ q_mu, const float* __restrict__ q_ls, int Q,
                                                         const float* __restrict__ g_mu, const float* __restrict__ g_ls, int N, int D,
                                                         int64_t col0, int64_t self0, int k, float* best_val, int64_t* best_idx,
                                                         int init, float* out, int64_t ldo) {
    typedef KnTraits<METRIC> TR;
    constexpr int TQ = 16 * MQ, LDQ = TQ + 4, LDG = KN_TG + 4, LDT = KN_TG + 1;
    constexpr int STAGE = 2 * KN_DC * (LDQ + LDG), TILE = TQ * LDT;
    constexpr int RW = TQ / 4;                         // query rows per merging wave
    constexpr bool COS = METRIC == SV_DIST_COSINE;
    __shared__ __attribute__((aligned(16))) float sm[STAGE > TILE ? STAGE : TILE];
    __shared__ double auxq[TQ], auxg[KN_TG];
    __shared__ float thr_key[TQ];
    __shared__ int64_t thr_idx[TQ];
    extern __shared__ __attribute__((aligned(16))) unsigned char kn_dyn[];
    float* Aq = sm;
    float* Bq = Aq + KN_DC * LDQ;
    float* Ag = Bq + KN_DC * LDQ;
    float* Bg = Ag + KN_DC * LDG;
    float* tile = sm;                                  // the finished keys of one tile: aliases the staging area
    int64_t* lidx = reinterpret_cast<int64_t*>(kn_dyn);
    float* lkey = reinterpret_cast<float*>(lidx + (PAIR ? 0 : (size_t)TQ * k));

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int J = (k + 63) >> 6;                       // list slots per lane: slot s = 64 j + lane
    const int kj = (k - 1) >> 6, kl = (k - 1) & 63;    // where the k-th entry (the threshold) sits

    if (!PAIR) {
        for (int rr = 0; rr < RW; ++rr) {
            const int row = wave * RW + rr;
            const bool live = q0 + row < Q && !init;
            for (int j = 0; j < J; ++j) {
                const int s = 64 * j + lane;
                if (s >= k) continue;
                float key = INFINITY;
                int64_t idx = KN_NOIDX;
                if (live) {
                    const int64_t gi = best_idx[(q0 + row) * k + s];
                    const float v = best_val[(q0 + row) * k + s];
                    if (gi >= 0) { idx = gi; key = COS ? -v : v; }
                }
                lkey[row * k + s] = key;
                lidx[row * k + s] = idx;
                if (s == k - 1) { thr_key[row] = key; thr_idx[row] = idx; }
            }
        }
    }

    float pqm[MQ], pql[MQ], pgm[4], pgl[4];            // the chunk in flight (prefetched while the previous one is multiplied)
    kn_load<METRIC, TQ>(q_mu, q_ls, q0, Q, 0, D, pqm, pql);
    kn_load<METRIC, KN_TG>(g_mu, g_ls, 0, N, 0, D, pgm, pgl);
    for (int64_t g0 = 0; g0 < N; g0 += KN_TG) {
        double acc[MQ][4], aq[MQ], ag[4];
#pragma unroll
        for (int m = 0; m < MQ; ++m) {
            aq[m] = 0.0;
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) ag[n] = 0.0;

        for (int d0 = 0; d0 < D; d0 += KN_DC) {
            __syncthreads();                           // the previous readers of sm (a chunk's products, a tile's merge) are done
            kn_store<METRIC, TQ, false>(pqm, pql, q0, Q, d0, D, Aq, Bq, aq);
            kn_store<METRIC, KN_TG, true>(pgm, pgl, g0, N, d0, D, Ag, Bg, ag);
            __syncthreads();
            {                                          // the next chunk: of this tile, or the first of the next (beyond the end: zeros)
                const bool last = d0 + KN_DC >= D;
                const int nd0 = last ? 0 : d0 + KN_DC;
                kn_load<METRIC, TQ>(q_mu, q_ls, q0, Q, nd0, D, pqm, pql);
                kn_load<METRIC, KN_TG>(g_mu, g_ls, last ? g0 + KN_TG : g0, N, nd0, D, pgm, pgl);
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
                        // explicit fmaf: the same roundings in every instantiation (no contraction left to the compiler)
                        const float dm = qa[m] - ga[n];
                        if (METRIC == SV_DIST_KL) {
                            part[m][n] = fmaf(fmaf(dm, dm, qb[m]), gb[n], part[m][n]);     // (sigma1^2 + (mu1 - mu2)^2) / sigma2^2
                        } else if (METRIC == SV_DIST_W2) {
                            const float ds = qb[m] - gb[n];
                            part[m][n] = fmaf(ds, ds, fmaf(dm, dm, part[m][n]));
                        } else if (METRIC == SV_DIST_EUCLID) {
                            part[m][n] = fmaf(dm, dm, part[m][n]);
                        } else {
                            part[m][n] = fmaf(qa[m], ga[n], part[m][n]);
                        }
                    }
            }
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += (double)part[m][n];
        }
        if (TR::AUX) {                                 // (tx, ty = the dimension and row index of the staging role)
#pragma unroll
            for (int i = 0; i < MQ; ++i) {
                const double t = kn_aux_reduce(aq[i]);
                if (tx == 0) auxq[ty + 16 * i] = t;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double t = kn_aux_reduce(ag[i]);
                if (tx == 0) auxg[ty + 16 * i] = t;
            }
        }
        __syncthreads();                               // the chunk's products are read; the row scalars are visible

#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int row = MQ * ty + m, col = 4 * tx + n;
                double v = acc[m][n];
                if (METRIC == SV_DIST_KL) v = fma(0.5, v, auxg[col] - auxq[row]) - 0.5 * (double)D;
                if (METRIC == SV_DIST_COSINE) v = v / (auxq[row] * auxg[col]);
                const float f = (float)v;
                const bool inside = g0 + col < N;
                if (PAIR) {
                    if (inside && q0 + row < Q) out[(q0 + row) * ldo + g0 + col] = f;
                } else {
                    const int64_t gi = col0 + g0 + col;
                    const bool skip = !inside || (self0 >= 0 && gi == self0 + q0 + row);
                    tile[row * LDT + col] = skip ? INFINITY : (COS ? -f : f);
                }
            }
        if (PAIR) continue;
        __syncthreads();

        // merge: one wave per query row, lane = the tile's column.  The candidates that beat the row's k-th entry are inserted one
        // by one, in column order, into the list held in registers (slot 64 j + lane); the list returns to LDS afterwards.
        for (int rr = 0; rr < RW; ++rr) {
            const int row = wave * RW + rr;
            if (q0 + row >= Q) continue;
            const float key = tile[row * LDT + lane];
            float tk = thr_key[row];
            int64_t ti = thr_idx[row];
            // key < +inf: a NaN, a +inf distance, an excluded or an out-of-range column never enters
            unsigned long long mask = __ballot(key < INFINITY && kn_before(key, col0 + g0 + lane, tk, ti));
            if (!mask) continue;
            float lk[4];
            int64_t li[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 64 * j + lane;
                const bool has = j < J && s < k;
                lk[j] = has ? lkey[row * k + s] : INFINITY;
                li[j] = has ? lidx[row * k + s] : KN_NOIDX;
            }
            while (mask) {
                const int c = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const float ck = __shfl(key, c);
                const int64_t ci = col0 + g0 + c;
                if (!kn_before(ck, ci, tk, ti)) continue;              // (the threshold tightens with every insertion)
                int pos = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < J) pos += __popcll(__ballot(kn_before(lk[j], li[j], ck, ci)));
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    if (j >= J) continue;
                    const int s = 64 * j + lane;
                    float pk = __shfl_up(lk[j], 1);
                    int64_t pi = __shfl_up(li[j], 1);
                    if (j > 0) {                                       // lane 0 takes the last slot of the row below (still unshifted)
                        const float wk = __shfl(lk[j - 1], 63);
                        const int64_t wi = __shfl(li[j - 1], 63);
                        if (lane == 0) { pk = wk; pi = wi; }
                    }
                    if (s == pos) { lk[j] = ck; li[j] = ci; }
                    else if (s > pos) { lk[j] = pk; li[j] = pi; }
                    if (s >= k) { lk[j] = INFINITY; li[j] = KN_NOIDX; }
                }
                const float sk = kj == 0 ? lk[0] : kj == 1 ? lk[1] : kj == 2 ? lk[2] : lk[3];
                const int64_t si = kj == 0 ? li[0] : kj == 1 ? li[1] : kj == 2 ? li[2] : li[3];
                tk = __shfl(sk, kl);
                ti = __shfl(si, kl);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = 64 * j + lane;
                if (j < J && s < k) { lkey[row * k + s] = lk[j]; lidx[row * k + s] = li[j]; }
            }
            if (lane == 0) { thr_key[row] = tk; thr_idx[row] = ti; }
        }
    }

    if (!PAIR) {
        // every list is read and written by its own wave alone: no barrier between the last merge and the write-out
        for (int rr = 0; rr < RW; ++rr) {
            const int row = wave * RW + rr;
            if (q0 + row >= Q) continue;
            for (int s = lane; s < k; s += 64) {
                const int64_t gi = lidx[row * k + s];
                const float key = lkey[row * k + s];
                const bool empty = gi == KN_NOIDX;
                best_idx[(q0 + row) * k + s] = empty ? -1 : gi;
                best_val[(q0 + row) * k + s] = empty ? (COS ? -INFINITY : INFINITY) : (COS ? -key : key);
            }
        }
    }
}

template <int MQ, bool PAIR>
static void knn_launch(int metric, int grid, size_t lds, hipStream_t s, const float* q_mu, const float* q_ls, int Q, const float* g_mu,
                       const float* g_ls, int N, int D, int64_t col0, int64_t self0, int k, float* best_val, int64_t* best_idx, int init,
                       float* out, int64_t ldo) {
#define KN_GO(M)                                                                                                              \
    hipLaunchKernelGGL((knn_kernel<M, MQ, PAIR>), dim3(grid), dim3(KN_THREADS), lds, s, q_mu, q_ls, Q, g_mu, g_ls, N, D, col0, \
                       self0, k, best_val, best_idx, init, out, ldo)
    switch (metric) {
        case SV_DIST_KL: KN_GO(SV_DIST_KL); break;
        case SV_DIST_W2: KN_GO(SV_DIST_W2); break;
        case SV_DIST_EUCLID: KN_GO(SV_DIST_EUCLID); break;
        default: KN_GO(SV_DIST_COSINE); break;
    }
#undef KN_GO
}

static bool kn_reads_ls(int metric) { return metric == SV_DIST_KL || metric == SV_DIST_W2; }

int sv_pairdist(int metric, const float* q_mu, const float* q_ls, int Q, const float* g_mu, const float* g_ls, int N, int D, float* out,
                int64_t ldo, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(metric >= SV_DIST_KL && metric <= SV_DIST_COSINE, SV_E_ARG, "sv_pairdist: bad metric %d", metric);
    SV_REQUIRE(q_mu && g_mu, SV_E_ARG, "sv_pairdist: q_mu or g_mu is NULL");
    SV_REQUIRE(!kn_reads_ls(metric) || (q_ls && g_ls), SV_E_ARG, "sv_pairdist: metric %d reads ls: q_ls or g_ls is NULL", metric);
    SV_REQUIRE(out, SV_E_ARG, "sv_pairdist: out is NULL");
    SV_REQUIRE(Q > 0 && N > 0 && D > 0, SV_E_ARG, "sv_pairdist: non-positive size (Q=%d N=%d D=%d)", Q, N, D);
    SV_REQUIRE(ldo >= N, SV_E_SHAPE, "sv_pairdist: ldo=%lld < N=%d", (long long)ldo, N);
    knn_launch<4, true>(metric, (Q + 63) / 64, 0, (hipStream_t)stream, q_mu, q_ls, Q, g_mu, g_ls, N, D, 0, -1, 1, nullptr, nullptr, 0, out,
                        ldo);
    return sv_check_launch("sv_pairdist");
}

int sv_knn_scan(int metric, const float* q_mu, const float* q_ls, int Q, const float* g_mu, const float* g_ls, int N, int D, int64_t col0,
                int64_t self0, int k, float* best_val, int64_t* best_idx, int init, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(metric >= SV_DIST_KL && metric <= SV_DIST_COSINE, SV_E_ARG, "sv_knn_scan: bad metric %d", metric);
    SV_REQUIRE(q_mu && g_mu, SV_E_ARG, "sv_knn_scan: q_mu or g_mu is NULL");
    SV_REQUIRE(!kn_reads_ls(metric) || (q_ls && g_ls), SV_E_ARG, "sv_knn_scan: metric %d reads ls: q_ls or g_ls is NULL", metric);
    SV_REQUIRE(best_val && best_idx, SV_E_ARG, "sv_knn_scan: a list (best_val, best_idx) is NULL");
    SV_REQUIRE(k >= 1 && k <= KN_KMAX, SV_E_ARG, "sv_knn_scan: k=%d outside [1, %d]", k, KN_KMAX);
    SV_REQUIRE(Q > 0 && N > 0 && D > 0, SV_E_ARG, "sv_knn_scan: non-positive size (Q=%d N=%d D=%d)", Q, N, D);
    SV_REQUIRE(col0 >= 0 && self0 >= -1, SV_E_ARG, "sv_knn_scan: col0=%lld must be >= 0 and self0=%lld >= -1", (long long)col0,
               (long long)self0);
    SV_REQUIRE(col0 <= INT64_MAX - N - 64, SV_E_SHAPE, "sv_knn_scan: col0=%lld + N overflows the index", (long long)col0);
    // 64 query rows per block while their lists (12 bytes per slot) fit 48 KiB of LDS, 32 beyond -- the same arithmetic per pair either
    // way.  With the 19 KiB of static LDS a block may pass 64 KiB: the opt-in (gfx950 has 160 KiB per CU)
    static bool optin = false;
    if (const int rc = sv_lds_optin(optin, 32 * KN_KMAX * 12, "knn_scan", &knn_kernel<SV_DIST_KL, 4, false>, &knn_kernel<SV_DIST_W2, 4, false>,
                                    &knn_kernel<SV_DIST_EUCLID, 4, false>, &knn_kernel<SV_DIST_COSINE, 4, false>,
                                    &knn_kernel<SV_DIST_KL, 2, false>, &knn_kernel<SV_DIST_W2, 2, false>,
                                    &knn_kernel<SV_DIST_EUCLID, 2, false>, &knn_kernel<SV_DIST_COSINE, 2, false>))
        return rc;
    if (k <= 64)
        knn_launch<4, false>(metric, (Q + 63) / 64, (size_t)64 * k * 12, (hipStream_t)stream, q_mu, q_ls, Q, g_mu, g_ls, N, D, col0, self0, k,
                             best_val, best_idx, init, nullptr, 0);
    else
        knn_launch<2, false>(metric, (Q + 31) / 32, (size_t)32 * k * 12, (hipStream_t)stream, q_mu, q_ls, Q, g_mu, g_ls, N, D, col0, self0, k,
                             best_val, best_idx, init, nullptr, 0);
    return sv_check_launch("sv_knn_scan");
}

// ------------------------------------------------------------------------------------------ sv_knn_vote
// One wave per query, KV_WAVES queries per block.  Lane c sums the weights of the neighbours of class c, c + 64, ... in slot order
// (a fixed order; no float atomic); the counters follow smooth_classify_kernel: the block's rows meet in LDS and thread 0 issues at
// most one integer atomic per counter and touched confusion cell.
constexpr int KV_WAVES = 4;

__global__ __launch_bounds__(64 * KV_WAVES) void knn_vote_kernel(const float* best_val, const int64_t* best_idx, int Q, int k,
                                                                 const int64_t* g_label, int64_t n_gallery, int K, int mode, float tau,
                                                                 const int64_t* q_label, int64_t* pred, float* votes,
                                                                 unsigned long long* counts, unsigned long long* confusion) {
    __shared__ int nl[KV_WAVES][KN_KMAX];
    __shared__ float nw[KV_WAVES][KN_KMAX];
    __shared__ int hit[KV_WAVES];
    __shared__ int64_t cell[KV_WAVES];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * KV_WAVES + w;          // (the same for the whole wave)
    if (q < Q)
        for (int s = l; s < k; s += 64) {
            const int64_t gi = best_idx[q * k + s];
            int lab = -1;
            float wt = 0.f;
            if (gi >= 0 && gi < n_gallery) {
                const int64_t y = g_label[gi];
                if (y >= 0 && y < K) {
                    lab = (int)y;
                    wt = mode == 0 ? 1.f : expf((mode == 1 ? -best_val[q * k + s] : best_val[q * k + s]) / tau);
                }
            }
            nl[w][s] = lab;
            nw[w][s] = wt;
        }
    __syncthreads();
    int my_hit = 0;
    int64_t my_cell = -1;
    if (q < Q) {
        float abest = -INFINITY;
        int amax = 0x7fffffff, nvote = 0;
        for (int c = l; c < K; c += 64) {
            float v = 0.f;
            for (int s = 0; s < k; ++s)
                if (nl[w][s] == c) { v += nw[w][s]; ++nvote; }
            if (votes) votes[q * K + c] = v;
            if (v > abest) { abest = v; amax = c; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(abest, off);
            const int oi = __shfl_xor(amax, off);
            nvote += __shfl_xor(nvote, off);
            if (ov > abest || (ov == abest && oi < amax)) { abest = ov; amax = oi; }
        }
        const int p = (nvote > 0 && amax < K) ? amax : -1;
        if (l == 0) {
            if (pred) pred[q] = p;
            if (q_label) {
                const int64_t y = q_label[q];
                my_hit = p >= 0 && y == p;
                if (p >= 0 && y >= 0 && y < K) my_cell = y * K + p;
            }
        }
    }
    if (!counts && !confusion) return;                 // (kernel arguments: the whole block leaves)
    if (l == 0) {
        hit[w] = my_hit;
        cell[w] = my_cell;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (counts) {
        int h = 0;
        for (int r = 0; r < KV_WAVES; ++r) h += hit[r];
        if (h) atomicAdd(&counts[0], (unsigned long long)h);
        if (blockIdx.x == 0) atomicAdd(&counts[1], (unsigned long long)Q);
    }
    if (confusion)
        for (int r = 0; r < KV_WAVES; ++r) {
            const int64_t c = cell[r];
            bool first = c >= 0;
            for (int t = 0; t < r; ++t) first = first && cell[t] != c;
            if (!first) continue;                      // (no cell, or an earlier row of the block has added this one's share)
            int n = 1;
            for (int t = r + 1; t < KV_WAVES; ++t) n += cell[t] == c;
            atomicAdd(&confusion[c], (unsigned long long)n);
        }
}

int sv_knn_vote(const float* best_val, const int64_t* best_idx, int Q, int k, const int64_t* g_label, int64_t n_gallery, int K, int mode,
                float tau, const int64_t* q_label, int64_t* pred, float* votes, int64_t* counts, int64_t* confusion, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(best_idx && g_label, SV_E_ARG, "sv_knn_vote: best_idx or g_label is NULL");
    SV_REQUIRE(mode >= 0 && mode <= 2, SV_E_ARG, "sv_knn_vote: bad mode %d", mode);
    SV_REQUIRE(mode == 0 || best_val, SV_E_ARG, "sv_knn_vote: weighted votes (mode %d) need best_val", mode);
    SV_REQUIRE(mode == 0 || (tau > 0.f && tau <= 3.0e38f), SV_E_ARG, "sv_knn_vote: tau=%g must be finite and > 0", (double)tau);
    SV_REQUIRE(pred || votes || counts || confusion, SV_E_ARG, "sv_knn_vote: no output (pred, votes, counts and confusion are all NULL)");
    SV_REQUIRE(q_label || (!counts && !confusion), SV_E_ARG, "sv_knn_vote: counts / confusion need the labels");
    SV_REQUIRE(Q > 0 && K > 0 && n_gallery > 0, SV_E_ARG, "sv_knn_vote: non-positive size (Q=%d K=%d n_gallery=%lld)", Q, K,
               (long long)n_gallery);
    SV_REQUIRE(k >= 1 && k <= KN_KMAX, SV_E_ARG, "sv_knn_vote: k=%d outside [1, %d]", k, KN_KMAX);
    hipLaunchKernelGGL(knn_vote_kernel, dim3((Q + KV_WAVES - 1) / KV_WAVES), dim3(64 * KV_WAVES), 0, (hipStream_t)stream, best_val, best_idx,
                       Q, k, g_label, n_gallery, K, mode, tau, q_label, pred, votes, reinterpret_cast<unsigned long long*>(counts),
                       reinterpret_cast<unsigned long long*>(confusion));
    return sv_check_launch("sv_knn_vote");
}
