// Latent-space clustering: one Lloyd iteration of k-means in three launches, and the contingency table of two label vectors (declared,
// with the exact definitions, in include/shotvae_hip.h):
//   sv_kmeans_assign   the nearest centroid of every row -- knn.hip's tiles with a running (value, index) minimum per row where the
//                      neighbour lists are; the [N][K] matrix never leaves the chip
//   sv_kmeans_accum    per-cluster sums, counts and the inertia into P partial states (aggpost.hip's rule: tile t to state t mod P)
//   sv_kmeans_finish   merges the states, divides, keeps the centroid of an empty cluster, and measures the shift
//   sv_contingency     table[a][b] += 1 under sv_knn_vote's counting rules
// Plain HIP C++, fp32 VALU; each takes a stream and allocates nothing: capturable.  A pair's distance is sv_pairdist's ONE sequence of
// operations; every floating-point sum is taken in a fixed order that depends only on the call's arguments; the only atomics are the
// integer ones of the table.  A repeated call sequence gives the same bits.
#include "common.h"
#include <math.h>

constexpr int KM_KMAX = 1024;         // sv_kmeans_accum: [K][slice] doubles of LDS
constexpr int KM_PMAX = 64;
constexpr int KM_LDS = 128 * 1024;    // the accumulators of one block (gfx950: 160 KiB per workgroup)
constexpr int64_t KM_NOIDX = INT64_MAX;

__device__ __forceinline__ bool km_before(float ka, int64_t ia, float kb, int64_t ib) { return ka < kb || (ka == kb && ia < ib); }

// ------------------------------------------------------------------------------------------ sv_kmeans_assign
// knn_kernel<SV_DIST_EUCLID, 4, true>'s tile: 64 rows x 64 centroids, 16 dimensions per staged chunk, the next chunk's global loads in
// flight while this one is multiplied.  Thread (ty, tx) keeps the minimum of its rows 4 ty .. over its columns 4 tx .. of every tile;
// the 16 minima of a row meet in a butterfly under the strict order (value, index).
__global__ __launch_bounds__(KN_THREADS, 2) void kmeans_assign_kernel(const float* __restrict__ x, int N, const float* __restrict__ c, int K,
                                                                      int D, int64_t* assign, float* dist) {
    constexpr int MQ = 4, TQ = 16 * MQ, LDQ = TQ + 4, LDG = KN_TG + 4;
    __shared__ __attribute__((aligned(16))) float sm[KN_DC * (LDQ + LDG)];
    float* Aq = sm;
    float* Ag = Aq + KN_DC * LDQ;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;

    float bv[MQ];
    int64_t bi[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) { bv[m] = INFINITY; bi[m] = KM_NOIDX; }

    float pq[MQ], pg[4], none[4];                      // the chunk in flight; (none: the ls operand the Euclid metric never reads)
    kn_load<SV_DIST_EUCLID, TQ>(x, nullptr, q0, N, 0, D, pq, none);
    kn_load<SV_DIST_EUCLID, KN_TG>(c, nullptr, 0, K, 0, D, pg, none);
    for (int64_t g0 = 0; g0 < K; g0 += KN_TG) {
        double acc[MQ][4];
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;

        for (int d0 = 0; d0 < D; d0 += KN_DC) {
            __syncthreads();                           // the previous chunk's products are read
            kn_store<SV_DIST_EUCLID, TQ, false>(pq, none, q0, N, d0, D, Aq, nullptr, nullptr);
            kn_store<SV_DIST_EUCLID, KN_TG, true>(pg, none, g0, K, d0, D, Ag, nullptr, nullptr);
            __syncthreads();
            {                                          // the next chunk: of this tile, or the first of the next (beyond the end: zeros)
                const bool last = d0 + KN_DC >= D;
                const int nd0 = last ? 0 : d0 + KN_DC;
                kn_load<SV_DIST_EUCLID, TQ>(x, nullptr, q0, N, nd0, D, pq, none);
                kn_load<SV_DIST_EUCLID, KN_TG>(c, nullptr, last ? g0 + KN_TG : g0, K, nd0, D, pg, none);
            }
            float part[MQ][4];
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) part[m][n] = 0.f;
#pragma unroll 4
            for (int dd = 0; dd < KN_DC; ++dd) {
                const f32x4 ga = *reinterpret_cast<const f32x4*>(&Ag[dd * LDG + 4 * tx]);
                float qa[MQ];
#pragma unroll
                for (int m = 0; m < MQ; ++m) qa[m] = Aq[dd * LDQ + MQ * ty + m];
#pragma unroll
                for (int m = 0; m < MQ; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const float dm = qa[m] - ga[n];
                        part[m][n] = fmaf(dm, dm, part[m][n]);         // sv_pairdist's SV_DIST_EUCLID term: the same roundings
                    }
            }
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += (double)part[m][n];
        }
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int64_t col = g0 + 4 * tx + n;
                const float f = (float)acc[m][n];
                // f < +inf: a NaN or an infinite value never becomes the minimum
                if (col < K && f < INFINITY && km_before(f, col, bv[m], bi[m])) { bv[m] = f; bi[m] = col; }
            }
    }

#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        float v = bv[m];
        int64_t i = bi[m];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const float ov = __shfl_xor(v, off);
            const int64_t oi = __shfl_xor(i, off);
            if (km_before(ov, oi, v, i)) { v = ov; i = oi; }
        }
        const int64_t row = q0 + MQ * ty + m;
        if (tx == 0 && row < N) {
            assign[row] = i == KM_NOIDX ? -1 : i;
            if (dist) dist[row] = v;                   // (+inf where no value was finite)
        }
    }
}

int sv_kmeans_assign(const float* x, int N, const float* c, int K, int D, int64_t* assign, float* dist, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && c, SV_E_ARG, "sv_kmeans_assign: x or c is NULL");
    SV_REQUIRE(assign, SV_E_ARG, "sv_kmeans_assign: assign is NULL");
    SV_REQUIRE(N > 0 && K > 0 && D > 0, SV_E_ARG, "sv_kmeans_assign: non-positive size (N=%d K=%d D=%d)", N, K, D);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((N - 1) / 64 + 1), dim3(KN_THREADS), 0, (hipStream_t)stream, x, N, c, K, D, assign, dist);
    return sv_check_launch("sv_kmeans_assign");
}

// ------------------------------------------------------------------------------------------ sv_kmeans_accum
// One wave per block.  Block (s, p), s < the number of slices: the wave owns dimensions s S .. s S + S - 1 (lane = dimension) of partial
// state p, holds its [K][S] double accumulators in LDS, and walks the tiles p, p + P, ... of the call row by row: every accumulator is
// touched by one lane only, in row order -- no atomic, no reduction tree.  The next tile's 64 loads are in flight while a tile is added, and
// four rows of four different clusters are added side by side (their accumulators are disjoint: the order per accumulator stands).  Block
// (number of slices, p) counts the rows per cluster (one LDS add per distinct cluster of a tile, by lane 0) and adds the distances of
// the state's rows in index order.  S = 64 while [K][64] doubles fit KM_LDS (K <= 256), then 32 (K <= 512), then 16.
// the 64 rows of tile t in this lane's dimension, and (lane = row) the tile's assignments: -1 for a row that is skipped (outside
// [0, K)) or beyond the end.  Every load is unconditional: a row beyond the end reads row N - 1 and a lane beyond D column D - 1 (in
// bounds; the value is never added: its assignment is -1, its lane inactive)
__device__ __forceinline__ int km_load_tile(const float* __restrict__ x, const int64_t* __restrict__ assign, int64_t t, int N, int D, int K,
                                            int d, float* v) {
    const int64_t r0 = t * 64, last = (int64_t)N - 1;
    const int64_t a = r0 + threadIdx.x <= last ? assign[r0 + threadIdx.x] : -1;
    const int dc = d < D ? d : D - 1;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const int64_t r = r0 + j <= last ? r0 + j : last;
        v[j] = x[r * D + dc];
    }
    return (a >= 0 && a < K) ? (int)a : -1;
}

__global__ __launch_bounds__(64) void kmeans_accum_kernel(const float* __restrict__ x, const int64_t* __restrict__ assign,
                                                          const float* __restrict__ dist, int N, int D, int K, int lgS, double* sums,
                                                          int64_t* counts, double* inertia, int P, int init) {
    extern __shared__ __attribute__((aligned(16))) double km_acc[];
    const int lane = threadIdx.x, p = blockIdx.y, S = 1 << lgS, nslice = gridDim.x - 1;
    const int64_t ntiles = ((int64_t)N + 63) / 64;
    if ((int)blockIdx.x < nslice) {
        const int d = blockIdx.x * S + lane;
        const bool active = lane < S && d < D;
        for (int i = lane; i < K * S; i += 64) {
            const int gd = blockIdx.x * S + (i & (S - 1));
            km_acc[i] = (!init && gd < D) ? sums[((int64_t)p * K + (i >> lgS)) * D + gd] : 0.0;
        }
        __syncthreads();
        float cur[64], nxt[64];
        int ka = km_load_tile(x, assign, p, N, D, K, d, cur);
        for (int64_t t = p; t < ntiles; t += P) {
            const int kn = km_load_tile(x, assign, t + P, N, D, K, d, nxt);          // in flight while this tile is added
#pragma unroll
            for (int j = 0; j < 64; j += 4) {
                const int k0 = __shfl(ka, j), k1 = __shfl(ka, j + 1), k2 = __shfl(ka, j + 2), k3 = __shfl(ka, j + 3);      // (uniform)
                if (!active) continue;
                double* const a0 = &km_acc[((k0 < 0 ? 0 : k0) << lgS) + lane];
                double* const a1 = &km_acc[((k1 < 0 ? 0 : k1) << lgS) + lane];
                double* const a2 = &km_acc[((k2 < 0 ? 0 : k2) << lgS) + lane];
                double* const a3 = &km_acc[((k3 < 0 ? 0 : k3) << lgS) + lane];
                const bool apart = (k0 < 0 || (k0 != k1 && k0 != k2 && k0 != k3)) && (k1 < 0 || (k1 != k2 && k1 != k3)) && (k2 < 0 || k2 != k3);
                if (apart) {                           // four different accumulators: the four read-add-write chains overlap
                    const double s0 = *a0, s1 = *a1, s2 = *a2, s3 = *a3;
                    if (k0 >= 0) *a0 = s0 + (double)cur[j];
                    if (k1 >= 0) *a1 = s1 + (double)cur[j + 1];
                    if (k2 >= 0) *a2 = s2 + (double)cur[j + 2];
                    if (k3 >= 0) *a3 = s3 + (double)cur[j + 3];
                } else {                               // a cluster repeats: one after the other, in row order
                    if (k0 >= 0) *a0 += (double)cur[j];
                    if (k1 >= 0) *a1 += (double)cur[j + 1];
                    if (k2 >= 0) *a2 += (double)cur[j + 2];
                    if (k3 >= 0) *a3 += (double)cur[j + 3];
                }
            }
#pragma unroll
            for (int j = 0; j < 64; ++j) cur[j] = nxt[j];
            ka = kn;
        }
        __syncthreads();
        for (int i = lane; i < K * S; i += 64) {
            const int gd = blockIdx.x * S + (i & (S - 1));
            if (gd < D) sums[((int64_t)p * K + (i >> lgS)) * D + gd] = km_acc[i];
        }
        return;
    }
    int64_t* cnt = reinterpret_cast<int64_t*>(km_acc);
    for (int k = lane; k < K; k += 64) cnt[k] = init ? 0 : counts[(int64_t)p * K + k];
    double in = (inertia && !init) ? inertia[p] : 0.0;
    __syncthreads();
    for (int64_t t = p; t < ntiles; t += P) {
        const int64_t row = t * 64 + lane;
        const int64_t a = row < N ? assign[row] : -1;
        const int ka = (a >= 0 && a < K) ? (int)a : -1;
        unsigned long long todo = __ballot(ka >= 0);
        while (todo) {                                 // (uniform: one turn per distinct cluster of the tile)
            const int kv = __shfl(ka, __ffsll((long long)todo) - 1);
            const unsigned long long same = __ballot(ka == kv);
            if (lane == 0) cnt[kv] += __popcll(same);
            todo &= ~same;
        }
        if (inertia) {
            const float dv = ka >= 0 ? dist[row] : 0.f;
            for (int j = 0; j < 64; ++j) {             // every lane forms the same sum, in row order
                const float r = __shfl(dv, j);
                const int kj = __shfl(ka, j);
                if (kj >= 0) in += (double)r;
            }
        }
    }
    __syncthreads();
    for (int k = lane; k < K; k += 64) counts[(int64_t)p * K + k] = cnt[k];
    if (inertia && lane == 0) inertia[p] = in;
}

static int km_slice_log2(int K) { return K <= KM_LDS / (64 * 8) ? 6 : K <= KM_LDS / (32 * 8) ? 5 : 4; }

int sv_kmeans_accum(const float* x, const int64_t* assign, const float* dist, int N, int D, int K, double* sums, int64_t* counts,
                    double* inertia, int P, int init, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && assign, SV_E_ARG, "sv_kmeans_accum: x or assign is NULL");
    SV_REQUIRE(sums && counts, SV_E_ARG, "sv_kmeans_accum: a state (sums, counts) is NULL");
    SV_REQUIRE(!inertia || dist, SV_E_ARG, "sv_kmeans_accum: the inertia needs dist, which is NULL");
    SV_REQUIRE(N > 0 && D > 0 && K > 0, SV_E_ARG, "sv_kmeans_accum: non-positive size (N=%d D=%d K=%d)", N, D, K);
    SV_REQUIRE(K <= KM_KMAX, SV_E_ARG, "sv_kmeans_accum: K=%d outside [1, %d]", K, KM_KMAX);
    SV_REQUIRE(P >= 1 && P <= KM_PMAX, SV_E_ARG, "sv_kmeans_accum: P=%d outside [1, %d]", P, KM_PMAX);
    // above 64 KiB of LDS a block needs the opt-in (gfx950 has 160 KiB per CU)
    static bool optin = false;
    if (const int rc = sv_lds_optin(optin, KM_LDS, "kmeans_accum", &kmeans_accum_kernel)) return rc;
    const int lgS = km_slice_log2(K), S = 1 << lgS;
    hipLaunchKernelGGL(kmeans_accum_kernel, dim3((D + S - 1) / S + 1, P), dim3(64), (size_t)K * S * sizeof(double), (hipStream_t)stream, x,
                       assign, dist, N, D, K, lgS, sums, counts, inertia, P, init);
    return sv_check_launch("sv_kmeans_accum");
}

// ------------------------------------------------------------------------------------------ sv_kmeans_finish
// Two launches.  kmeans_merge_kernel, one block per cluster: 256 dimensions at a time, every thread merges the P sums of its dimension
// in index order and writes the centroid (it reads c_old[k][d] before it writes c_new[k][d]: the two may alias), the squared shifts
// meet in LDS and thread 0 adds them in index order.  The cluster's shift travels to the second launch in count[k] (the bits of a
// double in the int64 slot: the entry point allocates nothing).  kmeans_stats_kernel, one block: adds the K shifts in index order,
// replaces each by the merged count, and adds the P inertias.
__global__ __launch_bounds__(256) void kmeans_merge_kernel(const double* sums, const int64_t* counts, int P, int K, int D, const float* c_old,
                                                           float* c_new, int64_t* count) {
    __shared__ double sq[256];
    const int tid = threadIdx.x, k = blockIdx.x;
    int64_t n = 0;
    for (int p = 0; p < P; ++p) n += counts[(int64_t)p * K + k];
    double shift = 0.0;
    for (int d0 = 0; d0 < D; d0 += 256) {
        const int d = d0 + tid;
        double t = 0.0;
        if (d < D) {
            const float old = c_old[(int64_t)k * D + d];
            float now = old;                           // an empty cluster keeps its centroid
            if (n > 0) {
                double s = 0.0;
                for (int p = 0; p < P; ++p) s += sums[((int64_t)p * K + k) * D + d];
                now = (float)(s / (double)n);
            }
            c_new[(int64_t)k * D + d] = now;
            t = (double)now - (double)old;
        }
        sq[tid] = t * t;
        __syncthreads();
        if (tid == 0) {
            const int nd = D - d0 < 256 ? D - d0 : 256;
            for (int i = 0; i < nd; ++i) shift += sq[i];
        }
        __syncthreads();
    }
    if (tid == 0) count[k] = __double_as_longlong(shift);
}

__global__ __launch_bounds__(1024) void kmeans_stats_kernel(const int64_t* counts, const double* inertia, int P, int K, int64_t* count,
                                                            float* stats) {
    __shared__ double sh[1024];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int k0 = 0; k0 < K; k0 += 1024) {
        const int k = k0 + tid;
        if (k < K) {
            sh[tid] = __longlong_as_double(count[k]);
            int64_t n = 0;
            for (int p = 0; p < P; ++p) n += counts[(int64_t)p * K + k];
            count[k] = n;
        }
        __syncthreads();
        if (tid == 0) {
            const int nk = K - k0 < 1024 ? K - k0 : 1024;
            for (int i = 0; i < nk; ++i) total += sh[i];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double in = 0.0;
        if (inertia)
            for (int p = 0; p < P; ++p) in += inertia[p];
        stats[0] = (float)total;
        stats[1] = (float)in;
    }
}

int sv_kmeans_finish(const double* sums, const int64_t* counts, const double* inertia, int P, int K, int D, const float* c_old, float* c_new,
                     int64_t* count, float* stats, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(sums && counts, SV_E_ARG, "sv_kmeans_finish: a state (sums, counts) is NULL");
    SV_REQUIRE(c_old && c_new, SV_E_ARG, "sv_kmeans_finish: c_old or c_new is NULL");
    SV_REQUIRE(count && stats, SV_E_ARG, "sv_kmeans_finish: an output (count, stats) is NULL");
    SV_REQUIRE(K > 0 && D > 0, SV_E_ARG, "sv_kmeans_finish: non-positive size (K=%d D=%d)", K, D);
    SV_REQUIRE(P >= 1 && P <= KM_PMAX, SV_E_ARG, "sv_kmeans_finish: P=%d outside [1, %d]", P, KM_PMAX);
    hipLaunchKernelGGL(kmeans_merge_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, sums, counts, P, K, D, c_old, c_new, count);
    hipLaunchKernelGGL(kmeans_stats_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, counts, inertia, P, K, count, stats);
    return sv_check_launch("sv_kmeans_finish");
}

// ------------------------------------------------------------------------------------------ sv_contingency
// A block takes CT_ROWS rows and counts them privately in an LDS hash table of 2 CT_ROWS slots keyed by the cell a * Kb + b (open
// addressing, LDS integer atomics: at most CT_ROWS distinct cells, so a free slot always exists) -- the same code for a 2 x 2 and a
// 2^20-cell table.  At its end every used slot issues ONE integer atomic to its cell, thread 0 one to counts[0].
constexpr int CT_THREADS = 256, CT_ROWS = 8 * CT_THREADS, CT_SLOTS = 2 * CT_ROWS;
constexpr int64_t CT_CELLS = (int64_t)1 << 20;

__global__ __launch_bounds__(CT_THREADS) void contingency_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int N, int Ka,
                                                                 int Kb, unsigned long long* table, unsigned long long* counts) {
    __shared__ int key[CT_SLOTS];
    __shared__ int num[CT_SLOTS];
    __shared__ int valid;
    const int tid = threadIdx.x;
    for (int s = tid; s < CT_SLOTS; s += CT_THREADS) { key[s] = -1; num[s] = 0; }
    if (tid == 0) valid = 0;
    __syncthreads();
    const int64_t r0 = (int64_t)blockIdx.x * CT_ROWS;
    int mine = 0;
    for (int j = 0; j < CT_ROWS / CT_THREADS; ++j) {
        const int64_t r = r0 + j * CT_THREADS + tid;
        if (r >= N) break;
        const int64_t av = a[r], bv = b[r];
        if (av < 0 || av >= Ka || bv < 0 || bv >= Kb) continue;        // a row, never a cell
        const int cell = (int)(av * Kb + bv);
        int s = (int)(((unsigned)cell * 2654435761u) >> 20) & (CT_SLOTS - 1);
        for (;;) {
            const int seen = atomicCAS(&key[s], -1, cell);
            if (seen == -1 || seen == cell) break;
            s = (s + 1) & (CT_SLOTS - 1);
        }
        atomicAdd(&num[s], 1);
        ++mine;
    }
    if (mine) atomicAdd(&valid, mine);
    __syncthreads();
    for (int s = tid; s < CT_SLOTS; s += CT_THREADS)
        if (num[s]) atomicAdd(&table[key[s]], (unsigned long long)num[s]);
    if (tid == 0) {
        if (valid) atomicAdd(&counts[0], (unsigned long long)valid);
        if (blockIdx.x == 0) atomicAdd(&counts[1], (unsigned long long)N);
    }
}

int sv_contingency(const int64_t* a, const int64_t* b, int N, int Ka, int Kb, int64_t* table, int64_t* counts, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(a && b, SV_E_ARG, "sv_contingency: a label vector (a, b) is NULL");
    SV_REQUIRE(table && counts, SV_E_ARG, "sv_contingency: an output (table, counts) is NULL");
    SV_REQUIRE(N > 0 && Ka > 0 && Kb > 0, SV_E_ARG, "sv_contingency: non-positive size (N=%d Ka=%d Kb=%d)", N, Ka, Kb);
    SV_REQUIRE((int64_t)Ka * Kb <= CT_CELLS, SV_E_SHAPE, "sv_contingency: Ka * Kb = %lld exceeds 2^20 cells", (long long)Ka * Kb);
    hipLaunchKernelGGL(contingency_kernel, dim3((N - 1) / CT_ROWS + 1), dim3(CT_THREADS), 0, (hipStream_t)stream, a, b, N, Ka, Kb,
                       reinterpret_cast<unsigned long long*>(table), reinterpret_cast<unsigned long long*>(counts));
    return sv_check_launch("sv_contingency");
}
