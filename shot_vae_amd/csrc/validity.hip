// Internal cluster validity in latent space: what the silhouette (Rousseeuw 1987), the Calinski-Harabasz index and the Davies-Bouldin
// index need from the device (declared, with the exact definitions, in include/shotvae_hip.h):
//   sv_sil_scan        part_a[p][i] = sum_j d(q_i, g_j) over the row's OWN cluster, part_b[p][i] = min over the other clusters c of
//                      (sum_j d(q_i, g_j)) / n_c -- over the clusters p, p + P, .. of a gallery that is grouped by cluster
//   sv_sil_finish      a, b and s = (b - a) / max(a, b) per row; the per-cluster sums of s in a fixed order
//   sv_cluster_spread  the squared distance of every row to its cluster's centroid; per cluster its sum and the sum of its roots
// ksum_scan_kernel's tile (64 queries x 64 gallery rows, 16 dimensions per staged chunk, the next chunk's global loads in flight while
// this one is multiplied) walked along a SEGMENT LIST: a tile never crosses a cluster, the first tile of a cluster starts at the
// cluster's first row, and the prefetch of "the next tile" follows the list.  The pair value is sv_pairdist's SV_DIST_EUCLID value
// bit for bit (ksum_scan_kernel's operations, one for one).  The state is a double sum per (row, cluster) in registers; at the end of
// a segment the 16 shares of a row meet in kn_aux_reduce's butterfly and the total becomes the row's own sum or enters its running
// minimum.  A block WRITES its slots: no atomic of any kind, no workspace, and which pairs meet in which order is a function of the
// arguments alone.  Plain HIP C++; every entry point takes a stream and allocates nothing: capturable.
#include "common.h"
#include <math.h>

constexpr int SIL_PMAX = 64;          // partial states
constexpr int SIL_KMAX = 1024;        // clusters (KMeans' limit)

__device__ __forceinline__ int64_t sil_clip(int64_t v, int64_t N) { return v < 0 ? 0 : v > N ? N : v; }

// a tile of the walk: rows [t0, min(t0 + 64, e)) of cluster c = rows [s, e) of the gallery (clipped); c >= K: the walk is over
struct SilTile {
    int c;
    int64_t s, e, t0;
};
// the first tile of the first non-empty cluster among c, c + P, ..
__device__ __forceinline__ SilTile sil_cluster(const int64_t* __restrict__ seg, int c, int K, int P, int64_t N) {
    for (; c < K; c += P) {
        const int64_t s = sil_clip(seg[c], N), e = sil_clip(seg[c + 1], N);
        if (e > s) return SilTile{c, s, e, s};
    }
    return SilTile{K, 0, 0, 0};
}
__device__ __forceinline__ SilTile sil_next(const int64_t* __restrict__ seg, const SilTile& t, int K, int P, int64_t N) {
    if (t.t0 + KN_TG < t.e) return SilTile{t.c, t.s, t.e, t.t0 + KN_TG};
    return sil_cluster(seg, t.c + P, K, P, N);
}
// the smaller of two values; a NaN on either side stays
__device__ __forceinline__ double sil_min(double m, double v) { return (v < m || v != v) ? v : m; }

// Block (x, p): query tile x, the clusters p, p + P, .. < K in increasing order.  Thread (ty, tx) owns rows 4 ty .., columns 4 tx ..
// of every tile.  A row beyond Q and a column at or beyond the segment's end are left out by predicate (kn_load stages them as 0).
template <int METRIC>
__global__ __launch_bounds__(KN_THREADS, 2) void sil_scan_kernel(const float* __restrict__ q, const int64_t* __restrict__ q_label, int Q,
                                                                 const float* __restrict__ g, const int64_t* __restrict__ seg, int N, int K,
                                                                 int D, int P, double* __restrict__ part_a, double* __restrict__ part_b) {
#pragma clang fp contract(off)
    constexpr int MQ = 4, TQ = 16 * MQ, LDQ = TQ + 4, LDG = KN_TG + 4;
    constexpr int ST = SV_DIST_EUCLID;                 // the staging role: one operand array, zeros beyond the end
    __shared__ __attribute__((aligned(16))) float sm[KN_DC * (LDQ + LDG)];
    float* Aq = sm;
    float* Ag = Aq + KN_DC * LDQ;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, p = blockIdx.y;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;

    double sum[MQ], own[MQ], other[MQ];
    int64_t lab[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        const int64_t row = q0 + MQ * ty + m;
        sum[m] = 0.0;
        own[m] = 0.0;
        other[m] = INFINITY;
        lab[m] = row < Q ? q_label[row] : -1;
    }

    SilTile cur = sil_cluster(seg, p, K, P, N);
    float pq[MQ], pg[4], unused[4];
    kn_load<ST, TQ>(q, nullptr, q0, Q, 0, D, pq, unused);
    kn_load<ST, KN_TG>(g, nullptr, cur.t0, cur.e, 0, D, pg, unused);
    while (cur.c < K) {
        const SilTile nxt = sil_next(seg, cur, K, P, N);
        double acc[MQ][4];
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = 0.0;

        for (int d0 = 0; d0 < D; d0 += KN_DC) {
            __syncthreads();                           // the previous chunk's products are read
            kn_store<ST, TQ, false>(pq, unused, q0, Q, d0, D, Aq, nullptr, nullptr);
            kn_store<ST, KN_TG, true>(pg, unused, cur.t0, cur.e, d0, D, Ag, nullptr, nullptr);
            __syncthreads();
            {                                          // the next chunk: of this tile, or the first of the list's next tile (none: zeros)
                const bool last = d0 + KN_DC >= D;
                const int nd0 = last ? 0 : d0 + KN_DC;
                kn_load<ST, TQ>(q, nullptr, q0, Q, nd0, D, pq, unused);
                kn_load<ST, KN_TG>(g, nullptr, last ? nxt.t0 : cur.t0, last ? nxt.e : cur.e, nd0, D, pg, unused);
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
                        // knn_kernel's operations, one for one: the value of a pair is sv_pairdist's
                        const float dm = qa[m] - ga[n];
                        part4[m][n] = fmaf(dm, dm, part4[m][n]);
                    }
            }
#pragma unroll
            for (int m = 0; m < MQ; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] += (double)part4[m][n];
        }

        // the 16 pair values in fp32, their root where the metric takes it, added in column order into the row's sum over this cluster
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                float v = (float)acc[m][n];
                if (METRIC == SV_SIL_EUCLID) v = sqrtf(v);
                const bool in = q0 + MQ * ty + m < Q && cur.t0 + 4 * tx + n < cur.e;
                if (in) sum[m] = sum[m] + (double)v;
            }

        if (nxt.c != cur.c) {                          // (uniform) the segment is complete: the shares meet, the sum finds its place
            const double n_c = (double)(cur.e - cur.s);
#pragma unroll
            for (int m = 0; m < MQ; ++m) {
                const double t = kn_aux_reduce(sum[m]);
                if (lab[m] == cur.c) {
                    own[m] = t;
                } else {
                    const double mean = t / n_c;
                    other[m] = sil_min(other[m], mean);
                }
                sum[m] = 0.0;
            }
        }
        cur = nxt;
    }

#pragma unroll
    for (int m = 0; m < MQ; ++m) {
        const int64_t row = q0 + MQ * ty + m;
        if (tx == 0 && row < Q) {
            part_a[(int64_t)p * Q + row] = own[m];
            part_b[(int64_t)p * Q + row] = other[m];
        }
    }
}

int sv_sil_scan(int metric, const float* q, const int64_t* q_label, int Q, const float* g, const int64_t* seg, int N, int K, int D, int P,
                double* part_a, double* part_b, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(metric == SV_SIL_EUCLID || metric == SV_SIL_SQEUCLID, SV_E_ARG, "sv_sil_scan: bad metric %d", metric);
    SV_REQUIRE(q && q_label && g && seg, SV_E_ARG, "sv_sil_scan: q, q_label, g or seg is NULL");
    SV_REQUIRE(part_a && part_b, SV_E_ARG, "sv_sil_scan: part_a or part_b is NULL");
    SV_REQUIRE(Q > 0 && N > 0 && D > 0, SV_E_ARG, "sv_sil_scan: non-positive size (Q=%d N=%d D=%d)", Q, N, D);
    SV_REQUIRE(K >= 1 && K <= SIL_KMAX, SV_E_ARG, "sv_sil_scan: K=%d outside [1, %d]", K, SIL_KMAX);
    SV_REQUIRE(P >= 1 && P <= SIL_PMAX, SV_E_ARG, "sv_sil_scan: P=%d outside [1, %d]", P, SIL_PMAX);
    const dim3 grid((Q + 63) / 64, P);
    if (metric == SV_SIL_EUCLID)
        hipLaunchKernelGGL(sil_scan_kernel<SV_SIL_EUCLID>, grid, dim3(KN_THREADS), 0, (hipStream_t)stream, q, q_label, Q, g, seg, N, K, D, P,
                           part_a, part_b);
    else
        hipLaunchKernelGGL(sil_scan_kernel<SV_SIL_SQEUCLID>, grid, dim3(KN_THREADS), 0, (hipStream_t)stream, q, q_label, Q, g, seg, N, K, D,
                           P, part_a, part_b);
    return sv_check_launch("sv_sil_scan");
}

// ------------------------------------------------------------------------------------------ sv_sil_finish
// one thread per row: the partial states in the order of p, then the row's a, b and s
__global__ __launch_bounds__(256) void sil_rows_kernel(const double* __restrict__ part_a, const double* __restrict__ part_b, int P, int64_t Q,
                                                       const int64_t* __restrict__ q_label, const int64_t* __restrict__ seg, int K, int64_t N,
                                                       double* __restrict__ s, double* __restrict__ a, double* __restrict__ b) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    double ta = part_a[i], tb = part_b[i];
    for (int p = 1; p < P; ++p) {
        ta = ta + part_a[(int64_t)p * Q + i];
        tb = sil_min(tb, part_b[(int64_t)p * Q + i]);
    }
    const int64_t lab = q_label[i];
    const bool known = lab >= 0 && lab < K;
    const int64_t n_own = known ? sil_clip(seg[lab + 1], N) - sil_clip(seg[lab], N) : 0;
    double av = NAN, sv = NAN;
    if (n_own > 1) av = ta / (double)(n_own - 1);
    if (n_own == 1) av = 0.0;
    // NaN first (an unknown label, an empty own cluster, no other cluster: b = +inf, a NaN anywhere), then the singleton, then 0 / 0
    if (n_own >= 1 && av == av && tb == tb && tb < INFINITY) {
        const double hi = av > tb ? av : tb;
        if (n_own == 1 || hi == 0.0) {
            sv = 0.0;
        } else {
            const double diff = tb - av;
            sv = diff / hi;
        }
    }
    s[i] = sv;
    if (a) a[i] = av;
    if (b) b[i] = tb;
}

// one block per cluster, ksum_total_kernel's merge order: thread t takes the rows t, t + 256, .. whose label is the cluster and whose s
// is no NaN, in order, then the 256 shares meet in a binary tree.  Block 0 also counts the rows whose s is NaN, whatever their label.
__global__ __launch_bounds__(256) void sil_cluster_kernel(const double* __restrict__ s, const int64_t* __restrict__ q_label, int64_t Q,
                                                          double* __restrict__ cluster_sum, int64_t* __restrict__ cluster_cnt,
                                                          int64_t* __restrict__ skipped) {
#pragma clang fp contract(off)
    __shared__ double sh[256];
    __shared__ int64_t sc[256];
    __shared__ int64_t sk[256];
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x;
    double t = 0.0;
    int64_t cnt = 0, nan = 0;
    for (int64_t i = tid; i < Q; i += 256) {
        const double v = s[i];
        if (v != v) {
            ++nan;
        } else if (q_label[i] == c) {
            t = t + v;
            ++cnt;
        }
    }
    sh[tid] = t;
    sc[tid] = cnt;
    sk[tid] = nan;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            sh[tid] = sh[tid] + sh[tid + h];
            sc[tid] += sc[tid + h];
            sk[tid] += sk[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        cluster_sum[c] = sh[0];
        cluster_cnt[c] = sc[0];
        if (c == 0) skipped[0] = sk[0];
    }
}

int sv_sil_finish(const double* part_a, const double* part_b, int P, int Q, const int64_t* q_label, const int64_t* seg, int K, int N,
                  double* s, double* a, double* b, double* cluster_sum, int64_t* cluster_cnt, int64_t* skipped, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(part_a && part_b, SV_E_ARG, "sv_sil_finish: part_a or part_b is NULL");
    SV_REQUIRE(q_label && seg && s, SV_E_ARG, "sv_sil_finish: q_label, seg or s is NULL");
    SV_REQUIRE((cluster_sum && cluster_cnt && skipped) || (!cluster_sum && !cluster_cnt && !skipped), SV_E_ARG,
               "sv_sil_finish: cluster_sum, cluster_cnt and skipped go together (all or none)");
    SV_REQUIRE(Q > 0 && N > 0, SV_E_ARG, "sv_sil_finish: non-positive size (Q=%d N=%d)", Q, N);
    SV_REQUIRE(K >= 1 && K <= SIL_KMAX, SV_E_ARG, "sv_sil_finish: K=%d outside [1, %d]", K, SIL_KMAX);
    SV_REQUIRE(P >= 1 && P <= SIL_PMAX, SV_E_ARG, "sv_sil_finish: P=%d outside [1, %d]", P, SIL_PMAX);
    hipLaunchKernelGGL(sil_rows_kernel, dim3((unsigned)((Q - 1) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, part_a, part_b, P, (int64_t)Q,
                       q_label, seg, K, (int64_t)N, s, a, b);
    if (cluster_sum)
        hipLaunchKernelGGL(sil_cluster_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, s, q_label, (int64_t)Q, cluster_sum,
                           cluster_cnt, skipped);
    return sv_check_launch("sv_sil_finish");
}

// ------------------------------------------------------------------------------------------ sv_cluster_spread
// sv_pairdist's SV_DIST_EUCLID value of the pair (row, centroid): 16 dimensions in fp32 with fmaf in index order from 0, the 16-blocks
// added in double in index order, rounded once to fp32
__device__ __forceinline__ float spread_d2(const float* __restrict__ x, const float* __restrict__ c, int D) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int d0 = 0; d0 < D; d0 += KN_DC) {
        float part = 0.f;
        const int d1 = d0 + KN_DC < D ? d0 + KN_DC : D;
        for (int d = d0; d < d1; ++d) {
            const float dm = x[d] - c[d];
            part = fmaf(dm, dm, part);
        }
        acc += (double)part;
    }
    return (float)acc;
}

__global__ __launch_bounds__(256) void spread_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ label, int64_t N, int D,
                                                          const float* __restrict__ c, int K, float* __restrict__ d2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int64_t k = label[i];
    d2[i] = (k >= 0 && k < K) ? spread_d2(x + i * D, c + k * D, D) : NAN;
}

// one block per cluster, sil_cluster_kernel's merge order over the rows of the cluster; every thread forms the distances of its rows
// itself (spread_rows_kernel's bits: the same operations)
__global__ __launch_bounds__(256) void spread_cluster_kernel(const float* __restrict__ x, const int64_t* __restrict__ label, int64_t N, int D,
                                                             const float* __restrict__ c, double* __restrict__ stat,
                                                             int64_t* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ double s2[256];
    __shared__ double s1[256];
    __shared__ int64_t sc[256];
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    double t2 = 0.0, t1 = 0.0;
    int64_t n = 0;
    for (int64_t i = tid; i < N; i += 256) {
        if (label[i] != k) continue;
        const float v = spread_d2(x + i * D, c + k * D, D);
        const float r = sqrtf(v);
        t2 = t2 + (double)v;
        t1 = t1 + (double)r;
        ++n;
    }
    s2[tid] = t2;
    s1[tid] = t1;
    sc[tid] = n;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s2[tid] = s2[tid] + s2[tid + h];
            s1[tid] = s1[tid] + s1[tid + h];
            sc[tid] += sc[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        stat[2 * k] = s2[0];
        stat[2 * k + 1] = s1[0];
        cnt[k] = sc[0];
    }
}

int sv_cluster_spread(const float* x, const int64_t* label, int N, int D, const float* c, int K, float* d2, double* stat, int64_t* cnt,
                      void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(x && label && c, SV_E_ARG, "sv_cluster_spread: x, label or c is NULL");
    SV_REQUIRE((stat && cnt) || (!stat && !cnt), SV_E_ARG, "sv_cluster_spread: stat and cnt go together (both or none)");
    SV_REQUIRE(d2 || stat, SV_E_ARG, "sv_cluster_spread: no output (d2, stat and cnt are NULL)");
    SV_REQUIRE(N > 0 && D > 0, SV_E_ARG, "sv_cluster_spread: non-positive size (N=%d D=%d)", N, D);
    SV_REQUIRE(K >= 1 && K <= SIL_KMAX, SV_E_ARG, "sv_cluster_spread: K=%d outside [1, %d]", K, SIL_KMAX);
    if (d2)
        hipLaunchKernelGGL(spread_rows_kernel, dim3((unsigned)((N - 1) / 256 + 1)), dim3(256), 0, (hipStream_t)stream, x, label, (int64_t)N, D, c,
                           K, d2);
    if (stat)
        hipLaunchKernelGGL(spread_cluster_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, x, label, (int64_t)N, D, c, stat, cnt);
    return sv_check_launch("sv_cluster_spread");
}
