// t-SNE of the latent space: the input affinities and one gradient-descent iteration in three entry points (declared, with the exact
// definitions, in include/shotvae_hip.h):
//   sv_tsne_affinity   the conditional affinities of every row's k-list: scikit-learn's bisection for beta, in double, one wave per row
//   sv_tsne_attract    the sparse attraction and the rows' share of the KL: a CSR gather, eight lanes per row, no scatter
//   sv_tsne_repulse    the exact all-pairs repulsion into P partial states (sv_kmeans_accum's rule: column tile t to state t mod P):
//                      one row per thread, the column tiles broadcast from LDS; the [N][N] matrix never exists
//   sv_tsne_update     merges the states in double, forms Z, the KL and |g|^2 in a fixed order, and applies gains, momentum and the step
// Plain HIP C++; each takes a stream and allocates nothing: capturable.  Every floating-point sum is taken in a fixed order that depends
// only on the call's arguments and there is no atomic of any kind: a repeated call sequence gives the same bits.
#include "common.h"
#include <math.h>

constexpr int TS_KMAX = 256;          // sv_tsne_affinity: four list slots per lane (sv_knn_scan's limit)
constexpr int TS_PMAX = 64;
constexpr int TS_ROWS = 256;          // sv_tsne_repulse: rows per block, one per thread
constexpr int TS_TILE = 64;           // columns per staged tile
constexpr int TS_LANES = 8;           // sv_tsne_attract: lanes per row

// w = 1 / a for a = 1 + r2 >= 1: the hardware reciprocal and one Newton step (two fmas).  Exact where 1 / a is a power of two.
__device__ __forceinline__ float ts_recip(float a) {
    const float w = __builtin_amdgcn_rcpf(a);
    return fmaf(w, fmaf(-a, w, 1.f), w);
}

// the sum of v over the 256 threads of the block: a binary tree in LDS, the same pairs whatever the values -> every thread
__device__ __forceinline__ double ts_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------ sv_tsne_affinity
// One wave per row; lane l holds the slots l, l + 64, l + 128, l + 192 of the row's list.  A sum over the row: every lane adds its slots
// in slot order, then the 64 lane sums meet in a butterfly (xor 32, 16, .., 1): a + b is commutative, so every lane holds the same bits
// and the search's branches are uniform.
__device__ __forceinline__ double ts_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void tsne_affinity_kernel(const float* __restrict__ dist, const int64_t* __restrict__ idx, int N, int k,
                                                            double target, double tol, int max_steps, float* __restrict__ p,
                                                            double* __restrict__ beta_out, int* __restrict__ steps_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;                              // (the whole wave: there is no block barrier below)
    const float* drow = dist + row * k;
    const int64_t* irow = idx + row * k;
    float* prow = p + row * k;

    double x[4];
    bool ok[4];
    float dmin = INFINITY;
    int mine = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int j = lane + 64 * s;
        float d = INFINITY;
        ok[s] = false;
        if (j < k) {
            d = drow[j];
            ok[s] = irow[j] >= 0 && fabsf(d) < INFINITY;           // (false for a NaN)
        }
        x[s] = (double)d;
        if (ok[s]) { dmin = fminf(dmin, d); ++mine; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        dmin = fminf(dmin, __shfl_xor(dmin, off));
        mine += __shfl_xor(mine, off);
    }
    const int nvalid = mine;
    if (nvalid < 2) {                                  // nothing to search: uniform over what the row has
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (lane + 64 * s < k) prow[lane + 64 * s] = ok[s] ? 1.f : 0.f;
        if (lane == 0) { beta_out[row] = 1.0; steps_out[row] = max_steps; }
        return;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = ok[s] ? x[s] - (double)dmin : 0.0;

    double beta = 1.0, lo = -INFINITY, hi = INFINITY, e[4], S = 1.0;
    int steps = max_steps;
    for (int it = 0; it < max_steps; ++it) {
        double s_e = 0.0, s_xe = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            // x == 0 is the closest slot: exp(0) whatever beta has become (0 x inf would be a NaN)
            e[s] = !ok[s] ? 0.0 : x[s] == 0.0 ? 1.0 : exp(-beta * x[s]);
            s_e += e[s];
            s_xe += x[s] * e[s];
        }
        S = ts_wave_sum(s_e);                          // >= 1: the closest slot
        const double T = ts_wave_sum(s_xe);
        const double H = log(S) + (T == 0.0 ? 0.0 : beta * (T / S));
        const double diff = H - target;
        if (fabs(diff) <= tol) { steps = it + 1; break; }
        if (it + 1 == max_steps) break;                // beta stays the value p is formed at
        if (diff > 0.0) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.0 : 0.5 * (beta + hi);
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5 : 0.5 * (beta + lo);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (lane + 64 * s < k) prow[lane + 64 * s] = (float)(e[s] / S);
    if (lane == 0) { beta_out[row] = beta; steps_out[row] = steps; }
}

int sv_tsne_affinity(const float* dist, const int64_t* idx, int N, int k, double perplexity, double tol, int max_steps, float* p,
                     double* beta, int* steps, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(dist && idx, SV_E_ARG, "sv_tsne_affinity: dist or idx is NULL");
    SV_REQUIRE(p && beta && steps, SV_E_ARG, "sv_tsne_affinity: an output (p, beta, steps) is NULL");
    SV_REQUIRE(N > 0, SV_E_ARG, "sv_tsne_affinity: non-positive size (N=%d)", N);
    SV_REQUIRE(k >= 1 && k <= TS_KMAX, SV_E_ARG, "sv_tsne_affinity: k=%d outside [1, %d]", k, TS_KMAX);
    SV_REQUIRE(perplexity > 1.0 && perplexity < (double)k, SV_E_ARG, "sv_tsne_affinity: perplexity=%g outside (1, k=%d)", perplexity, k);
    SV_REQUIRE(tol >= 0.0 && max_steps >= 1, SV_E_ARG, "sv_tsne_affinity: tol=%g < 0 or max_steps=%d < 1", tol, max_steps);
    hipLaunchKernelGGL(tsne_affinity_kernel, dim3((N - 1) / 4 + 1), dim3(256), 0, (hipStream_t)stream, dist, idx, N, k, log(perplexity), tol,
                       max_steps, p, beta, steps);
    return sv_check_launch("sv_tsne_affinity");
}

// ------------------------------------------------------------------------------------------ sv_tsne_attract
// Eight lanes per row: lane s of the row walks the entries s, s + 8, .. of its segment in order, each term formed in fp32 and added in
// double; the eight lane sums meet in a butterfly (xor 4, 2, 1) and are rounded once.  A row reads its own segment only.
template <int D>
__global__ __launch_bounds__(256) void tsne_attract_kernel(const float* __restrict__ y, int N, const int64_t* __restrict__ rowptr,
                                                           const int64_t* __restrict__ col, const float* __restrict__ val,
                                                           float* __restrict__ attr, float* __restrict__ rowkl) {
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / TS_LANES;
    const int s = threadIdx.x & (TS_LANES - 1);
    const bool live = row < N;
    double a[D], kl = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] = 0.0;
    if (live) {
        float yi[D];
#pragma unroll
        for (int c = 0; c < D; ++c) yi[c] = y[row * D + c];
        const int64_t end = rowptr[row + 1];
        for (int64_t q = rowptr[row] + s; q < end; q += TS_LANES) {
            const int64_t j = col[q];
            const float pv = val[q];
            if (j < 0 || j >= N) continue;             // (never read outside y)
            float df[D], r2 = 0.f;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                df[c] = yi[c] - y[j * D + c];
                r2 = fmaf(df[c], df[c], r2);
            }
            const float one = 1.f + r2;
            const float pw = pv * ts_recip(one);
#pragma unroll
            for (int c = 0; c < D; ++c) a[c] += (double)(pw * df[c]);
            if (pv > 0.f) kl += (double)(pv * logf(pv * one));
        }
    }
#pragma unroll
    for (int off = TS_LANES / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < D; ++c) a[c] += __shfl_xor(a[c], off);
        kl += __shfl_xor(kl, off);
    }
    if (live && s == 0) {
#pragma unroll
        for (int c = 0; c < D; ++c) attr[row * D + c] = (float)a[c];
        rowkl[row] = (float)kl;
    }
}

int sv_tsne_attract(const float* y, int N, int d, const int64_t* rowptr, const int64_t* col, const float* val, float* attr, float* rowkl,
                    void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(y && rowptr, SV_E_ARG, "sv_tsne_attract: y or rowptr is NULL");
    SV_REQUIRE(attr && rowkl, SV_E_ARG, "sv_tsne_attract: an output (attr, rowkl) is NULL");
    SV_REQUIRE(N > 0, SV_E_ARG, "sv_tsne_attract: non-positive size (N=%d)", N);
    SV_REQUIRE(d == 2 || d == 3, SV_E_SHAPE, "sv_tsne_attract: d=%d is neither 2 nor 3", d);
    const dim3 grid((unsigned)(((int64_t)N * TS_LANES - 1) / 256 + 1));
    if (d == 2)
        hipLaunchKernelGGL(tsne_attract_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, y, N, rowptr, col, val, attr, rowkl);
    else
        hipLaunchKernelGGL(tsne_attract_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, y, N, rowptr, col, val, attr, rowkl);
    return sv_check_launch("sv_tsne_attract");
}

// ------------------------------------------------------------------------------------------ sv_tsne_repulse
// Block (b, p): thread i owns row 256 b + i and walks the column tiles p, p + P, .. in order.  A tile's 64 points sit in LDS as float4
// (x, y, z or 0, 0): every lane reads the same address, a broadcast.  The next tile's global loads are in flight while this one is
// scanned, and the two LDS buffers alternate: one barrier per tile.  A tile that reaches beyond N or meets the block's own rows takes
// the masked form (w = 0 for a column >= N or == the row: by index, never by distance); every other tile the bare one.
template <int D, bool MASK>
__device__ __forceinline__ void ts_scan_tile(const float4* tile, const float* yi, int64_t row, int64_t c0, int N, float* acc, float& zs) {
#pragma unroll 8
    for (int j = 0; j < TS_TILE; ++j) {
        const float4 c = tile[j];
        float df[3];
        df[0] = yi[0] - c.x;
        df[1] = yi[1] - c.y;
        float r2 = fmaf(df[0], df[0], 0.f);
        r2 = fmaf(df[1], df[1], r2);
        if (D == 3) {
            df[2] = yi[2] - c.z;
            r2 = fmaf(df[2], df[2], r2);
        }
        float w = ts_recip(1.f + r2);
        if (MASK) w = (c0 + j < N && c0 + j != row) ? w : 0.f;
        zs += w;
        const float w2 = w * w;
#pragma unroll
        for (int q = 0; q < D; ++q) acc[q] = fmaf(w2, df[q], acc[q]);
    }
}

template <int D>
__global__ __launch_bounds__(TS_ROWS) void tsne_repulse_kernel(const float* __restrict__ y, int N, int P, float* __restrict__ rep,
                                                               float* __restrict__ z) {
    __shared__ float4 tile[2][TS_TILE];
    const int tid = threadIdx.x, p = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * TS_ROWS, row = r0 + tid;
    const int64_t ntiles = ((int64_t)N + TS_TILE - 1) / TS_TILE;
    float yi[3] = {0.f, 0.f, 0.f};
    if (row < N) {
#pragma unroll
        for (int c = 0; c < D; ++c) yi[c] = y[row * D + c];
    }
    float acc[3] = {0.f, 0.f, 0.f}, zs = 0.f;

    auto load = [&](int64_t t) {                       // lane = column of tile t; zeros beyond the end (masked anyway)
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int64_t c = t * TS_TILE + tid;
        if (tid < TS_TILE && c < N) {
            v.x = y[c * D];
            v.y = y[c * D + 1];
            if (D == 3) v.z = y[c * D + 2];
        }
        return v;
    };
    float4 nxt = load(p);
    if (tid < TS_TILE) tile[0][tid] = nxt;
    __syncthreads();
    int cur = 0;
    for (int64_t t = p; t < ntiles; t += P) {
        nxt = load(t + P);
        const int64_t c0 = t * TS_TILE;
        const bool mask = c0 + TS_TILE > N || (c0 < r0 + TS_ROWS && c0 + TS_TILE > r0);        // (uniform over the block)
        if (mask)
            ts_scan_tile<D, true>(tile[cur], yi, row, c0, N, acc, zs);
        else
            ts_scan_tile<D, false>(tile[cur], yi, row, c0, N, acc, zs);
        if (tid < TS_TILE) tile[cur ^ 1][tid] = nxt;   // (read last before the previous barrier)
        __syncthreads();
        cur ^= 1;
    }
    if (row < N) {
#pragma unroll
        for (int c = 0; c < D; ++c) rep[((int64_t)p * N + row) * D + c] = acc[c];
        z[(int64_t)p * N + row] = zs;
    }
}

int sv_tsne_repulse(const float* y, int N, int d, int P, float* rep, float* z, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(y, SV_E_ARG, "sv_tsne_repulse: y is NULL");
    SV_REQUIRE(rep && z, SV_E_ARG, "sv_tsne_repulse: an output (rep, z) is NULL");
    SV_REQUIRE(N > 0, SV_E_ARG, "sv_tsne_repulse: non-positive size (N=%d)", N);
    SV_REQUIRE(d == 2 || d == 3, SV_E_SHAPE, "sv_tsne_repulse: d=%d is neither 2 nor 3", d);
    SV_REQUIRE(P >= 1 && P <= TS_PMAX, SV_E_ARG, "sv_tsne_repulse: P=%d outside [1, %d]", P, TS_PMAX);
    const dim3 grid((N - 1) / TS_ROWS + 1, P);
    if (d == 2)
        hipLaunchKernelGGL(tsne_repulse_kernel<2>, grid, dim3(TS_ROWS), 0, (hipStream_t)stream, y, N, P, rep, z);
    else
        hipLaunchKernelGGL(tsne_repulse_kernel<3>, grid, dim3(TS_ROWS), 0, (hipStream_t)stream, y, N, P, rep, z);
    return sv_check_launch("sv_tsne_repulse");
}

// ------------------------------------------------------------------------------------------ sv_tsne_update
// Three launches over nb = ceil(N / 256) blocks of 256 rows; scratch is double [3 nb]: the blocks' shares of Z, of sum_i rowkl[i] and
// of |g|^2.  tsne_rowsum_kernel: a row's Z is its P states added in index order, a block's share the tree of its 256 rows.
// tsne_step_kernel: every block forms Z from the nb shares (thread t adds the shares t, t + 256, .., then the tree: the same bits in
// every block), merges its rows' repulsion states in index order, and applies the update.  tsne_stats_kernel, one block: the three
// sums of shares the same way, and stats.
__global__ __launch_bounds__(256) void tsne_rowsum_kernel(const float* __restrict__ z, const float* __restrict__ rowkl, int P, int N,
                                                          double* scratch) {
    __shared__ double sh[256];
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nb = gridDim.x;
    double zr = 0.0, kr = 0.0;
    if (row < N) {
        for (int p = 0; p < P; ++p) zr += (double)z[(int64_t)p * N + row];
        kr = (double)rowkl[row];
    }
    const double zb = ts_block_sum(zr, sh), kb = ts_block_sum(kr, sh);
    if (threadIdx.x == 0) {
        scratch[blockIdx.x] = zb;
        scratch[nb + blockIdx.x] = kb;
    }
}

__device__ __forceinline__ double ts_share_sum(const double* share, int nb, double* sh) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) v += share[i];
    return ts_block_sum(v, sh);
}

template <int D>
__global__ __launch_bounds__(256) void tsne_step_kernel(float* __restrict__ y, float* __restrict__ vel, float* __restrict__ gain,
                                                        const float* __restrict__ attr, const float* __restrict__ rep, int P, int N,
                                                        const float* __restrict__ hyper, double* scratch) {
    __shared__ double sh[256];
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nb = gridDim.x;
    const double Z = ts_share_sum(scratch, nb, sh);
    const double ex = (double)hyper[0], mom = (double)hyper[1], lr = (double)hyper[2];
    double g2 = 0.0;
    if (row < N) {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int64_t at = row * D + c;
            double R = 0.0;
            for (int p = 0; p < P; ++p) R += (double)rep[((int64_t)p * N + row) * D + c];
            const double g = 4.0 * (ex * (double)attr[at] - (Z > 0.0 ? R / Z : 0.0));
            const float v0 = vel[at], k0 = gain[at];
            const float k1 = fmaxf((double)v0 * g < 0.0 ? k0 + 0.2f : k0 * 0.8f, 0.01f);
            const float v1 = (float)(mom * (double)v0 - lr * (double)k1 * g);
            gain[at] = k1;
            vel[at] = v1;
            y[at] += v1;
            g2 += g * g;
        }
    }
    const double gb = ts_block_sum(g2, sh);
    if (threadIdx.x == 0) scratch[2 * (int64_t)nb + blockIdx.x] = gb;
}

__global__ __launch_bounds__(256) void tsne_stats_kernel(const double* scratch, int nb, float* stats) {
    __shared__ double sh[256];
    const double Z = ts_share_sum(scratch, nb, sh);
    const double kl = ts_share_sum(scratch + nb, nb, sh);
    const double g2 = ts_share_sum(scratch + 2 * (int64_t)nb, nb, sh);
    if (threadIdx.x == 0) {
        stats[0] = (float)(kl + (Z > 0.0 ? log(Z) : 0.0));
        stats[1] = (float)Z;
        stats[2] = (float)g2;
    }
}

int sv_tsne_update(float* y, float* vel, float* gain, const float* attr, const float* rowkl, const float* rep, const float* z, int P, int N,
                   int d, const float* hyper, double* scratch, float* stats, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(y && vel && gain, SV_E_ARG, "sv_tsne_update: a state (y, vel, gain) is NULL");
    SV_REQUIRE(attr && rowkl && rep && z, SV_E_ARG, "sv_tsne_update: an input (attr, rowkl, rep, z) is NULL");
    SV_REQUIRE(hyper && scratch && stats, SV_E_ARG, "sv_tsne_update: hyper, scratch or stats is NULL");
    SV_REQUIRE(N > 0, SV_E_ARG, "sv_tsne_update: non-positive size (N=%d)", N);
    SV_REQUIRE(d == 2 || d == 3, SV_E_SHAPE, "sv_tsne_update: d=%d is neither 2 nor 3", d);
    SV_REQUIRE(P >= 1 && P <= TS_PMAX, SV_E_ARG, "sv_tsne_update: P=%d outside [1, %d]", P, TS_PMAX);
    const int nb = (N - 1) / 256 + 1;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tsne_rowsum_kernel, dim3(nb), dim3(256), 0, s, z, rowkl, P, N, scratch);
    if (d == 2)
        hipLaunchKernelGGL(tsne_step_kernel<2>, dim3(nb), dim3(256), 0, s, y, vel, gain, attr, rep, P, N, hyper, scratch);
    else
        hipLaunchKernelGGL(tsne_step_kernel<3>, dim3(nb), dim3(256), 0, s, y, vel, gain, attr, rep, P, N, hyper, scratch);
    hipLaunchKernelGGL(tsne_stats_kernel, dim3(1), dim3(256), 0, s, scratch, nb, stats);
    return sv_check_launch("sv_tsne_update");
}
