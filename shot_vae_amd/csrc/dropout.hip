// Dropout between conv1 and norm2 of a wide unit (wideresnet.py:23-36): the forward pass with norm2's batch statistics, and the
// keep mask on its own.  The mask is the counter-based one of shotvae_hip.h (sv_dropout_args); the backward is a template flag
// of sv_bn_bwd_apply's kernel (small.hip).  gfx950.
#include <math.h>
#include "common.h"

namespace {

// One streaming pass: 16-byte vectors of 8 channels, two generator calls per vector (= one per 4 elements).  A block has
// nthr = the largest multiple of C/8 <= 256 threads, so a thread always meets the same 8 channels and keeps their (sum, sum of
// squares) in double registers; at the end the threads of a channel group meet in LDS in index order and thread cg < C/8
// adds the block's sums -- one fp64 atomic per channel and sum per block, into replica blockIdx.x % R -- or (slots != NULL,
// deterministic mode) stores them to the block's slot [G][grid][2C].
template <typename T>
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const T* x, int64_t M, int C, int ld, sv_dropout_args a, T* out,
                                                          double* stats, int R, double* slots) {
    typedef typename V8<T>::type V;
    __shared__ double red[256];
    const int grp = blockIdx.y;
    const int cv = C >> 3;
    const int nthr = blockDim.x;
    const int64_t gs = (int64_t)M * ld;
    x += grp * gs;
    out += grp * gs;
    const uint64_t key = (uint64_t)a.keys[grp];
    const int cg = threadIdx.x % cv;
    const int c = cg * 8;
    const int64_t rows_per_trip = (int64_t)gridDim.x * (nthr / cv);
    double s1[8], s2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.0;
    for (int64_t m = (int64_t)blockIdx.x * (nthr / cv) + threadIdx.x / cv; m < M; m += rows_per_trip) {
        const V xv = __builtin_nontemporal_load(reinterpret_cast<const V*>(x + m * ld + c));
        const uint32_t keep = sv_dropout_keep8(key, a.unit, a.thr, m * C + c);
        V ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const T y = ((keep >> j) & 1) ? (T)(to_f(xv[j]) * a.scale) : (T)0.f;
            ov[j] = y;
            const float yf = to_f(y);
            s1[j] += (double)yf;
            s2[j] += (double)yf * (double)yf;
        }
        *reinterpret_cast<V*>(out + m * ld + c) = ov;
    }
    if (!stats && !slots) return;
    // the nthr / cv threads of channel group cg, in index order (fixed: the block's sums do not depend on timing)
    double tot[16];
    for (int k = 0; k < 16; ++k) {
        __syncthreads();
        red[threadIdx.x] = k < 8 ? s1[k] : s2[k - 8];
        __syncthreads();
        double t = 0.0;
        if (threadIdx.x < cv)
            for (int r = threadIdx.x; r < nthr; r += cv) t += red[r];
        tot[k] = t;
    }
    if (threadIdx.x < cv) {
        if (slots) {
            double* s = slots + ((int64_t)grp * gridDim.x + blockIdx.x) * 2 * C;
#pragma unroll
            for (int j = 0; j < 8; ++j) { s[c + j] = tot[j]; s[C + c + j] = tot[8 + j]; }
        } else {
            double* s = stats + ((int64_t)grp * R + (blockIdx.x % R)) * 2 * C;
#pragma unroll
            for (int j = 0; j < 8; ++j) { atomicAdd(s + c + j, tot[j]); atomicAdd(s + C + c + j, tot[8 + j]); }
        }
    }
}

// deterministic mode: stats [G][R][2C] replica 0 += the P block slots [G][P][2C], added in index order (one adder per address)
__global__ __launch_bounds__(256) void dropout_collect_kernel(const double* slots, int P, int n, double* stats, int R) {
    const int i = blockIdx.x * 256 + threadIdx.x, grp = blockIdx.y;
    if (i >= n) return;
    const double* s = slots + (int64_t)grp * P * n + i;
    double t = 0.0;
    for (int p = 0; p < P; ++p) t += s[(int64_t)p * n];
    stats[(int64_t)grp * R * n + i] += t;
}

// out[e] = kept(e): one thread per 4 elements = one generator call
__global__ __launch_bounds__(256) void dropout_mask_kernel(const int64_t* keys, int unit, uint32_t thr, int64_t n4, uint8_t* out) {
    const int grp = blockIdx.y;
    const uint64_t key = (uint64_t)keys[grp];
    out += (int64_t)grp * n4 * 4;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (int64_t)gridDim.x * 256) {
        const sv_u32x4 r = sv_philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)unit, 0u, (uint32_t)key,
                                            (uint32_t)(key >> 32));
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w |= (uint32_t)(r.v[j] >= thr) << (8 * j);
        reinterpret_cast<uint32_t*>(out)[q] = w;
    }
}

}  // namespace

int sv_dropout_check(const sv_dropout_args* a, const char* who) {
    SV_REQUIRE(a, SV_E_ARG, "%s: dropout arguments missing", who);
    SV_REQUIRE(a->keys, SV_E_ARG, "%s: keys is NULL (one int64 key per group in device memory)", who);
    SV_REQUIRE(a->unit >= 0, SV_E_ARG, "%s: unit=%d must be >= 0", who, (int)a->unit);
    SV_REQUIRE(a->p > 0.f && a->p < 1.f, SV_E_ARG, "%s: dropout p=%g outside (0, 1)", who, (double)a->p);
    // thr = (uint32)(p * 2^32) and scale = (float)(1 / (1 - p)) are formed by the caller from its double p; the float p here
    // only has to agree with them to its own rounding
    const double p = (double)a->p, two32 = 4294967296.0;
    SV_REQUIRE(fabs((double)a->thr - p * two32) <= two32 * 1e-6 + 1.0, SV_E_ARG,
               "%s: thr=%u is inconsistent with p=%g (expected (uint32)(p * 2^32))", who, (unsigned)a->thr, p);
    SV_REQUIRE(fabs((double)a->scale * (1.0 - p) - 1.0) <= 1e-5, SV_E_ARG,
               "%s: scale=%g is inconsistent with p=%g (expected 1 / (1 - p))", who, (double)a->scale, p);
    return SV_OK;
}

extern "C" {

int sv_dropout_fwd(int dtype, const void* x, int64_t M, int C, int ld, const sv_dropout_args* a, void* out, sv_acc_t* stats,
                   int replicas, int groups, void* stream) {
    SvProfScope prof_scope(stream);
    const int rc = sv_dropout_check(a, "sv_dropout_fwd");
    if (rc) return rc;
    SV_REQUIRE(x && out && M > 0 && C > 0, SV_E_ARG, "sv_dropout_fwd: bad argument");
    SV_REQUIRE(C % 8 == 0 && ld % 8 == 0 && ld >= C, SV_E_SHAPE, "sv_dropout_fwd: C=%d ld=%d must be multiples of 8, ld >= C", C, ld);
    SV_REQUIRE(C <= 2048, SV_E_SHAPE, "sv_dropout_fwd: C=%d too large (at most 2048)", C);
    SV_REQUIRE(!stats || (replicas >= 1 && (replicas & (replicas - 1)) == 0), SV_E_ARG,
               "sv_dropout_fwd: replicas=%d must be a power of two >= 1", replicas);
    SV_REQUIRE(dtype == SV_F32 || dtype == SV_BF16, SV_E_ARG, "bad dtype %d", dtype);
    groups = sv_ngroups(groups);
    SV_REQUIRE(groups <= SV_MAX_GROUPS, SV_E_ARG, "sv_dropout_fwd: groups=%d (at most %d)", groups, SV_MAX_GROUPS);
    const int cv = C / 8;
    const int nthr = cv <= 256 ? 256 / cv * cv : 0;
    SV_REQUIRE(nthr >= 64, SV_E_SHAPE, "sv_dropout_fwd: C=%d leaves fewer than 64 threads per block", C);
    // enough blocks to fill the chip twice over across the groups, each a few dozen vectors per thread at the headline shape
    const int64_t rows_per_block = nthr / cv;
    int64_t grid = (M + rows_per_block - 1) / rows_per_block;
    const int64_t cap = 2048 / groups;
    if (grid > cap) grid = cap;
    double* slots = nullptr;
    if (stats && sv_det_stats()) {
        const int64_t dcap = ((int64_t)1 << 19) / ((int64_t)groups * 2 * C);      // (the slots stay well inside the scratch ring)
        if (grid > dcap) grid = dcap > 0 ? dcap : 1;
        slots = reinterpret_cast<double*>(sv_det_scratch((size_t)2 * groups * grid * 2 * C));
        if (!slots) return SV_E_HIP;
    }
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SV_BF16)
        hipLaunchKernelGGL((dropout_fwd_kernel<bf16>), dim3((int)grid, groups), dim3(nthr), 0, s, (const bf16*)x, M, C, ld, *a,
                           (bf16*)out, stats, replicas, slots);
    else
        hipLaunchKernelGGL((dropout_fwd_kernel<float>), dim3((int)grid, groups), dim3(nthr), 0, s, (const float*)x, M, C, ld, *a,
                           (float*)out, stats, replicas, slots);
    if (slots)
        hipLaunchKernelGGL(dropout_collect_kernel, dim3((2 * C + 255) / 256, groups), dim3(256), 0, s, slots, (int)grid, 2 * C,
                           stats, replicas);
    return sv_check_launch("sv_dropout_fwd");
}

int sv_dropout_mask(const int64_t* keys, int unit, uint32_t thr, int64_t M, int C, int groups, uint8_t* out, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(keys, SV_E_ARG, "sv_dropout_mask: keys is NULL (one int64 key per group in device memory)");
    SV_REQUIRE(out && M > 0 && C > 0 && unit >= 0, SV_E_ARG, "sv_dropout_mask: bad argument");
    SV_REQUIRE(C % 8 == 0, SV_E_SHAPE, "sv_dropout_mask: C=%d must be a multiple of 8", C);
    groups = sv_ngroups(groups);
    SV_REQUIRE(groups <= SV_MAX_GROUPS, SV_E_ARG, "sv_dropout_mask: groups=%d (at most %d)", groups, SV_MAX_GROUPS);
    const int64_t n4 = M * C / 4;
    int64_t grid = (n4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((int)grid, groups), dim3(256), 0, (hipStream_t)stream, keys, unit, thr, n4, out);
    return sv_check_launch("sv_dropout_mask");
}

}  // extern "C"
