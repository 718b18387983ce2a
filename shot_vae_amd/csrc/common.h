// Shared device helpers for libshotvae_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "shotvae_hip.h"

typedef __bf16 bf16;
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <typename T> struct V8;
template <> struct V8<float> { typedef f32x8 type; };
template <> struct V8<bf16> { typedef bf16x8 type; };
template <typename T> struct V4;
template <> struct V4<float> { typedef f32x4 type; };
template <> struct V4<bf16> { typedef bf16x4 type; };

// D(16x16) += A(16xK) * B(Kx16) for one 32-deep k chunk.  Lane l supplies A[row l&15][k=8(l>>4)+j]
// and B[k=8(l>>4)+j][col l&15], j=0..7.  bf16: one v_mfma_f32_16x16x32_bf16.  fp32: eight
// v_mfma_f32_16x16x4_f32 (exact fp32), step j consuming element j of every lane group -- the k order
// is a permutation of the same 32 products, so both dtypes share one fragment layout.
__device__ __forceinline__ void mma32(f32x4& acc, const bf16x8& a, const bf16x8& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma32(f32x4& acc, const f32x8& a, const f32x8& b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], acc, 0, 0, 0);
}

__device__ __forceinline__ float to_f(float v) { return v; }
__device__ __forceinline__ float to_f(bf16 v) { return (float)v; }

// LeakyReLU / ReLU; every entry point rejects slopes outside [0, 1], where max(u, slope*u) is the activation
__device__ __forceinline__ float act_fwd(float u, float slope) { return fmaxf(u, u * slope); }
__device__ __forceinline__ float act_grad(float u, float slope) { return u > 0.f ? 1.f : slope; }

// BatchNorm-apply + LeakyReLU / ReLU of 8 consecutive channels (the load prologue of every conv-like kernel):
// o[j] = act(x[j] * s[j] + t[j]).  (A version on packed fp32 pairs -- v_pk_fma_f32 / v_pk_mul_f32, 28 instead of ~40 VALU
// instructions per vector -- measured SLOWER on gfx950: conv3x3p forward 90.4 vs 88.4 us, the generic stride-2 forward 532
// vs 517 us; the packed fp32 instructions issue at half rate.)
__device__ __forceinline__ bf16x8 bn_act8(const bf16x8& x, const f32x4& s0, const f32x4& s1, const f32x4& t0, const f32x4& t1,
                                          float slope) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float u0 = (float)x[j] * s0[j] + t0[j], u1 = (float)x[j + 4] * s1[j] + t1[j];
        o[j] = (bf16)fmaxf(u0, u0 * slope);
        o[j + 4] = (bf16)fmaxf(u1, u1 * slope);
    }
    return o;
}
__device__ __forceinline__ f32x8 bn_act8(const f32x8& x, const f32x4& s0, const f32x4& s1, const f32x4& t0, const f32x4& t1,
                                         float slope) {
    f32x8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float u0 = x[j] * s0[j] + t0[j], u1 = x[j + 4] * s1[j] + t1[j];
        o[j] = fmaxf(u0, u0 * slope);
        o[j + 4] = fmaxf(u1, u1 * slope);
    }
    return o;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// packed per-tap offsets: 4 bits per tap, biased by 8
__device__ __forceinline__ uint64_t pack_taps(const int8_t* d) {
    uint64_t p = 0;
#pragma unroll
    for (int t = 0; t < SV_MAX_TAPS; ++t) p |= (uint64_t)((d[t] + 8) & 15) << (4 * t);
    return p;
}
__device__ __forceinline__ int tap_off(uint64_t p, int t) { return (int)((p >> (4 * t)) & 15) - 8; }

// Batched launch (sv_igemm_args::groups): blockIdx.y = group; a group is an independent instance of the layer whose
// tensors / coefficient vectors / accumulators follow those of the previous group.  The HOST expands the caller's
// arguments into one argument block per group (all of them travel as the kernel parameter); a kernel starts with
// `const sv_igemm_args& a = A.g[blockIdx.y];` -- a reference into kernel-argument memory, so every field is still a scalar
// load at its point of use (a modified COPY of the block would pin ~40 SGPRs for the kernel's lifetime: measured +40 % on
// the persistent 3x3 kernel) -- and runs on (g, a) exactly as for a single instance.
constexpr int SV_MAX_GROUPS = 4;          // the four forwards of a SHOT-VAE step
struct sv_igemm_args_g { sv_igemm_args g[SV_MAX_GROUPS]; };
__host__ __device__ __forceinline__ int sv_ngroups(int groups) { return groups > 0 ? groups : 1; }
inline sv_igemm_args_g sv_expand_groups(const sv_geom& g, const sv_igemm_args& a, int es) {
    sv_igemm_args_g A;
    const int64_t xs = (int64_t)g.B * g.Hin * g.Win * g.ldx * es, os = (int64_t)g.B * g.Hout * g.Wout * g.ldo * es;
    for (int64_t grp = 0; grp < SV_MAX_GROUPS; ++grp) {
        sv_igemm_args r = a;
        if (grp > 0 && grp < sv_ngroups(a.groups)) {
            r.x = reinterpret_cast<const char*>(a.x) + grp * xs;
            r.out = reinterpret_cast<char*>(a.out) + grp * os;
            if (a.residual) r.residual = reinterpret_cast<const char*>(a.residual) + grp * os;
            if (a.ex) r.ex = reinterpret_cast<const char*>(a.ex) + grp * os;
            if (a.pro_scale) { r.pro_scale = a.pro_scale + grp * g.Cin; r.pro_shift = a.pro_shift + grp * g.Cin; }
            if (a.fold_stats) {
                r.fold_stats = a.fold_stats + grp * (int64_t)a.fold_replicas * 2 * g.Cin;
                r.fold_mean = a.fold_mean + grp * g.Cin;
                r.fold_rstd = a.fold_rstd + grp * g.Cin;
            }
            if (a.stats) r.stats = a.stats + grp * (int64_t)a.replicas * 2 * g.N;
            if (a.ex) {
                r.ex_scale = a.ex_scale + grp * g.N; r.ex_shift = a.ex_shift + grp * g.N;
                r.ex_mean = a.ex_mean + grp * g.N; r.ex_rstd = a.ex_rstd + grp * g.N;
                r.bsums = a.bsums + grp * (int64_t)a.replicas * 2 * g.N;
            }
        }
        A.g[grp] = r;
    }
    return A;
}
// the same for the weight-gradient parameter blocks (fields x, dy, pro_scale, pro_shift): the groups' operands follow
// each other, the gradient of the SHARED weights sums over the groups
template <typename P> struct sv_wg_g { P g[SV_MAX_GROUPS]; };
template <typename P>
inline sv_wg_g<P> sv_expand_wg(const sv_geom& g, const P& p, int groups, int es) {
    sv_wg_g<P> A;
    for (int64_t grp = 0; grp < SV_MAX_GROUPS; ++grp) {
        P r = p;
        if (grp > 0 && grp < groups) {
            r.x = reinterpret_cast<const char*>(p.x) + grp * ((int64_t)g.B * g.Hin * g.Win * g.ldx * es);
            r.dy = reinterpret_cast<const char*>(p.dy) + grp * ((int64_t)g.B * g.Hout * g.Wout * g.ldo * es);
            if (p.pro_scale) { r.pro_scale = p.pro_scale + grp * g.Cin; r.pro_shift = p.pro_shift + grp * g.Cin; }
        }
        A.g[grp] = r;
    }
    return A;
}

// BatchNorm finalisation folded into a consumer kernel (sv_igemm_args::fold_*): all 256 threads of the block sum the R replicas
// of (sum, sum of squares) of the C <= 64 channels (a fixed partition: thread tid takes channel tid % C and the replicas
// tid / C, + 256 / C, ...; the partial sums meet in LDS in index order), derive scale / shift -- sv_bn_finalize's arithmetic --
// into sc_out / sh_out (LDS, C floats each), and `writer` blocks also store scale / shift / mean / rstd to global memory.
// `scratch`: 2 * 256 DOUBLES of LDS (4 KB).  Ends with a barrier.
// The accumulators are doubles (sv_acc_t): sums of the producers' fp32 partial sums, exact in any order; mean and variance are
// formed in double (no E[x^2] - E[x]^2 cancellation in fp32) and rounded once -- the same arithmetic as bn_finalize_kernel.
__device__ __forceinline__ void sv_bn_moments(double s1, double s2, float count, float eps, float& mu, float& var, float& rs) {
    const double m = s1 / (double)count;
    double v = s2 / (double)count - m * m;
    v = v > 0.0 ? v : 0.0;
    mu = (float)m;
    var = (float)v;
    rs = rsqrtf(var + eps);
}
// <256, false>: the form above.  <512, true>: the 512-thread kernels with register-resident weights (tconv.hip, sconv.hip),
// C = 32 / 64 / 128 channels (C divides 512: every thread has a part), the coefficients as [C] pairs {scale, shift} in LDS
// (sc_out = the pairs, sh_out = sc_out + 1); `scratch`: 2 * 512 doubles of LDS (8 KB).
template <int THREADS, bool PAIRS>
__device__ __forceinline__ void sv_bn_fold_block(const sv_igemm_args& a, int C, double* scratch, float* sc_out, float* sh_out,
                                                 bool writer) {
    constexpr int S = PAIRS ? 2 : 1;
    const int tid = threadIdx.x, c = tid % C, part = tid / C, parts = THREADS / C;
    double s1 = 0.0, s2 = 0.0;
    if (PAIRS || part < parts)
        for (int r = part; r < a.fold_replicas; r += parts) {
            s1 += a.fold_stats[(size_t)r * 2 * C + c];
            s2 += a.fold_stats[(size_t)r * 2 * C + C + c];
        }
    scratch[tid] = s1;
    scratch[THREADS + tid] = s2;
    __syncthreads();
    if (tid < C) {
        double t1 = 0.0, t2 = 0.0;
        for (int q = 0; q < parts; ++q) { t1 += scratch[q * C + tid]; t2 += scratch[THREADS + q * C + tid]; }
        float mu, var, rs;
        sv_bn_moments(t1, t2, a.fold_count, a.fold_eps, mu, var, rs);
        const float sc = a.fold_gamma[tid] * rs, sh = a.fold_beta[tid] - mu * sc;
        sc_out[S * tid] = sc;
        sh_out[S * tid] = sh;
        if (writer) {
            const_cast<float*>(a.pro_scale)[tid] = sc;
            const_cast<float*>(a.pro_shift)[tid] = sh;
            a.fold_mean[tid] = mu;
            a.fold_rstd[tid] = rs;
        }
    }
    __syncthreads();
}

// ---- dropout mask (sv_dropout_fwd, sv_bn_bwd_apply_dropout, sv_dropout_mask; definition in shotvae_hip.h) -----------------
// Philox-4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between rounds.
struct sv_u32x4 { uint32_t v[4]; };
__host__ __device__ __forceinline__ sv_u32x4 sv_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                              uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
    }
    return sv_u32x4{{c0, c1, c2, c3}};
}
// keep bits of the 8 elements e0 .. e0 + 7 (e0 % 8 == 0: two generator calls, counters q = e0 / 4 and q + 1); bit j = element e0 + j
__device__ __forceinline__ uint32_t sv_dropout_keep8(uint64_t key, int unit, uint32_t thr, int64_t e0) {
    const uint64_t q = (uint64_t)e0 >> 2;
    const sv_u32x4 a = sv_philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)unit, 0u, (uint32_t)key, (uint32_t)(key >> 32));
    const sv_u32x4 b = sv_philox4x32_10((uint32_t)(q + 1), (uint32_t)((q + 1) >> 32), (uint32_t)unit, 0u, (uint32_t)key,
                                        (uint32_t)(key >> 32));
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m |= (uint32_t)(a.v[j] >= thr) << j;
        m |= (uint32_t)(b.v[j] >= thr) << (j + 4);
    }
    return m;
}
// Four standard normals from one generator call (sv_latent_draw, sv_latent_sweep; definition in shotvae_hip.h): counter
// (low32(row), high32(row), c2, tag); Box-Muller on the word pairs (0, 1) and (2, 3): cos, sin of each pair
__device__ __forceinline__ void sv_normals4(uint64_t key, uint64_t row, uint32_t c2, uint32_t tag, float n[4]) {
    const sv_u32x4 r = sv_philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), c2, tag, (uint32_t)key, (uint32_t)(key >> 32));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = (float)((r.v[2 * p] >> 8) + 1u) * 0x1p-24f;          // (0, 1]: exact in fp32, log finite
        const float u2 = (float)(r.v[2 * p + 1] >> 8) * 0x1p-24f;             // [0, 1)
        const float rad = sqrtf(-2.f * logf(u1)), ang = 6.283185307179586f * u2;
        n[2 * p] = rad * cosf(ang);
        n[2 * p + 1] = rad * sinf(ang);
    }
}
// the argument check every dropout entry point runs before it launches (keys, p in (0, 1), thr / scale consistent with p)
int sv_dropout_check(const sv_dropout_args* a, const char* who);

// Interleaved tile order of the one-block-per-CU kernels (bwd3x3f.hip, fwd3x3f.hip) for ANY grid size: at its step k a block takes tile
// k * NC + slot of its group, and the blocks that share an XCD (the hardware deals blocks to the eight XCDs round-robin in linear
// block-id order, x fastest) own CONSECUTIVE slots, so that vertically adjacent tiles -- which share halo rows -- meet in one L2.
// (With NC a multiple of 8 this is conv3x3p_kernel's mapping; a batched launch of four groups on 248 blocks has NC = 62.)
__device__ __forceinline__ int sv_window_slot(int NC, int group, int bx) {
    const int l0 = group * NC;                                   // linear id of the group's first block
    const int xcd = (l0 + bx) & 7;
    int prefix = 0;
    for (int y = 0; y < 8; ++y) {
        const int first = (y - l0) & 7;                          // first bx of the group on XCD y
        const int cnt = first < NC ? (NC - first + 7) >> 3 : 0;
        if (y < xcd) prefix += cnt;
    }
    return prefix + ((bx - ((xcd - l0) & 7)) >> 3);
}

// ---- log-sum-exp state (score.hip, aggpost.hip) ---------------------------------------------------------------------------
// (m, a): the value m + log(a) with m the running maximum; a term of -inf has weight 0; m = +inf is absorbing; a NaN term makes the
// result NaN (fmax alone would drop it)
struct ScoreLse { double m, a; };
__device__ __forceinline__ ScoreLse score_lse_merge(ScoreLse p, ScoreLse q) {
    if (p.m != p.m || q.m != q.m) return ScoreLse{NAN, 0.0};
    const double m = fmax(p.m, q.m);
    if (!(m > -INFINITY) || !(m < INFINITY)) return ScoreLse{m, m == INFINITY ? 1.0 : 0.0};    // all -inf so far, or +inf (or NaN)
    return ScoreLse{m, p.a * exp(p.m - m) + q.a * exp(q.m - m)};                                // exp(-inf - m) = 0
}
__device__ __forceinline__ double score_lse_value(ScoreLse p) { return (p.m > -INFINITY && p.m < INFINITY) ? p.m + log(p.a) : p.m; }

// ---- posterior tiles (knn.hip, aggpost.hip): 64 gallery rows x 16 dimensions per staged chunk, 256 threads ------------------
constexpr int KN_THREADS = 256;       // 16 x 16 threads; thread (ty, tx) owns rows MQ * ty .., columns 4 * tx .. of the tile
constexpr int KN_TG = 64;             // gallery rows per tile
constexpr int KN_DC = 16;             // dimensions per staged chunk

template <int METRIC> struct KnTraits {
    static constexpr bool TWO = METRIC == SV_DIST_KL || METRIC == SV_DIST_W2;          // a second operand array (from ls)
    static constexpr bool AUX = METRIC == SV_DIST_KL || METRIC == SV_DIST_COSINE;      // a per-row scalar (sum ls / |mu|^2)
};

// Staging of rows [r0, r0 + ROWS) x dimensions [d0, d0 + 16), in two halves so that the global loads of the next chunk are in
// flight while the current one is multiplied: kn_load reads mu (and ls where the metric reads it) into registers -- 16 consecutive
// threads take the 16 dimensions of one row --, kn_store writes A[d][ROWS + 4] (mu) and B[d][ROWS + 4] (from ls: KL sigma^2 for a query
// row and 1 / sigma^2 for a gallery row, W2 sigma); rows and dimensions beyond the end are staged as the metric's neutral element.
// aux[i] (double) gathers the thread's share of the row scalar of its i-th row (KL: sum ls, cosine: |mu|^2) over the chunks;
// kn_aux_reduce adds the 16 shares of a row with an xor-butterfly (a fixed order).
template <int METRIC, int ROWS>
__device__ __forceinline__ void kn_load(const float* __restrict__ mu, const float* __restrict__ ls, int64_t r0, int64_t nrows, int d0,
                                        int D, float* m, float* l) {
    const int d = d0 + (threadIdx.x & 15), rr = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < ROWS / 16; ++i) {
        const int64_t gr = r0 + rr + 16 * i;
        const bool ok = gr < nrows && d < D;
        m[i] = ok ? mu[gr * D + d] : 0.f;
        l[i] = (KnTraits<METRIC>::TWO && ok) ? ls[gr * D + d] : 0.f;
    }
}
template <int METRIC, int ROWS, bool GALLERY>
__device__ __forceinline__ void kn_store(const float* m, const float* l, int64_t r0, int64_t nrows, int d0, int D, float* A, float* B,
                                         double* aux) {
    constexpr int LD = ROWS + 4;
    const int dd = threadIdx.x & 15, rr = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < ROWS / 16; ++i) {
        const int r = rr + 16 * i;
        const bool ok = r0 + r < nrows && d0 + dd < D;
        A[dd * LD + r] = m[i];
        if (METRIC == SV_DIST_KL) {
            B[dd * LD + r] = ok ? expf(GALLERY ? -2.f * l[i] : 2.f * l[i]) : 0.f;
            aux[i] += (double)l[i];
        } else if (METRIC == SV_DIST_W2) {
            B[dd * LD + r] = ok ? expf(l[i]) : 0.f;
        } else if (METRIC == SV_DIST_COSINE) {
            aux[i] += (double)m[i] * (double)m[i];
        }
    }
}
__device__ __forceinline__ double kn_aux_reduce(double x) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// host side ------------------------------------------------------------------------------------------
void sv_set_error(const char* fmt, ...);
bool sv_disabled(int kernel_bit);        // sv_set_option(SV_OPT_DISABLE_MASK, ...): a specialised kernel is switched off
int sv_wide_min_blocks();
bool sv_enabled(int kernel_bit);       // sv_set_option(SV_OPT_ENABLE_MASK, ...): a kernel that is OFF by default is switched on
bool sv_halo_all();
int sv_persistent_blocks();            // block budget of the persistent kernels: the launch's own (sv_igemm_args::block_budget,
                                       // sv_wgrad_args::block_budget) if it has one, else sv_set_option(SV_OPT_PERSISTENT_BLOCKS, ...)
// scope of one entry-point call on the calling thread: its launches see `budget` (> 0) as their block budget
struct SvBudgetScope {
    int old;
    explicit SvBudgetScope(int budget);
    ~SvBudgetScope();
};
bool sv_deterministic();               // sv_set_option(SV_OPT_DETERMINISTIC, 1): every accumulation in a fixed order
bool sv_det_stats();                   // ... 1 or 2: the BatchNorm statistics / backward sums in a fixed order (2: only those)
float* sv_det_scratch(size_t floats);  // deterministic mode: a slice of the library's scratch ring (nullptr + error text on failure)
enum { SV_FLAG_DET = 1 };              // sv_igemm_args::flags
// sv_igemm_query_blocks: sv_igemm_launch calls sv_dry_run(grid) right before its launch; it returns true (and records
// the grid) when the calling thread is inside a query -- the caller then returns SV_OK without launching.  In deterministic
// mode it also checks the replica count of a real launch (returns true with *rc < 0 when it is too small).
bool sv_dry_run(int grid_x, const sv_igemm_args* a, int* rc);
bool sv_in_query();                    // the calling thread is inside sv_igemm_query_blocks (nothing may be launched)
// BatchNorm fold protocol (runtime.hip): sv_igemm announces a pending fold; a launcher whose kernel folds claims it (can =
// the kernel's own limits hold, e.g. fold_replicas <= 64) and passes fold_stats on, everybody else passes fold_stats = NULL;
// an unclaimed fold is materialised by the launch gate (sv_bn_finalize as a launch of its own)
void sv_fold_begin(const sv_geom* g, const sv_igemm_args* a, void* stream);
void sv_fold_end();
bool sv_fold_claim(bool can);
// sv_igemm_args::start_flag: the first block of every kernel of the family announces its start (see shotvae_hip.h)
__device__ __forceinline__ void sv_start_signal(const sv_igemm_args& a) {
    if (a.start_flag && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0)
        __hip_atomic_store(a.start_flag, a.start_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
int sv_check_launch(const char* what);
void sv_prof_begin(hipStream_t s);
void sv_prof_end(hipStream_t s);
// brackets the launches of one entry point with the in-situ timing events (no-ops unless sv_prof_enable(1))
struct SvProfScope {
    hipStream_t s;
    explicit SvProfScope(void* st) : s((hipStream_t)st) { sv_prof_begin(s); }
    ~SvProfScope() { sv_prof_end(s); }
};
// The argument block a launcher's kernel gets: *a, with fold_stats kept only if the launcher claims the pending fold.
inline sv_igemm_args sv_fold_resolve(const sv_igemm_args& a, bool can) {
    sv_igemm_args b = a;
    if (!sv_fold_claim(can)) b.fold_stats = nullptr;
    return b;
}
// the label of the calling thread's last launch through sv_igemm_launch (sv_debug_last_kernel: tests name the kernel that ran)
void sv_note_kernel(const char* label);
// The one launch path of the sv_igemm family: the gate (sv_dry_run -- a grid query, the deterministic replica check and the
// materialisation of an unclaimed fold; its rc is returned when nothing is to be launched), then `kernel` on grid_x x groups
// blocks of `threads` threads with (*g, the per-group argument blocks, extra...).  `es`: the element size of x / out.
template <typename K, typename... X>
inline int sv_igemm_launch(K* kernel, int grid_x, int threads, size_t lds, const sv_geom* g, const sv_igemm_args* a, int es,
                           hipStream_t s, const char* label, X... extra) {
    int rc = SV_OK;
    if (sv_dry_run(grid_x, a, &rc)) return rc;
    sv_note_kernel(label);
    sv_prof_begin(s);
    hipLaunchKernelGGL(kernel, dim3(grid_x, sv_ngroups(a->groups)), dim3(threads), lds, s, *g, sv_expand_groups(*g, *a, es), extra...);
    sv_prof_end(s);
    return sv_check_launch(label);
}
// Raises the dynamic-LDS limit of `kernels` (more than 64 KiB per block needs the opt-in; gfx950 has 160 KiB per CU) to `bytes`,
// once per call site: `done` is the site's own `static bool`, one per kernel instantiation; after the first call this is that
// flag's test and nothing else.  A failure is reported through sv_check_launch as "hipFuncSetAttribute(<name>)".
// Like the dispatcher options the flag assumes one device and no concurrent first calls.
int sv_lds_optin_set(const void* kernel, int bytes, const char* name);      // runtime.hip
template <typename... K>
inline int sv_lds_optin(bool& done, int bytes, const char* name, K*... kernels) {
    if (done) return SV_OK;
    int rc = SV_OK;
    ((rc = rc != SV_OK ? rc : sv_lds_optin_set(reinterpret_cast<const void*>(kernels), bytes, name)), ...);
    done = rc == SV_OK;
    return rc;
}
// exact log2 of a power of two, -1 for anything else (v <= 0 included)
inline int sv_ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
// One-block-per-CU launchers: `n` work items (bands, images) dealt to at most `per` blocks in rounds; the smallest grid that
// needs no more rounds than `per` blocks would.
inline int sv_block_slots(int n, int per) {
    if (per < 1) per = 1;
    if (per > n) per = n;
    const int rounds = (n + per - 1) / per;
    return (n + rounds - 1) / rounds;
}
// adds `nslabs` partial slabs of n floats (plain stores of a weight-gradient kernel, in ws) to dw in a fixed order (wgrad3x3.hip)
void sv_slab_reduce(const float* ws, int nslabs, int64_t n, float* dw, hipStream_t s);
// The specialised candidates of sv_igemm (igemm.hip, whose generic kernels are its tail): each returns 1 and sets *rc when it
// takes the launch.  (sv_conv3x3_try tries sv_conv3x3w_try first, which tries sv_conv3x3x_try.)
typedef int sv_igemm_try_fn(const sv_geom* g, int dtype, const sv_igemm_args* a, hipStream_t s, int* rc);
sv_igemm_try_fn sv_conv3x3_try, sv_halo_try, sv_tconvr_try, sv_sconv_try, sv_pconv_try, sv_dconv_try, sv_thconv_try, sv_conv3x3w_try, sv_pixgemm_try;
int sv_conv3x3x_try(const sv_geom* g, const sv_igemm_args* a, bool fwd, hipStream_t s, int* rc);
// The specialised candidates of the weight-gradient dispatch (wgrad.hip, whose generic kernels are its tail with the same
// signature), in its order: each returns 1 and sets *rc when it takes the launch.  `a` is the checked operand block with
// a.groups normalised (sv_ngroups).
typedef int sv_wgrad_try_fn(const sv_geom* g, int dtype, const sv_wgrad_args& a, hipStream_t s, int* rc);
sv_wgrad_try_fn sv_wgrad3x3_try, sv_thwgrad_try, sv_k4wgrad_try, sv_s2wgrad_try, sv_hwgrad_try;
// the operands every weight-gradient parameter block carries (the structs order them differently)
template <typename P>
inline void sv_wg_operands(P& p, const sv_wgrad_args& a) {
    p.x = a.x; p.pro_scale = a.pro_scale; p.pro_shift = a.pro_shift; p.pro_slope = a.pro_slope; p.dy = a.dy;
}

#define SV_REQUIRE(cond, code, ...)                \
    do {                                           \
        if (!(cond)) {                             \
            sv_set_error(__VA_ARGS__);             \
            return code;                           \
        }                                          \
    } while (0)
