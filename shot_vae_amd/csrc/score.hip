// Per-image ELBO terms and the importance-weighted bound on log p(x) (declared, with the exact definitions, in
// include/shotvae_hip.h):
//   sv_latent_sweep  the decoder's input rows [z_{b,s} | onehot | 0-pad] over samples and classes, and lw = log p(z) - log q(z|x)
//   sv_recon_rows    the reconstruction term nll of every decoded row against its image
//   sv_score_reduce  recon / kl_c / kl_d / elbo / log_px per image from the [B][S][Kd] terms
// Plain HIP C++; each takes a stream and allocates nothing, the sweep reads its key from device memory: capturable.  Every sum has a
// fixed order (per-thread partial sums in index order, then a shared-memory tree) and no atomics: the outputs are bit-reproducible.
#include "common.h"
#include <math.h>

// sum of v over the block's NT threads (NT a power of two), fixed order; every thread receives the result
template <int NT>
__device__ __forceinline__ double score_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();                                   // the previous use of sh is over
    sh[tid] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// ------------------------------------------------------------------------------------------ sv_latent_sweep
constexpr int SW_THREADS = 128;

// one block per decoded row
template <typename T>
__global__ __launch_bounds__(SW_THREADS) void latent_sweep_kernel(const float* mu, const float* ls, const int64_t* key, int64_t row0,
                                                                  const int64_t* label, int S, int Kd, int K, int ldc, int Lpad,
                                                                  int64_t j0, T* latent, float* lw) {
    __shared__ double sh[SW_THREADS];
    const int tid = threadIdx.x;
    const int64_t J = j0 + blockIdx.x, per = (int64_t)S * Kd;
    const int64_t b = J / per, rem = J - b * per;
    const int s = (int)(rem / Kd), k = (int)(rem - (int64_t)s * Kd);
    T* out = latent + (int64_t)blockIdx.x * Lpad;
    const uint64_t kv = key ? (uint64_t)key[0] : 0u;
    const uint64_t row = (uint64_t)(row0 + b);
    double acc = 0.0;
    for (int j = tid; 4 * j < ldc; j += SW_THREADS) {
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (key) sv_normals4(kv, row, ((uint32_t)s << 16) | (uint32_t)j, SV_SCORE_PHILOX_TAG, n);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * j + q;
            if (d < ldc) {
                const int64_t i = b * ldc + d;
                const float m = mu[i], l = ls[i];
                const float z = key ? m + expf(l) * n[q] : m;
                out[d] = (T)z;
                acc += 0.5 * (double)n[q] * (double)n[q] - 0.5 * (double)z * (double)z + (double)l;
            }
        }
    }
    for (int j = ldc + K + tid; j < Lpad; j += SW_THREADS) out[j] = (T)0.f;
    int hot = k;
    if (label) {
        const int64_t l = label[b];
        hot = (l >= 0 && l < K) ? (int)l : -1;                  // out of range: no class is set
    }
    for (int c = tid; c < K; c += SW_THREADS) out[ldc + c] = (T)(c == hot ? 1.f : 0.f);
    if (k == 0) {                                               // (block-uniform) the first class row of (b, s) writes lw
        const double t = score_block_sum<SW_THREADS>(acc, sh);
        if (tid == 0) lw[b * S + s] = (float)t;
    }
}

int sv_latent_sweep(int dtype, const float* mu, const float* ls, const int64_t* key, int64_t row0, const int64_t* label, int B, int S,
                    int K, int ldc, int Lpad, int64_t j0, int R, void* latent, float* lw, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(mu && ls, SV_E_ARG, "sv_latent_sweep: mu or ls is NULL");
    SV_REQUIRE(latent && lw, SV_E_ARG, "sv_latent_sweep: an output (latent, lw) is NULL");
    SV_REQUIRE(dtype == SV_F32 || dtype == SV_BF16, SV_E_ARG, "sv_latent_sweep: bad dtype %d", dtype);
    SV_REQUIRE(B > 0 && S > 0 && K > 0 && ldc > 0, SV_E_ARG, "sv_latent_sweep: non-positive size (B=%d S=%d K=%d ldc=%d)", B, S, K, ldc);
    SV_REQUIRE(S <= 65536 && ldc <= (1 << 18), SV_E_SHAPE, "sv_latent_sweep: S=%d > 65536 or ldc=%d > 2^18 (the counter's fields)", S, ldc);
    SV_REQUIRE(Lpad >= ldc + K, SV_E_SHAPE, "sv_latent_sweep: Lpad=%d < ldc + K = %d", Lpad, ldc + K);
    SV_REQUIRE(row0 >= 0, SV_E_ARG, "sv_latent_sweep: row0=%lld must be >= 0", (long long)row0);
    const int Kd = label ? 1 : K;
    const int64_t total = (int64_t)B * S * Kd;
    SV_REQUIRE(R > 0 && j0 >= 0 && j0 + R <= total, SV_E_SHAPE, "sv_latent_sweep: rows [%lld, %lld) outside the sweep's %lld rows",
               (long long)j0, (long long)(j0 + R), (long long)total);
    if (dtype == SV_BF16)
        hipLaunchKernelGGL((latent_sweep_kernel<bf16>), dim3(R), dim3(SW_THREADS), 0, (hipStream_t)stream, mu, ls, key, row0, label, S, Kd,
                           K, ldc, Lpad, j0, (bf16*)latent, lw);
    else
        hipLaunchKernelGGL((latent_sweep_kernel<float>), dim3(R), dim3(SW_THREADS), 0, (hipStream_t)stream, mu, ls, key, row0, label, S, Kd,
                           K, ldc, Lpad, j0, (float*)latent, lw);
    return sv_check_launch("sv_latent_sweep");
}

// ------------------------------------------------------------------------------------------ sv_recon_rows
constexpr int RR_THREADS = 256;

// one block per decoded row; thread t takes pixels t, t + 256, ...: consecutive threads read consecutive pixels of the decoder's NHWC
// output and consecutive floats of each image plane.  Terms in fp32, sums in double.
template <typename T>
__global__ __launch_bounds__(RR_THREADS) void recon_rows_kernel(const T* rec, const float* image, int64_t j0, int64_t rows_per_image,
                                                                int C, int HW, int ld, int bce, double scale, float* nll) {
    __shared__ double sh[RR_THREADS];
    const int64_t j = blockIdx.x;
    const int64_t img = (j0 + j) / rows_per_image;
    const T* src = rec + j * HW * ld;
    const float* x = image + img * C * HW;
    double acc = 0.0;
    for (int p = threadIdx.x; p < HW; p += RR_THREADS) {
        for (int c = 0; c < C; ++c) {
            const float r = to_f(src[(int64_t)p * ld + c]), t = x[(int64_t)c * HW + p];
            float v;
            if (bce) {
                v = fmaxf(r, 0.f) - r * t + log1pf(expf(-fabsf(r)));
            } else {
                const float e = 1.f / (1.f + expf(-r)) - t;     // expf overflows to inf for r < -88.7: the sigmoid is 0, as it should
                v = e * e;
            }
            acc += (double)v;
        }
    }
    const double t = score_block_sum<RR_THREADS>(acc, sh);
    if (threadIdx.x == 0) nll[j] = (float)(t * scale);
}

int sv_recon_rows(int dtype, const void* rec, const float* image, int B, int64_t j0, int R, int64_t rows_per_image, int C, int H, int W,
                  int ld, int bce, float x_sigma, float* nll, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(rec && image && nll, SV_E_ARG, "sv_recon_rows: a pointer (rec, image, nll) is NULL");
    SV_REQUIRE(dtype == SV_F32 || dtype == SV_BF16, SV_E_ARG, "sv_recon_rows: bad dtype %d", dtype);
    SV_REQUIRE(B > 0 && R > 0 && C > 0 && H > 0 && W > 0 && rows_per_image > 0, SV_E_ARG,
               "sv_recon_rows: non-positive size (B=%d R=%d C=%d H=%d W=%d rows_per_image=%lld)", B, R, C, H, W, (long long)rows_per_image);
    SV_REQUIRE(ld >= C, SV_E_SHAPE, "sv_recon_rows: ld=%d < C=%d", ld, C);
    SV_REQUIRE(bce == 0 || bce == 1, SV_E_ARG, "sv_recon_rows: bce flag %d", bce);
    SV_REQUIRE(bce || (x_sigma > 0.f && x_sigma <= 3.0e38f), SV_E_ARG, "sv_recon_rows: x_sigma=%g must be finite and > 0", (double)x_sigma);
    SV_REQUIRE(j0 >= 0 && (j0 + R - 1) / rows_per_image < B, SV_E_SHAPE, "sv_recon_rows: rows [%lld, %lld) reach past image %d",
               (long long)j0, (long long)(j0 + R), B - 1);
    const double scale = bce ? 1.0 : 1.0 / (2.0 * (double)x_sigma * (double)x_sigma);
    if (dtype == SV_BF16)
        hipLaunchKernelGGL((recon_rows_kernel<bf16>), dim3(R), dim3(RR_THREADS), 0, (hipStream_t)stream, (const bf16*)rec, image, j0,
                           rows_per_image, C, H * W, ld, bce, scale, nll);
    else
        hipLaunchKernelGGL((recon_rows_kernel<float>), dim3(R), dim3(RR_THREADS), 0, (hipStream_t)stream, (const float*)rec, image, j0,
                           rows_per_image, C, H * W, ld, bce, scale, nll);
    return sv_check_launch("sv_recon_rows");
}

// ------------------------------------------------------------------------------------------ sv_score_reduce
constexpr int SR_THREADS = 256;

// (ScoreLse, score_lse_merge and score_lse_value -- the log-sum-exp state -- are in common.h: aggpost.hip merges with them too)

// one block per image
__global__ __launch_bounds__(SR_THREADS) void score_reduce_kernel(const float* nll, const float* lw, const float* la, const float* mu,
                                                                  const float* ls, int S, int Kd, int K, int ldc, double log_px_add,
                                                                  float* recon, float* kl_c, float* kl_d, float* elbo, float* log_px) {
    __shared__ double sh[SR_THREADS];
    __shared__ ScoreLse shl[SR_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* t = nll + (int64_t)b * S * Kd;
    const float* lab = la + (int64_t)b * K;
    const double logK = log((double)K);
    const bool need_terms = recon || elbo;
    if (kl_c || elbo || kl_d || recon) {
        double c = 0.0, d = 0.0, r = 0.0;
        if (kl_c || elbo)
            for (int i = tid; i < ldc; i += SR_THREADS) {
                const double m = mu[(int64_t)b * ldc + i], l = ls[(int64_t)b * ldc + i];
                c += m * m + exp(2.0 * l) - 2.0 * l - 1.0;
            }
        if (kl_d || elbo)
            for (int k = tid; k < K; k += SR_THREADS) {
                const double l = lab[k], q = exp(l);
                if (!(q == 0.0)) d += q * (l + logK);               // q = 0: the term's limit, 0; a NaN la propagates
            }
        if (need_terms)
            for (int64_t i = tid; i < (int64_t)S * Kd; i += SR_THREADS) {
                if (Kd == 1) {
                    r += (double)t[i];
                } else {
                    const double q = exp((double)lab[i % Kd]);
                    if (!(q == 0.0)) r += q * (double)t[i];         // a class of probability 0 is skipped: no 0 * inf
                }
            }
        c = 0.5 * score_block_sum<SR_THREADS>(c, sh);
        d = score_block_sum<SR_THREADS>(d, sh);
        r = score_block_sum<SR_THREADS>(r, sh) / (double)S;
        if (tid == 0) {
            if (recon) recon[b] = (float)r;
            if (kl_c) kl_c[b] = (float)c;
            if (kl_d) kl_d[b] = (float)d;
            if (elbo) elbo[b] = (float)(-(r + c + d));
        }
    }
    if (log_px) {
        // inner: LSE over the classes of one sample (a thread per sample, classes in index order); outer: over the samples
        ScoreLse o{-INFINITY, 0.0};
        for (int s = tid; s < S; s += SR_THREADS) {
            double inner;
            if (Kd == 1) {
                inner = -(double)t[s];
            } else {
                ScoreLse in{-INFINITY, 0.0};
                for (int k = 0; k < Kd; ++k) in = score_lse_merge(in, ScoreLse{-(double)t[(int64_t)s * Kd + k] - logK, 1.0});
                inner = score_lse_value(in);
            }
            o = score_lse_merge(o, ScoreLse{(double)lw[(int64_t)b * S + s] + inner, 1.0});
        }
        shl[tid] = o;
        __syncthreads();
        for (int w = SR_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) shl[tid] = score_lse_merge(shl[tid], shl[tid + w]);
            __syncthreads();
        }
        if (tid == 0) log_px[b] = (float)(score_lse_value(shl[0]) - log((double)S) + log_px_add);
    }
}

int sv_score_reduce(const float* nll, const float* lw, const float* la, const float* mu, const float* ls, int B, int S, int Kd, int K,
                    int ldc, double log_px_add, float* recon, float* kl_c, float* kl_d, float* elbo, float* log_px, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(nll && la && mu && ls, SV_E_ARG, "sv_score_reduce: an input (nll, la, mu, ls) is NULL");
    SV_REQUIRE(recon || kl_c || kl_d || elbo || log_px, SV_E_ARG, "sv_score_reduce: no output (all five are NULL)");
    SV_REQUIRE(!log_px || lw, SV_E_ARG, "sv_score_reduce: log_px needs lw");
    SV_REQUIRE(B > 0 && S > 0 && Kd > 0 && K > 0 && ldc > 0, SV_E_ARG, "sv_score_reduce: non-positive size (B=%d S=%d Kd=%d K=%d ldc=%d)",
               B, S, Kd, K, ldc);
    SV_REQUIRE(Kd == 1 || Kd == K, SV_E_SHAPE, "sv_score_reduce: Kd=%d must be 1 (labelled) or K=%d (the class sweep)", Kd, K);
    SV_REQUIRE(log_px_add == log_px_add && log_px_add > -INFINITY && log_px_add < INFINITY, SV_E_ARG,
               "sv_score_reduce: log_px_add must be finite");
    hipLaunchKernelGGL(score_reduce_kernel, dim3(B), dim3(SR_THREADS), 0, (hipStream_t)stream, nll, lw, la, mu, ls, S, Kd, K, ldc,
                       log_px_add, recon, kl_c, kl_d, elbo, log_px);
    return sv_check_launch("sv_score_reduce");
}
