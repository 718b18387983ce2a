// Inference-side entry points of the SHOT-VAE (declared, with the exact definitions, in include/shotvae_hip.h):
//   sv_latent_draw  the decoder's input [z | c | 0-pad] from a counter-based normal stream and a class code
//   sv_image_out    the decoder's NHWC output -> NCHW fp32 (logits or sigmoid) and / or NHWC uint8 pixels
// Plain HIP C++; both take a stream, allocate nothing and read their key from device memory: capturable.
#include "common.h"
#include <math.h>

// ------------------------------------------------------------------------------------------ sv_latent_draw
// the four standard normals of columns 4j .. 4j + 3 of absolute row `row` (shotvae_hip.h: the stream's definition)
__device__ __forceinline__ void latent_normals4(uint64_t key, uint64_t row, uint32_t j, float n[4]) {
    sv_normals4(key, row, j, SV_LATENT_PHILOX_TAG, n);
}

constexpr int LD_THREADS = 128;

// (value, index) order of the argmax: the larger value, on a tie the lower index; a NaN never wins
__device__ __forceinline__ bool latent_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// one block per row
template <typename T>
__global__ __launch_bounds__(LD_THREADS) void latent_draw_kernel(const float* mu, const float* ls, const int64_t* key, float tau,
                                                                 int64_t row0, int mode, const int64_t* label, const float* cls,
                                                                 int ldc, int K, int Lpad, T* latent, float* z_out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    T* out = latent + (int64_t)b * Lpad;
    const uint64_t k = key ? (uint64_t)key[0] : 0u;
    const uint64_t row = (uint64_t)(row0 + b);
    for (int j = tid; 4 * j < ldc; j += LD_THREADS) {
        float n[4] = {0.f, 0.f, 0.f, 0.f};
        if (key) latent_normals4(k, row, (uint32_t)j, n);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = 4 * j + q;
            if (d < ldc) {
                const int64_t i = (int64_t)b * ldc + d;
                const float m = mu ? mu[i] : 0.f;
                const float z = key ? m + (tau * (ls ? expf(ls[i]) : 1.f)) * n[q] : m;
                out[d] = (T)z;
                if (z_out) z_out[i] = z;
            }
        }
    }
    for (int j = ldc + K + tid; j < Lpad; j += LD_THREADS) out[j] = (T)0.f;
    if (mode == 1) {
        for (int c = tid; c < K; c += LD_THREADS) out[ldc + c] = (T)cls[(int64_t)b * K + c];
        return;
    }
    int hot;
    if (mode == 0) {
        const int64_t l = label[b];
        hot = (l >= 0 && l < K) ? (int)l : -1;                  // out of range: no class is set
    } else {
        __shared__ float sv[LD_THREADS];
        __shared__ int si[LD_THREADS];
        float bv = -INFINITY;
        int bi = K;
        for (int c = tid; c < K; c += LD_THREADS) {
            const float v = cls[(int64_t)b * K + c];
            if (latent_better(v, c, bv, bi)) { bv = v; bi = c; }
        }
        sv[tid] = bv;
        si[tid] = bi;
        __syncthreads();
        for (int s = LD_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s && latent_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) { sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; }
            __syncthreads();
        }
        hot = si[0] < K ? si[0] : -1;                           // a row of NaNs only: no class is set
    }
    for (int c = tid; c < K; c += LD_THREADS) out[ldc + c] = (T)(c == hot ? 1.f : 0.f);
}

int sv_latent_draw(int dtype, const float* mu, const float* ls, const int64_t* key, float tau, int64_t row0, int mode,
                   const int64_t* label, const float* cls, int B, int ldc, int K, int Lpad, void* latent, float* z_out,
                   void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(latent, SV_E_ARG, "sv_latent_draw: latent is NULL");
    SV_REQUIRE(dtype == SV_F32 || dtype == SV_BF16, SV_E_ARG, "sv_latent_draw: bad dtype %d", dtype);
    SV_REQUIRE(B > 0 && ldc > 0 && K > 0, SV_E_ARG, "sv_latent_draw: non-positive size (B=%d ldc=%d K=%d)", B, ldc, K);
    SV_REQUIRE(Lpad >= ldc + K, SV_E_SHAPE, "sv_latent_draw: Lpad=%d < ldc + K = %d", Lpad, ldc + K);
    SV_REQUIRE(mode >= 0 && mode <= 2, SV_E_ARG, "sv_latent_draw: unknown class mode %d", mode);
    SV_REQUIRE(mode != 0 || label, SV_E_ARG, "sv_latent_draw: mode 0 needs the labels");
    SV_REQUIRE(mode == 0 || cls, SV_E_ARG, "sv_latent_draw: mode %d needs the class rows", mode);
    SV_REQUIRE(tau >= 0.f && tau <= 3.0e38f, SV_E_ARG, "sv_latent_draw: tau=%g must be finite and >= 0", (double)tau);
    SV_REQUIRE(row0 >= 0, SV_E_ARG, "sv_latent_draw: row0=%lld must be >= 0", (long long)row0);
    if (dtype == SV_BF16)
        hipLaunchKernelGGL((latent_draw_kernel<bf16>), dim3(B), dim3(LD_THREADS), 0, (hipStream_t)stream, mu, ls, key, tau, row0, mode,
                           label, cls, ldc, K, Lpad, (bf16*)latent, z_out);
    else
        hipLaunchKernelGGL((latent_draw_kernel<float>), dim3(B), dim3(LD_THREADS), 0, (hipStream_t)stream, mu, ls, key, tau, row0, mode,
                           label, cls, ldc, K, Lpad, (float*)latent, z_out);
    return sv_check_launch("sv_latent_draw");
}

// ------------------------------------------------------------------------------------------ sv_image_out
// one thread per pixel: its C channels are consecutive in the source and in the uint8 output, and the threads of a wave write
// consecutive floats of each fp32 plane
template <typename T>
__global__ __launch_bounds__(256) void image_out_kernel(const T* in, int64_t npix, int C, int HW, int ld, int sigmoid, float* out_f32,
                                                        uint8_t* out_u8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // over B * HW
    if (i >= npix) return;
    const int64_t b = i / HW, p = i - b * HW;
    const T* src = in + i * ld;
    if (!sigmoid && !out_u8) {                                            // raw logits only: a layout change, no transcendental
        for (int c = 0; c < C; ++c) out_f32[(b * C + c) * HW + p] = to_f(src[c]);
        return;
    }
    for (int c = 0; c < C; ++c) {
        const float x = to_f(src[c]);
        const float s = 1.f / (1.f + expf(-x));
        if (out_f32) out_f32[(b * C + c) * HW + p] = sigmoid ? s : x;
        if (out_u8) out_u8[i * C + c] = (uint8_t)floorf(255.f * s + 0.5f);
    }
}

int sv_image_out(int dtype, const void* in, int B, int C, int H, int W, int ld, int sigmoid, float* out_f32, uint8_t* out_u8,
                 void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(in, SV_E_ARG, "sv_image_out: input is NULL");
    SV_REQUIRE(out_f32 || out_u8, SV_E_ARG, "sv_image_out: no output (fp32 NCHW and uint8 NHWC are both NULL)");
    SV_REQUIRE(dtype == SV_F32 || dtype == SV_BF16, SV_E_ARG, "sv_image_out: bad dtype %d", dtype);
    SV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, SV_E_ARG, "sv_image_out: non-positive size (B=%d C=%d H=%d W=%d)", B, C, H, W);
    SV_REQUIRE(ld >= C, SV_E_SHAPE, "sv_image_out: ld=%d < C=%d", ld, C);
    SV_REQUIRE(sigmoid == 0 || sigmoid == 1, SV_E_ARG, "sv_image_out: sigmoid flag %d", sigmoid);
    const int64_t npix = (int64_t)B * H * W;
    SV_REQUIRE((npix + 255) / 256 <= 0x7fffffff, SV_E_SHAPE, "sv_image_out: too many pixels");
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (dtype == SV_BF16)
        hipLaunchKernelGGL((image_out_kernel<bf16>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)in, npix, C, H * W, ld, sigmoid,
                           out_f32, out_u8);
    else
        hipLaunchKernelGGL((image_out_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (const float*)in, npix, C, H * W, ld, sigmoid,
                           out_f32, out_u8);
    return sv_check_launch("sv_image_out");
}
