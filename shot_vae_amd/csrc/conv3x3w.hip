// Wide stride-1 3x3 convolution (forward and data gradient), bf16, MFMA-bound shapes (Cin >= 96: the WRN-28-10
// body convs 160/320/640 channels, reference shot_vae_model/wideresnet.py:29-35).  gfx950.
//
// conv3x3.hip's tiles (32 pixels x 80 channels per wave) read ~7 LDS fragments per 10 MFMAs: LDS-bound on these
// layers.  This kernel is built like a large-tile GEMM instead:
//   * block = 256 output pixels (whole image rows) x 32*NF output channels, 4 waves; every wave owns 64 pixels x
//     32*NF channels = 2 x NF accumulators of v_mfma_f32_32x32x16_bf16 (weights = A operand, pixels = B operand)
//     -> 14 fragment reads per 20 MFMAs;
//   * TWO blocks per CU (<= 80 KB of LDS, <= 256 registers): one block's prologue, epilogue (HBM-bound: residual /
//     raw-tensor reads + output stores) and barrier waits run under the other block's MFMAs;
//   * K loop = (32-channel chunk) x (9 taps).  The input halo of a chunk is staged ONCE by LDS-DMA, raw, two buffers;
//     BatchNorm-apply + LeakyReLU + zero padding are applied IN PLACE (LDS->LDS, spread over the MFMA steps of the
//     previous chunk) and the tile then serves all nine taps (tap shift = immediate LDS offset);
//   * the [32*NF][32] weight slice of every (chunk, tap) step arrives by LDS-DMA (global_load_lds_dwordx4) two steps
//     ahead into a ring of three buffers; one raw s_barrier per step with counted vmcnt (the DMA queue is never
//     drained inside the loop);
//   * both LDS images are lane-linear (an LDS-DMA requirement) with 64-byte rows; the 16-byte k-quarter inside a row
//     is XOR-swizzled on the DMA SOURCE address -- weights by (row/4)%4, pixels by a function of the halo column --
//     which makes every ds_read_b128 fragment read conflict-free (checked by brute force for W = 32, 16, 8);
//   * epilogue per 32-channel group through a wave-private LDS transpose: 16-byte coalesced residual / raw-tensor
//     reads and output stores, BatchNorm sums (or activation-backward + BatchNorm-backward sums) in registers.
// Same sv_geom / packed weights / sv_igemm_args contract as the other conv-like kernels.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "common.h"

#ifndef SV_W3_EPD
#define SV_W3_EPD 1
#endif

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* glb_ptr;

__device__ __forceinline__ void glds16(const void* gsrc, void* ldst) {
    __builtin_amdgcn_global_load_lds((glb_ptr)gsrc, (lds_ptr)ldst, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const void* gsrc, void* ldst) {
    __builtin_amdgcn_global_load_lds((glb_ptr)gsrc, (lds_ptr)ldst, 4, 0, 0);
}
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void barrier() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

template <int NF, int WLOG>
struct WCfg {
    static constexpr int BN = 32 * NF;
    static constexpr int W = 1 << WLOG, TR = 256 / W, WP = W + 2;
    static constexpr int HH = TR < W ? TR : W, SEG = TR / HH, LROWS = TR + SEG + 1;   // images are square
    static constexpr int HPIX = LROWS * WP;                 // halo pixels (incl. padding columns / spacer rows)
    static constexpr int HS = 4 * HPIX;                     // 16-byte slots of one halo buffer (64 B per pixel)
    static constexpr int HI = (HS + 255) / 256;             // DMA instructions / transform slots per thread
    static constexpr int HB = HS * 16;                      // bytes per halo buffer
    static constexpr int SWS = WLOG == 5 ? 2 : 1;           // pixel swizzle: k-quarter ^= (halo column >> SWS) & 3
    static constexpr int WS = 4 * BN;                       // 16-byte slots of one weight buffer
    static constexpr int WI = (WS + 255) / 256;
    static constexpr int WBUF = WS * 16;
    static constexpr int OFF_W = 2 * HB, OFF_CO = OFF_W + 3 * WBUF,
                         OFF_SSUM = OFF_CO + 2048;
    // channel sums: one copy per wave (no LDS float atomics: the block adds the copies in a fixed order and is the only adder of
    // its replica in deterministic mode).  Where four copies behind the buffers would cost the second block per CU (160-channel
    // tiles at 8 x 8) copies 0..2 lie over the tail of the -- by then dead -- weight / coefficient buffers
    static constexpr bool WS_ALIAS = 2 * (OFF_SSUM + 4 * 2 * BN * 4) > 160 * 1024;
    static constexpr int OFF_WSUM = WS_ALIAS ? OFF_SSUM - 3 * 2 * BN * 4 : OFF_SSUM, LDS = OFF_WSUM + 4 * 2 * BN * 4;
    static constexpr int SCR = 64 * 36 * 4;                 // epilogue transpose scratch per wave
    static_assert(4 * SCR + 4 * 4096 + 5 * BN * 4 <= OFF_WSUM, "epilogue scratch must fit in the halo + weight + coefficient buffers");
    static_assert(HI <= 6, "transform schedule covers at most 6 slots per thread");
    static_assert(2 * LDS <= 160 * 1024, "two blocks per CU");
};

// MODE: the epilogue's fusion flags at compile time (conv3x3w_epilogue.inc: 0 = from the arguments, 1 = statistics,
// 2 = residual + statistics, 3 = activation-backward)
template <int NF, int WLOG, bool REV, int MODE>
__global__ __launch_bounds__(256, 2) void conv3x3w_kernel(const sv_geom g, const sv_igemm_args_g AG) {
    const sv_igemm_args& a = AG.g[blockIdx.y];
    sv_start_signal(a);
    using C = WCfg<NF, WLOG>;
    constexpr int BN = C::BN, W = C::W, TR = C::TR, WP = C::WP, HH = C::HH, SEG = C::SEG, HI = C::HI, WI = C::WI;
    constexpr int HS = C::HS, HB = C::HB, WS = C::WS, WBUF = C::WBUF, SWS = C::SWS;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const ssum = reinterpret_cast<float*>(smem + C::OFF_WSUM);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);        // scalar: DMA destinations stay in SGPRs
    const int r = lane & 31, h = lane >> 5;
    const int H = g.Hin, BH = g.B * H, nT = BH / TR, nNt = g.N / BN;
    const int Cin = g.Cin, nck = Cin / 32, KT = 9 * nck;

    // XCD-affine mapping: the 32 CUs of an XCD work on consecutive pixel tiles (shared halo rows and one copy of the
    // weights in that XCD's L2); the channel tiles of a pixel tile are neighbours on the same XCD
    const int per = (nT + 7) >> 3;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int in_i = slot % nNt, mt = xcd * per + slot / nNt;
    if (mt >= nT) return;
    const int n0 = in_i * BN, gr0 = mt * TR;

    const sv_phase& P = g.phase[0];
    const char* const Xb = reinterpret_cast<const char*>(a.x);
    const char* const Wb = reinterpret_cast<const char*>(reinterpret_cast<const bf16*>(a.w) + P.w_off + (int64_t)n0 * 9 * Cin);
    const bool has_pro = a.pro_scale != nullptr;
    const float slope = has_pro ? a.pro_slope : 1.f;
    // BatchNorm coefficients of a chunk: one 4-byte DMA per wave (lanes 0..31 scale, 32..63 shift) into the wave's own
    // 256-byte copy; without a prologue every wave reads the identity from a constant image instead
    // (without a prologue the same DMA is issued from a dummy source, so every wave's vmcnt arithmetic is the same,
    // and the transform only writes the padding zeros)
    const char* const sclo = reinterpret_cast<const char*>(a.pro_scale < a.pro_shift ? a.pro_scale : a.pro_shift);
    const char* const cob = has_pro ? sclo : Xb;               // uniform base + one 32-bit per-lane offset
    const uint32_t cooff = has_pro ? (lane < 32 ? (uint32_t)(reinterpret_cast<const char*>(a.pro_scale) - sclo) + 4u * lane
                                                : (uint32_t)(reinterpret_cast<const char*>(a.pro_shift) - sclo) + 4u * (lane - 32))
                                   : 4u * lane;
    const uint32_t costep = has_pro ? 128u : 0u;


    // ---- DMA slots (uniform instruction count per wave: the last, partial wave-instruction is shifted back so that it
    //      ends at the end of the image and re-copies a few slots -- same source, same destination) -----------------
    uint32_t hsrc[HI];          // byte offset into x (channel chunk 0)
    int hbase[HI];              // wave-uniform first slot of DMA instruction j
#pragma unroll
    for (int j = 0; j < HI; ++j) {
        hbase[j] = min((j * 4 + wave) * 64, HS - 64);
        const int s = hbase[j] + lane, pix = s >> 2;
        const int lr = pix / WP, xx = pix - lr * WP;
        const int q = (s & 3) ^ ((xx >> SWS) & 3);
        const int seg = lr / (HH + 1), off = lr - seg * (HH + 1);
        int rel = lr - 1 - seg;
        if (off == 0 && SEG == 1) rel = seg == 0 ? -1 : TR;
        const int grc = min(max(gr0 + rel, 0), BH - 1), xc = min(max(xx - 1, 0), W - 1);
        hsrc[j] = (uint32_t)((grc * W + xc) * g.ldx + 8 * q) * 2u;
    }
    uint32_t wsrc[WI];
    int wbase[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        wbase[i] = min((i * 4 + wave) * 64, WS - 64);
        const int s = wbase[i] + lane, row = s >> 2, q = (s & 3) ^ ((row >> 2) & 3);
        wsrc[i] = (uint32_t)(row * 9 * Cin + 8 * q) * 2u;
    }
    auto issue_h = [&](int c, int buf) {
#pragma unroll
        for (int j = 0; j < HI; ++j) {
            uint32_t o = hsrc[j];
            asm volatile("" : "+v"(o));                           // (keeps the per-tap sums out of loop-invariant hoisting)
            o += (uint32_t)(c * 64);                              // one 32-bit offset: SGPR base + VGPR offset form
            glds16(Xb + o, smem + buf * HB + hbase[j] * 16);
        }
        {
            uint32_t o = cooff;
            asm volatile("" : "+v"(o));
            o += costep * (uint32_t)c;
            glds4(cob + o, smem + C::OFF_CO + (c & 1) * 1024 + wave * 256);
        }
    };
    auto issue_w = [&](int c, int t, int buf) {
        const uint32_t o = (uint32_t)(t * Cin + c * 32) * 2u;
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            uint32_t oo = wsrc[i];
            asm volatile("" : "+v"(oo));
            oo += o;
            glds16(Wb + oo, smem + C::OFF_W + buf * WBUF + wbase[i] * 16);
        }
    };
    // ---- in-place transform slots: thread handles slots 256 j + tid (a partition of the image) ----------------------
    uint32_t hokm = 0;          // bit j: slot j is a real pixel (else: zero padding / spacer)
    uint32_t qcm = 0;           // 2 bits per j: logical k-quarter (8-channel group) of slot j
    {
        const bool top_ok = (gr0 & (H - 1)) != 0, bot_ok = ((gr0 + TR) & (H - 1)) != 0;
#pragma unroll
        for (int j = 0; j < HI; ++j) {
            const int s = 256 * j + tid, pix = s >> 2;
            const int lr = pix / WP, xx = pix - lr * WP;
            const int seg = lr / (HH + 1), off = lr - seg * (HH + 1);
            int kind = 1;
            if (off == 0) kind = SEG == 1 ? (seg == 0 ? 2 : 3) : 0;
            if (xx == 0 || xx == WP - 1) kind = 0;
            if (kind == 1 || (kind == 2 && top_ok) || (kind == 3 && bot_ok)) hokm |= 1u << j;
            qcm |= (uint32_t)((s & 3) ^ ((xx >> SWS) & 3)) << (2 * j);
        }
    }
    auto transform = [&](int c, auto jc, int buf) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        if (256 * j + tid < HS) {
            int toff = 16 * tid;
            asm volatile("" : "+v"(toff));                         // (not hoisted: one address register, not HI)
            bf16x8* ptr = reinterpret_cast<bf16x8*>(smem + buf * HB + 4096 * j + toff);
            if (has_pro) {
                uint32_t qm = qcm;
                asm volatile("" : "+v"(qm));
                const float* co = reinterpret_cast<const float*>(smem + C::OFF_CO + (c & 1) * 1024 + wave * 256) +
                                  8 * ((qm >> (2 * j)) & 3);
                const bool ok = (hokm >> j) & 1u;
                typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));
                typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {               // four channels at a time: few live registers
                    const f32x4 sc = *reinterpret_cast<const f32x4*>(co + 4 * hf);
                    const f32x4 sh = *reinterpret_cast<const f32x4*>(co + 32 + 4 * hf);
                    uint2* p4 = reinterpret_cast<uint2*>(ptr) + hf;
                    const uint2 v = *p4;
                    // bf16 -> f32 is a shift / mask of the packed word
                    const float x0 = __uint_as_float(v.x << 16), x1 = __uint_as_float(v.x & 0xffff0000u);
                    const float x2 = __uint_as_float(v.y << 16), x3 = __uint_as_float(v.y & 0xffff0000u);
                    const float u0 = x0 * sc[0] + sh[0], u1 = x1 * sc[1] + sh[1];
                    const float u2 = x2 * sc[2] + sh[2], u3 = x3 * sc[3] + sh[3];
                    const f32x2 a01 = {fmaxf(u0, u0 * slope), fmaxf(u1, u1 * slope)};   // LeakyReLU (0.01) / ReLU (0)
                    const f32x2 a23 = {fmaxf(u2, u2 * slope), fmaxf(u3, u3 * slope)};
                    const bf16x2 b01 = __builtin_convertvector(a01, bf16x2), b23 = __builtin_convertvector(a23, bf16x2);
                    uint2 o;
                    o.x = ok ? *reinterpret_cast<const uint32_t*>(&b01) : 0u;          // packed select: padding stays zero
                    o.y = ok ? *reinterpret_cast<const uint32_t*>(&b23) : 0u;
                    *p4 = o;
                }
            } else if (!((hokm >> j) & 1u)) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(ptr) = z;
            }
        }
    };

    // ---- fragment addressing -----------------------------------------------------------------------------------
    // pixel fragments: 64 * (pixel - one halo row - one column) + 16 * (lane half ^ swizzle of the tap's column); the tap
    // shift and the halo buffer are immediates; the second k half is the same address ^ 32
    int bb[2], pc[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int p = 64 * wave + 32 * f + r, prow = p >> WLOG;
        pc[f] = p & (W - 1);
        bb[f] = ((prow + prow / HH) * WP + pc[f]) * 64;
    }
    int ab0 = C::OFF_W + 16 * (4 * r + (h ^ ((r >> 2) & 3)));           // k half 0 (channels 0..15)
    int ab1 = C::OFF_W + 16 * (4 * r + ((2 + h) ^ ((r >> 2) & 3)));     // k half 1 (channels 16..31)
    asm volatile("" : "+v"(ab0), "+v"(ab1));      // opaque bases: ring slot / fragment index stay 16-bit immediates

    bf16x8 A[2][NF], Bf[2][2];
    f32x16 acc[2][NF];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[f][i][e] = 0.f;

    auto load_frags = [&](auto tc, auto parc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value, par = decltype(parc)::value;
        constexpr int ty = REV ? 2 - t / 3 : t / 3, tx = REV ? 2 - t % 3 : t % 3;
        constexpr int sh = (ty * WP + tx) * 64 + par * HB;
        constexpr int wo = (t % 3) * WBUF;
#pragma unroll
        for (int i = 0; i < NF; ++i) A[0][i] = *reinterpret_cast<const bf16x8*>(smem + ab0 + wo + i * 2048);
        int bx[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            int pcf = pc[f];
            asm volatile("" : "+v"(pcf));        // recompute the swizzle here: hoisted out of the loop, the 12 addresses
                                                  // of all tap columns would not fit in the 256-register budget
            bx[f] = bb[f] + 16 * (h ^ (((pcf + tx) >> SWS) & 3));
            Bf[0][f] = *reinterpret_cast<const bf16x8*>(smem + bx[f] + sh);
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) A[1][i] = *reinterpret_cast<const bf16x8*>(smem + ab1 + wo + i * 2048);
#pragma unroll
        for (int f = 0; f < 2; ++f) Bf[1][f] = *reinterpret_cast<const bf16x8*>(smem + (bx[f] ^ 32) + sh);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;

    // ---- prologue ---------------------------------------------------------------------------------------------
    if (has_pro && a.fold_stats) {
        // the BatchNorm in front of this layer has not been finalised (sv_igemm_args::fold_*): every block derives the
        // coefficients from the raw statistics itself and stores them -- all blocks the same values -- where the chunk DMAs
        // below read them (the halo buffers are free until the first DMA; the block's stores and its later loads take the
        // same path through the CU's vector cache to L2, in order)
        float* fs = reinterpret_cast<float*>(smem);
        sv_bn_fold_block<256, false>(a, Cin, reinterpret_cast<double*>(smem), fs + 1024, fs + 1024 + Cin, true);
        __threadfence_block();
    }
    __syncthreads();                                   // ssum / identity coefficients visible (no DMA in flight yet)
    issue_h(0, 0);
    issue_w(0, 0, 0);
    issue_w(0, 1, 1);
    wait_vm<0>();
    barrier();                                         // every wave's DMA has landed
    transform(0, I0{}, 0);
    if (HI > 1) transform(0, std::integral_constant<int, (HI > 1 ? 1 : 0)>{}, 0);
    if (HI > 2) transform(0, std::integral_constant<int, (HI > 2 ? 2 : 0)>{}, 0);
    if (HI > 3) transform(0, std::integral_constant<int, (HI > 3 ? 3 : 0)>{}, 0);
    if (HI > 4) transform(0, std::integral_constant<int, (HI > 4 ? 4 : 0)>{}, 0);
    if (HI > 5) transform(0, std::integral_constant<int, (HI > 5 ? 5 : 0)>{}, 0);
    wait_lds();
    barrier();

    // ---- one (chunk, tap) step: weights of step k live in ring slot k % 3 = t % 3 ---------------------------------------
    auto step = [&](int c, auto tc, auto parc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value, par = decltype(parc)::value;
        const int k = c * 9 + t;
        const bool more_c = c + 1 < nck;
        const bool w_issue = k + 2 < KT;
        // (1) asynchronous copies: weights two steps ahead (into the slot step k-1 released), the next chunk's raw halo
        //     and BatchNorm coefficients at the chunk's first step
        if (w_issue) issue_w(c + (t + 2) / 9, (t + 2) % 9, (t + 2) % 3);
        if (t == 0 && more_c) issue_h(c + 1, par ^ 1);
        // (2) this step's fragments
        load_frags(tc, parc);
        // (3) BatchNorm-apply + LeakyReLU + padding of the next chunk's halo, in place, spread over steps 3..7
        //     (unconditional: after the last chunk it rewrites an unused buffer)
        if (t >= 3 && t <= 7) {
            const int cn = min(c + 1, nck - 1);
            if (t == 3) {
                transform(cn, I0{}, par ^ 1);
                if (HI > 1) transform(cn, std::integral_constant<int, (HI > 1 ? 1 : 0)>{}, par ^ 1);
            } else if (t - 2 < HI) {
                transform(cn, std::integral_constant<int, (t - 2 < HI ? (t >= 4 ? t - 2 : 0) : 0)>{}, par ^ 1);
            }
        }
        // (4) this step's 4 NF MFMAs
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int i = 0; i < NF; ++i)
                    acc[f][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[ks][i], Bf[ks][f], acc[f][i], 0, 0, 0);
        // (5) the weights of step k+1 must have landed; everything issued after them may stay in flight: this step's
        //     weights, and the raw halo (+ coefficients) for two more steps
        const bool h_fly = t <= 1 && more_c;
        if (w_issue) {
            if (h_fly) wait_vm<WI + HI + 1>(); else wait_vm<WI>();
        } else {
            if (h_fly) wait_vm<HI + 1>(); else wait_vm<0>();
        }
        wait_lds();
        barrier();
    };
    auto chunk = [&](int c, auto parc) __attribute__((always_inline)) {
        step(c, std::integral_constant<int, 0>{}, parc);
        step(c, std::integral_constant<int, 1>{}, parc);
        step(c, std::integral_constant<int, 2>{}, parc);
        step(c, std::integral_constant<int, 3>{}, parc);
        step(c, std::integral_constant<int, 4>{}, parc);
        step(c, std::integral_constant<int, 5>{}, parc);
        step(c, std::integral_constant<int, 6>{}, parc);
        step(c, std::integral_constant<int, 7>{}, parc);
        step(c, std::integral_constant<int, 8>{}, parc);
    };
    for (int c = 0; c < nck; c += 2) {
        chunk(c, I0{});
        if (c + 1 < nck) chunk(c + 1, I1{});
    }

    constexpr int SV_EPD = SV_W3_EPD;
#define SV_EPI_NSCR 1
#define SV_EPI_BASE 0
#define SV_EPI_ALIAS 0
#define SV_EPI_MODE MODE
#define SV_EPI_WAVE_SUMS 1
#include "conv3x3w_epilogue.inc"
#undef SV_EPI_MODE
#undef SV_EPI_WAVE_SUMS
#undef SV_EPI_NSCR
#undef SV_EPI_BASE
#undef SV_EPI_ALIAS
}

template <int NF, int WLOG, bool REV, int MODE>
int launch_w4(const sv_geom* g, const sv_igemm_args* a, hipStream_t s) {
    using C = WCfg<NF, WLOG>;
    const int nT = g->B * g->Hin / C::TR, nNt = g->N / C::BN;
    const int grid = 8 * ((nT + 7) / 8) * nNt;
    const size_t lds = (size_t)C::LDS;
    static bool optin = false;
    if (const int rc = sv_lds_optin(optin, (int)lds, "conv3x3w", &conv3x3w_kernel<NF, WLOG, REV, MODE>)) return rc;
    // BatchNorm finalisation folded into this launch: the blocks sum the replicas themselves (256 threads = 256 / Cin parts)
    const sv_igemm_args b = sv_fold_resolve(*a, a->fold_stats && 256 % g->Cin == 0 && a->fold_replicas <= 64 && (size_t)(1024 + 2 * g->Cin) * 4 <= (size_t)C::HB);
    // (deterministic mode: a replica per block -- the gate checks replicas >= 4 * grid)
    return sv_igemm_launch(&conv3x3w_kernel<NF, WLOG, REV, MODE>, grid, 256, lds, g, &b, 2, s, "sv_igemm(conv3x3w)");
}

// the 128-channel tiles at 8 x 8 (the last stage of WRN-28-2, 14 launches per step) take the binaries with their fusion flags
// at compile time; every other shape / flag combination the run-time-flag binary
template <int NF, int WLOG, bool REV>
int launch_w3(const sv_geom* g, const sv_igemm_args* a, hipStream_t s) {
    if constexpr (NF == 4 && WLOG == 3) {
        if (!a->bias) {
            if constexpr (REV) {
                if (a->ex && !a->residual) return launch_w4<NF, WLOG, REV, 3>(g, a, s);
            } else {
                if (a->stats && a->residual && !a->ex) return launch_w4<NF, WLOG, REV, 2>(g, a, s);
                if (a->stats && !a->residual && !a->ex) return launch_w4<NF, WLOG, REV, 1>(g, a, s);
            }
        }
    }
    return launch_w4<NF, WLOG, REV, 0>(g, a, s);
}

template <int NF, bool REV>
int launch_w2(const sv_geom* g, const sv_igemm_args* a, hipStream_t s) {
    switch (g->Win) {
        case 32: return launch_w3<NF, 5, REV>(g, a, s);
        case 16: return launch_w3<NF, 4, REV>(g, a, s);
        default: return launch_w3<NF, 3, REV>(g, a, s);
    }
}

}  // namespace

// Returns 1 and sets *rc when the geometry is a wide bf16 stride-1 3x3 convolution this kernel covers.
// (The caller, sv_conv3x3_try, has already checked the generic stride-1 3x3 / square-image conditions.)
int sv_conv3x3w_try(const sv_geom* g, int dtype, const sv_igemm_args* a, hipStream_t s, int* rc) {
    if (sv_disabled(SV_K_CONV3X3W) || dtype != SV_BF16) return 0;
    if (g->Cin < 96 || g->Cin % 32 != 0 || g->ldx % 8 != 0 || g->ldo % 8 != 0) return 0;
    if (g->N % 160 != 0 && g->N % 64 != 0) return 0;
    const int TR = 256 / g->Win;
    if ((g->B * g->Hin) % TR != 0) return 0;
    // 256-pixel x 160/128/64-channel tiles: below one block per CU the small-tile kernels of conv3x3.hip are faster
    // (measured: WRN-28-2 stage 3 as 128 blocks of 128 channels, 38 vs 24 us); sv_set_option(SV_OPT_WIDE_MIN_BLOCKS) moves
    // the bound (tests use 1 to reach these kernels at small batch sizes).
    // Narrower channel tiles are taken only when the wider ones do not fill the chip.
    const int min_blocks = sv_wide_min_blocks();
    const int64_t nTiles = (int64_t)g->B * g->Hin / TR * sv_ngroups(a->groups);      // of the whole (batched) launch
    int bn = 0;
    if (g->N % 160 == 0) bn = 160;
    else if (g->N % 128 == 0 && nTiles * (g->N / 128) >= min_blocks) bn = 128;
    else if (nTiles * (g->N / 64) >= min_blocks && (!a->pro_scale || min_blocks <= 1)) bn = 64;   // measured on 128 ch at
                                        // 8x8: data gradient 21.6 vs 24.7 us, forward (BatchNorm pass) 26.7 vs 25.8 us
    else if (g->N % 128 == 0 && min_blocks <= 1) bn = 128;
    if (bn == 0 || nTiles * (g->N / bn) < min_blocks) return 0;
    if ((int64_t)g->B * g->Hin * g->Win * g->ldx * 2 >= ((int64_t)1 << 31)) return 0;
    if ((int64_t)g->N * 9 * g->Cin * 2 >= ((int64_t)1 << 31)) return 0;
    // tap order: canonical (forward) or reversed (data gradient)
    const sv_phase& P = g->phase[0];
    bool fwd = true, rev = true;
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        fwd = fwd && P.dy[t] == dy && P.dx[t] == dx;
        rev = rev && P.dy[t] == -dy && P.dx[t] == -dx;
    }
    if (!fwd && !rev) return 0;
    if (a->pro_scale) {         // the coefficient DMA addresses scale and shift from one base with a 32-bit offset
        const int64_t d = (const char*)a->pro_shift - (const char*)a->pro_scale;
        if (d >= ((int64_t)1 << 31) || -d >= ((int64_t)1 << 31)) return 0;
    }
    if (bn == 160 && sv_conv3x3x_try(g, a, fwd, s, rc)) return 1;      // one wave per SIMD, gap-scheduled (conv3x3x.hip)
    if (bn == 160) *rc = fwd ? launch_w2<5, false>(g, a, s) : launch_w2<5, true>(g, a, s);
    else if (bn == 128) *rc = fwd ? launch_w2<4, false>(g, a, s) : launch_w2<4, true>(g, a, s);
    else *rc = fwd ? launch_w2<2, false>(g, a, s) : launch_w2<2, true>(g, a, s);
    return 1;
}
