// Weight gradient of the stride-2 3x3 convolution 32 -> 64 at 32x32 -> 16x16 (wideresnet.py:29-30, first convolution of block 2) with
// the layer's whole gradient ([64][9][32] = 18 432 floats) in every block.  gfx950.
// swgrad.hip's loop (every input staged ONCE into a row / column parity-split, pixel-major LDS image; the pixel index is the k dimension
// of v_mfma_f32_16x16x32_bf16, both operands read back with ds_read_b64_tr_b16) on BANDS of 8 output rows (17 input rows), with a
// gradient small enough for the final atomics to be affordable (4.7 M adds per launch; swgrad's 64 -> 128 layer has 18.9 M and loses):
// wave (nt, ct) owns dW[16 nt .. + 15][9][16 ct .. + 15] -- nine accumulator tiles -- and runs all four 32-pixel chunks of a band.
// The generic kernel stages dy and the activated input once per tap (nine passes through L2): 96 us for 201 MB.
// The 64 -> 128 layer at 16x16 -> 8x8 (swgrad.hip's layer) on the same kernel with the OUTPUT CHANNELS SPLIT over four blocks: a
// block holds dW[32 of 128][9][64] (the same 18 432 floats), reads its quarter of dy and all of x -- the tensors are 8 + 17 MB, x
// comes from L2 three times out of four -- and the launch ends in 4.7 M atomics instead of swgrad's 18.9 M.
// Same sv_wgrad contract: a fast path inside it (SV_K_S2WGRAD disables); declines the deterministic mode.
#include "common.h"

namespace {

struct s2wg_params {
    const void* x;
    const void* dy;
    const float* pro_scale;
    const float* pro_shift;
    float pro_slope;
    float* dw;
};

// CIN input channels, NB output channels per block (of NTOT), WO x WO outputs from (2 WO) x (2 WO) inputs; a band = 8 output rows
template <int CIN_, int NB_, int NTOT_, int WO_>
struct s2wg_cfg {
    static constexpr int CIN = CIN_, NB = NB_, NTOT = NTOT_, WO = WO_, HIN = 2 * WO_;
    static constexpr int NT = NB / 16, CT = CIN / 16;              // 16-channel tiles of dy / of the input: one wave each
    static constexpr int LDX = CIN + 8, LDY = NB + 8;              // LDS row strides (elements)
    static constexpr int SC = WO + 1, SUBPIX = 9 * SC, SUB = SUBPIX * LDX * 2;   // a parity sub-image: 9 rows x (WO + 1) columns (row 0 / column 0: the halo)
    static constexpr int XIMG = 4 * SUB, YIMG = 8 * WO * LDY * 2, IMG = XIMG + YIMG;
    static constexpr int NTH = 512, XROW = HIN * (CIN / 8), XVEC = 17 * XROW, XV = (XVEC + NTH - 1) / NTH, YVEC = 8 * WO * (NB / 8), YV = (YVEC + NTH - 1) / NTH;
    static constexpr int RPI = NTH / XROW;                         // input rows per staging trip of the block
    static constexpr int NCH = 8 * WO / 32, RPC = 32 / WO;         // 32-pixel chunks of a band, output rows per chunk
    static constexpr int LDS = 2 * IMG;
    static_assert(NT * CT == 8 && (YVEC % NTH == 0 || YVEC < NTH) && NTH % XROW == 0 && (RPI % 2) == 0 && LDS <= 160 * 1024, "waves / staging / LDS budget");
};

__device__ __forceinline__ bf16x8 s2wg_frag(const char* a0, int ldb) {      // (see swgrad.hip)
    typedef __attribute__((address_space(3))) s16x4 lds_v4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4*)(a0 + 4 * ldb));
    union { s16x4 s[2]; bf16x8 b; } u;
    u.s[0] = lo;
    u.s[1] = hi;
    return u.b;
}

template <typename C>
__global__ __launch_bounds__(512, 1) void s2wgrad_kernel(const sv_geom g, const sv_wg_g<s2wg_params> PG, const int nparts) {
    constexpr int CIN = C::CIN, NB = C::NB, NTOT = C::NTOT, WO = C::WO, HIN = C::HIN, LDX = C::LDX, LDY = C::LDY, SUB = C::SUB, IMG = C::IMG, NTH = C::NTH;
    constexpr int XV = C::XV, YV = C::YV, SC = C::SC;
    const s2wg_params& p = PG.g[blockIdx.y];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = wave % C::NT, ct = wave / C::NT;                // 16-channel tiles of dy (n) and of the input (c)
    const int gq = lane >> 4, li = lane & 15;
    const sv_phase& P = g.phase[0];
    const bf16* __restrict__ X = reinterpret_cast<const bf16*>(p.x);
    const bf16* __restrict__ DY = reinterpret_cast<const bf16*>(p.dy);
    constexpr int BPI = WO / 8;                                    // bands per image
    const int nband = g.B * BPI;
    // the nparts blocks of one slot walk the same bands, each with its NB output channels -- on ONE XCD (blocks are dealt to the
    // eight XCDs round-robin), so that the slot's input bands come from that XCD's L2 for all but the first of them
    const int nslot = gridDim.x / nparts, bid = blockIdx.x;
    const bool xcd_map = (nslot & 7) == 0;
    const int part = xcd_map ? (bid >> 3) % nparts : bid % nparts, n0 = part * NB;
    int band = xcd_map ? (bid & 7) + 8 * (bid / (8 * nparts)) : bid / nparts;

    // ---- a band's vectors: x = the 17 input rows 16 b - 1 .. 16 b + 15 (XROW vectors each, contiguous), dy = 8 rows, NB of NTOT channels
    bf16x8 xr[XV], yr[YV];
    auto x_ok = [&](int b, int v) { return v < C::XVEC && (b > 0 || v >= C::XROW); };
    auto request = [&](int bd) __attribute__((always_inline)) {
        const int im = bd / BPI, b = bd - im * BPI;
        const bf16* const xi = X + ((int64_t)im * HIN + 16 * b - 1) * (HIN * CIN);
        const bf16* const yi = DY + ((int64_t)im * WO + 8 * b) * (WO * NTOT) + n0;
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int v = tid + NTH * i;
            bf16x8 z;
#pragma unroll
            for (int j = 0; j < 8; ++j) z[j] = (bf16)0.f;
            xr[i] = x_ok(b, v) ? *reinterpret_cast<const bf16x8*>(xi + v * 8) : z;
        }
#pragma unroll
        for (int i = 0; i < YV; ++i) {
            const int v = tid + NTH * i;
            if (v < C::YVEC) yr[i] = *reinterpret_cast<const bf16x8*>(yi + (v / (NB / 8)) * NTOT + 8 * (v % (NB / 8)));
        }
    };
    if (band < nband) request(band);
    const bool has_pro = p.pro_scale != nullptr;
    const float slope = has_pro ? p.pro_slope : 1.f;
    // prologue coefficients of this thread's 8 channels (chunk tid % (CIN / 8): the same for all of its vectors)
    f32x4 s0 = {1.f, 1.f, 1.f, 1.f}, s1 = s0, t0 = {0.f, 0.f, 0.f, 0.f}, t1 = t0;
    if (has_pro) {
        const int c0 = 8 * (tid % (CIN / 8));
        s0 = *reinterpret_cast<const f32x4*>(p.pro_scale + c0); s1 = *reinterpret_cast<const f32x4*>(p.pro_scale + c0 + 4);
        t0 = *reinterpret_cast<const f32x4*>(p.pro_shift + c0); t1 = *reinterpret_cast<const f32x4*>(p.pro_shift + c0 + 4);
    }
    for (int i = tid; i < C::LDS / 16; i += NTH) *reinterpret_cast<f32x4*>(smem + 16 * i) = f32x4{0.f, 0.f, 0.f, 0.f};      // (halo = padding)
    // staging: x vector i = input row r = tid / XROW + RPI i (RPI even: the same parity for every i), pixel, 8-channel chunk
    int xdst;
    {
        const int r = tid / C::XROW, rowidx = (r + 1) >> 1, pr = (r & 1) ^ 1, ix = (tid % C::XROW) / (CIN / 8), pc = ix & 1, colidx = (ix >> 1) + 1;
        xdst = (2 * pr + pc) * SUB + ((rowidx * SC + colidx) * LDX + 8 * (tid % (CIN / 8))) * 2;
    }
    auto stage = [&](int buf, int bd) __attribute__((always_inline)) {
        char* const base = smem + buf * IMG;
        const int b = bd % BPI;
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int v = tid + NTH * i;
            if (v < C::XVEC) {
                // (the padding row stays zero: it is not transformed; vector i is RPI / 2 sub-image rows below vector i - 1)
                const bf16x8 val = (has_pro && x_ok(b, v)) ? bn_act8(xr[i], s0, s1, t0, t1, slope) : xr[i];
                *reinterpret_cast<bf16x8*>(base + xdst + i * ((C::RPI / 2) * SC * LDX * 2)) = val;
            }
        }
#pragma unroll
        for (int i = 0; i < YV; ++i) {
            const int v = tid + NTH * i;
            if (v < C::YVEC) *reinterpret_cast<bf16x8*>(base + C::XIMG + ((v / (NB / 8)) * LDY + 8 * (v % (NB / 8))) * 2) = yr[i];
        }
    };
    // fragment addresses (byte offsets inside an image) of chunk 0; chunk kc = output rows RPC kc .. + RPC - 1 (WO pixels each).  The
    // lane's k group gq = 8 pixels: row 8 gq / WO of the chunk, columns (8 gq) % WO ..
    const int yoff = C::XIMG + ((8 * gq + (li >> 2)) * LDY + 16 * nt + 4 * (li & 3)) * 2;            // (+ 32 pixels per chunk)
    int xoff[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = P.dy[t], dx = P.dx[t];
        const int row = (2 * (dy & 1) + (dx & 1)) * C::SUBPIX + ((8 * gq) / WO + (dy >= 0 ? 1 : 0)) * SC + (8 * gq) % WO + (dx >= 0 ? 1 : 0);
        xoff[t] = ((row + (li >> 2)) * LDX + 16 * ct + 4 * (li & 3)) * 2;                            // (+ RPC sub-image rows per chunk)
    }
    f32x4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    if (band < nband) stage(0, band);
    __syncthreads();

    {
        const int step = nslot;
        int buf = 0;
        for (; band < nband; band += step, buf ^= 1) {
            const int nxt = band + step;
            const bool has_next = nxt < nband;
            if (has_next) request(nxt);
            const char* const IB = smem + buf * IMG;
#pragma unroll
            for (int kc = 0; kc < C::NCH; ++kc) {
                const bf16x8 af = s2wg_frag(IB + yoff + kc * (32 * LDY * 2), LDY * 2);
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const bf16x8 bf_ = s2wg_frag(IB + xoff[t] + kc * (C::RPC * SC * LDX * 2), LDX * 2);
                    mma32(acc[t], af, bf_);
                }
            }
            if (has_next) stage(buf ^ 1, nxt);
            __syncthreads();
        }
    }
    // ---- dW[n][torig][c] += : acc[t][e] = (n = 16 nt + 4 gq + e, c = 16 ct + li)
    {
        const int T = g.T_orig;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int to = P.torig[t];
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(p.dw + ((size_t)(n0 + 16 * nt + 4 * gq + e) * T + to) * CIN + 16 * ct + li, acc[t][e]);
        }
    }
}

}  // namespace

namespace {

template <typename C>
int launch_s2wgrad(const sv_geom* g, const s2wg_params& p, int groups, hipStream_t s) {
    constexpr int nparts = C::NTOT / C::NB;
    const int nband = g->B * (C::WO / 8);
    const int slots = sv_block_slots(nband, sv_persistent_blocks() / 2 / groups / nparts);      // band slots: one block per CU, nparts blocks per slot
    static bool optin = false;
    if (const int rc = sv_lds_optin(optin, C::LDS, "s2wgrad", &s2wgrad_kernel<C>)) return rc;
    sv_prof_begin(s);
    hipLaunchKernelGGL((s2wgrad_kernel<C>), dim3(slots * nparts, groups), dim3(C::NTH), C::LDS, s, *g, sv_expand_wg(*g, p, groups, 2), nparts);
    sv_prof_end(s);
    return sv_check_launch("sv_wgrad(s2wgrad)");
}

}  // namespace

// Returns 1 and sets *rc when the launch is the weight gradient of a stride-2 3x3 convolution of the WideResNet: 32 -> 64 at 32x32,
// 64 -> 128 at 16x16.
int sv_s2wgrad_try(const sv_geom* g, int dtype, const sv_wgrad_args& a, hipStream_t s, int* rc) {
    if (sv_disabled(SV_K_S2WGRAD) || dtype != SV_BF16 || sv_deterministic()) return 0;
    if (g->nphase != 1 || g->sy != 2 || g->sx != 2 || g->osy != 1 || g->osx != 1) return 0;
    const sv_phase& P = g->phase[0];
    if (P.ntap != 9 || g->T_orig != 9) return 0;
    for (int t = 0; t < 9; ++t)
        if (P.dy[t] < -1 || P.dy[t] > 1 || P.dx[t] < -1 || P.dx[t] > 1) return 0;
    if (g->Hin != g->Win || g->Hout != g->Wout || g->Hin != 2 * g->Hout || g->ldx != g->Cin || g->ldo != g->N) return 0;
    s2wg_params p;
    sv_wg_operands(p, a);
    p.dw = a.dw;
    if (g->Cin == 32 && g->N == 64 && g->Hout == 16) { *rc = launch_s2wgrad<s2wg_cfg<32, 64, 64, 16>>(g, p, a.groups, s); return 1; }
    if (g->Cin == 64 && g->N == 128 && g->Hout == 8) { *rc = launch_s2wgrad<s2wg_cfg<64, 32, 128, 8>>(g, p, a.groups, s); return 1; }
    return 0;
}
