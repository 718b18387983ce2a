// Per-pixel GEMMs for the weight-heavy ConvTranspose2d(4, 2, 1) layers on SMALL maps and their data gradients (bf16, gfx950):
//   forward        convT_like, 4 x 4 taps, stride 2, pad 1, Hin = Win <= 4   (1x1 -> 2x2, 2x2 -> 4x4, 4x4 -> 8x8)
//   data gradient  conv_like,  4 x 4 taps, stride 2, pad 1, Hin = Win <= 8   (2x2 -> 1x1, 4x4 -> 2x2, 8x8 -> 4x4)
//
// On these maps the gather-GEMM's row dimension B * Hq * Wq mixes pixels whose taps fall into the padding with pixels whose taps
// do not: a tile multiplies the zeros of the former (44 % of all (pixel, tap) pairs at 2x2 <-> 4x4, 23 % at 4x4 <-> 8x8).  Here
// every OUTPUT PIXEL is a dense GEMM of its own:
//   rows    = the images of one BatchNorm group (A row b = Cin contiguous values at x + (b * Hin * Win + input pixel) * ldx),
//   columns = the channels of that output pixel,
//   K       = the pixel's VALID (input pixel, tap) pairs x Cin -- nothing else is loaded or multiplied.
// A host-side table (PgTable, built from sv_geom per launch; sv_debug_pixgemm_table exposes it) lists per output pixel its
// phase, its valid taps -- as indices into the phase's EXISTING packed weights [N][ntap][Cin] at phase[].w_off -- and each tap's
// input pixel.  Work items = (group, output pixel, image tile, channel tile); the pixels are ordered by falling tap count so
// that the items with the long K loops (centre pixels: 4x the corners') start first.
//
// Tile loop: both operands global -> LDS by DMA, 64 channels deep per chunk.  A wave instruction moves 8 rows x 128 bytes -- whole
// cache lines; igemm_dma's 32-deep chunks fetch 16 half lines -- into a lane-linear image whose 16-byte k-pieces are swizzled on
// the SOURCE address (piece p of row r sits at p ^ ((r >> 1) & 7)), which makes the ds_read_b128 fragment reads conflict-free.
// A ring of 2-4 stages with counted vmcnt waits and a RAW s_barrier keeps the DMAs of the next chunks in flight across the
// barrier (__syncthreads() would fence them with vmcnt(0) on every chunk).  16x16x32 MFMAs with the weights as the A operand, so
// that gemm_epilogue (epilogue.h: BatchNorm statistics per group / activation backward + BatchNorm-backward sums, ldo, replicas)
// applies unchanged; a wave owns 16 MS images x all channels of the tile.  Cin % 64 == 32: the last chunk of a tap reads its
// upper half from a zero page.  Rows beyond the batch / channels beyond N load a valid row and are dropped by the epilogue.
// What bounds it (profiles/decoder_gemm_layers.txt): the rate at which a CU fills its LDS from L2, ~50 GB/s -- every tile
// re-reads its K x (rows + channels) operand bytes -- then the 8-byte output stores of the shared epilogue; not the MFMAs.
// Tiles: 128 images x 128 channels, 128 x 64 or 64 x 64, whichever puts the fewest operand bytes on the busiest CU (the data
// gradients have only 2 x 512 rows: 1x1 <- 2x2 is ONE pixel x 1024 channels, 256 tiles of 64 x 64).  No K split: the summation
// order inside an item is fixed (taps in table order, channels ascending), so the deterministic mode (SV_FLAG_DET) is HONOURED
// the way igemm_dma honours it -- gemm_epilogue's one-adder-per-replica sums; sv_igemm_query_blocks reports this kernel's grid.
// Not persistent: sv_igemm_args::block_budget has nothing to bound here.
#include <string.h>

#include "common.h"
#include "epilogue.h"

namespace {

constexpr int PG_MAX_PIX = 64;        // output pixels (8 x 8 forward, 4 x 4 data gradient)
constexpr int PG_MAX_ENT = 256;       // valid (pixel, tap) pairs: 196 at 4x4 <-> 8x8

struct PgTable {                      // travels as a kernel argument; 32-bit words: a block reads its own with scalar loads
    int32_t npix;
    uint32_t item[PG_MAX_PIX];        // by work slot (falling tap count): oy | ox << 3 | phase << 6 | valid taps << 8 | first entry << 13
    uint32_t ent[PG_MAX_ENT];         // tap index inside the phase | input pixel (iy * Win + ix) << 4
};
__host__ __device__ inline int pg_oy(uint32_t it) { return it & 7; }
__host__ __device__ inline int pg_ox(uint32_t it) { return (it >> 3) & 7; }
__host__ __device__ inline int pg_phase(uint32_t it) { return (it >> 6) & 3; }
__host__ __device__ inline int pg_ntap(uint32_t it) { return (it >> 8) & 31; }
__host__ __device__ inline int pg_first(uint32_t it) { return it >> 13; }

// the geometries above, recognised by their taps (k = 4, stride 2, pad 1)
bool pg_geometry(const sv_geom* g) {
    if (g->T_orig != 16 || g->Hin != g->Win || g->Hq != g->Wq || g->Hout != g->Wout || g->Hin < 1) return false;
    if (g->nphase == 4) {             // ConvTranspose forward
        if (g->sy != 1 || g->sx != 1 || g->osy != 2 || g->osx != 2 || g->Hq != g->Hin || g->Hout != 2 * g->Hin || g->Hin > 4) return false;
        for (int p = 0; p < 4; ++p) {
            const sv_phase& P = g->phase[p];
            if (P.ooy != p / 2 || P.oox != p % 2 || P.ntap < 1 || P.ntap > 4) return false;
            for (int t = 0; t < P.ntap; ++t)
                if (2 * P.dy[t] != P.ooy + 1 - P.torig[t] / 4 || 2 * P.dx[t] != P.oox + 1 - P.torig[t] % 4) return false;
        }
        return true;
    }
    if (g->nphase == 1) {             // its data gradient: a 4x4 stride-2 convolution
        const sv_phase& P = g->phase[0];
        if (g->sy != 2 || g->sx != 2 || g->osy != 1 || g->osx != 1 || g->Hin > 8 || g->Hin != 2 * g->Hq || g->Hout != g->Hq) return false;
        if (P.ooy != 0 || P.oox != 0 || P.ntap < 1 || P.ntap > SV_MAX_TAPS) return false;
        for (int t = 0; t < P.ntap; ++t)
            if (P.dy[t] != P.torig[t] / 4 - 1 || P.dx[t] != P.torig[t] % 4 - 1) return false;
        return true;
    }
    return false;
}

bool pg_build(const sv_geom* g, PgTable* T) {
    if (!pg_geometry(g)) return false;
    const int npix = g->Hout * g->Wout;
    if (npix > PG_MAX_PIX || g->Hout > 8 || g->Hin * g->Win > 64) return false;
    memset(T, 0, sizeof(*T));
    T->npix = npix;
    bool seen[PG_MAX_PIX] = {};
    uint32_t byp[PG_MAX_PIX];         // the items by output pixel
    int nent = 0, count = 0;
    for (int ph = 0; ph < g->nphase; ++ph) {
        const sv_phase& P = g->phase[ph];
        for (int qy = 0; qy < g->Hq; ++qy)
            for (int qx = 0; qx < g->Wq; ++qx) {
                const int oy = qy * g->osy + P.ooy, ox = qx * g->osx + P.oox;
                if (oy < 0 || oy >= g->Hout || ox < 0 || ox >= g->Wout) return false;
                const int pix = oy * g->Wout + ox;
                if (seen[pix]) return false;
                seen[pix] = true;
                ++count;
                const int first = nent;
                int n = 0;
                for (int t = 0; t < P.ntap; ++t) {
                    const int iy = qy * g->sy + P.dy[t], ix = qx * g->sx + P.dx[t];
                    if (iy < 0 || iy >= g->Hin || ix < 0 || ix >= g->Win) continue;
                    if (nent >= PG_MAX_ENT) return false;
                    T->ent[nent++] = (uint32_t)(t | ((iy * g->Win + ix) << 4));
                    ++n;
                }
                byp[pix] = (uint32_t)(oy | ox << 3 | ph << 6 | n << 8 | first << 13);
            }
    }
    if (count != npix) return false;
    int slot = 0;                     // falling tap count, pixels of equal count in index order
    for (int n = SV_MAX_TAPS; n >= 0; --n)
        for (int pix = 0; pix < npix; ++pix)
            if (pg_ntap(byp[pix]) == n) T->item[slot++] = byp[pix];
    return true;
}

typedef __attribute__((address_space(3))) void* pg_lds_ptr;
typedef const __attribute__((address_space(1))) void* pg_glb_ptr;
__device__ __attribute__((aligned(256))) const unsigned char pg_zero_page[256] = {0};

template <int NT, int MS, int NST>
__global__ __launch_bounds__(256, 2) void pixgemm_kernel(const sv_geom g, const sv_igemm_args_g A, const PgTable T) {
    const sv_igemm_args& a = A.g[blockIdx.y];
    sv_start_signal(a);
    typedef bf16 E;
    typedef bf16x8 V;
    constexpr int BM = 64 * MS, BN = 16 * NT;
    static_assert(BM % 32 == 0 && BN % 32 == 0, "every wave takes part in every DMA pass (the counted waits)");
    constexpr int PA = BM / 32, PB = BN / 32;        // 32-row DMA passes over the two operand tiles
    constexpr int STAGE = (BM + BN) * 128;           // bytes per stage: [BM][64] + [BN][64] bf16

    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* ssum = reinterpret_cast<double*>(smem);  // [2][BN] over the operand buffers, after the k loop

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nMt = (g.B + BM - 1) / BM;
    const int nNt = (g.N + BN - 1) / BN;
    const int per = nMt * nNt;
    const int slot = blockIdx.x / per, rest = blockIdx.x - slot * per;
    const int mt = rest / nNt, n0 = (rest - mt * nNt) * BN;
    const uint32_t item = T.item[slot];
    const int oy = pg_oy(item), ox = pg_ox(item);
    const sv_phase& P = g.phase[pg_phase(item)];
    const int ntap = pg_ntap(item), e0 = pg_first(item);
    const int Krow = P.ntap * g.Cin;                 // row stride of the phase's packed weights
    const int cpt = (g.Cin + 63) / 64;               // chunks per tap; with Cin % 64 == 32 the last one is half zeros
    const bool ragged = (g.Cin & 32) != 0;
    const int nk = ntap * cpt;
    const E* __restrict__ X = reinterpret_cast<const E*>(a.x);
    const E* __restrict__ W = reinterpret_cast<const E*>(a.w) + P.w_off;

    // ---- DMA slots: one wave instruction = 8 rows x 128 bytes; lane -> (row lr + 32 i, 16-byte position q of the LDS row), which
    // holds k-piece q ^ ((row >> 1) & 7): the swizzle, applied on the SOURCE address, makes the ds_read_b128 fragment reads below
    // conflict-free (the 16 lanes of a read group hit 16 distinct 16-byte bank groups).  Rows beyond the batch / channels beyond
    // N load a valid row instead (the epilogue neither stores nor sums them).
    const int q = tid & 7, lr = tid >> 3;
    const int ps = q ^ ((lr >> 1) & 7);              // the k-piece (8 elements) this slot holds
    const E* const zp = reinterpret_cast<const E*>(pg_zero_page) + 8 * q;
    const bool hi = ps >= 4;                         // beyond Cin in the half chunk of a ragged tap
    const E* xb[PA];
    const E* wb[PB];
#pragma unroll
    for (int i = 0; i < PA; ++i)
        xb[i] = X + (int64_t)min(mt * BM + lr + 32 * i, g.B - 1) * (g.Hin * g.Win) * g.ldx + 8 * ps;
#pragma unroll
    for (int i = 0; i < PB; ++i) wb[i] = W + (int64_t)min(n0 + lr + 32 * i, g.N - 1) * Krow + 8 * ps;
    // block-uniform: the next chunk to issue is chunk cu of table entry e0 + tapu, at element offsets aoff / woff of the rows
    int cu = 0, tapu = 0;
    int64_t aoff = 0;
    int woff = 0;
    auto set_tap = [&](int e) {
        const int ent = (int)T.ent[e0 + e];
        aoff = (int64_t)(ent >> 4) * g.ldx;
        woff = (ent & 15) * g.Cin;
    };
    set_tap(0);
    auto issue = [&](int stage) {
        char* const sb = smem + stage * STAGE;
        const bool cut = ragged && cu == cpt - 1 && hi;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const E* src = cut ? zp : xb[i] + aoff;
            __builtin_amdgcn_global_load_lds((pg_glb_ptr)src, (pg_lds_ptr)(sb + (32 * i + 8 * wave) * 128), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const E* src = cut ? zp : wb[i] + woff;
            __builtin_amdgcn_global_load_lds((pg_glb_ptr)src, (pg_lds_ptr)(sb + BM * 128 + (32 * i + 8 * wave) * 128), 16, 0, 0);
        }
        aoff += 64;
        woff += 64;
        if (++cu == cpt) {      // (uniform) the next chunk starts the next valid tap
            cu = 0;
            if (++tapu < ntap) set_tap(tapu);
        }
    };

    f32x4 acc[NT][MS];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MS; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    const int sw = (fr >> 1) & 7;                    // swizzle of rows fr, fr + 16, ...
    // NST stages: chunks k+1 .. k+NST-1 are in flight during the MFMAs of chunk k.  Every wave issues exactly D = PA + PB
    // DMAs per chunk (all of one kind), so vmcnt(j * D) in front of the barrier leaves the j youngest chunks outstanding.
    // The barrier of the loop is a RAW s_barrier: __syncthreads() fences with vmcnt(0) while an LDS-DMA is pending and would
    // drain the ring on every chunk.  Ordering without it: a stage is read one barrier AFTER the counted wait of every wave
    // that filled it, and refilled one barrier after the lgkmcnt(0) that retired its last fragment reads.
    constexpr int D = PA + PB;
    auto wait_for = [&](int younger) {               // chunks issued AFTER the one that has to have landed
        if (NST >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * D) : "memory");
        else if (NST >= 3 && younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    auto ring_barrier = [&]() {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    static_assert(NST >= 2 && NST <= 4, "");
#pragma unroll
    for (int j = 0; j < NST - 1; ++j)
        if (nk > j) issue(j);
    wait_for(min(nk, NST - 1) - 1);
    ring_barrier();
    int st = 0;                 // stage of chunk kc
    for (int kc = 0; kc < nk; ++kc) {
        if (kc + NST - 1 < nk) issue(st == 0 ? NST - 1 : st - 1);        // the stage chunk kc - 1 has released
        const char* const sb = smem + st * STAGE;
        const char* Ab = sb + (16 * MS * (tid >> 6) + fr) * 128;
        const char* Bb = sb + BM * 128 + fr * 128;
#pragma unroll
        for (int s = 0; s < 2; ++s) {                // the two 32-deep halves of the chunk
            const int po = 16 * ((4 * s + fq) ^ sw);
            V af[MS];
#pragma unroll
            for (int j = 0; j < MS; ++j) af[j] = *reinterpret_cast<const V*>(Ab + 16 * j * 128 + po);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const V wf = *reinterpret_cast<const V*>(Bb + 16 * i * 128 + po);
#pragma unroll
                for (int j = 0; j < MS; ++j) mma32(acc[i][j], wf, af[j]);
            }
        }
        wait_for(min(nk - 1, kc + NST - 1) - (kc + 1));      // chunk kc + 1 has landed
        ring_barrier();
        st = st == NST - 1 ? 0 : st + 1;
    }

    // ---- epilogue -----------------------------------------------------------------------------------------------
    for (int i = tid; i < 2 * BN; i += 256) ssum[i] = 0.0;
    __syncthreads();
    int64_t obase[MS];
    bool oval[MS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms) {
        const int m = mt * BM + 16 * MS * (tid >> 6) + 16 * ms + fr;
        oval[ms] = m < g.B;
        obase[ms] = ((int64_t)((oval[ms] ? m : 0) * g.Hout + oy) * g.Wout + ox) * g.ldo;
    }
    gemm_epilogue<E, NT, MS>(acc, obase, oval, n0, g.N, a, ssum, reinterpret_cast<float*>(ssum + 2 * BN));
}

template <int NT, int MS>
int64_t pg_items(const sv_geom* g, const sv_igemm_args* a, const PgTable& T) {
    return (int64_t)((g->B + 64 * MS - 1) / (64 * MS)) * ((g->N + 16 * NT - 1) / (16 * NT)) * T.npix * sv_ngroups(a->groups);
}
// What bounds these launches is the rate at which ONE CU fills its LDS from L2 (both operands are re-read by every tile that
// shares them): the operand bytes of the busiest CU -- rounds of `cus` concurrent items x (rows + channels) of a tile.
template <int NT, int MS>
int64_t pg_cost(const sv_geom* g, const sv_igemm_args* a, const PgTable& T, int64_t cus) {
    return (pg_items<NT, MS>(g, a, T) + cus - 1) / cus * (64 * MS + 16 * NT);
}

template <int NT, int MS, int NST>
int launch_pixgemm(const sv_geom* g, const sv_igemm_args* a, const PgTable& T, hipStream_t s) {
    const int64_t grid = pg_items<NT, MS>(g, a, T) / sv_ngroups(a->groups);
    constexpr int lds = NST * (64 * MS + 16 * NT) * 128;
    static bool optin = false;
    if (lds > 64 * 1024)
        if (const int rc = sv_lds_optin(optin, lds, "pixgemm", &pixgemm_kernel<NT, MS, NST>)) return rc;
    return sv_igemm_launch(&pixgemm_kernel<NT, MS, NST>, (int)grid, 256, (size_t)lds, g, a, 2, s, "sv_igemm(pixel)", T);
}

}  // namespace

int sv_pixgemm_try(const sv_geom* g, int dtype, const sv_igemm_args* a, hipStream_t s, int* rc) {
    if (sv_disabled(SV_K_PIXGEMM) || dtype != SV_BF16) return 0;
    if (a->pro_scale || a->bias || a->residual || a->sparse_out) return 0;
    if (g->Cin % 32 != 0 || g->N % 32 != 0 || g->ldx % 8 != 0 || g->B < 1) return 0;
    PgTable T;
    if (!pg_build(g, &T)) return 0;
    // the tile with the fewest operand bytes on the busiest of SV_OPT_WIDE_MIN_BLOCKS CUs (256; tests: 1 = the widest tile),
    // the wider one on a tie; 128-channel tiles only where N is a multiple of 128
    const int64_t cus = sv_wide_min_blocks();
    const int64_t c8 = g->N % 128 == 0 ? pg_cost<8, 2>(g, a, T, cus) : INT64_MAX, c4 = pg_cost<4, 2>(g, a, T, cus), c1 = pg_cost<4, 1>(g, a, T, cus);
    // Stages: as many as leave room for TWO blocks per CU (160 KB of LDS) -- the second block's K loop covers the first one's
    // epilogue -- except that a launch of 128 x 128 tiles with at most one item per CU takes four (128 KB, alone on its CU).
    if (c8 <= c4 && c8 <= c1) {
        if (pg_items<8, 2>(g, a, T) <= cus) *rc = launch_pixgemm<8, 2, 4>(g, a, T, s);
        else *rc = launch_pixgemm<8, 2, 2>(g, a, T, s);
    } else if (c4 <= c1) {
        *rc = launch_pixgemm<4, 2, 3>(g, a, T, s);
    } else {
        *rc = launch_pixgemm<4, 1, 4>(g, a, T, s);
    }
    return 1;
}

extern "C" int sv_debug_pixgemm_table(const sv_geom* g, int* npix, int* pixels, int* taps) {
    SV_REQUIRE(g && npix && pixels && taps, SV_E_ARG, "sv_debug_pixgemm_table: null argument");
    PgTable T;
    *npix = 0;
    SV_REQUIRE(pg_build(g, &T), SV_E_SHAPE, "sv_debug_pixgemm_table: not a 4x4 stride-2 pad-1 ConvTranspose (Hin <= 4) or convolution (Hin <= 8)");
    *npix = T.npix;
    for (int slot = 0; slot < T.npix; ++slot) {
        const uint32_t it = T.item[slot];
        const sv_phase& P = g->phase[pg_phase(it)];
        int* p = pixels + 4 * slot;
        p[0] = pg_oy(it); p[1] = pg_ox(it); p[2] = pg_phase(it); p[3] = pg_ntap(it);
        for (int e = 0; e < SV_MAX_TAPS; ++e) {
            int* q = taps + 4 * (SV_MAX_TAPS * slot + e);
            if (e < pg_ntap(it)) {
                const int ent = (int)T.ent[pg_first(it) + e], t = ent & 15, ipix = ent >> 4;
                q[0] = t; q[1] = ipix / g->Win; q[2] = ipix % g->Win;
                q[3] = (int)(P.w_off + (int64_t)t * g->Cin);          // element offset of the tap's [Cin] slice in weight row 0
            } else {
                q[0] = q[1] = q[2] = q[3] = -1;
            }
        }
    }
    return SV_OK;
}
