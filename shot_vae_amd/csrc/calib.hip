// How far can the class posterior q(y | x) be trusted?  Per-row softmax statistics, the reliability histogram, a temperature fitted by
// Newton steps on the device, and the rank counts behind AUROC / AUPR / risk-coverage (declared, with the exact definitions, in
// include/shotvae_hip.h):
//   sv_calib_rows    prediction, confidence, NLL, Brier score and entropy of every row of logits or probabilities
//   sv_calib_accum   the rows into B confidence bins (integer counts) and P partial states of double sums (aggpost.hip's rule: tile t to
//                    state t mod P, rows in index order)
//   sv_calib_finish  merges the states: accuracy, ECE, MCE, the means, and the reliability diagram
//   sv_temp_accum    dL/dbeta, d2L/dbeta2 and L of the summed NLL at beta = 1 / T, under the same partial-state rule
//   sv_temp_update   one clamped Newton step on beta, in one block: a fit never reads the host
//   sv_rank_scan     greater[i] += sum_j w_j [g_j > q_i], equal[i] += sum_j w_j [g_j == q_i]; the [Q][N] comparison matrix is never stored
// Plain HIP C++, fp32 VALU, double accumulators; each takes a stream and allocates nothing: capturable.  Every floating-point sum is
// taken in a fixed order that depends only on the call's arguments; the only atomics are integer ones.  A repeated call sequence gives
// the same bits.
#include "common.h"
#include <limits.h>
#include <math.h>

constexpr int CB_THREADS = 256;
constexpr int CB_BMAX = 1024, CB_PMAX = 64;
constexpr int CB_RV = 4;              // values of a row a lane keeps in registers: rows of up to 4 x 64 classes are read once

// ------------------------------------------------------------------------------------------ a row on a group of lanes
// A row of K classes is taken by G = min(64, the power of two >= K) neighbouring lanes (class k on lane k mod G), so a wave holds 64 / G
// rows: K = 10 runs four rows per wave on 16 lanes each, 10 of them busy, K = 100 one row per wave.  The sums of a row meet in an xor
// butterfly inside the group: every lane of the group ends with the same bits.  Rows beyond the end are computed on the last row and
// never stored, so every lane takes part in every shuffle.
template <int KIND>
__device__ __forceinline__ float cb_load(const float* __restrict__ xr, int k) {
    const float v = xr[k];
    return KIND == SV_CAL_PROB ? logf(v) : v;          // log 0 = -inf: a class of probability 0; log of a negative value: NaN
}
__device__ __forceinline__ float cb_gsum(float v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int cb_gor(int v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}
// the maximum and the smallest index that attains it
__device__ __forceinline__ void cb_gmax(float& m, int& mi, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) {
        const float om = __shfl_xor(m, off);
        const int oi = __shfl_xor(mi, off);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
}
// the classes of this lane, in index order; REG: at most CB_RV of them, kept in registers between the passes
#define CB_EACH(i, k) _Pragma("unroll 4") for (int i = 0, k = li; i < (REG ? CB_RV : INT_MAX) && k < K; ++i, k += G)

// ------------------------------------------------------------------------------------------ sv_calib_rows
template <int KIND, bool REG>
__global__ __launch_bounds__(CB_THREADS) void calib_rows_kernel(const float* __restrict__ x, int ldx, int N, int K, int lgG,
                                                                const float* __restrict__ temp, const int64_t* __restrict__ label,
                                                                int64_t* pred, float* conf, float* nll, float* brier, float* entropy) {
    const int G = 1 << lgG, li = threadIdx.x & (G - 1);
    const int64_t row = (int64_t)blockIdx.x * (CB_THREADS >> lgG) + (threadIdx.x >> lgG);
    const bool live = row < N;
    const float* xr = x + (live ? row : (int64_t)N - 1) * ldx;
    const float T = temp ? temp[0] : 1.f;
    const int64_t lab64 = (label && live) ? label[row] : -1;
    const int lab = (lab64 >= 0 && lab64 < K) ? (int)lab64 : -1;

    float z[CB_RV];
    float m = -INFINITY;
    int mi = INT_MAX, bad = !(T > 0.f);
    CB_EACH(i, k) {
        const float v = cb_load<KIND>(xr, k) / T;
        if (REG) z[i] = v;
        bad |= (v != v) | (v == INFINITY);
        if (v > m) { m = v; mi = k; }
    }
    cb_gmax(m, mi, G);
    bad = cb_gor(bad, G) | (m == -INFINITY);           // a NaN, a +inf, or nothing but -inf

    float S = 0.f, W = 0.f, zl = 0.f;
    CB_EACH(i, k) {
        const float v = REG ? z[i] : cb_load<KIND>(xr, k) / T;
        const float d = v - m, e = expf(d);
        S += e;
        if (e > 0.f) W = fmaf(e, d, W);                // 0 log 0 = 0
        if (k == lab) zl = v;
    }
    S = cb_gsum(S, G);
    W = cb_gsum(W, G);
    zl = cb_gsum(zl, G);                               // one lane holds it, the others 0
    const float logS = logf(S);

    float bs = 0.f;
    if (brier) {
        CB_EACH(i, k) {
            const float v = REG ? z[i] : cb_load<KIND>(xr, k) / T;
            const float t = expf(v - m) / S - (k == lab ? 1.f : 0.f);
            bs = fmaf(t, t, bs);
        }
        bs = cb_gsum(bs, G);
    }
    if (li != 0 || !live) return;
    if (pred) pred[row] = bad ? -1 : mi;
    if (conf) conf[row] = bad ? NAN : 1.f / S;         // exp(0) / S
    if (entropy) entropy[row] = bad ? NAN : logS - W / S;
    if (nll) nll[row] = (bad || lab < 0) ? NAN : logS - (zl - m);
    if (brier) brier[row] = (bad || lab < 0) ? NAN : bs;
}

static int cb_group_log2(int K) {
    int l = 0;
    while (l < 6 && (1 << l) < K) ++l;
    return l;
}

int sv_calib_rows(int kind, const float* x, int ldx, int N, int K, const float* temp, const int64_t* label, int64_t* pred, float* conf,
                  float* nll, float* brier, float* entropy, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(kind == SV_CAL_LOGIT || kind == SV_CAL_PROB, SV_E_ARG, "sv_calib_rows: unknown kind %d", kind);
    SV_REQUIRE(x, SV_E_ARG, "sv_calib_rows: x is NULL");
    SV_REQUIRE(pred || conf || nll || brier || entropy, SV_E_ARG, "sv_calib_rows: every output is NULL");
    SV_REQUIRE(N > 0 && K > 0, SV_E_ARG, "sv_calib_rows: non-positive size (N=%d K=%d)", N, K);
    SV_REQUIRE(ldx >= K, SV_E_SHAPE, "sv_calib_rows: ldx=%d < K=%d", ldx, K);
    const int lgG = cb_group_log2(K), rows = CB_THREADS >> lgG;
    const dim3 grid((unsigned)(((int64_t)N + rows - 1) / rows));
    const bool reg = K <= (CB_RV << lgG);
#define CB_ROWS_LAUNCH(KIND, REG)                                                                                                      \
    hipLaunchKernelGGL((calib_rows_kernel<KIND, REG>), grid, dim3(CB_THREADS), 0, (hipStream_t)stream, x, ldx, N, K, lgG, temp, label,  \
                       pred, conf, nll, brier, entropy)
    if (kind == SV_CAL_LOGIT) {
        if (reg) CB_ROWS_LAUNCH(SV_CAL_LOGIT, true); else CB_ROWS_LAUNCH(SV_CAL_LOGIT, false);
    } else {
        if (reg) CB_ROWS_LAUNCH(SV_CAL_PROB, true); else CB_ROWS_LAUNCH(SV_CAL_PROB, false);
    }
#undef CB_ROWS_LAUNCH
    return sv_check_launch("sv_calib_rows");
}

// ------------------------------------------------------------------------------------------ sv_calib_accum
// the number of inner edges below c (e[i] = edges[i + 1], i < nin, non-decreasing): a NaN lands in bin 0
__device__ __forceinline__ int cb_bin(const float* e, int nin, float c) {
    int lo = 0, hi = nin;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

constexpr int CA_ROWS = 8 * CB_THREADS;                // rows of a counting block

// Blocks 0 .. P - 1, one wave each, own a partial state: lane l keeps the confidence sums of bins l, l + 64, ... in NB registers and
// walks the tiles p, p + P, ... of the call; the 64 rows of a tile are handed round in index order (a row's bin and values are wave
// uniform), so every accumulator is touched by one lane only, in row order: no atomic, no reduction tree.  Every lane forms the three
// totals.  The blocks behind them count: 2048 rows each into an LDS histogram, then ONE integer atomic per touched bin.
template <int NB>
__global__ __launch_bounds__(CB_THREADS) void calib_accum_kernel(const float* __restrict__ conf, const int64_t* __restrict__ pred,
                                                                 const int64_t* __restrict__ label, const float* __restrict__ nll,
                                                                 const float* __restrict__ brier, const float* __restrict__ entropy, int N,
                                                                 int K, const float* __restrict__ edges, int B,
                                                                 unsigned long long* bin_count, unsigned long long* bin_correct,
                                                                 unsigned long long* counts, double* sums, int P, int init) {
    __shared__ float se[CB_BMAX];
    __shared__ int hc[CB_BMAX], hk[CB_BMAX], tot[2];
    const int tid = threadIdx.x, nin = B - 1;
    const bool counting = (int)blockIdx.x >= P;
    for (int i = tid; i < nin; i += CB_THREADS) se[i] = edges[i + 1];
    for (int i = tid; i < B; i += CB_THREADS) { hc[i] = 0; hk[i] = 0; }
    if (tid < 2) tot[tid] = 0;
    __syncthreads();
    if (counting) {
        const int64_t r0 = (int64_t)(blockIdx.x - P) * CA_ROWS;
        int nv = 0, nk = 0;
        for (int j = 0; j < CA_ROWS / CB_THREADS; ++j) {
            const int64_t r = r0 + j * CB_THREADS + tid;
            if (r >= N) break;
            const int64_t pr = pred[r], lb = label[r];
            if (pr < 0 || lb < 0 || lb >= K) continue;
            const int b = cb_bin(se, nin, conf[r]);
            atomicAdd(&hc[b], 1);
            ++nv;
            if (pr == lb) { atomicAdd(&hk[b], 1); ++nk; }
        }
        if (nv) atomicAdd(&tot[0], nv);
        if (nk) atomicAdd(&tot[1], nk);
        __syncthreads();
        for (int i = tid; i < B; i += CB_THREADS) {
            if (hc[i]) atomicAdd(&bin_count[i], (unsigned long long)hc[i]);
            if (hk[i]) atomicAdd(&bin_correct[i], (unsigned long long)hk[i]);
        }
        if (tid == 0) {
            if (tot[0]) atomicAdd(&counts[0], (unsigned long long)tot[0]);
            if (tot[1]) atomicAdd(&counts[1], (unsigned long long)tot[1]);
            if ((int)blockIdx.x == P) atomicAdd(&counts[2], (unsigned long long)N);
        }
        return;
    }
    if (tid >= 64) return;                             // (one wave from here on: no block-wide barrier below)
    const int lane = tid, p = blockIdx.x;
    double* st = sums + (int64_t)p * (B + 3);
    double acc[NB], tn, tb, te;
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = (!init && lane + 64 * q < B) ? st[lane + 64 * q] : 0.0;
    tn = init ? 0.0 : st[B];
    tb = init ? 0.0 : st[B + 1];
    te = init ? 0.0 : st[B + 2];
    const int64_t ntiles = ((int64_t)N + 63) / 64;
    for (int64_t t = p; t < ntiles; t += P) {
        const int64_t r = t * 64 + lane;
        int bin = -1;
        float c = 0.f, vn = 0.f, vb = 0.f, ve = 0.f;
        if (r < N) {
            const int64_t pr = pred[r], lb = label[r];
            if (pr >= 0 && lb >= 0 && lb < K) {
                c = conf[r];
                bin = cb_bin(se, nin, c);
                if (nll) vn = nll[r];
                if (brier) vb = brier[r];
                if (entropy) ve = entropy[r];
            }
        }
#pragma unroll 8
        for (int j = 0; j < 64; ++j) {                 // (j is wave uniform: the row's values travel through scalar registers)
            const int bj = __builtin_amdgcn_readlane(bin, j);
            if (bj < 0) continue;
            const double cj = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), j));
#pragma unroll
            for (int q = 0; q < NB; ++q)
                if (bj == lane + 64 * q) acc[q] += cj;
            tn += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(vn), j));
            tb += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(vb), j));
            te += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(ve), j));
        }
    }
#pragma unroll
    for (int q = 0; q < NB; ++q)
        if (lane + 64 * q < B) st[lane + 64 * q] = acc[q];
    if (lane == 0) {
        if (nll || init) st[B] = tn;
        if (brier || init) st[B + 1] = tb;
        if (entropy || init) st[B + 2] = te;
    }
}

int sv_calib_accum(const float* conf, const int64_t* pred, const int64_t* label, const float* nll, const float* brier, const float* entropy,
                   int N, int K, const float* edges, int B, int64_t* bin_count, int64_t* bin_correct, int64_t* counts, double* sums, int P,
                   int init, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(conf && pred && label, SV_E_ARG, "sv_calib_accum: a row array (conf, pred, label) is NULL");
    SV_REQUIRE(edges, SV_E_ARG, "sv_calib_accum: edges is NULL");
    SV_REQUIRE(bin_count && bin_correct && counts && sums, SV_E_ARG, "sv_calib_accum: an output (bin_count, bin_correct, counts, sums) is NULL");
    SV_REQUIRE(N > 0 && K > 0, SV_E_ARG, "sv_calib_accum: non-positive size (N=%d K=%d)", N, K);
    SV_REQUIRE(B >= 1 && B <= CB_BMAX, SV_E_SHAPE, "sv_calib_accum: B=%d outside [1, %d]", B, CB_BMAX);
    SV_REQUIRE(P >= 1 && P <= CB_PMAX, SV_E_SHAPE, "sv_calib_accum: P=%d outside [1, %d]", P, CB_PMAX);
    const dim3 grid((unsigned)(P + ((int64_t)N + CA_ROWS - 1) / CA_ROWS));
#define CB_ACCUM_LAUNCH(NB)                                                                                                            \
    hipLaunchKernelGGL((calib_accum_kernel<NB>), grid, dim3(CB_THREADS), 0, (hipStream_t)stream, conf, pred, label, nll, brier, entropy, \
                       N, K, edges, B, reinterpret_cast<unsigned long long*>(bin_count),                                                \
                       reinterpret_cast<unsigned long long*>(bin_correct), reinterpret_cast<unsigned long long*>(counts), sums, P, init)
    if (B <= 64) CB_ACCUM_LAUNCH(1);
    else if (B <= 256) CB_ACCUM_LAUNCH(4);
    else CB_ACCUM_LAUNCH(16);
#undef CB_ACCUM_LAUNCH
    return sv_check_launch("sv_calib_accum");
}

// ------------------------------------------------------------------------------------------ sv_calib_finish
// One block.  Thread b merges the P confidence sums of bin b in index order; thread 0 adds the B terms in bin order.
__global__ __launch_bounds__(CB_BMAX) void calib_finish_kernel(const int64_t* bin_count, const int64_t* bin_correct, const int64_t* counts,
                                                               const double* sums, int P, int B, float* out, float* diagram) {
    __shared__ double term[CB_BMAX], gap[CB_BMAX], sc[CB_BMAX];
    const int b = threadIdx.x;
    const double n = (double)counts[0];
    if (b < B) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += sums[(int64_t)p * (B + 3) + b];
        const int64_t nb = bin_count[b];
        const double a = (double)bin_correct[b] / (double)nb, c = s / (double)nb;          // (0 / 0: NaN for an empty bin)
        const double d = fabs(a - c);
        sc[b] = s;
        gap[b] = nb > 0 ? d : -1.0;
        term[b] = nb > 0 ? (double)nb / n * d : 0.0;
        if (diagram) {
            diagram[b] = nb > 0 ? (float)a : NAN;
            diagram[B + b] = nb > 0 ? (float)c : NAN;
        }
    }
    __syncthreads();
    if (b != 0) return;
    double ece = 0.0, mce = -1.0, cs = 0.0, tn = 0.0, tb = 0.0, te = 0.0;
    for (int i = 0; i < B; ++i) {
        ece += term[i];
        mce = gap[i] > mce ? gap[i] : mce;
        cs += sc[i];
    }
    for (int p = 0; p < P; ++p) {
        const double* st = sums + (int64_t)p * (B + 3) + B;
        tn += st[0];
        tb += st[1];
        te += st[2];
    }
    const bool none = !(n > 0.0);
    out[0] = none ? NAN : (float)((double)counts[1] / n);
    out[1] = none ? NAN : (float)(cs / n);
    out[2] = none ? NAN : (float)ece;
    out[3] = (none || mce < 0.0) ? NAN : (float)mce;
    out[4] = none ? NAN : (float)(tn / n);
    out[5] = none ? NAN : (float)(tb / n);
    out[6] = none ? NAN : (float)(te / n);
    out[7] = (float)n;
}

int sv_calib_finish(const int64_t* bin_count, const int64_t* bin_correct, const int64_t* counts, const double* sums, int P, int B, float* out,
                    float* diagram, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(bin_count && bin_correct && counts && sums, SV_E_ARG, "sv_calib_finish: a state (bin_count, bin_correct, counts, sums) is NULL");
    SV_REQUIRE(out, SV_E_ARG, "sv_calib_finish: out is NULL");
    SV_REQUIRE(B >= 1 && B <= CB_BMAX, SV_E_SHAPE, "sv_calib_finish: B=%d outside [1, %d]", B, CB_BMAX);
    SV_REQUIRE(P >= 1 && P <= CB_PMAX, SV_E_SHAPE, "sv_calib_finish: P=%d outside [1, %d]", P, CB_PMAX);
    hipLaunchKernelGGL(calib_finish_kernel, dim3(1), dim3(CB_BMAX), 0, (hipStream_t)stream, bin_count, bin_correct, counts, sums, P, B, out,
                       diagram);
    return sv_check_launch("sv_calib_finish");
}

// ------------------------------------------------------------------------------------------ sv_temp_accum
// Block p owns partial state p and walks the tiles p, p + P, ... of the call.  The 256 threads take the 64 rows of a tile 256 / G at a
// time (the row-on-a-group mapping above) and leave (a, v, nll) of every valid row in LDS; threads 0 .. 2 then add one quantity each
// over the 64 rows in index order in double, thread 3 counts.
template <int KIND, bool REG>
__global__ __launch_bounds__(CB_THREADS) void temp_accum_kernel(const float* __restrict__ x, int ldx, int N, int K, int lgG,
                                                                const int64_t* __restrict__ label, const double* __restrict__ beta,
                                                                double* sums, int64_t* count, int P, int init) {
    __shared__ float sq[3][64];
    __shared__ int sval[64];
    const int tid = threadIdx.x, G = 1 << lgG, li = tid & (G - 1), gi = tid >> lgG, RB = CB_THREADS >> lgG, p = blockIdx.x;
    const float bf = (float)beta[0];
    double acc = (!init && tid < 3) ? sums[p * 3 + tid] : 0.0;
    int64_t cnt = (!init && tid == 3) ? count[p] : 0;
    const int64_t ntiles = ((int64_t)N + 63) / 64;
    for (int64_t t = p; t < ntiles; t += P) {
        for (int r0 = 0; r0 < 64; r0 += RB) {
            const int rt = r0 + gi;
            const int64_t row = t * 64 + rt;
            const bool live = rt < 64 && row < N;
            const float* xr = x + (live ? row : (int64_t)N - 1) * ldx;
            const int64_t lab64 = live ? label[row] : -1;
            const int lab = (lab64 >= 0 && lab64 < K) ? (int)lab64 : -1;
            float u[CB_RV];
            float m = -INFINITY;
            int mi = INT_MAX, bad = 0;
            CB_EACH(i, k) {
                const float uk = cb_load<KIND>(xr, k);
                if (REG) u[i] = uk;
                const float v = bf * uk;
                bad |= (v != v) | (v == INFINITY);
                if (v > m) { m = v; mi = k; }
            }
            cb_gmax(m, mi, G);
            bad = cb_gor(bad, G) | (m == -INFINITY);
            float S = 0.f, SU = 0.f, ul = 0.f;
            CB_EACH(i, k) {
                const float uk = REG ? u[i] : cb_load<KIND>(xr, k);
                const float e = expf(bf * uk - m);
                S += e;
                if (e > 0.f) SU = fmaf(e, uk, SU);
                if (k == lab) ul = uk;
            }
            S = cb_gsum(S, G);
            SU = cb_gsum(SU, G);
            ul = cb_gsum(ul, G);
            const float mean = SU / S;
            float V = 0.f;
            CB_EACH(i, k) {
                const float uk = REG ? u[i] : cb_load<KIND>(xr, k);
                const float e = expf(bf * uk - m), d = uk - mean;
                if (e > 0.f) V = fmaf(e, d * d, V);
            }
            V = cb_gsum(V, G);
            if (li == 0 && rt < 64) {
                const bool ok = live && !bad && lab >= 0;
                sval[rt] = ok;
                sq[0][rt] = mean - ul;
                sq[1][rt] = V / S;
                sq[2][rt] = logf(S) - (bf * ul - m);
            }
        }
        __syncthreads();
        if (tid < 3) {
            for (int j = 0; j < 64; ++j)
                if (sval[j]) acc += (double)sq[tid][j];
        } else if (tid == 3) {
            for (int j = 0; j < 64; ++j) cnt += sval[j];
        }
        __syncthreads();                               // the tile is read
    }
    if (tid < 3) sums[p * 3 + tid] = acc;
    else if (tid == 3) count[p] = cnt;
}

int sv_temp_accum(int kind, const float* x, int ldx, int N, int K, const int64_t* label, const double* beta, double* sums, int64_t* count,
                  int P, int init, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(kind == SV_CAL_LOGIT || kind == SV_CAL_PROB, SV_E_ARG, "sv_temp_accum: unknown kind %d", kind);
    SV_REQUIRE(x && label && beta, SV_E_ARG, "sv_temp_accum: an input (x, label, beta) is NULL");
    SV_REQUIRE(sums && count, SV_E_ARG, "sv_temp_accum: a state (sums, count) is NULL");
    SV_REQUIRE(N > 0 && K > 0, SV_E_ARG, "sv_temp_accum: non-positive size (N=%d K=%d)", N, K);
    SV_REQUIRE(ldx >= K, SV_E_SHAPE, "sv_temp_accum: ldx=%d < K=%d", ldx, K);
    SV_REQUIRE(P >= 1 && P <= CB_PMAX, SV_E_SHAPE, "sv_temp_accum: P=%d outside [1, %d]", P, CB_PMAX);
    const int lgG = cb_group_log2(K);
    const bool reg = K <= (CB_RV << lgG);
#define CB_TEMP_LAUNCH(KIND, REG)                                                                                                      \
    hipLaunchKernelGGL((temp_accum_kernel<KIND, REG>), dim3(P), dim3(CB_THREADS), 0, (hipStream_t)stream, x, ldx, N, K, lgG, label, beta, \
                       sums, count, P, init)
    if (kind == SV_CAL_LOGIT) {
        if (reg) CB_TEMP_LAUNCH(SV_CAL_LOGIT, true); else CB_TEMP_LAUNCH(SV_CAL_LOGIT, false);
    } else {
        if (reg) CB_TEMP_LAUNCH(SV_CAL_PROB, true); else CB_TEMP_LAUNCH(SV_CAL_PROB, false);
    }
#undef CB_TEMP_LAUNCH
    return sv_check_launch("sv_temp_accum");
}

// ------------------------------------------------------------------------------------------ sv_temp_update
__global__ __launch_bounds__(64) void temp_update_kernel(const double* sums, const int64_t* count, int P, double* beta, float* temp,
                                                         float* stats) {
    if (threadIdx.x != 0) return;
    double A = 0.0, V = 0.0, Ls = 0.0;
    int64_t n = 0;
    for (int p = 0; p < P; ++p) {
        A += sums[p * 3];
        V += sums[p * 3 + 1];
        Ls += sums[p * 3 + 2];
        n += count[p];
    }
    const double b = beta[0];
    double bn = b;
    if (b > 0.0 && V > 0.0 && isfinite(A) && isfinite(V)) bn = fmin(fmax(b - A / V, 0.25 * b), 4.0 * b);
    beta[0] = bn;
    temp[0] = (float)(1.0 / bn);
    stats[0] = (float)(Ls / (double)n);                // (0 / 0: NaN without a valid row)
    stats[1] = (float)(A / (double)n);
    stats[2] = (float)(bn - b);
    stats[3] = (float)bn;
}

int sv_temp_update(const double* sums, const int64_t* count, int P, double* beta, float* temp, float* stats, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(sums && count, SV_E_ARG, "sv_temp_update: a state (sums, count) is NULL");
    SV_REQUIRE(beta && temp && stats, SV_E_ARG, "sv_temp_update: an output (beta, temp, stats) is NULL");
    SV_REQUIRE(P >= 1 && P <= CB_PMAX, SV_E_SHAPE, "sv_temp_update: P=%d outside [1, %d]", P, CB_PMAX);
    hipLaunchKernelGGL(temp_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, count, P, beta, temp, stats);
    return sv_check_launch("sv_temp_update");
}

// ------------------------------------------------------------------------------------------ sv_rank_scan
// Thread = query row, in a register.  Block (x, p) stages the gallery chunks p, p + P, ... of 1024 scores (and weights) in LDS; every
// thread reads the same element (a broadcast), compares, and keeps two private counts -- 32-bit per chunk without weights, 64-bit with
// them -- that leave the block as ONE integer atomic per row and count.  Elements beyond the end are staged as NaN: they count nowhere.
constexpr int RS_CHUNK = 1024;

template <bool WEIGHTED>
__global__ __launch_bounds__(CB_THREADS) void rank_scan_kernel(const float* __restrict__ q, int Q, const float* __restrict__ g,
                                                               const int64_t* __restrict__ g_w, int N, int P,
                                                               unsigned long long* greater, unsigned long long* equal) {
    __shared__ __attribute__((aligned(16))) float sg[RS_CHUNK];
    __shared__ __attribute__((aligned(16))) unsigned long long sw[WEIGHTED ? RS_CHUNK : 1];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * CB_THREADS + tid;
    const float qv = i < Q ? q[i] : NAN;
    unsigned long long gt = 0, eq = 0;
    for (int64_t c0 = (int64_t)blockIdx.y * RS_CHUNK; c0 < N; c0 += (int64_t)P * RS_CHUNK) {
        __syncthreads();                               // the previous chunk is read
        for (int j = tid; j < RS_CHUNK; j += CB_THREADS) {
            const bool in = c0 + j < N;
            sg[j] = in ? g[c0 + j] : NAN;
            if (WEIGHTED) sw[j] = in ? (unsigned long long)g_w[c0 + j] : 0ull;
        }
        __syncthreads();
        if (WEIGHTED) {
#pragma unroll 8
            for (int j = 0; j < RS_CHUNK; ++j) {
                const float gv = sg[j];
                const unsigned long long w = sw[j];
                gt += gv > qv ? w : 0ull;
                eq += gv == qv ? w : 0ull;
            }
        } else {
            unsigned cg = 0, ce = 0;
#pragma unroll 4
            for (int j = 0; j < RS_CHUNK; j += 4) {
                const f32x4 gv = *reinterpret_cast<const f32x4*>(&sg[j]);
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    cg += gv[n] > qv;
                    ce += gv[n] == qv;
                }
            }
            gt += cg;
            eq += ce;
        }
    }
    if (i < Q) {
        if (gt) atomicAdd(&greater[i], gt);
        if (eq) atomicAdd(&equal[i], eq);
    }
}

int sv_rank_scan(const float* q, int Q, const float* g, const int64_t* g_w, int N, int P, int64_t* greater, int64_t* equal, void* stream) {
    SvProfScope prof_scope(stream);
    SV_REQUIRE(q && g, SV_E_ARG, "sv_rank_scan: q or g is NULL");
    SV_REQUIRE(greater && equal, SV_E_ARG, "sv_rank_scan: an output (greater, equal) is NULL");
    SV_REQUIRE(Q > 0 && N > 0, SV_E_ARG, "sv_rank_scan: non-positive size (Q=%d N=%d)", Q, N);
    SV_REQUIRE(P >= 1 && P <= CB_PMAX, SV_E_SHAPE, "sv_rank_scan: P=%d outside [1, %d]", P, CB_PMAX);
    const dim3 grid((unsigned)(((int64_t)Q + CB_THREADS - 1) / CB_THREADS), P);
    unsigned long long* gr = reinterpret_cast<unsigned long long*>(greater);
    unsigned long long* er = reinterpret_cast<unsigned long long*>(equal);
    if (g_w)
        hipLaunchKernelGGL((rank_scan_kernel<true>), grid, dim3(CB_THREADS), 0, (hipStream_t)stream, q, Q, g, g_w, N, P, gr, er);
    else
        hipLaunchKernelGGL((rank_scan_kernel<false>), grid, dim3(CB_THREADS), 0, (hipStream_t)stream, q, Q, g, g_w, N, P, gr, er);
    return sv_check_launch("sv_rank_scan");
}
