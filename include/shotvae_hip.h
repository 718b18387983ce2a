/*
 * shotvae_hip.h  --  C ABI of libshotvae_hip.so: the MI355X (gfx950) compute path of the
 * SHOT-VAE training step.
 *
 * The reference (FengHZ/SHOT-VAE) is pure Python on torch.nn; it has no FFI.  Each entry point
 * below replaces the torch operator(s) that the cited reference lines dispatch (SURVEY.md §2.1
 * K1-K20).  Conventions for every function:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless noted;
 *   - asynchronous on `stream` (a hipStream_t passed as void*); no allocation, no host sync,
 *     no exceptions -- safe to capture into a hipGraph;
 *   - returns 0 on success, <0 on error (SV_E_*); sv_last_error() gives the message;
 *   - activations are NHWC with an explicit channel stride, element type `dtype`
 *     (SV_F32 exact-fp32 MFMA mode for parity, SV_BF16 throughput mode); statistics,
 *     parameters, gradients of parameters and loss terms are always fp32.
 */
#ifndef SHOTVAE_HIP_H
#define SHOTVAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_ABI_VERSION 8

enum { SV_F32 = 0, SV_BF16 = 1 };
/* ABI 6: the per-channel ACCUMULATORS of the BatchNorm statistics and backward sums (sv_igemm_args::stats / bsums / fold_stats,
 * sv_bn_finalize, sv_bn_branch::bsums, sv_pool_bwd, sv_bn_bwd_affine) are DOUBLES.  The partial sums of a launch's waves and
 * blocks meet there through atomic adds in an order that varies from run to run; as fp32 adds that order reached the results
 * (two repeats of the same bf16 step: 2e-5 relative in the forward scalars, amplified by 28 BatchNorm layers to a 0.97-0.98
 * cosine between the two gradients), as fp64 adds of fp32 partial sums it does not -- the additions are exact unless the
 * partial sums of one channel span more than ~2^29, so two runs agree bit for bit (measured) at no cost in time.            */
typedef double sv_acc_t;
enum { SV_OK = 0, SV_E_ARG = -1, SV_E_SHAPE = -2, SV_E_HIP = -3 };
enum { SV_MAX_TAPS = 16, SV_MAX_PHASES = 4 };

/* One sub-pixel phase of a (transposed / strided) convolution written as a gather-GEMM. */
typedef struct {
    int32_t ooy, oox;               /* output offset: oy = qy*osy + ooy                              */
    int32_t ntap;                   /* taps of this phase (0 => the phase's outputs are zero)        */
    int8_t dy[SV_MAX_TAPS];         /* input offset per tap: iy = qy*sy + dy[t] (zero outside)       */
    int8_t dx[SV_MAX_TAPS];
    int8_t torig[SV_MAX_TAPS];      /* tap index in the MASTER weight layout [N][T_orig][Cin]        */
    int64_t w_off;                  /* element offset of this phase's packed weights [N][ntap][Cin]  */
} sv_phase;

/* Geometry of one conv-like layer:  out[b, qy*osy+ooy, qx*osx+oox, n] =
 *     sum_{t,c} act(x[b, qy*sy+dy[t], qx*sx+dx[t], c]) * w[n][t][c]
 * The leading dimensions (ldx >= Cin, ldo >= N; sv_igemm: ldx % 8 == 0, ldo % 4 == 0; sv_wgrad: both % 8 == 0):
 *   - Columns [N, ldo) of every output pixel row belong to the caller and are not written.
 *   - Columns [Cin, ldx) of the input may hold anything and do not influence the result.
 *   - `residual` and `ex` have the output's layout, including ldo.
 * So `out = base + c0` with ldo = C_total is a channel-slice write into a wider tensor (the only reason the fields exist); a batched
 * launch strides its groups by B*Hin*Win*ldx and B*Hout*Wout*ldo elements.  Hin / Win and Hq / Wq are independent and need not be
 * powers of two: the specialised kernels decline what they do not cover (their *_try guards) and the generic kernels answer.
 * sv_bwd3x3 alone is restricted: square 8 / 16 / 32-pixel maps, ldx == Cin, ldo == N (SV_E_SHAPE otherwise).
 * (tests/test_conv_geometry_gpu.py)                                                                                         */
typedef struct {
    int32_t B, Hin, Win, Cin, ldx;          /* input  tensor [B,Hin,Win,ldx],  Cin  % 16 == 0        */
    int32_t Hq, Wq, sy, sx;                 /* per-phase output grid and input stride                */
    int32_t Hout, Wout, N, ldo, osy, osx;   /* output tensor [B,Hout,Wout,ldo], N % 16 == 0          */
    int32_t T_orig;                         /* taps in the master weight layout                      */
    int32_t nphase;
    sv_phase phase[SV_MAX_PHASES];
} sv_geom;

/* ---- K1/K2/K3/K12/K13 forward and every dgrad: fused gather-GEMM on MFMA -----------------------
 * Replaces nn.Conv2d / nn.ConvTranspose2d forward (wideresnet.py:13-14,29-30,34-35,41-43;
 * decoder.py:13-58) fused with the preceding BatchNorm2d-apply + LeakyReLU/ReLU (wideresnet.py:
 * 27-28,32-33,39-40; decoder.py:19-20,...) as a load prologue, and with the residual add
 * (wideresnet.py:49) and the *next* BatchNorm's batch statistics as an epilogue.  With the
 * `ex` fields set it is the conv/convT input-gradient fused with the activation backward and the
 * two BatchNorm-backward reductions (autograd of the same lines).                                  */
typedef struct {
    const void* x;              /* input activations                                                 */
    const float* pro_scale;     /* [Cin] BN-apply scale (NULL: no prologue)                          */
    const float* pro_shift;     /* [Cin]                                                             */
    float pro_slope;            /* LeakyReLU slope in [0,1] (0 = ReLU)                                     */
    const void* w;              /* packed weights, element type = dtype                              */
    const float* bias;          /* [N] or NULL                                                       */
    const void* residual;       /* same layout as out, or NULL                                       */
    void* out;
    sv_acc_t* stats;            /* [R][2N] += (sum y, sum y^2) or NULL; block b adds to replica b % R  */
    const void* ex;             /* act-backward epilogue: raw tensor at the output positions / NULL  */
    const float* ex_scale;      /* [N] each                                                          */
    const float* ex_shift;
    const float* ex_mean;
    const float* ex_rstd;
    float ex_slope;
    sv_acc_t* bsums;            /* [R][2N] += (sum g, sum g*xhat)                                    */
    int32_t replicas;           /* R: power of two >= 1; spreads the per-channel atomics of the many
                                   blocks of a launch over R copies (consumers sum the copies)        */
    int32_t groups;             /* G >= 1 (0 = 1): BATCHED launch of G independent instances of the layer that
                                   share the weights and the bias -- the four forwards of a SHOT-VAE step
                                   (main_shot_vae.py:288,311,329,356) each with its OWN BatchNorm statistics.
                                   g->B is the batch of ONE group; x / out / residual / ex hold the groups back
                                   to back ([G][B][H][W][ld]); pro_scale / pro_shift are [G][Cin], the ex_*
                                   vectors [G][N], stats / bsums [G][R][2N].                            */
    int32_t block_budget;       /* > 0: block budget of THIS launch if it takes a persistent kernel (conv3x3p, halop),
                                   overriding SV_OPT_PERSISTENT_BLOCKS -- the paired backward gives a layer's weight and
                                   data gradient half the chip each without touching process-wide state; 0 = the option */
    int32_t flags;              /* reserved: written by the library (bit 0 = deterministic accumulation of this launch) */
    int32_t sparse_out;         /* 1: output positions of phases WITHOUT taps are left unwritten (and their epilogue operands
                                   unread) instead of zero-filled -- the data gradient of a stride-2 1x1 convolution is zero at
                                   three of four positions; its only consumer, sv_bn_bwd_apply with sv_bn_branch::sparse = 1,
                                   does not read them.  0: every output position is written.                              */
    int32_t reserved0;          /* 0 (ABI 5's ex_mode: the recomputing data gradient lost to the streaming pass twice and left the tree) */
    /* ABI 4: BatchNorm finalisation FOLDED into the consumer.  fold_stats != NULL: the prologue's BatchNorm has not been
       finalised yet -- fold_stats [R = fold_replicas][2 Cin] are the raw (sum, sum of squares) its producer accumulated over
       fold_count samples per channel; pro_scale / pro_shift (and fold_mean / fold_rstd) are then OUTPUT locations [Cin]:
       scale = gamma * rstd, shift = beta - mean * scale, exactly sv_bn_finalize's arithmetic.  A kernel that supports it
       (the persistent 3x3 kernel of the narrow body layers) lets every block derive the coefficients of its channels
       itself -- a few dozen loads at its start instead of a launch of its own between two layers -- and block 0 stores the
       four vectors for the backward pass / sv_bn_running_update; for every other kernel sv_igemm runs sv_bn_finalize first.
       Groups: fold_stats [G][R][2 Cin], the outputs [G][Cin].  (main_shot_vae.py has 33 BatchNorms per forward.)          */
    const sv_acc_t* fold_stats;
    const float* fold_gamma;
    const float* fold_beta;
    float* fold_mean;
    float* fold_rstd;
    float fold_count;
    float fold_eps;
    int32_t fold_replicas;
    int32_t reserved1;
    /* ABI 5: start signal.  start_flag != NULL: the first block of the launch stores start_value to *start_flag (device
       memory, 4 bytes) as soon as it starts -- i.e. when everything enqueued on the stream before this launch has completed.
       A second stream that waits for the value (sv_stream_wait_flag) is thereby forked off IN FRONT of this launch without
       an event in this stream's queue: the weight gradient beside its data gradient (an event record costs the recording
       queue ~6 us of idle time in front of the next kernel on MI355X, 34 times per step).                                  */
    uint32_t* start_flag;
    uint32_t start_value;
    int32_t reserved2;
} sv_igemm_args;

int sv_igemm(const sv_geom* g, int dtype, const sv_igemm_args* a, void* stream);
/* The affine coefficients of a BatchNorm backward from its two sums (sv_igemm_args::bsums of the data gradient behind it, [G][R][2C],
 * replicas summed in index order):  with A = gamma * rstd, m1 = sum g / count, m2 = sum g xhat / count
 *     scale_g[g][c] = A,   scale_x[g][c] = -A * m2 * rstd,   shift[g][c] = -A * m1 + A * m2 * rstd * mean
 * so that scale_g * g + scale_x * x + shift = A * (g - m1 - xhat * m2), the autograd of wideresnet.py:27,32 -- the operands
 * dy_scale / dy_scale2 / dy_shift of sv_bwd3x3_args, which forms that BatchNorm backward in its load path instead of a pass of its own
 * (sv_bn_bwd_apply: two reads and a write of the tensor between two layers) -- and, what sv_bn_bwd_apply does on the side,
 * dbeta[c] += sum g, dgamma[c] += sum g xhat over all groups (either may be NULL).
 * (ABI 6 carried the same fusion as sv_igemm_args::x2 / sv_wgrad_args::dy2, each launch of the pair forming it for itself: one pass
 *  saved, two consumers taxed, slower in the step -- docs/lab_notes_r05.md; removed in ABI 7.)                                      */
int sv_bn_bwd_affine(const sv_acc_t* bsums, int replicas, int C, float count, const float* gamma, const float* mean, const float* rstd,
                     float* dgamma, float* dbeta, float* scale_g, float* scale_x, float* shift, int groups, void* stream);
/* The grid (blocks in x) sv_igemm WOULD launch for these arguments under the current options; nothing is launched.  With
 * SV_OPT_DETERMINISTIC the per-channel accumulators (`stats` / `bsums`) need replicas >= 4 * blocks (next power of two):
 * every wave of every block then adds to a replica of its own.                                                        */
int sv_igemm_query_blocks(const sv_geom* g, int dtype, const sv_igemm_args* a, int* blocks);

/* ---- K19 weight gradient: dW[n][torig][c] += sum_m dy[m][n] * act(x[m,t][c]) --------------------
 * Replaces autograd's convolution_backward (weight part) for the same layers.  `splits` = number
 * of M ranges of the generic kernel (0 = choose).  `ws` is an optional caller-owned fp32 workspace
 * (ws_elems floats, contents irrelevant on entry): stride-1 3x3 layers publish per-block partial
 * slabs there with plain stores and reduce them in a second launch instead of contending on float
 * atomics; without it (or when it is too small) partials go to dw through float atomics.
 * groups (0 = 1): batched launch as in sv_igemm_args -- x / dy hold G instances back to back (g->B = one group's
 * batch), pro_scale / pro_shift are [G][Cin]; the gradient of the shared weights sums over the groups.              */
int sv_wgrad(const sv_geom* g, int dtype, const void* x, const float* pro_scale, const float* pro_shift,
             float pro_slope, const void* dy, float* dw, int splits, int use_tr, float* ws, int64_t ws_elems,
             int groups, void* stream);

/* The same launch with its arguments in a struct (ABI 3): adds the per-launch block budget of the persistent weight-gradient
 * kernels (0 = SV_OPT_PERSISTENT_BLOCKS).  sv_wgrad(...) == sv_wgrad_ex with block_budget = 0.                          */
typedef struct {
    const void* x;
    const float* pro_scale;
    const float* pro_shift;
    float pro_slope;
    const void* dy;
    float* dw;
    int32_t splits;
    int32_t use_tr;
    float* ws;
    int64_t ws_elems;
    int32_t groups;
    int32_t block_budget;
} sv_wgrad_args;
int sv_wgrad_ex(const sv_geom* g, int dtype, const sv_wgrad_args* a, void* stream);

/* ---- fused backward of a narrow stride-1 3x3 convolution (ABI 7): data gradient + weight gradient in ONE launch ----------
 * Replaces, for the 32 -> 32 channel body convolutions of WideResNet-28-2 (wideresnet.py:29-35 under autograd; 8 / 16 / 32-pixel
 * maps) and the 64 -> 64 channel ones (16-pixel maps; C below is the channel count), the PAIR
 *     sv_igemm(geom_dgrad, x = dy, ex = raw input ...)   +   sv_wgrad_ex(geom_fwd, x = raw input, dy ...)
 * and, in the two-tensor form (dy2 != NULL), the sv_bn_bwd_apply pass in front of that pair too.  One persistent kernel stages a
 * tile of dy (with its halo) and of the raw input ONCE and feeds both products from the same LDS image: 3 tensor passes (4 in the
 * two-tensor form) where the pair makes 5 (8).  `g` is the layer's DATA-gradient geometry (one phase of nine taps); bf16 only.
 *   out[q][c]         = act'(x[q][c] * x_scale[c] + x_shift[c]) * sum_{t,n} dyeff[q + d(t)][n] * w[c][t][n]        (= sv_igemm's
 *                       ex epilogue, bit for bit), bsums[R][2C] += (sum out, sum out * (x - x_mean) * x_rstd)
 *   dw[n][torig(t)][c] += sum_q dyeff[q + d(t)][n] * act(x[q][c] * x_scale[c] + x_shift[c])
 *   dyeff = dy, or dy_scale[n] * dy + dy_scale2[n] * dy2 + dy_shift[n] (the coefficients of sv_bn_bwd_affine: the BatchNorm
 *           backward of the layer BEHIND the convolution; same expression and rounding as sv_igemm_args::x2 / sv_wgrad_args::dy2)
 * groups (0 = 1): as sv_igemm_args -- tensors [G][B][H][W][C], vectors [G][C], bsums [G][R][2C]; dw sums over the groups.
 * ws: caller-owned fp32 workspace of >= blocks * groups * 9 C^2 floats (blocks <= block_budget, default 256), contents irrelevant:
 * one partial slab per block, reduced into dw (+=, float atomics) by a second launch.  Not available under SV_OPT_DETERMINISTIC. */
typedef struct {
    const void* dy;             /* [G][B,H,W,32] gradient behind the convolution's output (or behind the BatchNorm after it)   */
    const void* dy2;            /* NULL, or that BatchNorm's raw input (= the convolution's own output)                         */
    const float* dy_scale;      /* [G][32] each; required with dy2                                                             */
    const float* dy_scale2;
    const float* dy_shift;
    const void* dy3;            /* NULL, or (with dy2) a third tensor ADDED to the two-tensor form: dyeff = dy_scale * dy + dy_scale2 *
                                   dy2 + dy_shift + dy3 -- for conv2 of a residual unit: (dy, dy2) = the data gradient behind the NEXT
                                   unit's norm1 and that BatchNorm's raw input (this unit's output), dy3 = the gradient arriving at the
                                   next unit's output: BatchNorm backward + skip connection of wideresnet.py:45-49 in the load path      */
    void* dy_out;               /* required with dy3: receives dyeff (the gradient at this unit's output: the previous unit's skip
                                   branch needs the tensor), every element written once                                                  */
    const void* x;              /* [G][B,H,W,32] RAW input of the BatchNorm in front of the convolution                        */
    const float* x_scale;       /* [G][32] each: that BatchNorm's scale / shift / mean / rstd (sv_bn_finalize)                 */
    const float* x_shift;
    const float* x_mean;
    const float* x_rstd;
    float x_slope;              /* LeakyReLU slope in [0, 1]                                                                   */
    const void* w;              /* the layer's data-gradient pack (sv_repack with geom_dgrad), bf16                            */
    void* out;                  /* [G][B,H,W,32]                                                                                */
    sv_acc_t* bsums;            /* [G][R][64]                                                                                   */
    int32_t replicas;
    int32_t groups;
    float* dw;                  /* master layout [32][9][32], += */
    float* ws;
    int64_t ws_elems;
    int32_t block_budget;       /* 0 = 256 */
    int32_t reserved0;
    /* ABI 8: the coefficients of the two- / three-tensor forms derived IN the launch (sv_bn_bwd_affine's arithmetic, every block from the
       raw sums; block 0 of a group adds dgamma / dbeta): one small launch less in front of every fused backward.  With fold_bsums set,
       dy_scale / dy_scale2 / dy_shift are not read (may be NULL). */
    const sv_acc_t* fold_bsums; /* NULL, or (with dy2) [G][fold_replicas][2C]: the backward sums of the BatchNorm BEHIND the convolution  */
    const float* fold_gamma;    /* [C]                                                                                               */
    const float* fold_mean;     /* [G][C]                                                                                            */
    const float* fold_rstd;     /* [G][C]                                                                                            */
    float* fold_dgamma;         /* [C], += ; may be NULL                                                                             */
    float* fold_dbeta;          /* [C], += ; may be NULL                                                                             */
    float fold_count;           /* elements per channel and group (B * H * W)                                                        */
    int32_t fold_replicas;
} sv_bwd3x3_args;
int sv_bwd3x3(const sv_geom* g, int dtype, const sv_bwd3x3_args* a, void* stream);

/* column sums: out[n] += sum_m y[m*ld + n]   (conv0 bias gradient)                                  */
int sv_colsum(int dtype, const void* y, int64_t M, int N, int ld, float* out, void* stream);

/* ---- K4 BatchNorm2d train-mode finalize (nn.BatchNorm2d semantics, eps/momentum explicit) -------
 * stats=[R][sum, sumsq] -> scale=gamma*rstd, shift=beta-mean*scale; saves mean/rstd; updates running
 * stats (unbiased var) unless running_mean is NULL.  groups (0 = 1): G sets of statistics [G][R][2C] of the same
 * BatchNorm (gamma / beta shared) -> outputs [G][C]; running_mean must then be NULL (sv_bn_running_update).   */
int sv_bn_finalize(const sv_acc_t* stats, int replicas, int C, float count, const float* gamma, const float* beta,
                   float eps, float momentum, float* running_mean, float* running_var,
                   float* scale, float* shift, float* mean, float* rstd, int groups, void* stream);
/* Deferred running-statistics update of all nbn BatchNorms of ONE forward from the (mean, rstd) that
 * sv_bn_finalize saved (called with running_mean = NULL): table[bn] = {offset of the BN's
 * [scale|shift|mean|rstd] block (each `align`-padded) in bnbuf, running_mean offset, running_var offset
 * (both into bufs), C}; counts[bn] = samples per channel.  Lets the four forwards of a step run on several
 * streams while the momentum updates are still applied in the reference's order (1)(2)(3)(4).  groups (0 = 1): each
 * of the four arrays of a block is [groups][C] (the block padded to `align` as a whole); the groups' updates are
 * applied in group order.                                                                                  */
int sv_bn_running_update(const int32_t* table, const float* counts, int nbn, const float* bnbuf, float* bufs,
                         float eps, float momentum, int align, int groups, void* stream);
/* The same with an explicit order of the momentum updates: order[k] = the group whose statistics the k-th forward of the
 * reference left (HOST array of `groups` ints, a permutation; NULL = group order).  A batched launch may hold the forwards
 * in any order -- e.g. (1)(3)(2)(4), so that the two forwards whose reconstruction enters the loss are adjacent -- and the
 * running statistics still receive the updates as the reference applies them.                                         */
int sv_bn_running_update_ex(const int32_t* table, const float* counts, int nbn, const float* bnbuf, float* bufs,
                            float eps, float momentum, int align, int groups, const int32_t* order, void* stream);
/* eval-mode affine from running statistics (main_shot_vae.py:409-510 path)                         */
int sv_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, float* scale, float* shift, void* stream);
/* BatchNorm-apply + LeakyReLU / ReLU as a pass of its own: out = act(x * scale[c] + shift[c]), x / out [groups][M][C]
 * (contiguous channels, C % 8 == 0), scale / shift [groups][C].  The conv-like kernels fuse this into their load prologue;
 * for weight-heavy layers (the first ConvTranspose layers of the decoder: a few MB of activations against MBs of weights)
 * the prologue is re-applied once per output-channel tile and bounds the GEMM (VALU), so the step materialises it once and
 * the GEMM runs prologue-free.                                                                                        */
int sv_bn_act(int dtype, const void* x, const float* scale, const float* shift, float slope, int64_t M, int C, void* out,
              int groups, void* stream);
/* BatchNorm backward, second phase: dx = sum_br gamma*rstd*(g - mean(g) - xhat*mean(g*xhat)) (+res)
 * for one or two BN branches that share the input x; dgamma/dbeta accumulate (+=).  groups (0 = 1): G instances,
 * M = rows of ONE group; x / g / residual / dx [G][M][ld], mean / rstd [G][C], bsums [G][R][2C].               */
typedef struct {
    const void* g; const sv_acc_t* bsums; const float* gamma; float* dgamma; float* dbeta;
    int32_t replicas;           /* bsums is [replicas][2C]                                           */
    int32_t sparse;             /* wlog + 1 > 0: g is the data gradient of a STRIDE-2 layer written with sv_igemm_args::
                                   sparse_out -- defined at the even (row, column) positions of the 2^wlog-wide, 2^wlog-high
                                   maps only and taken as zero elsewhere (not read there); 0: dense;
                                   -(wlog + 1) < 0 (ABI 5): the same positions stored COMPACTLY, g [M / 4][ld] -- the data
                                   gradient of a stride-2 1x1 layer computed as a dense 1x1 product over the stride-2 grid
                                   (its raw tensor gathered with sv_gather_even)                                       */
} sv_bn_branch;
int sv_bn_bwd_apply(int dtype, int64_t M, int C, int ld, const void* x, const float* mean,
                    const float* rstd, float count, const sv_bn_branch* br, int nbranch,
                    const void* residual, void* dx, int groups, void* stream);

/* ---- dropout between conv1 and norm2 of a wide unit (wideresnet.py:23-36, nn.Dropout(drop_rate)) ----------------------------
 * Masks are never stored: the forward and the backward regenerate them from a key, so nothing is saved and a captured graph
 * stays valid.  The mask of element e -- its flat NHWC index inside ITS group's [B][H][W][C] tensor (the channel stride ld
 * does not enter) -- is
 *     r = word (e & 3) of Philox-4x32-10(counter = (q_lo, q_hi, unit, 0), key = (key_lo, key_hi)),  q = e >> 2
 *     kept  <=>  r >= thr,     thr = (uint32)(p * 2^32) formed in double by the caller,   scale = (float)(1 / (1 - p))
 *     out = kept ? round_to_dtype((float)x * scale) : 0          (round to nearest even; the same mask in both dtypes)
 * key = keys[group] (an int64 in DEVICE memory, read by the kernels: a graph replays with whatever keys were drawn into it),
 * unit = the 0-based index of the wide unit in the encoder.  Every entry point refuses (SV_E_ARG / SV_E_SHAPE, nothing
 * launched): keys == NULL, p outside (0, 1), thr or scale inconsistent with p, C % 8 != 0.                                   */
typedef struct {
    const int64_t* keys;        /* [G]: the key of each group                                                                */
    int32_t unit;
    float p;
    float scale;
    uint32_t thr;
} sv_dropout_args;
/* out = dropout(x) (out may equal x: in place is the intended use) and, when stats != NULL, BatchNorm statistics of the STORED
 * values: stats [G][R][2C] += (sum, sum of squares) -- the layout the conv epilogue fills (sv_igemm_args::stats), so that
 * sv_bn_finalize / a folded consumer take them unchanged.  x / out [G][M][ld], M = rows of ONE group.  Block b adds to replica
 * b % R; under SV_OPT_DETERMINISTIC the blocks store their partial sums to slots and a second pass adds them in index order
 * (replica 0).                                                                                                               */
int sv_dropout_fwd(int dtype, const void* x, int64_t M, int C, int ld, const sv_dropout_args* a, void* out, sv_acc_t* stats,
                   int replicas, int groups, void* stream);
/* sv_bn_bwd_apply of the BatchNorm behind a dropout, with the dropout's backward applied to its result:
 * dx = kept ? dx_bn * scale : 0, rounded once.  residual must be NULL.                                                       */
int sv_bn_bwd_apply_dropout(int dtype, int64_t M, int C, int ld, const void* x, const float* mean, const float* rstd, float count,
                            const sv_bn_branch* br, int nbranch, const void* residual, void* dx, int groups,
                            const sv_dropout_args* a, void* stream);
/* the keep mask itself: out [G][M][C] bytes, 1 = kept (tests, tools; the step never materialises it)                        */
int sv_dropout_mask(const int64_t* keys, int unit, uint32_t thr, int64_t M, int C, int groups, uint8_t* out, void* stream);

/* out [B][H/2][W/2][C] = in [B][2y][2x][C]: the even positions of an NHWC tensor (C a multiple of 8)                      */
int sv_gather_even(int dtype, const void* in, int B, int H, int W, int C, void* out, void* stream);

/* ---- K8 global average pool fused with the transition BN+LeakyReLU (vae.py:107,143) ------------- */
/* groups (0 = 1): B = ALL images, image b belongs to group b / (B / groups); coefficients [G][C], bsums [G][2C]     */
int sv_pool_fwd(int dtype, const void* x, const float* scale, const float* shift, float slope,
                int B, int HW, int C, int ld, float* feat, int groups, void* stream);
int sv_pool_bwd(int dtype, const void* x, const float* scale, const float* shift, float slope,
                const float* mean, const float* rstd, const float* dfeat, int B, int HW, int C, int ld,
                void* g, sv_acc_t* bsums, int groups, void* stream);

/* ---- K9 the three inference heads + LogSoftmax (vae.py:10-15,144-146) ----------------------------
 * W is [2*ldc+K][C] (rows: mean, log_sigma, disc), bias [2*ldc+K].                                   */
int sv_head_fwd(const float* feat, int B, int C, const float* W, const float* bias, int ldc, int K,
                float* mu, float* ls, float* la, void* stream);
/* dW/dbias accumulate (+=); dout_ws is a caller-owned [B][2*ldc+K] fp32 workspace                    */
int sv_head_bwd(const float* feat, int B, int C, const float* W, int ldc, int K, const float* la,
                const float* dmu, const float* dls, const float* dla, float* dfeat, float* dW,
                float* dbias, float* dout_ws, void* stream);

/* ---- classifier tail (classifier_model/wideresnet.py:94-102, main_classifier.py:101): one Linear(C, K) that returns the raw
 * logits, and nn.CrossEntropyLoss() (mean) on int64 labels.  Added under ABI 8: new symbols only, no struct or signature changed.
 * sv_fc_fwd: logits [B][K] = feat [B][C] . W^T ([K][C]) + bias, fp32.
 * sv_fc_bwd: dfeat [B][C] = dlogits . W is WRITTEN; dW / dbias accumulate (+=) through the heads' weight-gradient kernel (in
 *   deterministic mode its 128-sample slices run one after the other).
 * sv_ce_fwd: row_loss[b] = logsumexp(logits[b]) - logits[b][label[b]] ([B], may be NULL); *loss is WRITTEN = their mean, summed
 *   by one block in a fixed order (no atomics, no pre-zeroed output, the same bits in every mode).  A label outside [0, K) is
 *   never used as an index: that row's loss, and so the mean, is NaN.
 * sv_ce_bwd: dlogits[b] = (softmax(logits[b]) - onehot(label[b])) * gout[0] / B (gout: device scalar); all zeros for a row whose
 *   label is outside [0, K).
 * Null pointers and non-positive sizes are refused before any launch.                                                      */
int sv_fc_fwd(const float* feat, int B, int C, const float* W, const float* bias, int K, float* logits, void* stream);
int sv_fc_bwd(const float* feat, int B, int C, const float* W, int K, const float* dlogits, float* dfeat, float* dW,
              float* dbias, void* stream);
int sv_ce_fwd(const float* logits, const int64_t* label, int B, int K, float* row_loss, float* loss, void* stream);
int sv_ce_bwd(const float* logits, const int64_t* label, int B, int K, const float* gout, float* dlogits, void* stream);

/* ---- K10/K11 reparameterisation sampler (vae.py:23-86) -------------------------------------------
 * mode 0: gumbel-softmax from u; 1: one-hot(label); 2: lam*onehot(label)+(1-lam)*onehot(label_mix).
 * latent is [B][Lpad] of `dtype` = [z | c | 0-pad]; csoft [B][K] fp32 keeps c for the backward.     */
/* lam_dev (optional, device scalar) overrides lam: keeps the step capturable into a hipGraph             */
int sv_sample_fwd(int dtype, const float* mu, const float* ls, const float* la, const float* eps,
                  const float* u, const int64_t* label, const int64_t* label_mix, float lam, const float* lam_dev, int mode,
                  float temperature, int B, int ldc, int K, int Lpad, void* latent, float* csoft,
                  void* stream);
/* dmu/dls/dla accumulate (+=) the sampler path of the latent gradient                              */
int sv_sample_bwd(int dtype, const void* dlatent, const float* ls, const float* eps, const float* csoft,
                  int mode, float temperature, int B, int ldc, int K, int Lpad,
                  float* dmu, float* dls, float* dla, void* stream);

/* Every group of a batched launch in ONE grid (added under ABI 8: new symbols and a new struct only).  The groups tile the rows
 * of mu / ls ([rows][ldc]), la / csoft ([rows][K]), eps and latent: group i covers rows [row0, row0 + rows), row0 = the end of
 * group i - 1 (0 for the first).  mode, lam / lam_dev as above; u ([rows][K], mode 0), label, label_mix ([rows], modes 1, 2) are
 * the GROUP's own arrays, indexed by the row within the group.  Each row is computed by the code of sv_sample_fwd / sv_sample_bwd:
 * the results equal one call per group, bit for bit.  The table is read on the host before the launch (not kept): capturable.
 * sv_sample_bwd_groups reads mode, row0 and rows only.                                                                        */
#define SV_MAX_SAMPLE_GROUPS 8
typedef struct {
    int32_t mode, row0, rows, reserved0;
    const float* u; const int64_t* label; const int64_t* label_mix;
    float lam; int32_t reserved1; const float* lam_dev;
} sv_sample_group;
int sv_sample_fwd_groups(int dtype, const float* mu, const float* ls, const float* la, const float* eps,
                         const sv_sample_group* groups, int ngroups, float temperature, int ldc, int K, int Lpad, void* latent,
                         float* csoft, void* stream);
int sv_sample_bwd_groups(int dtype, const void* dlatent, const float* ls, const float* eps, const float* csoft,
                         const sv_sample_group* groups, int ngroups, float temperature, int ldc, int K, int Lpad,
                         float* dmu, float* dls, float* dla, void* stream);

/* ---- inference: the decoder's input from a counter-based normal stream, and the decoder's output as an image (latent.hip).
 * Added under ABI 8: new symbols only, no struct or signature changed.  Both validate their arguments before any HIP call
 * (null pointers, non-positive sizes, Lpad < ldc + K, unknown mode / dtype: SV_E_ARG / SV_E_SHAPE, nothing launched), take a
 * stream and allocate nothing: they can be captured into a hipGraph.
 *
 * sv_latent_draw writes latent [B][Lpad] of `dtype` = [z | c | 0-pad] (sv_sample_fwd's layout; the pad columns are zeroed) and,
 * if z_out is not NULL, the fp32 z as [B][ldc]; the latent's z is that fp32 value rounded once.  ldc is arbitrary (not
 * necessarily a multiple of 4).
 *   z[b][d] = (mu ? mu[b][d] : 0) + (tau * (ls ? expf(ls[b][d]) : 1)) * n(row0 + b, d)          mu, ls: [B][ldc] fp32 or NULL
 * n(row, d), a standard normal that depends only on (key, row, d) -- rows row0 .. row0 + B - 1 drawn in one call equal the same
 * rows drawn in several calls, bit for bit:
 *   key  = *key, an int64 read FROM DEVICE MEMORY (a captured graph is replayed with another key by writing it there);
 *          key == NULL: n = 0 and z[b][d] = (mu ? mu[b][d] : 0) exactly, the posterior mean;
 *   r[0..3] = Philox-4x32-10(counter = (low32(row), high32(row), d >> 2, SV_LATENT_PHILOX_TAG), key = (low32(key), high32(key)))
 *          -- the generator of the dropout masks, whose fourth counter word is 0: the streams are disjoint;
 *   p = (d >> 1) & 1,   u1 = ((r[2p] >> 8) + 1) * 2^-24  in (0, 1],   u2 = (r[2p + 1] >> 8) * 2^-24  in [0, 1)   (exact in fp32)
 *   rad = sqrtf(-2 * logf(u1)),   ang = (float)(2 pi) * u2,   n = (d & 1) ? rad * sinf(ang) : rad * cosf(ang)      (Box-Muller)
 *          -- one generator call serves the four columns 4j .. 4j + 3: words 0, 1 columns 4j, 4j + 1; words 2, 3 the other two;
 *          u1 > 0, so every n is finite (|n| <= sqrt(48 ln 2) = 5.77).
 * The class part c [K], by `mode`:
 *   0  one-hot of label[b] (int64 [B]); a label outside [0, K) gives an all-zero class part;
 *   1  a copy of cls[b] (fp32 [B][K]), a soft class vector;
 *   2  one-hot of argmax_k cls[b][k]; the lowest index wins ties; NaN entries never win (a row of NaNs only: all zero).
 * tau must be finite and >= 0, row0 >= 0.                                                                                   */
#define SV_LATENT_PHILOX_TAG 0x4C41544Eu
int sv_latent_draw(int dtype, const float* mu, const float* ls, const int64_t* key, float tau, int64_t row0, int mode,
                   const int64_t* label, const float* cls, int B, int ldc, int K, int Lpad, void* latent, float* z_out,
                   void* stream);
/* sv_image_out reads NHWC `dtype` [B][H][W][ld] (first C channels: the last ConvTranspose's output) and writes either or both of
 *   out_f32  NCHW fp32 [B][C][H][W]: the raw values x (sigmoid = 0, exact) or s = 1 / (1 + expf(-x)) (sigmoid = 1);
 *   out_u8   NHWC uint8 [B][H][W][C] = floorf(255 * s + 0.5): the byte layout sv_augment reads, so generated images can be fed back
 * (the torch.sigmoid of main_shot_vae.py:381 and the layout change in one pass).  At least one output is required.            */
int sv_image_out(int dtype, const void* in, int B, int C, int H, int W, int ld, int sigmoid, float* out_f32, uint8_t* out_u8,
                 void* stream);

/* ---- per-image ELBO terms and the importance-weighted bound on log p(x) (score.hip).  Added under ABI 8: new symbols only, no
 * struct or signature changed.  All three validate their arguments before any HIP call (null pointers, non-positive sizes,
 * Lpad < ldc + K, unknown dtype / flag, a row range outside the sweep: SV_E_ARG / SV_E_SHAPE, nothing launched), take a stream and
 * allocate nothing: they can be captured into a hipGraph.  Every sum runs in a fixed order without atomics: bit-reproducible.
 *
 * The sweep enumerates the decoder's input rows J = (b * S + s) * Kd + k for image b < B, sample s < S and class row k < Kd, where
 * Kd = K (label == NULL: every class) or Kd = 1 (label[b], int64 [B]).  sv_latent_sweep writes rows J = j0 .. j0 + R - 1 of it
 * (a chunk; 0 <= j0, j0 + R <= B * S * Kd) as latent [R][Lpad] of `dtype` = [z_{b,s} | onehot | 0-pad], and lw[b][s] (fp32 [B][S],
 * the whole array's base is passed; the row with k == 0 writes its entry):
 *   z[b][s][d] = mu[b][d] + expf(ls[b][d]) * n(row0 + b, s, d)     in fp32; the latent holds that value rounded once to `dtype`
 *   lw[b][s]   = log p(z) - log q(z | x) = sum_d (n^2 / 2 - z^2 / 2 + ls[b][d])     on the fp32 z and n, summed in double
 *   onehot     = class k (sweep), or label[b] (a label outside [0, K) gives an all-zero class part, as in sv_latent_draw)
 * n(row, s, d), a standard normal that depends only on (key, row, s, d):
 *   r[0..3] = Philox-4x32-10(counter = (low32(row), high32(row), (s << 16) | (d >> 2), SV_SCORE_PHILOX_TAG), key = *key)
 *   and the word-to-column Box-Muller mapping of sv_latent_draw (above).  S <= 65536 and ldc <= 2^18 keep the two fields of the
 *   third counter word apart (anything larger: SV_E_SHAPE); the tag differs from SV_LATENT_PHILOX_TAG and from the dropout masks' 0.
 *   key is an int64 read FROM DEVICE MEMORY; key == NULL: n = 0, z = mu exactly and lw = sum_d (-mu^2 / 2 + ls).
 * mu, ls: fp32 [B][ldc], both required.  row0 >= 0 is the absolute index of image 0.                                          */
#define SV_SCORE_PHILOX_TAG 0x53434F52u
int sv_latent_sweep(int dtype, const float* mu, const float* ls, const int64_t* key, int64_t row0, const int64_t* label, int B, int S,
                    int K, int ldc, int Lpad, int64_t j0, int R, void* latent, float* lw, void* stream);
/* sv_recon_rows: nll[j], j < R, the reconstruction term of decoded row j -- NHWC `dtype` rec [R][H][W][ld], first C channels, the
 * logits r -- against image (j0 + j) / rows_per_image of the NCHW fp32 image [B][C][H][W] (values x); (j0 + R - 1) / rows_per_image
 * must be < B.
 *   bce = 1:  sum over C * H * W of  max(r, 0) - r * x + log1pf(expf(-|r|))              (BCE with logits; stable for any finite r)
 *   bce = 0:  sum of (1 / (1 + expf(-r)) - x)^2, times 1 / (2 x_sigma^2)                  (x_sigma finite and > 0)
 * Each term in fp32, the sum in double in a fixed order (lib/criterion.py:44-48 on a batch of one).                            */
int sv_recon_rows(int dtype, const void* rec, const float* image, int B, int64_t j0, int R, int64_t rows_per_image, int C, int H, int W,
                  int ld, int bce, float x_sigma, float* nll, void* stream);
/* sv_score_reduce: from nll [B][S][Kd] (Kd = K: the class sweep; Kd = 1: labelled), lw [B][S], la [B][K] (log q(y | x)), mu, ls
 * [B][ldc] it writes any of the fp32 [B] outputs (NULL skips one; at least one; lw may be NULL without log_px), with q_k = exp(la_k):
 *   kl_c   = 1/2 sum_d (mu^2 + exp(2 ls) - 2 ls - 1)
 *   kl_d   = sum_k q_k (la_k + log K)                                                    (a class with q_k = 0 contributes 0)
 *   recon  = 1/S sum_s sum_k q_k nll[s][k]   (Kd = K; a class with q_k = 0 is skipped: no 0 * inf)   |   1/S sum_s nll[s]  (Kd = 1)
 *   elbo   = -(recon + kl_c + kl_d)
 *   log_px = LSE_s( lw[s] + LSE_k(-nll[s][k] - log K) ) - log S + log_px_add   (Kd = K)   |   inner term -nll[s]  (Kd = 1)
 * LSE is a two-level log-sum-exp about the running maximum: a term of -inf has weight 0, a row of -inf only gives -inf (not NaN), a
 * term of +inf gives +inf; a NaN in nll, lw or la makes every output it enters NaN (it is never dropped).  One block per image, arithmetic in double.  log_px_add must be finite (MSE mode, normalised:
 * -(D / 2) log(2 pi x_sigma^2)).                                                                                              */
int sv_score_reduce(const float* nll, const float* lw, const float* la, const float* mu, const float* ls, int B, int S, int Kd, int K,
                    int ldc, double log_px_add, float* recon, float* kl_c, float* kl_d, float* elbo, float* log_px, void* stream);

/* ---- posterior distances and k-nearest neighbours in latent space (lib/utils/calculate_dist.py) ----------------
 * Added under ABI 8: new symbols only.  mu and ls are fp32 [rows][D] with row stride D; ls is LOG SIGMA (sigma^2 = exp(ls)^2, the
 * SHOT-VAE convention; half a smooth model's logvar).  The query comes first in every metric:
 *   SV_DIST_KL      kl[i][j] = KL(N(q_i) || N(g_j)) = sum_d (ls2 - ls1) + ((sigma1^2 + (mu1 - mu2)^2) / sigma2^2 - 1) / 2
 *                   (pairwise_norm_kl_dist_gpu)
 *   SV_DIST_W2      sum_d (mu1 - mu2)^2 + sum_d (sigma1 - sigma2)^2              (pairwise_norm_wasserstein_dist_gpu)
 *   SV_DIST_EUCLID  sum_d (mu1 - mu2)^2; ls is not read and may be NULL          (pairwise_square_euclidean_gpu)
 *   SV_DIST_COSINE  mu1 . mu2 / (|mu1|^2 |mu2|^2) -- the reference's formula, SQUARED norms -- a similarity: larger is closer; ls is not
 *                   read and may be NULL                                        (calculate_mean_dist_pairwise, distance="cosine")
 * All sums are over the differences themselves (no |a|^2 + |b|^2 - 2 a.b expansion): the Euclid and W2 distance of a row to itself is
 * exactly 0.  Products in fp32; 16 dimensions are summed in fp32 in index order, the 16-blocks in double in index order: the value of a
 * pair does not depend on the shape of the problem around it, and sv_pairdist and sv_knn_scan give the same bits for the same pair.
 *
 * sv_pairdist: out[i * ldo + j] (fp32, ldo >= N) = the metric of query i and gallery row j.  For small problems and reference parity.
 *
 * sv_knn_scan: merges the N gallery rows of this call -- row r has the global index col0 + r -- into the running lists best_val (fp32
 *   [Q][k]) and best_idx (int64 [Q][k]) of the k closest rows per query, closest first; the [Q][N] matrix is never stored.
 *   init != 0 empties the lists first (the caller need not initialise them); with init == 0 they are read as an earlier call left them.
 *   An empty slot is idx = -1 and val = +inf (-inf for the cosine).  Equal values order by the smaller global index.  A NaN value, a
 *   distance of +inf (a similarity of -inf) and, with self0 >= 0, the global index self0 + i for query i (leave-one-out over a gallery
 *   that holds the queries) never enter a list.  The lists are the k first pairs of a strict total order on (value, index): after a
 *   gallery has been scanned they hold the same bits however it was cut into calls.  1 <= k <= 256; any Q, N, D >= 1.
 *
 * sv_knn_vote: class votes of every query's neighbours.  A slot votes when 0 <= idx < n_gallery and its label g_label[idx] (int64) is
 *   in [0, K); its weight is 1 (mode 0), exp(-val / tau) (mode 1: distances) or exp(val / tau) (mode 2: the cosine similarity).
 *   votes (fp32 [Q][K], optional) = the sums in slot order; pred (int64 [Q], optional) = the first maximum of the votes, -1 when no slot
 *   voted.  With q_label (int64 [Q]): counts[0] += #(pred == q_label), counts[1] += Q (int64 [2]), confusion[q_label][pred] += 1 (int64
 *   [K][K]) for the rows with both indices in [0, K) -- the counting rules of sv_smooth_classify: integer atomics only, at most one per
 *   block and counter, a label outside [0, K) or a pred of -1 is a row and never a hit or a cell, the counters ACCUMULATE across calls.
 *   best_val may be NULL in mode 0.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): a null pointer, an unknown metric / mode, a NULL ls under KL
 * or W2, k outside [1, 256], a non-positive size, ldo < N, a negative col0, self0 < -1, tau not finite and > 0 in modes 1 / 2, no
 * output, counters without q_label.  No float atomics anywhere; each takes a stream and allocates nothing: capturable.              */
enum { SV_DIST_KL = 0, SV_DIST_W2 = 1, SV_DIST_EUCLID = 2, SV_DIST_COSINE = 3 };
int sv_pairdist(int metric, const float* q_mu, const float* q_ls, int Q, const float* g_mu, const float* g_ls, int N, int D, float* out,
                int64_t ldo, void* stream);
int sv_knn_scan(int metric, const float* q_mu, const float* q_ls, int Q, const float* g_mu, const float* g_ls, int N, int D, int64_t col0,
                int64_t self0, int k, float* best_val, int64_t* best_idx, int init, void* stream);
int sv_knn_vote(const float* best_val, const int64_t* best_idx, int Q, int k, const int64_t* g_label, int64_t n_gallery, int K, int mode,
                float tau, const int64_t* q_label, int64_t* pred, float* votes, int64_t* counts, int64_t* confusion, void* stream);

/* ---- the aggregate posterior q(z) = 1/N sum_j q(z | x_j) of a gallery of posteriors (aggpost.hip) ---------------
 * Added under ABI 8: new symbols only.  mu, ls, z are fp32 [rows][D] with row stride D; ls is LOG SIGMA, as in the sections above.
 *
 * sv_aggpost_sample: for query row i < Q and the sample index s,
 *   z[i][d] = mu[i][d] + expf(ls[i][d]) * n(row0 + i, s, d)      n: THE STREAM OF sv_latent_sweep (tag SV_SCORE_PHILOX_TAG, counter
 *             (low32(row), high32(row), (s << 16) | (d >> 2), tag), the same Box-Muller mapping; 0 <= s < 65536, D <= 2^18, anything
 *             larger: SV_E_SHAPE), so that (key, row, s) gives the sample score(samples = S, key = ...) uses; key (int64 in device
 *             memory) == NULL: n = 0 and z = mu exactly
 *   lqx[i]  = log q(z_i | x_i) = sum_d (-n^2 / 2 - ls) - D/2 log(2 pi)
 *   lpz[i]  = log p(z_i)       = sum_d (-z^2 / 2)      - D/2 log(2 pi)       terms in fp32, sums in double in index order; fp32 [Q]
 *
 * sv_aggpost_scan: the joint density.  The value of query i and gallery row j is
 *   v(i, j) = -1/2 sum_d (z_id - mu_jd)^2 exp(-2 ls_jd) - sum_d ls_jd - D/2 log(2 pi)          (= log N(z_i; mu_j, sigma_j^2))
 *   by sv_pairdist's one-value-per-pair rule: direct differences, 16 dimensions summed in fp32 with explicit fmaf in index order
 *   (fmaf((z - mu) * (z - mu), expf(-2 ls), sum)), the 16-blocks and the row scalar sum_d ls summed in double.
 *   A partial state is a running maximum m and s = sum exp(v - m) over the gallery rows merged into it so far: m, s double [P][Q].
 *   init != 0 empties the states first (m = -inf, s = 0; the caller need not initialise them); with init == 0 they are read as an
 *   earlier call left them.  The N rows of this call -- row r has the global index col0 + r -- are dealt to the P partial states in
 *   tiles of 64 rows (tile t to state t mod P): a fixed function of the arguments.  With self0 >= 0 the pair col0 + r == self0 + i is
 *   skipped (leave-one-out).  A term of -inf has weight 0; a term of +inf makes the state +inf; a NaN pair value makes that query's
 *   state NaN (m = NaN): it is never dropped.  1 <= P <= 64; P = 1 is valid.
 *
 * sv_aggpost_dims: the per-dimension marginals: the same arguments with states [P][Q][D] and, per (i, d), the fp32 term
 *   v_d(i, j) = fmaf((z_id - mu_jd)^2, -0.5f * expf(-2 ls_jd), -ls_jd - (float)(log(2 pi) / 2))
 *   -- one online log-sum-exp per (i, d), no sum over d.  The maximum is kept in fp32 (exact), the sum in double; a term's weight is
 *   exp(v - m) evaluated in fp32.  Rows are dealt to the states as in the scan; D <= 2^22.
 *
 * sv_aggpost_finish: out[r] = M + log(sum_p s_p exp(m_p - M)) - log(count), M = max_p m_p, for r < R over the states m, s [P][R]; in
 *   double, the partials in index order, rounded once to fp32.  A row whose partials are all empty gives -inf (not NaN), a +inf stays
 *   +inf, a NaN stays NaN.  R = Q serves the scan, R = Q * D the dims.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): a null pointer (key excepted), a non-positive size, a
 * negative col0 or row0, self0 < -1, s < 0, P outside [1, 64], count < 1.  Each takes a stream and allocates nothing: capturable.  No
 * atomics: two runs of the same call sequence give the same bits.                                                                  */
int sv_aggpost_sample(const float* mu, const float* ls, const int64_t* key, int64_t row0, int s, int Q, int D, float* z, float* lqx,
                      float* lpz, void* stream);
int sv_aggpost_scan(const float* z, int Q, const float* g_mu, const float* g_ls, int N, int D, int64_t col0, int64_t self0, double* m,
                    double* s, int P, int init, void* stream);
int sv_aggpost_dims(const float* z, int Q, const float* g_mu, const float* g_ls, int N, int D, int64_t col0, int64_t self0, double* m,
                    double* s, int P, int init, void* stream);
int sv_aggpost_finish(const double* m, const double* s, int P, int64_t R, int64_t count, float* out, void* stream);

/* ---- membership counts of k-th-neighbour balls: precision / recall, density / coverage (manifold.hip) -----------
 * Added under ABI 8: new symbols only.  mu and ls are fp32 [rows][D] with row stride D; ls is LOG SIGMA, as in the sections above.
 *
 * sv_ball_scan: gallery row j of this call -- global index col0 + j -- carries a ball of radius g_r[j] (fp32 [N], in the metric's own,
 *   squared, units: a value of sv_knn_scan's list).  v(i, j) is THE VALUE sv_pairdist GIVES THE PAIR, bit for bit (direct differences,
 *   16 dimensions in fp32 with explicit fmaf in index order, the 16-blocks in double in index order, rounded once to fp32).  Query i
 *   is inside ball j when
 *       v(i, j) is finite,   v(i, j) <= g_r[j],   and   col0 + j != self0 + i   (self0 = -1: no exclusion)
 *   so a NaN radius or value contains nothing, a radius of +inf every finite pair, a negative radius nothing, a radius of 0 the
 *   coincident rows only.  Then
 *       q_count[i] += the number of balls of the call that query i is inside        (int64 [Q])
 *       g_count[j] += the number of queries of the call inside ball j               (int64 [N])
 *   Either may be NULL, not both.  Both are ADDED TO (sv_knn_vote's rule for its counters): the caller zeroes them.  SV_DIST_EUCLID and
 *   SV_DIST_W2 only: KL is not symmetric (a k-th-neighbour radius has no single meaning under it) and the cosine is a similarity; both
 *   are refused.  The grid is ceil(Q / 64) x P blocks, gallery tile t (64 rows) of the call goes to block t mod P, 1 <= P <= 64.  The
 *   counts are integers of the pair set: a gallery cut into calls (col0, shifted g_r / g_count), a query set cut into calls (shifted
 *   q_count, self0 + the cut) and any P give identical results.  Counts meet in registers / LDS inside a block, which issues at most
 *   one integer atomic per row at its end and one per touched column and tile; no float atomics.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): an unknown, KL or cosine metric; NULL q_mu, g_mu or g_r;
 * a NULL ls under W2; both counters NULL; Q, N or D < 1; a negative col0; self0 < -1; P outside [1, 64]; col0 + N or self0 + Q beyond
 * the index (SV_E_SHAPE).  Takes a stream and allocates nothing: capturable.                                                        */
int sv_ball_scan(int metric, const float* q_mu, const float* q_ls, int Q, const float* g_mu, const float* g_ls, const float* g_r, int N,
                 int D, int64_t col0, int64_t self0, int P, int64_t* q_count, int64_t* g_count, void* stream);

/* ---- latent-space clustering: fused k-means and the contingency table of two partitions (cluster.hip) -----------
 * Added under ABI 8: new symbols only.  Rows x are fp32 [N][D] with row stride D, centroids c fp32 [K][D].  Squared Euclid only: the W2
 * distance of diagonal Gaussians is the squared Euclid distance of the concatenated rows [mu, exp(ls)] -- cluster those.
 *
 * sv_kmeans_assign: v(i, j) is THE VALUE sv_pairdist GIVES THE PAIR (x_i, c_j) UNDER SV_DIST_EUCLID, bit for bit (direct differences,
 *   16 dimensions in fp32 with explicit fmaf in index order, the 16-blocks in double in index order, rounded once to fp32).
 *       assign[i] = the smallest j that attains the minimum over the FINITE v(i, .); -1 when no value is finite (a NaN or infinite row,
 *                   every centroid NaN)                                                                            (int64 [N])
 *       dist[i]   = that minimum; +inf when assign[i] is -1                                                       (fp32 [N], may be NULL)
 *   The [N][K] matrix is never stored; K is tiled like sv_knn_scan's gallery: any K >= 1.  A row's result does not depend on the rows
 *   around it: rows cut into calls give the same bits.
 *
 * sv_kmeans_accum: the N rows of the call are dealt to the P partial states in tiles of 64 rows (tile t to state t mod P).  A state is
 *       sums    double [P][K][D]    sums[p][k][d] += (double)x[i][d] for the state's rows with assign[i] == k, IN ROW ORDER, one double
 *                                   add per (row, dimension)
 *       counts  int64  [P][K]       the number of those rows
 *       inertia double [P]          += (double)dist[i] over the state's rows with assign[i] in [0, K), in row order (may be NULL; needs dist)
 *   A row with assign[i] outside [0, K) is skipped.  init != 0 zeroes the states first (the caller need not initialise them); with
 *   init == 0 they continue as an earlier call left them.  Hence: a repeated call gives the same bits; with P = 1 the rows may be cut
 *   into calls at any multiple of 64, with P > 1 at any multiple of 64 P, and the states hold the bits of the one call.  No atomics.
 *   1 <= K <= 1024 (a block keeps [K][slice] doubles in LDS, slice = 64 dimensions for K <= 256, 32 for K <= 512, 16 beyond);
 *   1 <= P <= 64.
 *
 * sv_kmeans_finish: with n_k = sum_p counts[p][k] and s_kd = sum_p sums[p][k][d], both in index order (s in double):
 *       c_new[k][d] = (float)(s_kd / (double)n_k)     n_k > 0;      = c_old[k][d]     n_k == 0: an empty cluster KEEPS its centroid
 *       count[k]    = n_k                                                                                          (int64 [K])
 *       stats[0]    = (float) sum_k ( sum_d ((double)c_new[k][d] - (double)c_old[k][d])^2 )    in double; the inner sums over d in index
 *                     order, then the K inner sums in index order; rounded once
 *       stats[1]    = (float) sum_p inertia[p]    in double, index order; 0 when inertia is NULL                  (fp32 [2])
 *   c_new may alias c_old.  Between its two launches count[] carries the inner sums of stats[0]; it holds n_k when the call's work is done.
 *
 * sv_contingency: table[a[i]][b[i]] += 1 (int64 [Ka][Kb]) for the rows with a[i] in [0, Ka) and b[i] in [0, Kb); counts[0] += the number
 *   of such rows, counts[1] += N (int64 [2]).  a, b: int64 [N].  Everything ACCUMULATES (the caller zeroes), under sv_knn_vote's counting
 *   rules: integer atomics only, a block counts its rows privately and issues at most one atomic per touched cell at its end.
 *   Ka * Kb <= 2^20.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): a null pointer (dist and inertia excepted; an inertia
 * without dist), a size < 1, K > 1024 for the accumulation, P outside [1, 64], Ka * Kb > 2^20 (SV_E_SHAPE).  No float atomics anywhere;
 * each takes a stream and allocates nothing: capturable; a repeated call sequence gives the same bits.                              */
int sv_kmeans_assign(const float* x, int N, const float* c, int K, int D, int64_t* assign, float* dist, void* stream);
int sv_kmeans_accum(const float* x, const int64_t* assign, const float* dist, int N, int D, int K, double* sums, int64_t* counts,
                    double* inertia, int P, int init, void* stream);
int sv_kmeans_finish(const double* sums, const int64_t* counts, const double* inertia, int P, int K, int D, const float* c_old,
                     float* c_new, int64_t* count, float* stats, void* stream);
int sv_contingency(const int64_t* a, const int64_t* b, int N, int Ka, int Kb, int64_t* table, int64_t* counts, void* stream);

/* ---- calibration, temperature scaling and rank counts for the class posterior q(y | x) (calib.hip) ---------------
 * Added under ABI 8: new symbols only.  x is fp32 [N][ldx]; only the first K columns of a row are ever read (ldx >= K).
 *   kind SV_CAL_LOGIT   u = x          logits or log-probabilities
 *        SV_CAL_PROB    u = log(x)     probabilities, x >= 0 (a zero is a class of probability 0; a negative entry makes the row NaN)
 *
 * sv_calib_rows: with T = *temp (a DEVICE float, read on the device: a captured call follows a refitted temperature; NULL: T = 1),
 *   z = u / T in fp32 and p = softmax(z):
 *       pred[i]    = the smallest k that attains max_k z_k                                                       (int64 [N])
 *       conf[i]    = p[pred]                entropy[i] = -sum_k p_k log p_k,  0 log 0 = 0                        (fp32 [N] each)
 *       nll[i]     = -log p[label]          brier[i]   = sum_k (p_k - [k == label])^2      for a label[i] in [0, K)
 *   A row whose K entries hold a NaN or +inf, or nothing but -inf -- or any row when T is not > 0 -- gives pred = -1 and NaN elsewhere.
 *   A finite row whose label is outside [0, K), or label == NULL, gives NaN for nll and brier only.  Every output pointer is optional;
 *   one at least must be given; an output that is NULL is not written.  Any K >= 1: a row is taken by min(64, the power of two >= K)
 *   neighbouring lanes, and up to 256 classes are read once.  A row's result does not depend on the rows around it.
 *
 * sv_calib_accum: a row is VALID when pred[i] >= 0 and label[i] is in [0, K).  Its bin is b = #{ i in 1 .. B-1 : edges[i] < conf[i] }
 *   (edges fp32 [B + 1], NON-DECREASING; only the inner edges are read, compared in fp32: intervals (lo, hi], every value lands in a bin).
 *       bin_count[b] += 1      bin_correct[b] += (pred == label)                                                 (int64 [B] each)
 *       counts[0..2] += (valid rows, rows with pred == label among them, N)                                      (int64 [3])
 *   These are integer adds: exact, they ACCUMULATE (the caller zeroes them; `init` does not touch them).
 *       sums   double [P][B + 3]    [p][b] += (double)conf[i] for the state's valid rows of bin b; [p][B], [p][B + 1], [p][B + 2] +=
 *                                   (double)nll[i], brier[i], entropy[i] of the state's valid rows
 *   under sv_kmeans_accum's partial-state rule: tile t (64 rows) of the call goes to state t mod P; inside a state the rows are added in
 *   index order, one double add per row and quantity; init != 0 zeroes the states first, otherwise they continue.  nll, brier and entropy
 *   may be NULL: that total is left untouched (zero after init).  Hence: a repeated call gives the same bits; with P = 1 the rows may be
 *   cut into calls at any multiple of 64, with P > 1 at any multiple of 64 P.  No float atomic.
 *
 * sv_calib_finish: with n_b = bin_count[b], k_b = bin_correct[b], s_b = sum_p sums[p][b] (index order), n = counts[0]; acc_b = k_b / n_b,
 *   conf_b = s_b / n_b, everything in double and rounded once:
 *       out[0..7] = counts[1] / n,  (sum_b s_b) / n,  ECE = sum_b n_b / n |acc_b - conf_b|,  MCE = max over n_b > 0 of |acc_b - conf_b|,
 *                   the means of nll, brier and entropy (sum_p sums[p][B + .] / n),  (float)n                    (fp32 [8])
 *       diagram   = acc_b, then conf_b; NaN for an empty bin                                                     (fp32 [2][B], may be NULL)
 *   the sums over b in bin order.  With n == 0 out[0..6] are NaN.
 *
 * sv_temp_accum: with beta = *beta (a DEVICE double, 1 / T; used as (float)beta) and p = softmax(beta u) in fp32, per row with a finite
 *   u (the rule of sv_calib_rows) and a label in [0, K):
 *       a = E_p[u] - u[label]      v = sum_k p_k (u_k - E_p[u])^2      nll = -log p[label]
 *   sums double [P][3] += (a, v, nll) and count int64 [P] += 1 under the partial-state rule above (init zeroes both).  The sums of a and v
 *   are dL/dbeta and d2L/dbeta2 of the summed NLL L(beta), which is convex in beta.
 *
 * sv_temp_update: one block.  A, V, L, n = the states merged in index order.  beta_new = beta - A / V clamped to [beta / 4, 4 beta] when
 *   beta > 0, V > 0 and A, V are finite; beta otherwise.  Writes *beta = beta_new, *temp = (float)(1 / beta_new) -- the pointer
 *   sv_calib_rows reads -- and stats[0..3] = L / n (at the OLD beta), A / n, beta_new - beta, beta_new (fp32 [4]; NaN means for n == 0).
 *   A fit of `iters` iterations is 2 iters launches and no host read.
 *
 * sv_rank_scan: greater[i] += sum_j w_j [g_j > q_i], equal[i] += sum_j w_j [g_j == q_i] (int64 [Q] each; they ACCUMULATE, the caller
 *   zeroes them).  q fp32 [Q], g fp32 [N], g_w int64 [N], non-negative (NULL: every weight 1).  IEEE comparisons: a NaN on either side
 *   counts nowhere, infinities compare as numbers, -0 == 0.  The [Q][N] matrix is never stored; the gallery is staged through LDS in
 *   chunks of 1024, chunk c by the blocks of grid row c mod P; a block issues one integer atomic per row and count.  Exact, and
 *   independent of P, of the grid and of any cut of the gallery into calls.  The weights are a MASK: no caller compacts a gallery.
 *
 * Validated before any HIP call (nothing launched): a NULL required pointer, a size < 1 (N, K, Q), an unknown kind: SV_E_ARG; ldx < K, B
 * outside [1, 1024], P outside [1, 64]: SV_E_SHAPE.  Each takes a stream and allocates nothing: capturable.                            */
enum { SV_CAL_LOGIT = 0, SV_CAL_PROB = 1 };
int sv_calib_rows(int kind, const float* x, int ldx, int N, int K, const float* temp, const int64_t* label, int64_t* pred, float* conf,
                  float* nll, float* brier, float* entropy, void* stream);
int sv_calib_accum(const float* conf, const int64_t* pred, const int64_t* label, const float* nll, const float* brier, const float* entropy,
                   int N, int K, const float* edges, int B, int64_t* bin_count, int64_t* bin_correct, int64_t* counts, double* sums, int P,
                   int init, void* stream);
int sv_calib_finish(const int64_t* bin_count, const int64_t* bin_correct, const int64_t* counts, const double* sums, int P, int B, float* out,
                    float* diagram, void* stream);
int sv_temp_accum(int kind, const float* x, int ldx, int N, int K, const int64_t* label, const double* beta, double* sums, int64_t* count,
                  int P, int init, void* stream);
int sv_temp_update(const double* sums, const int64_t* count, int P, double* beta, float* temp, float* stats, void* stream);
int sv_rank_scan(const float* q, int Q, const float* g, const int64_t* g_w, int N, int P, int64_t* greater, int64_t* equal, void* stream);

/* ---- t-SNE of the latent space: input affinities and one exact gradient-descent iteration (tsne.hip) --------------
 * Added under ABI 8: new symbols only.  van der Maaten & Hinton 2008 with the sparse input affinities of van der Maaten 2014; the
 * defaults of the Python layer are scikit-learn 1.7's.  d_ij is the value the index's metric gives the pair, used as is (the squared
 * Euclid distance, KL, W2).  The embedding y is fp32 [N][d], d in {2, 3}.
 *
 * sv_tsne_affinity: dist fp32 [N][k], idx int64 [N][k]: a row's k-list, closest first.  A slot with idx < 0 or a dist that is not
 *   finite is INVALID: p = 0.  Over the valid slots, with x_j = (double)d_ij - (double)d_i,min,
 *       p_j|i = e_j / S,   e_j = exp(-beta_i x_j)  (1 where x_j == 0, whatever beta_i),   S = sum_j e_j
 *       H_i   = log S + beta_i (sum_j x_j e_j) / S        (the Shannon entropy of p_.|i in nats; 0 for the second term when its sum is 0)
 *   beta_i by scikit-learn's bisection, everything in double: beta = 1, bracket (-inf, +inf); at most max_steps evaluations of H; stop
 *   when |H - log(perplexity)| <= tol; H too large: lo = beta, beta = 2 beta while hi = +inf, else (beta + hi) / 2; H too small: hi =
 *   beta, beta = beta / 2 while lo = -inf, else (beta + lo) / 2.  After the last evaluation beta is NOT moved again:
 *       p      fp32   [N][k]   the double results at the returned beta, rounded once
 *       beta   double [N]      the beta of the last evaluation
 *       steps  int32  [N]      the number of evaluations when the stop rule was met; max_steps when it never was
 *   A row with fewer than two valid slots: p = 1 on its valid slot (if any), beta = 1, steps = max_steps.  A sum over the row: slot j
 *   belongs to lane j mod 64, a lane adds its slots in slot order, the 64 lane sums meet in a butterfly (xor 32, .., 1).  A row's result
 *   depends on that row alone.  1 <= k <= 256, 1 < perplexity < k, tol >= 0, max_steps >= 1.
 *
 * Low-dimensional side: r2_ij = sum_c (y_ic - y_jc)^2 over the differences themselves, explicit fmaf from 0 in dimension order;
 *   w_ij = 1 / (1 + r2_ij) by the HARDWARE RECIPROCAL AND ONE NEWTON STEP, w = fma(w0, fma(-a, w0, 1), w0) with a = 1 + r2: exact where
 *   1 / a is a power of two.  Z = sum over i != j of w_ij.  A pair is left out because i == j AS INDICES, never because r2 == 0:
 *   duplicated points repel with force 0 and count 1 each into Z.  The joint P = (P_cond + P_cond^T) / (2N) comes as CSR (rowptr int64
 *   [N + 1], non-decreasing from 0; col int64; val fp32): shot_vae_amd.embed.symmetrize.
 *
 * sv_tsne_attract: per row i over ITS segment q = rowptr[i] .. rowptr[i + 1] - 1, j = col[q], P = val[q] (an entry with j outside [0, N)
 *   is skipped):
 *       attr[i][c] = (float) sum_q (double)((P w_ij) (y_ic - y_jc))                                               (fp32 [N][d])
 *       rowkl[i]   = (float) sum_q (double)(P logf(P (1 + r2_ij)))      over the entries with P > 0                (fp32 [N])
 *   each term in fp32, the sums in double: lane s of the row's eight lanes adds the entries s, s + 8, .. in order, the eight lane sums meet
 *   in a butterfly (xor 4, 2, 1).  Degrees are unbounded.  No scatter, no atomic; a row's result is a function of its segment and y.
 *
 * sv_tsne_repulse: the all-pairs scan.  Column tile t (64 points) goes to partial state t mod P (sv_kmeans_accum's rule):
 *       rep[p][i][c] = sum_j w_ij^2 (y_ic - y_jc)     z[p][i] = sum_j w_ij       over the columns j != i of state p's tiles
 *   in fp32, IN COLUMN ORDER (rep by fmaf(w^2, y_ic - y_jc, .), z by one add per column) from 0.       (fp32 [P][N][d], fp32 [P][N])
 *   Columns >= N are masked out (w = 0), not placed far away.  The [N][N] matrix never exists.  1 <= P <= 64.
 *
 * sv_tsne_update: hyper is a DEVICE fp32 [3] = (exaggeration e, momentum, learning rate), read on the device: a captured call follows
 *   a rewritten hyper.  With R_ic = sum_p rep[p][i][c] and Z_i = sum_p z[p][i] in double in index order, nb = ceil(N / 256) and
 *   SUM(v) = the blocks' binary trees over 256 rows each, the nb block values added by thread t = b mod 256 in index order and one more
 *   tree (a fixed order that depends on N alone), all in double:
 *       Z        = SUM(Z_i)               g_ic = 4 (e attr[i][c] - R_ic / Z)    (the second term 0 when Z is not > 0: N = 1)
 *       inc      = (double)vel * g < 0    gain = max(inc ? gain + 0.2f : gain * 0.8f, 0.01f)                        (fp32)
 *       vel      = (float)(momentum vel - lr gain g)     in double, rounded once;      y += vel      (fp32; no recentring)
 *       stats[0] = (float)(SUM(rowkl[i]) + log Z)   the KL of the UNEXAGGERATED P at the y the call STARTED from
 *       stats[1] = (float)Z        stats[2] = (float)SUM(sum_c g_ic^2)                                             (fp32 [3])
 *   y, vel and gain are updated in place.  scratch: caller-provided double [3 nb] (shot_vae_amd.embed.update_scratch(N)), overwritten.
 *   Three launches.  y must be finite, and so must every r2 (|y| < 1e19): a NaN or an overflow propagates into y and stats as NaN;
 *   nothing loops on data, nothing hangs or faults on it.
 *
 * Validated before any HIP call (nothing launched): a NULL pointer (col and val are read only through rowptr), N < 1, k outside
 * [1, 256], perplexity outside (1, k), tol < 0, max_steps < 1, P outside [1, 64]: SV_E_ARG; d outside {2, 3}: SV_E_SHAPE.  No atomics
 * anywhere; each takes a stream and allocates nothing: capturable; a repeated call sequence gives the same bits.                    */
int sv_tsne_affinity(const float* dist, const int64_t* idx, int N, int k, double perplexity, double tol, int max_steps, float* p,
                     double* beta, int* steps, void* stream);
int sv_tsne_attract(const float* y, int N, int d, const int64_t* rowptr, const int64_t* col, const float* val, float* attr, float* rowkl,
                    void* stream);
int sv_tsne_repulse(const float* y, int N, int d, int P, float* rep, float* z, void* stream);
int sv_tsne_update(float* y, float* vel, float* gain, const float* attr, const float* rowkl, const float* rep, const float* z, int P, int N,
                   int d, const float* hyper, double* scratch, float* stats, void* stream);

/* ---- diagonal Gaussian mixtures on the latent space, fitted by fused EM (mixture.hip) ---------------------------
 * Added under ABI 8: new symbols only.  Rows x are fp32 [N][D] with row stride D; every matrix has row stride = its width.
 *   the model            logw fp32 [K] (log mixing weights; -inf: a component that takes part in nothing), mean [K][D], var [K][D]
 *   the derived table    ivar [K][D], cst [K], cdf [K] -- what the scans and the sampler read
 *
 * THE VALUE OF A PAIR, the same bits wherever it is formed (one device function serves both scans):
 *       v(i, k) = cst_k - 1/2 sum_d (x_id - mean_kd)^2 ivar_kd
 *   under sv_pairdist's summation rule: direct differences, 16 dimensions in fp32 as fmaf(dm * dm, ivar_kd, .) in index order, the
 *   16-blocks in double in index order, then (float) fma(-0.5, sum, (double) cst_k): rounded once.  cst_k = -inf gives v = -inf.  A
 *   sum that is NaN or infinite -- a row with a NaN or infinite entry -- gives v = NaN for every k.
 *
 * sv_gmm_prepare:  ivar = 1 / var in fp32;
 *       cst_k = (float)(logw_k - 1/2 (D log 2 pi + sum_d log var_kd))      in double, d in index order, rounded once
 *       cdf_k = (float)(sum_{j <= k} exp(logw_j) / sum_j exp(logw_j))      in double, index order, rounded once; the LAST component of
 *               positive weight gets exactly 1
 *   Between its two launches (cst[k], cdf[k]) carry the two halves of the double sum_d log var_kd.
 *
 * sv_gmm_estep:  lse[i] = log sum_k exp v(i, k) as an online log-sum-exp over tiles of 64 components in index order: the maximum in fp32,
 *   the sum in double, expf on fp32 differences; lse = (float)((double) max + log(sum)), rounded once.       (fp32 [N])
 *       assign[i] = the smallest k that attains the maximum over the FINITE v(i, .)                         (int64 [N], may be NULL)
 *       resp[i][k] = expf(v(i, k) - lse[i])                                                                 (fp32 [N][K], may be NULL)
 *   A row with a NaN or infinite entry gives lse = NaN, assign = -1 and a NaN resp row; a row for which every component has weight 0
 *   gives lse = -inf, assign = -1.  K is tiled: any K >= 1; the [N][K] matrix exists only when resp is passed.  A row's result does not
 *   depend on the rows around it: rows cut into calls give the same bits.
 *
 * sv_gmm_accum:  recomputes v and r_ik = expf(v(i, k) - lse[i]) -- bit-equal to sv_gmm_estep's resp -- and adds into P partial states
 *   under sv_kmeans_accum's rule: tile t of 64 rows goes to state t mod P; inside a state the rows are added in index order.  State p is
 *   sums + p (K (2 D + 1) + 1), doubles:
 *       [k (2 D + 1)]                  += (double) r
 *       [k (2 D + 1) + 1 + d]          += (double) r * (double) x_d                       (the product is exact)
 *       [k (2 D + 1) + 1 + D + d]      += ((double) r * (double) x_d) * (double) x_d      (the second product rounded, then added)
 *       [K (2 D + 1)]  -- THE LAST DOUBLE OF THE STATE --  += (double) lse[i]   over the finite rows, in row order
 *   one double add per (row, accumulator), never fused with the products; and counts int64 [P][2]: [p][0] += the rows added, [p][1] += the
 *   rows skipped because lse[i] is not finite.  init != 0 zeroes the states first; with init == 0 they continue.  Hence a repeated call
 *   gives the same bits; with P = 1 the rows may be cut at any multiple of 64, with P > 1 at any multiple of 64 P, and the states hold the
 *   bits of the one call.  No atomic of any kind.  1 <= P <= 64; D <= 2^20 (a block owns 32 dimensions: the grid's second dimension) and
 *   K (2 D + 1) < 2^31 (SV_E_SHAPE beyond).
 *
 * sv_gmm_finish:  scikit-learn's M-step for covariance_type="diag", in double, the P states merged in index order, IN PLACE on the model:
 *       n_k    = sum_p r-sums + 10 DBL_EPSILON         mean_kd = (float)(S1_kd / n_k)
 *       var_kd = (float)((S2_kd / n_k - (S1_kd / n_k)^2) + reg_covar)                     logw_k = (float) log(n_k / sum_k n_k)
 *   and then ivar, cst, cdf from those fp32 values as sv_gmm_prepare writes them.  A component whose r-sums add up to exactly 0 keeps its
 *   mean and var, gets logw = -inf and has no share in sum_k n_k.  stats fp32 [4]:
 *       [0] the mean of lse over the finite rows (scikit-learn's lower_bound_ at the parameters the E-step used; NaN without a finite row)
 *       [1] the number of finite rows      [2] the number of skipped rows      [3] the smallest var written (+inf if none was)
 *
 * sv_gmm_sample:  z[b][d] = fmaf(sqrtf(var[c][d]), n(row0 + b, d), mean[c][d]), n = sv_latent_draw's counter and Box-Muller mapping under
 *   SV_GMM_PHILOX_TAG (disjoint from the draw, score and dropout streams).  c = the first k with cdf_k > u (K - 1 if there is none),
 *       u = (r[0] >> 8) * 2^-24,   r = Philox-4x32-10(counter = (low32(row), high32(row), 0xFFFFFFFF, SV_GMM_PHILOX_TAG), key = *key)
 *   D <= 2^30 keeps d >> 2 away from 0xFFFFFFFF (SV_E_SHAPE beyond).  key is an int64 read FROM DEVICE MEMORY (required).  A row depends
 *   only on (key, row0 + b).  comp (int64 [B], may be NULL) returns c.  A component of weight 0 is never drawn.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): a null pointer other than assign, resp, comp; a size < 1; P
 * outside [1, 64]; a negative row0; reg_covar negative or not finite; the limits above.  Each takes a stream and allocates nothing:
 * capturable; a repeated call sequence gives the same bits.                                                                          */
#define SV_GMM_PHILOX_TAG 0x474D4D58u
int sv_gmm_prepare(const float* logw, const float* mean, const float* var, int K, int D, float* ivar, float* cst, float* cdf, void* stream);
int sv_gmm_estep(const float* x, int N, const float* ivar, const float* mean, const float* cst, int K, int D, float* lse, int64_t* assign,
                 float* resp, void* stream);
int sv_gmm_accum(const float* x, const float* lse, int N, const float* ivar, const float* mean, const float* cst, int K, int D, double* sums,
                 int64_t* counts, int P, int init, void* stream);
int sv_gmm_finish(const double* sums, const int64_t* counts, int P, int K, int D, double reg_covar, float* logw, float* mean, float* var,
                  float* ivar, float* cst, float* cdf, float* stats, void* stream);
int sv_gmm_sample(const float* mean, const float* var, const float* cdf, int K, int D, const int64_t* key, int64_t row0, int B, float* z,
                  int64_t* comp, void* stream);

/* ---- linear probes on the latent space: fused softmax regression (probe.hip) -------------------------------------
 * Added under ABI 8: new symbols only.  Rows x are fp32 [N][D] with row stride D; every matrix has row stride = its width.
 *   the model the scans read     w fp32 [K][D], b fp32 [K]
 *   the iterates                 theta, look double [K][D + 1]: element [k][0] is the intercept, [k][1 + d] the weight of dimension d
 *   the objective                F = 1/n sum_i (lse_i - v(i, y_i)) + lambda / 2 sum_kd w_kd^2 over the n used rows; the intercept is not
 *                                penalised.  lambda = 1 / (C n) makes it scikit-learn's LogisticRegression(C=C) objective over C n.
 *
 * THE SCORE OF A PAIR, the same bits wherever it is formed (one device function serves both scans):
 *       v(i, k) = b_k + sum_d x_id w_kd
 *   under sv_pairdist's summation rule: 16 dimensions in fp32 as fmaf(x_id, w_kd, .) in index order, the 16-blocks in double in index
 *   order, then (float)(sum + (double) b_k): rounded once.  A sum that is NaN or infinite -- a row with a NaN or infinite entry -- gives
 *   v = NaN for every k.
 *
 * sv_probe_rows:  lse[i] = log sum_k exp v(i, k) as an online log-sum-exp over tiles of 64 classes (16 for K <= 16) in index order: the
 *   maximum in fp32, the sum in double, expf on fp32 differences; lse = (float)((double) max + log(sum)), rounded once.     (fp32 [N])
 *       loss[i]  = lse[i] - v(i, label[i]) in fp32; NaN where label[i] is outside [0, K)               (fp32 [N], may be NULL; needs label)
 *       pred[i]  = the smallest k that attains the maximum of v(i, .)                                  (int64 [N], may be NULL)
 *       proba[i][k] = expf(v(i, k) - lse[i]), from a second pass over the tiles                        (fp32 [N][K], may be NULL)
 *   label is int64 [N] and may be NULL when loss is.  A row with a NaN or infinite entry gives lse = NaN, loss = NaN, pred = -1 and a NaN
 *   proba row.  K is tiled: any K >= 2; the [N][K] matrix exists only when proba is passed.  A row's result does not depend on the rows
 *   around it: rows cut into calls give the same bits.
 *
 * sv_probe_accum:  recomputes v and r_ik = expf(v(i, k) - lse[i]) - [k == label[i]] in fp32, the subtraction rounded once -- expf(.) is
 *   bit-equal to sv_probe_rows' proba -- and adds into P partial states under sv_kmeans_accum's rule: tile t of 64 rows goes to state
 *   t mod P; inside a state the rows are added in index order.  A row is USED iff lse[i] is finite and label[i] is in [0, K); every other
 *   row is skipped.  State p is sums + p (K (D + 1) + 1), doubles:
 *       [k (D + 1)]              += (double) r                                   (the intercept's gradient)
 *       [k (D + 1) + 1 + d]      += (double) r * (double) x_d                    (the product is exact)
 *       [K (D + 1)]  -- THE LAST DOUBLE OF THE STATE --  += (double) loss[i]     over the used rows, in row order
 *   one double add per (row, accumulator), never fused with the product; and counts int64 [P][2]: [p][0] += the rows used, [p][1] += the
 *   rows skipped.  init != 0 zeroes the states first; with init == 0 they continue.  Hence a repeated call gives the same bits; with
 *   P = 1 the rows may be cut at any multiple of 64, with P > 1 at any multiple of 64 P, and the states hold the bits of the one call.
 *   resid (fp32 [N][K], may be NULL) receives r (0 for a skipped row).  No atomic of any kind.  1 <= P <= 64; D <= 2^20 (a block owns
 *   32 dimensions: the grid's second dimension) and K (D + 1) < 2^31 (SV_E_SHAPE beyond).
 *
 * sv_probe_update:  one step of Nesterov's method with constant momentum, in double, every operation rounded once, in two launches.
 *   With n = sum_p counts[p][0] and G = the P states added in index order (from 0):
 *       g_k0 = G_k0 / n                         g_k,1+d = G_k,1+d / n + lambda look_k,1+d            (the gradient of F at look)
 *   g is written INTO STATE 0 of sums (the states are consumed: the next sv_probe_accum starts with init != 0), and the class's partials
 *   max_e |g_ke| and sum_d look_k,1+d^2 go to stats[4 + 2 k], stats[5 + 2 k]; thread t of 256 adds its elements e = t, t + 256, ... in
 *   index order and thread 0 adds the 256 shares in index order.  Then, element by element,
 *       theta_new = look - inv_L g              look_new = theta_new + beta (theta_new - theta)
 *   are written in place, with b_k = (float) look_new_k0 and w_kd = (float) look_new_k,1+d.  stats is double [4 + 2 K]:
 *       [0] F at the OLD look: (sum_p loss sums) / n + 0.5 (lambda sum_k stats[5 + 2 k]), p and k in index order
 *       [1] max_k stats[4 + 2 k]                [2] n, the rows used                [3] the rows skipped
 *   With n = 0 neither theta, look, w nor b is written, and stats[0] = stats[1] = NaN.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): a null pointer other than label (without loss), loss, pred,
 * proba, resid; N or D < 1; K < 2; P outside [1, 64]; lambda or inv_L not finite or <= 0; beta outside [0, 1); the limits above.  Each
 * takes a stream and allocates nothing: capturable; a repeated call sequence gives the same bits.                                     */
int sv_probe_rows(const float* x, int N, const float* w, const float* b, int K, int D, const int64_t* label, float* lse, float* loss,
                  int64_t* pred, float* proba, void* stream);
int sv_probe_accum(const float* x, const int64_t* label, const float* lse, const float* loss, int N, const float* w, const float* b, int K,
                   int D, double* sums, int64_t* counts, int P, int init, float* resid, void* stream);
int sv_probe_update(double* sums, const int64_t* counts, int P, int K, int D, double lambda, double inv_L, double beta, double* theta,
                    double* look, float* w, float* b, double* stats, void* stream);

/* ---- label spreading and propagation on a CSR graph (labelprop.hip) -----------------------------------------------
 * Added under ABI 8: new symbols only.  The graph is the CSR form embed.symmetrize returns and sv_tsne_attract reads: rowptr int64
 * [N + 1], col int64 [nnz], val fp32 [nnz].  A row's segment is [rowptr[i], rowptr[i + 1]) clamped to [0, nnz]; an entry whose column is
 * outside the matrix is NO EDGE and is skipped: nothing is read outside the arrays whatever rowptr and col hold.  Weights are expected
 * finite and >= 0; a NaN weight reaches the rows that read it and the statistics, nothing else.  col, val / sval may be NULL when
 * nnz == 0.  Every matrix has row stride = its width.
 *
 * sv_lp_normalize (square graphs: columns in [0, N)), two launches:
 *       deg[i]  = the sum of row i's valid weights in double: lane s of eight adds the valid entries s, s + 8, .. of the segment in
 *                 order (from 0.0), the eight lane sums meet as ((l0 + l4) + (l2 + l6)) + ((l1 + l5) + (l3 + l7))       (double [N])
 *       sval[q] = mode SV_LP_SYM:  w_q / sqrt(deg[i] deg[j])    (Zhou et al.'s D^-1/2 W D^-1/2; 0 where deg[i] deg[j] == 0)
 *                 mode SV_LP_ROW:  w_q / deg[i]                 (D^-1 W; 0 where deg[i] == 0)
 *                 product, root and quotient each rounded once in double, the result once to fp32; 0 for an entry that is no edge
 *                 (fp32 [nnz]; entries outside every segment are not written)
 *
 * sv_lp_step: one iteration f_in fp32 [M][K] -> f_out fp32 [N][K] over a graph of N rows and M columns (M == N during a fit).
 *       acc(i, c) = sum_q (double) sval[q] * (double) f_in[col[q]][c]  over row i's valid entries IN SEGMENT ORDER, from 0.0: every
 *                   product is exact in double, every addition rounded once.
 *   label is int64 [N]; a value outside [0, K) (-1 by convention) marks an unlabelled row.  With every operation rounded once in
 *   double (no contraction) and the result once to fp32:
 *       SV_LP_SPREADING     f_out = alpha * acc + (c == label[i] ? one_minus_alpha : 0.0)
 *       SV_LP_PROPAGATION   a labelled row: the one-hot of its label; an unlabelled row: acc / s with s = the sum of acc(i, .) in CLASS
 *                           ORDER from 0.0, s == 0 replaced by 1 (scikit-learn's per-iteration normalisation and hard clamp)
 *       SV_LP_PRODUCT       f_out = acc; label may be NULL
 *   Statistics (stats != NULL; needs scratch and M == N): every block of 256 threads -- 16 rows for K <= 16, else 4 -- leaves the sum and
 *   the maximum of |(double) f_out - (double) f_in| over its elements in scratch[2 b], scratch[2 b + 1] (a thread's elements in class
 *   order, then a binary tree over the threads); a one-block launch merges them -- thread t the blocks t, t + 256, .. in order, then the
 *   same tree -- into stats[0] = delta_l1, stats[1] = delta_max (a NaN is kept by both).  scratch is double [2 ceil(N / rows per
 *   block)].  A row's f_out is a function of its own segment and of the rows it names: rows cut into calls through offset pointers
 *   (rowptr + r, label + r, f_out + r K; stats NULL) give the same bits.  f_out must not overlap f_in.  1 <= K <= 1024; the indices are
 *   64-bit.
 *
 * sv_lp_finish: per row of f fp32 [N][K], s = the sum in class order in double, s' = (s == 0 ? 1 : s):
 *       proba[i][c] = (float)((double) f[i][c] / s')                                                  (fp32 [N][K], may be NULL)
 *       pred[i]     = the smallest c that attains the maximum of f[i][.]; -1 where s == 0 (no label reached the row) or the row holds
 *                     a NaN                                                                           (int64 [N], may be NULL)
 *       conf[i]     = proba at that c (the largest probability for s > 0)                             (fp32 [N], may be NULL)
 *       counts      = {rows without a NaN and s != 0, rows without a NaN and s == 0}, from a one-block launch of its own
 *                                                                                                     (int64 [2], may be NULL)
 *   Every subset of the outputs gives the same bits in the others; at least one is required; proba must not be f.
 *
 * Validated before any HIP call (SV_E_ARG, nothing launched): a NULL required pointer, N or M < 1, nnz < 0, K outside [1, 1024], an
 * unknown mode or variant, a NULL label outside the product variant, alpha or one_minus_alpha not finite under spreading, an f_out that
 * overlaps f_in, stats without scratch or with M != N.  Each takes a stream and allocates nothing: capturable; no atomic of any kind; a
 * repeated call sequence gives the same bits.                                                                                        */
#define SV_LP_SYM 0
#define SV_LP_ROW 1
#define SV_LP_SPREADING 0
#define SV_LP_PROPAGATION 1
#define SV_LP_PRODUCT 2
int sv_lp_normalize(const int64_t* rowptr, const int64_t* col, const float* val, int N, int64_t nnz, int mode, double* deg, float* sval,
                    void* stream);
int sv_lp_step(const float* f_in, int M, const int64_t* rowptr, const int64_t* col, const float* sval, int64_t nnz, int N, int K,
               const int64_t* label, int variant, double alpha, double one_minus_alpha, float* f_out, double* scratch, double* stats,
               void* stream);
int sv_lp_finish(const float* f, int N, int K, float* proba, int64_t* pred, float* conf, int64_t* counts, void* stream);

/* ---- kernel two-sample statistics: weighted kernel row sums for MMD, KID, witness and permutation test (ksum.hip) ----
 * Added under ABI 8: new symbols only.  Rows are fp32 [rows][D] with row stride D.
 *
 * sv_ksum_scan: for each of S problems s, each query row i < Q and each partial state p < P
 *       part[s][p][i] = sum_j w_j k(q_i, g_j)                                                          (double [S][P][Q], WRITTEN)
 *   over the columns j of the gallery tiles p, p + P, .. (64 rows each) of the call, columns in index order within a tile and tiles in
 *   order, every product (double) w_j * k and every addition rounded once in double, from 0.0.  A block that owns no tile writes 0.
 *   Pair value: v(i, j) is THE VALUE sv_pairdist GIVES THE PAIR UNDER SV_DIST_EUCLID, bit for bit (direct differences, 16 dimensions in
 *   fp32 with explicit fmaf in index order, the 16-blocks in double in index order, rounded once to fp32); u(i, j) is the dot product
 *   by the same rule with part = fmaf(q, g, part).  kparam is a DEVICE array double [n_scale][2] = (a_s, b_s), shared by the S
 *   problems; with x = (double) v or (double) u and every operation rounded once in double (no contraction):
 *       SV_KSUM_RBF    k = sum_s b_s * exp(-(a_s * x))            in scale order from 0.0; 1 <= n_scale <= 8
 *       SV_KSUM_IMQ    k = sum_s b_s / (1.0 + a_s * x)            in scale order from 0.0; 1 <= n_scale <= 8
 *       SV_KSUM_POLY   k = b^degree, b = a_0 * x + b_0            r = b, then degree - 1 times r = r * b; n_scale == 1, 1 <= degree <= 8
 *   g_w is fp32 [N] and may be NULL: every weight 1.  A column beyond N, a row beyond Q and the self pair col0 + j == self0 + i
 *   (self0 = -1: none) are left out BY PREDICATE: k(q, 0) and 0 * NaN never enter a sum; a NaN or infinite row or weight reaches
 *   exactly the sums that read it.  q_stride, g_stride (elements of q, g) and w_stride (elements of g_w) place problem s at
 *   q + s q_stride, g + s g_stride, g_w + s w_stride; 0 shares the array among the problems, any other value must be at least the
 *   array's size (Q D, N D, N).  The grid is ceil(Q / 64) x P x S blocks, 1 <= P <= 64, 1 <= S <= 65535.  Which pairs meet in which
 *   state in which order is a function of the arguments alone: a repeated call gives the same bits; a gallery cut into calls
 *   (col0, sv_ksum_finish's accumulate) changes the order of the additions.
 *
 * sv_ksum_finish:
 *       row_sum[s][i] = (accumulate ? row_sum[s][i] + t : t),  t = part[s][0][i] + part[s][1][i] + .. in the order of p   (double [S][Q])
 *       total[s]      = sum_i (double) q_w[s w_stride + i] * row_sum[s][i]                        (double [S]; NULL: no second launch)
 *   q_w is fp32 and may be NULL: weights of 1 (w_stride as above, against Q).  total follows sv_lp_step's merge order: thread t of
 *   256 adds the rows t, t + 256, .. in order from 0.0, then a binary tree over the threads (sh[t] += sh[t + h], h = 128 .. 1).  Both
 *   outputs keep a NaN.
 *
 * Validated before any HIP call (SV_E_ARG / SV_E_SHAPE, nothing launched): an unknown kind; n_scale or degree out of range; NULL
 * kparam, q, g, part or row_sum; q_w without total; Q, N or D < 1; S or P out of range; a stride that is neither 0 nor at least the
 * array's size, or that overflows the index with S (SV_E_SHAPE); a negative col0; self0 < -1; col0 + N or self0 + Q beyond the index
 * (SV_E_SHAPE).  Each takes a stream and allocates nothing: capturable; no atomic of any kind; nothing is read on the host.          */
#define SV_KSUM_RBF 0
#define SV_KSUM_IMQ 1
#define SV_KSUM_POLY 2
int sv_ksum_scan(int kind, const double* kparam, int n_scale, int degree, const float* q, int Q, int64_t q_stride, const float* g,
                 const float* g_w, int N, int64_t g_stride, int64_t w_stride, int D, int S, int64_t col0, int64_t self0, int P,
                 double* part, void* stream);
int sv_ksum_finish(const double* part, int S, int P, int Q, int accumulate, double* row_sum, const float* q_w, int64_t w_stride,
                   double* total, void* stream);

/* ---- internal cluster validity: silhouette, and what Calinski-Harabasz and Davies-Bouldin need (validity.hip) ----
 * Added under ABI 8: new symbols only.  Rows are fp32 [rows][D] with row stride D; labels and segment bounds are int64 ON THE DEVICE.
 *
 * sv_sil_scan: the gallery g [N][D] is GROUPED BY CLUSTER: with lo_c = clip(seg[c]), hi_c = clip(seg[c + 1]), clip(v) = min(max(v, 0), N),
 *   cluster c < K is the rows lo_c .. hi_c - 1 of g and n_c = hi_c - lo_c (<= 0: the cluster is empty and is skipped).  Every bound is
 *   clipped before use: a wrong seg gives wrong numbers, never a read outside g.  For each query row i < Q and partial state p < P
 *       part_a[p][i] = T(i, q_label[i])                       if q_label[i] is one of the non-empty clusters p, p + P, .. < K;  else 0.0
 *       part_b[p][i] = min over the OTHER non-empty clusters c (c != q_label[i]) among p, p + P, .. of  T(i, c) / (double) n_c,
 *                      one double division per (row, cluster); +inf when there is none; a NaN among the means stays (a running minimum
 *                      m = (v < m || v != v) ? v : m over the clusters in increasing order)                (double [P][Q], both WRITTEN)
 *   T(i, c) = sum over the rows j of cluster c of (double) d(i, j), in THIS order: the cluster is cut into tiles of 64 rows from lo_c
 *   (tile t = rows lo_c + 64 t ..; the first tile need not be aligned, a tile never crosses a cluster); the 16 threads of a row each
 *   add the columns 4 tx .. 4 tx + 3 of every tile in index order, the tiles in order, from 0.0 -- thread tx's share --; at the end
 *   of the cluster the 16 shares meet in the xor butterfly x += shfl_xor(x, 8), 4, 2, 1.  Every addition is rounded once in double.
 *   Pair value: v(i, j) is THE VALUE sv_pairdist GIVES THE PAIR UNDER SV_DIST_EUCLID, bit for bit (direct differences, 16 dimensions in
 *   fp32 with explicit fmaf in index order, the 16-blocks in double in index order, rounded once to fp32): a row is at distance exactly
 *   0 from itself and from a duplicate.  d = v under SV_SIL_SQEUCLID, d = sqrtf(v) -- the correctly rounded fp32 root -- under
 *   SV_SIL_EUCLID.  A column at or beyond hi_c and a row beyond Q are left out BY PREDICATE; a NaN or infinite gallery row reaches exactly
 *   the (row, cluster) sums that read it.  A query row is taken to be a member of the gallery when q_label[i] is in [0, K): its own pair
 *   (distance 0) is in T(i, q_label[i]) and sv_sil_finish divides by n - 1.  The grid is ceil(Q / 64) x P blocks, 1 <= P <= 64, 1 <= K <=
 *   1024; a block whose p >= K owns no cluster and writes (0.0, +inf).
 *
 * sv_sil_finish: per row, with ta = part_a[0][i] + part_a[1][i] + .. in the order of p (one term is non-zero: exact for every P), tb =
 *   the running minimum above over part_b[p][i] in the order of p, and n = n_c of c = q_label[i] (0 for a label outside [0, K)):
 *       a[i] = ta / (double)(n - 1)    n > 1;      0.0    n == 1;      NaN    n < 1                        (double [Q], may be NULL)
 *       b[i] = tb                                                                                          (double [Q], may be NULL)
 *       s[i] = NaN                     n < 1, a or b NaN, b = +inf (no other non-empty cluster)  -- decided first
 *            = 0.0                     n == 1 (a singleton), or max(a, b) == 0
 *            = (b - a) / max(a, b)     otherwise: one subtraction, one division                             (double [Q])
 *   Then, unless cluster_sum, cluster_cnt and skipped are NULL (all three or none), one block per cluster c < K in sv_ksum_finish's
 *   merge order: thread t of 256 adds s[i] over the rows i = t, t + 256, .. with q_label[i] == c and s[i] not NaN, in order from 0.0,
 *   then a binary tree over the threads (sh[t] += sh[t + h], h = 128 .. 1):
 *       cluster_sum[c] (double [K]),  cluster_cnt[c] = the number of those rows (int64 [K]),  skipped[0] = the number of rows whose s is
 *       NaN, whatever their label (int64 [1]).  All WRITTEN.  This pass reads K Q labels.
 *
 * sv_cluster_spread: rows x [N][D], label int64 [N] (any order), centroids c fp32 [K][D].
 *       d2[i]      = THE VALUE sv_pairdist GIVES THE PAIR (x_i, c_label[i]) UNDER SV_DIST_EUCLID, bit for bit; NaN for a label outside
 *                    [0, K)                                                                                (fp32 [N], may be NULL)
 *       stat[k][0] = sum (double) d2[i],  stat[k][1] = sum (double) sqrtf(d2[i])  over the rows with label[i] == k, in the merge order
 *                    above (thread t of 256: its rows t, t + 256, .. in order from 0.0; then the binary tree)        (double [K][2])
 *       cnt[k]     = the number of those rows                                                              (int64 [K])
 *   stat and cnt go together and may both be NULL.  A row that is not finite makes its cluster's stat NaN: give it a label of -1.
 *
 * Validated before any HIP call (SV_E_ARG, nothing launched): an unknown metric; NULL q, q_label, g, seg, part_a, part_b, s, x, label
 * or c; cluster_sum, cluster_cnt, skipped not all or none; stat without cnt or the reverse; no output at all; Q, N or D < 1; K outside
 * [1, 1024]; P outside [1, 64].  Each takes a stream and allocates nothing: capturable; no atomic of any kind; nothing is read on the
 * host; a repeated call gives the same bits; s, a and b do not depend on P or on how the queries are cut into calls.               */
#define SV_SIL_EUCLID 0
#define SV_SIL_SQEUCLID 1
int sv_sil_scan(int metric, const float* q, const int64_t* q_label, int Q, const float* g, const int64_t* seg, int N, int K, int D, int P,
                double* part_a, double* part_b, void* stream);
int sv_sil_finish(const double* part_a, const double* part_b, int P, int Q, const int64_t* q_label, const int64_t* seg, int K, int N,
                  double* s, double* a, double* b, double* cluster_sum, int64_t* cluster_cnt, int64_t* skipped, void* stream);
int sv_cluster_spread(const float* x, const int64_t* label, int N, int D, const float* c, int K, float* d2, double* stat, int64_t* cnt,
                      void* stream);

/* ---- K14/K15 smooth-ELBO terms (lib/criterion.py:32-57) -----------------------------------------
 * out3 = [recon, KL_c, KL_d] already divided by B (and 2*sigma^2 for MSE); must be zeroed by the
 * caller.  x / x_rec are NCHW fp32 (API edge).                                                      */
int sv_elbo_fwd(const float* x, const float* x_rec, int64_t n_per_img, const float* mu, const float* ls,
                const float* la, int B, int ldc, int K, int bce, float x_sigma, float* out3, void* stream);
/* gout3: device pointer to the three upstream gradients; writes dx_rec, dmu, dls, dla (=, not +=)  */
int sv_elbo_bwd(const float* x, const float* x_rec, int64_t n_per_img, const float* mu, const float* ls,
                const float* la, int B, int ldc, int K, int bce, float x_sigma, const float* gout3,
                float* dx_rec, float* dmu, float* dls, float* dla, void* stream);

/* ---- K16 ClsCriterion (lib/criterion.py:97-108): out += -mean_b sum_c predict*label*weight ------ */
int sv_cls_fwd(const float* predict, const float* label, const float* weight, int B, int K, float* out,
               void* stream);
int sv_cls_bwd(const float* label, const float* weight, int B, int K, const float* gout, float* dpredict,
               void* stream);
/* posterior terms of main_shot_vae.py:319-321,359-361: out += (sum (mu-mt)^2 + sum (exp(ls)-st)^2)/B */
int sv_post_fwd(const float* mu, const float* ls, const float* mu_t, const float* sigma_t, int B, int D,
                float* out, void* stream);
int sv_post_bwd(const float* mu, const float* ls, const float* mu_t, const float* sigma_t, int B, int D,
                const float* gout, float* dmu, float* dls, void* stream);

/* ---- top-1 / top-k accuracy counts of valid() / test() (main_shot_vae.py:441-447, :493-499): for every row b the rank
 * of class label[b] among score[b][0..K) (descending; ties: lower index first); hits[0] += #(rank < 1),
 * hits[1] += #(rank < k).  score may be exp(disc_log_alpha) or disc_log_alpha itself (monotone).  hits: 2 floats,
 * accumulated (+=) across calls = across the batches of an epoch.                                              */
int sv_topk_hits(const float* score, const int64_t* label, int B, int K, int k, float* hits, void* stream);

/* ---- K17 mixup / label smoothing gather-lerp (lib/utils/mixup.py:22-25,36-39) --------------------
 * out[b] = lam*f(a[b]) + (1-lam)*f(a[index[b]]), f = exp when `exp_space` else identity.           */
int sv_mix_lerp(const float* a, const int64_t* index, float lam, const float* lam_dev, int B, int64_t row,
                int exp_space, float* out, void* stream);

/* The input side of the single-launch step in one pass (added under ABI 8: a new symbol only): from image_l, image_u (fp32 NCHW
 * [B][C][H][W]), two pairings (int64 [B], values in [0, B)) and two mixing coefficients (host value, or device scalar when lam_*_dev
 * is not NULL), out = NHWC `dtype` [4B][H][W][Cpad], channels >= C zero, holding the groups in the step's launch order:
 * image_l | image_u | sv_mix_lerp(image_l, perm_l, lam_l) | sv_mix_lerp(image_u, perm_u, lam_u) -- bit for bit what sv_mix_lerp x 2,
 * a concatenation and sv_nchw_to_nhwc give.  sm_img / mx_img (fp32 NCHW [B][C][H][W], each may be NULL) receive the two mixed
 * batches as sv_mix_lerp writes them.  No allocation, no synchronisation: capturable.                                          */
int sv_mix_pack(int dtype, const float* image_l, const float* image_u, const int64_t* perm_l, const int64_t* perm_u, float lam_l,
                const float* lam_l_dev, float lam_u, const float* lam_u_dev, int B, int C, int H, int W, int Cpad, void* out,
                float* sm_img, float* mx_img, void* stream);

/* random permutations from uniform keys (the device-side replacement of torch.randperm, mixup.py:20,34): perm[rank of
 * key i] = i within each of `batches` key vectors of length n (<= 16384); ties: the lower index first.                */
int sv_rank_permutation(const float* keys, int n, int batches, int64_t* perm, void* stream);

/* ---- fused loss stage of the SHOT-VAE step (main_shot_vae.py:289-323,340-363) ---------------------------------------
 * sv_shot_targets: the targets of the mixed forwards (2) and (4) in one launch -- label_smoothing / mixup_vae_data
 * (lib/utils/mixup.py:22-25,36-39) applied to the outputs of forwards (1) [mu_l, ls_l] and (3) [mu_u, ls_u, la_u]:
 *   sm_mu = lerp(mu_l, perm_l, lam_l), sm_sigma = lerp(exp(ls_l), ...), mx_mu / mx_sigma / mx_alpha likewise with
 *   (perm_u, lam_u), lab_mix = lam_l * onehot(label_l) + (1 - lam_l) * onehot(label_l[perm_l]) -- the ONE soft label
 *   that replaces the two ClsCriterion terms of :316-318 (the criterion is linear in its label).  lam_*_dev (optional
 *   device scalars) override lam_* (hipGraph capture).  All outputs fp32 [B][D] / [B][K].
 * sv_shot_compose: terms[0..9] = recon_l, KLc_l, KLd_l, recon_u, KLc_u, KLd_u, disc_post_l, cont_post_l, disc_post_u,
 *   cont_post_u (as written by sv_elbo_fwd / sv_cls_fwd / sv_post_fwd) -> terms[10] = loss_supervised, terms[11] =
 *   loss_unsupervised; coef[i] = d loss / d terms[i] (10 floats).
 * sv_shot_scale: gvec[i] = coef[i] * (upstream gradient of the loss term i belongs to): the `gout` operands of
 *   sv_elbo_bwd (gvec, gvec + 3), sv_cls_bwd (gvec + 6, gvec + 8) and sv_post_bwd (gvec + 7, gvec + 9).              */
typedef struct { float ew, kl_beta_c, kl_beta_d, cmi, dmi, pwm, ucw; } sv_shot_schedule;
int sv_shot_targets(const float* mu_l, const float* ls_l, const float* mu_u, const float* ls_u, const float* la_u,
                    const int64_t* label_l, const int64_t* perm_l, const int64_t* perm_u, float lam_l, const float* lam_l_dev,
                    float lam_u, const float* lam_u_dev, int B, int D, int K, float* sm_mu, float* sm_sigma, float* lab_mix,
                    float* mx_mu, float* mx_sigma, float* mx_alpha, void* stream);
int sv_shot_compose(float* terms, const sv_shot_schedule* sch, float* coef, void* stream);
int sv_shot_scale(const float* coef, const float* g_sup, const float* g_unsup, float* gvec, void* stream);

/* The whole loss stage of one grouped step in ONE call (the nine forward and six backward launches above, issued back to back
 * by the library: at ~5 us per kernel the stage is bound by the caller's per-launch host time otherwise).  Outputs of the four
 * batched forwards in the group order (1)(3)(2)(4): rec [2B][n_per_img] (groups (1), (3) only), mu / ls [4B][D], la [4B][K].
 * Upstream gradients 1 for both objectives (`(loss_supervised + loss_unsupervised).backward()`).
 * terms [12] must be ZEROED by the caller; coef [10], tgt [4BD + 2BK] and the four gradient tensors are plain outputs.    */
typedef struct {
    const float* rec; const float* mu; const float* ls; const float* la;
    const float* image_l; const float* image_u;
    const int64_t* label_l; const int64_t* perm_l; const int64_t* perm_u;
    float lam_l; const float* lam_l_dev; float lam_u; const float* lam_u_dev;
    int32_t B, D, K, bce; int64_t n_per_img; float x_sigma;
    sv_shot_schedule sch;
    float* terms; float* coef; float* tgt;
    float* d_rec; float* d_mu; float* d_ls; float* d_la;
} sv_shot_loss_args;
int sv_shot_loss_step(const sv_shot_loss_args* a, void* stream);

/* ABI 4: the same stage for a step whose forwards were NOT one batched launch of four equal groups -- the ragged last
 * batch of an epoch (main_shot_vae.py:280 zips a 4 000-label loader, 7 x 512 + 416, with the unlabelled one: B_l != B_u)
 * and --om (lib/utils/mixup.py:9-18: the pairing of forward (4) needs the outputs of forward (3)).  Every group has its own
 * pointers, order (1)(3)(2)(4) as above; groups (1), (2) have Bl rows, (3), (4) Bu rows; rec / d_rec: groups (1), (3).
 * tgt [2 Bl D + 2 Bu D + Bl K + Bu K].  sv_shot_targets2 = sv_shot_targets with the two batch sizes.                     */
typedef struct {
    const float* rec[2]; const float* mu[4]; const float* ls[4]; const float* la[4];
    const float* image_l; const float* image_u;
    const int64_t* label_l; const int64_t* perm_l; const int64_t* perm_u;
    float lam_l; const float* lam_l_dev; float lam_u; const float* lam_u_dev;
    int32_t Bl, Bu, D, K, bce, reserved0; int64_t n_per_img; float x_sigma;
    sv_shot_schedule sch;
    float* terms; float* coef; float* tgt;
    float* d_rec[2]; float* d_mu[4]; float* d_ls[4]; float* d_la[4];
} sv_shot_loss_args2;
int sv_shot_loss_step2(const sv_shot_loss_args2* a, void* stream);
int sv_shot_targets2(const float* mu_l, const float* ls_l, const float* mu_u, const float* ls_u, const float* la_u,
                     const int64_t* label_l, const int64_t* perm_l, const int64_t* perm_u, float lam_l, const float* lam_l_dev,
                     float lam_u, const float* lam_u_dev, int Bl, int Bu, int D, int K, float* sm_mu, float* sm_sigma, float* lab_mix,
                     float* mx_mu, float* mx_sigma, float* mx_alpha, void* stream);

/* The same stage on the decoder's own output (added under ABI 8: a new symbol and a new struct only): the reconstruction logits
 * are read where the last ConvTranspose left them, rec[i] = NHWC `dtype` [B][HW][ld_rec] (channels < C), and the reconstruction
 * gradient is written as the decoder's backward reads it, d_rec[i] = NHWC `dtype` [B][HW][ld_drec], channels >= C zero.
 * base.rec / base.d_rec are ignored; everything else is sv_shot_loss_step2's, and base.n_per_img = C * HW.  Every reduction visits
 * the logits in the order of the fp32 NCHW tensor, and the gradient is the fp32 value of sv_shot_loss_step2 rounded to `dtype`
 * once: terms, the latent gradients and d_rec equal sv_nhwc_to_nchw -> sv_shot_loss_step2 -> sv_nchw_to_nhwc bit for bit (in
 * deterministic mode too).  At most 2^31 - 1 logits per group.                                                               */
typedef struct {
    sv_shot_loss_args2 base;
    int32_t dtype, C, HW, ld_rec, ld_drec, reserved0;
    const void* rec[2]; void* d_rec[2];
} sv_shot_loss_args3;
int sv_shot_loss_step3(const sv_shot_loss_args3* a, void* stream);

/* ---- K18 optimal-match pairing (lib/utils/mixup.py:9-18,93-99): index[i] = argmin_{j!=rank0} ----
 * second-smallest entry of row i of the pairwise Gaussian-KL matrix.                               */
int sv_optimal_match(const float* mu, const float* ls, int B, int D, int64_t* index, void* stream);

/* ---- the one-stage smooth-ELBO conv-VAEs (BASELINE configs 1 / 5: smooth_vae_model/svhn_vae.py, mnist_vae.py) -----
 * sv_smooth_latent_fwd: everything between the fused head GEMM and the decoder (svhn_vae.py:137-208).  o [B][ldo] =
 *   [mean (Dc) | log-variance (Dc) | logits (Dd) | pad] of `dtype`; alpha = softmax(logits); z = mean + exp(logvar / 2) *
 *   eps in training mode, else mean; gs = Gumbel-softmax sample softmax((log(alpha + 1e-12) + g) / T), g = -log(-log(u +
 *   1e-12) + 1e-12) in training mode, else one-hot(argmax alpha); c = one-hot(label) when label != NULL, else gs.
 *   Outputs: mean, logvar [B][Dc], alpha, gs [B][Dd] (fp32), latent [B][Lpad] = [z | c | 0] of `dtype` (the decoder's
 *   input), latent32 [B][Dc + Dd] fp32 (the API's latent_sample).
 * sv_smooth_latent_bwd: d_o [B][ldo] from the latent's gradient dlat [B][Lpad] (`dtype`) and the loss' gradients
 *   dmean / dlogvar / dalpha (fp32, NULL = none); sample_path = 1 when c was the Gumbel-softmax sample.               */
int sv_smooth_latent_fwd(int dtype, const void* o, int ldo, const float* eps, const float* u, const int64_t* label,
                         float temperature, int training, int B, int Dc, int Dd, int Lpad, float* mean, float* logvar,
                         float* alpha, float* gs, void* latent, float* latent32, void* stream);
int sv_smooth_latent_bwd(int dtype, const void* dlat, int Lpad, const float* dmean, const float* dlogvar, const float* dalpha,
                         const float* logvar, const float* eps, const float* alpha, const float* gs, float temperature,
                         int training, int sample_path, int B, int Dc, int Dd, void* d_o, int ldo, void* stream);
/* sv_smooth_classify: the classification tail of the encoder -- what Trainer.eval (main_smooth_ELBO_svhn.py:217-226) needs of a
 * forward, counted on the device.  Added under ABI 8: a new symbol only.  o [B][ldo] of `dtype` is the head GEMM's output as
 * sv_smooth_latent_fwd reads it, [mean (Dc) | log-variance (Dc) | logits (Dd) | pad]; the pad columns are never read.
 *   alpha     fp32 [B][Dd] or NULL: softmax(logits) by the very code of sv_smooth_latent_fwd (one device function serves both
 *             kernels): bit-equal to that kernel's alpha.
 *   pred      int64 [B] or NULL: the index of the first maximum of that fp32 alpha (the lowest index wins ties: torch.max(alpha, 1)[1]).
 *             A row whose alpha holds a NaN -- a NaN or +inf logit, or all logits -inf -- gives -1 (sv_smooth_latent_fwd's
 *             eval-mode one-hot is all zero there).
 *   label     int64 [B] or NULL; counts and confusion need it.
 *   counts    int64 [2] or NULL:  counts[0] += #(rows with pred == label),  counts[1] += B.
 *   confusion int64 [Dd][Dd] or NULL:  confusion[label][pred] += 1 for the rows with both indices in [0, Dd).
 *             A label outside [0, Dd) or a pred of -1 is a miss: counted in counts[1] and nowhere else.
 * counts and confusion ACCUMULATE across calls (the caller zeroes them once: a whole test set is evaluated without a host read).
 * The sums are integer adds -- independent of the block order, bit-reproducible -- with at most one atomic per block and counter
 * (the rows of a block are combined first).  One wave per row, any Dd.  Validated before any HIP call: o NULL, no output at all,
 * counts / confusion without label, a non-positive B / Dc / Dd or an unknown dtype give SV_E_ARG, ldo < 2 Dc + Dd SV_E_SHAPE.
 * Takes a stream and allocates nothing: capturable.                                                                          */
int sv_smooth_classify(int dtype, const void* o, int ldo, int B, int Dc, int Dd, const int64_t* label, float* alpha, int64_t* pred,
                       int64_t* counts, int64_t* confusion, void* stream);
/* reconstruction = tanh(f[..., :C]) of the decoder's NHWC output f [B][H][W][ld] as NCHW fp32 (svhn_vae.py:118-120), and
 * the backward d_f = d_out * (1 - out^2) in NHWC (channels >= C zero)                                                  */
int sv_tanh_to_nchw(int dtype, const void* f, int B, int C, int H, int W, int ld, float* out, void* stream);
int sv_tanh_to_nchw_bwd(int dtype, const float* d_out, const float* out, int B, int C, int H, int W, int ld, void* d_f, void* stream);
/* Trainer._loss_function (main_smooth_ELBO_svhn.py:228-310,312-335,368-388) in two launches: the raw reductions and the
 * composition.  terms [9] (zeroed by the caller): [0] num_pixels * MSE, [1] KL_c, [2] sum alpha log(alpha + 1e-12) / B
 * (KL_d = log D + [2]), [3] BCE(alpha, one-hot(label)) (label may be NULL), [4] the loss, [5..8] its four parts
 * (reconstruction, gamma_c |C_c - KL_c|, gamma_d |C_d - KL_d|, alpha_cls * BCE); coef [4] = d loss / d terms[0..3].
 * Capacities C = min((max - min) * steps / iters + min, max) (C_d also <= log D); steps_dev (optional device scalar)
 * replaces sch->steps (hipGraph replay).                                                                               */
typedef struct {
    float cont_min, cont_max, cont_iters, cont_gamma, disc_min, disc_max, disc_iters, disc_gamma, alpha_cls, steps;
} sv_smooth_schedule;
int sv_smooth_elbo_fwd(const float* data, const float* rec, int64_t n_per_img, const float* mean, const float* logvar,
                       const float* alpha, const int64_t* label, int B, int Dc, int Dd, const sv_smooth_schedule* sch,
                       const float* steps_dev, float* terms, float* coef, void* stream);
/* gradients of the loss (times the upstream gradient gout[0]) w.r.t. rec, mean, logvar, alpha (=, not +=)            */
int sv_smooth_elbo_bwd(const float* data, const float* rec, int64_t n_per_img, const float* mean, const float* logvar,
                       const float* alpha, const int64_t* label, int B, int Dc, int Dd, const float* coef, const float* gout,
                       float* d_rec, float* d_mean, float* d_logvar, float* d_alpha, void* stream);
/* torch.optim.Adam (no weight decay / amsgrad; main_smooth_ELBO_svhn.py:428) on a flat buffer: m, v = first / second
 * moments; step = 1-based update count (host) or step_dev (device scalar, hipGraph replay); g is scaled by grad_scale
 * first (1 / world after the gradient all-reduce).                                                                    */
int sv_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float step,
            const float* step_dev, float grad_scale, void* stream);

/* ---- K20 SGD(momentum, weight decay) on the flat parameter buffer (torch.optim.SGD semantics) ---- */
int sv_sgd(float* p, const float* g, float* v, int64_t n, float lr, float momentum, float weight_decay,
           float grad_scale, int first_step, void* stream);

/* ---- layout / packing helpers --------------------------------------------------------------------*/
/* NCHW fp32 [B,C,H,W] -> NHWC `dtype` [B,H,W,Cpad] (channels >= C zero-filled)                     */
int sv_nchw_to_nhwc(int dtype, const float* in, int B, int C, int H, int W, int Cpad, void* out, void* stream);
/* NHWC `dtype` [B,H,W,ld] (first C channels) -> NCHW fp32                                           */
int sv_nhwc_to_nchw(int dtype, const void* in, int B, int C, int H, int W, int ld, float* out, void* stream);
/* ---- K21 device-side input pipeline (lib/dataloader.py:58-70: Pad(4, reflect) -> RandomHorizontalFlip ->
 * RandomCrop(H) -> ToTensor) fused with the batch gather: sample b = data[index[b]] (uint8 HWC, [N][H][W][C]),
 * reflect-padded by `pad`, flipped if params[3b+2] != 0, cropped at (params[3b], params[3b+1]) in the padded image
 * (0 <= offset <= 2*pad), scaled by 1/255.  nhwc_cpad == 0: out = fp32 NCHW [B][C][H][W] (the model's API input);
 * nhwc_cpad > 0: out = `dtype` NHWC [B][H][W][nhwc_cpad], channels >= C zero (the stem convolution's input layout).
 * params == NULL: no augmentation (evaluation: ToTensor only).                                                  */
int sv_augment(int dtype, const uint8_t* data, const int64_t* index, const int32_t* params, int B, int H, int W, int C,
               int pad, int nhwc_cpad, void* out, void* stream);

/* master fp32 [N][T_orig][C] -> packed `dtype` per phase [n'][ntap][c'] (transpose swaps n and c)  */
int sv_repack(int dtype, const float* master, int N, int T_orig, int C, int transpose,
              const sv_geom* g, void* dst, void* stream);
/* ABI 4: the same packing straight from a tensor in ANOTHER layout -- element (n, tap, c) at src[n * sn + tap * st + c * sc],
 * zero beyond n_real / c_real (channel padding to the MFMA multiples): a torch Conv2d weight (OIHW: sn = c_real * T, st = 1,
 * sc = T), a ConvTranspose2d weight (IOHW: sn = T, st = 1, sc = n_real * T) or a Linear weight, without the intermediate
 * master copy (the smooth-ELBO models keep torch's own parameter tensors: smooth_vae_model/svhn_vae.py:62-132).          */
int sv_repack_strided(int dtype, const float* src, int n_real, int c_real, int64_t sn, int64_t st, int64_t sc, int N, int T_orig,
                      int C, int transpose, const sv_geom* g, void* dst, void* stream);

/* All packs of a network in one launch (68 sv_repack launches per optimizer step otherwise).  jobs: DEVICE array, one
 * entry per (layer, direction, phase) with taps, sorted by block0; a job owns ceil(size / 1024) consecutive blocks from
 * block0; total_blocks = their sum.  Offsets are in elements from master_base (fp32) / dst_base (`dtype`).             */
typedef struct {
    int64_t master_off, dst_off, size;      /* size = N * C * ntap elements of this phase's pack                     */
    int32_t N, T_orig, C, transpose, ntap, block0;
    int8_t torig[SV_MAX_TAPS];
} sv_repack_job;
int sv_repack_batch(int dtype, const float* master_base, const sv_repack_job* jobs, int njobs, int total_blocks,
                    void* dst_base, void* stream);

/* ABI 6: the same for parameters that live in torch's OWN layouts (the smooth-ELBO models keep nn.Conv2d / nn.ConvTranspose2d /
 * nn.Linear parameters): one launch gathers every weight pack -- and, with dtype SV_F32 into a float buffer, every padded bias
 * vector -- of a model straight from the parameter tensors, and one launch scatters the weight / bias gradients the kernels left
 * in master layout back into the parameters' .grad tensors (+=).  A job describes one (layer, direction, phase):
 *   element (n, tap t, c) of the layer  <->  ptr[n_hi * sn_hi + n_lo * sn_lo + torig[t] * st + c * sc],  n = n_hi * n_lo_count + n_lo
 * (n_lo_count > 1: a Linear layer whose output index is a permuted (c, y, x) flattening).  Gather: destination element i of the job
 * (pack order [n][tap][c], or [c][tap][n] when `transpose`) at dst_base[dst_off + i], zero beyond (n_real, c_real); with dst_ld the outer index has
 * its own stride (several jobs filling column ranges of one pack).  Scatter: the
 * master-layout gradient at src_base[dst_off + (n * ntap + t) * C + c] is ADDED to the parameter gradient element (torig[t] = t;
 * transpose = 1: the source at float offset dst_off is an array of DOUBLES -- the channel sums (sv_acc_t) of a data gradient's epilogue,
 * which are the bias gradient of the layer in front).
 * block0 = first block of the job; a job has ceil(size / 1024) blocks; jobs sorted by block0 (device array).                      */
typedef struct {
    float* ptr;                 /* the parameter (gather) / its gradient (scatter) */
    int64_t dst_off, size;
    int64_t dst_ld;             /* gather: destination stride of the OUTER index (n, or c when transposed); 0 = dense */
    int64_t sn_hi, sn_lo, st, sc;
    int32_t n_lo_count, N, C, ntap, transpose, n_real, c_real, block0;
    int8_t torig[SV_MAX_TAPS];
} sv_param_job;
int sv_param_gather(int dtype, const sv_param_job* jobs, int njobs, int total_blocks, void* dst_base, void* stream);
int sv_param_scatter_add(const sv_param_job* jobs, int njobs, int total_blocks, const float* src_base, void* stream);

/* ---- in-situ kernel timing (HIP events around launches of sv_igemm / sv_wgrad) -------------------
 * sv_prof_enable(1) starts recording; every launch is filed under the current tag (sv_prof_tag).
 * sv_prof_collect synchronises the device and returns, per tag, total milliseconds and launches.   */
int sv_prof_enable(int on);
int sv_prof_tag(int tag);
/* Launches the library issues on its own inside an entry point (the sv_bn_finalize of a folded sv_igemm whose kernel does not
 * derive the coefficients itself) are filed under `tag`; -1 (default): they are not recorded -- never as a second launch of
 * the layer's tag.                                                                                                        */
int sv_prof_nested_tag(int tag);
/* kind 0 = the folded BatchNorm finalisation (same as sv_prof_nested_tag), kind 1 = the materialised two-tensor prologue of
 * sv_igemm_args::x2 (the streaming launch sv_igemm issues for kernels that do not form it in their load path)             */
int sv_prof_nested_tag_kind(int kind, int tag);
int sv_prof_collect(int max_tags, double* ms, int* count);

/* ---- introspection (host only, no GPU): the compile-time "tile program" of the wide weight-gradient kernel.
 * halo_vectors = 3 or 4 (halo 16-byte vectors per thread; 4 for 32 x 32 maps).  items = int[180][3]: for the gap behind
 * every MFMA of one tile iteration (4 phases x 45) up to three item codes, 0 = none, 1000 + 41*vector + step = one
 * single-instruction step of the halo transform (step 40 = its LDS store), 2000 + k = dy DMA instruction k,
 * 3000 + v = global load of halo vector v (tile after next, into the second register set), 5000 + 4*v + d = the move of
 * dword d of vector v from the second register set into the first.  The kernel has no counted vmcnt wait (one vmcnt(0)
 * in front of its barrier, which follows gap 134): waits = int[5], [0..3] = 0, [4] = the gap of the last VMEM instruction
 * before that barrier.                                                                                      */
int sv_debug_wgrad_tile_program(int halo_vectors, int* items, int* waits);

/* The chunk program of the wide forward / data-gradient kernel (conv3x3x.hip): items = int[180][6], the gap behind every
 * MFMA of one 32-channel chunk (9 taps x 20).  Codes: 1000 + 41*vector + step (BatchNorm pass), 2000 + 3*slice + i (weight
 * DMA instruction; slice 0..3 = this chunk's taps 5..8, 4..8 = the next chunk's taps 0..4), 3000 + v (halo load),
 * 3500 + q (coefficient load), 4000 + v / 4500 (vmcnt waits), 5000 (stage flip).  waits = int[10]: vmcnt of the waits
 * before vectors 0..5, before the coefficients (each = the YOUNGER REGISTER LOADS only), and before the barriers after
 * taps 1, 4, 7 (each = the younger LDS-DMA instructions only: zero).                                               */
int sv_debug_conv_chunk_program(int* items, int* waits);

/* The work table of the per-pixel GEMM kernel (pixgemm.hip) for geometry g -- ConvTranspose2d(4, 2, 1) forward on maps of up to
 * 4 x 4 pixels, or its data gradient (a 4x4 stride-2 pad-1 convolution) on maps of up to 8 x 8; SV_E_SHAPE for anything else.
 * *npix = output pixels; in the kernel's work order (falling tap count) pixels = int[64][4] {oy, ox, phase, valid taps} and
 * taps = int[64][16][4] {tap index inside the phase, iy, ix, element offset of the tap's [Cin] slice in row 0 of the packed
 * weights (phase[].w_off + tap * Cin; row n adds n * phase[].ntap * Cin)}, -1 beyond the pixel's valid taps.               */
int sv_debug_pixgemm_table(const sv_geom* g, int* npix, int* pixels, int* taps);
/* The label of the calling thread's last launch of the sv_igemm family ("sv_igemm", "sv_igemm(dma)", "sv_igemm(pixel)", ...; ""
 * before the first) as a C string in buf[len]: tests assert which kernel a dispatch took.  A grid query launches nothing. */
int sv_debug_last_kernel(char* buf, int len);

/* ---- dispatcher options (process-wide; set them between launches, not concurrently with them) --------------------
 * SV_OPT_DISABLE_MASK: OR of SV_K_* bits; a set bit routes the layers a specialised kernel would take to the next more
 * general one (sv_igemm: conv3x3x -> conv3x3w -> conv3x3 / conv3x3p / conv3x3m -> halo -> the generic gather-GEMM; sv_wgrad:
 * wgrad3x3w -> wgrad3x3 -> hwgrad -> the generic weight-gradient kernel).  Default 0.  The parity tests use it to compare every
 * specialised kernel with the general one on the same inputs (conv3x3x against conv3x3w bit for bit).
 * SV_OPT_WIDE_MIN_BLOCKS: minimum grid (blocks) for which the 256-pixel wide-tile kernels are chosen; default 256 (one
 * block per CU).  Tests set 1 to reach those kernels at small batch sizes.
 * SV_OPT_HALO_ALL: 1 = the LDS-halo gather-GEMM (halo.hip) takes every geometry it covers, not only the layers it is
 * faster on (tests: the kernel's whole range against the references).  Default 0.
 * SV_OPT_PERSISTENT_BLOCKS: block budget of the persistent narrow 3x3 kernels (conv3x3p, wgrad3x3), shared among the
 * groups of a batched launch.  Default 512 (two blocks per CU); tools/tune_blocks.py sweeps it.
 * SV_OPT_DETERMINISTIC: 1 = every floating-point accumulation of the library has a FIXED summation order, so that two runs
 * on the same inputs agree bit for bit (parity tests, reproducible training; since round 4 about 1.4x the step time of the
 * default mode on WRN-28-2 and 1.8x on WRN-28-10; the accumulator replicas grow with the grid):
 *   - BatchNorm statistics / BatchNorm-backward sums of the conv-like kernels: no LDS float atomics, every wave of every
 *     block adds its partial sums to a replica of its own, or (conv3x3w / conv3x3x) the block adds its waves' private sums in a
 *     fixed order (ONE adder per address; needs replicas >= 4 * blocks, see sv_igemm_query_blocks; sv_igemm fails with
 *     SV_E_ARG otherwise); the consumers sum the replicas in index order (sv_bn_bwd_apply after a 256 : 1 pre-pass);
 *   - weight gradients: partial slabs in the workspace + the ordered slab reduction (3x3 stride 1 and the tap-fused thin
 *     layers: a slab per block; the generic and the cooperative wide kernel: a zeroed slab per M range); without a workspace
 *     of at least two slabs ONE M range; the groups of a batched launch one after the other (a single adder per weight);
 *   - the small reductions (pool backward, column sums, loss terms) run in two passes: the blocks of the first own a slot
 *     each in a scratch ring the library allocates at the first use (32 MB; that first call must not be inside a stream
 *     capture), the second adds the slots in index order; the head weight gradient one slice after the other; BatchNorm
 *     dgamma / dbeta of a batched launch by one block, the groups in index order.
 * Default 0.
 * SV_OPT_ENABLE_MASK: OR of SV_K_* bits of kernels that are OFF by default (SV_K_MAP4_CONV: the chunked conv3x3 kernel on 4 x 4 maps,
 * which did not beat the gather-GEMM on the 512 -> 512 layers of the PreActResNets).                                      */
enum { SV_OPT_DISABLE_MASK = 0, SV_OPT_WIDE_MIN_BLOCKS = 1, SV_OPT_HALO_ALL = 2, SV_OPT_PERSISTENT_BLOCKS = 3,
       SV_OPT_DETERMINISTIC = 4, SV_OPT_ENABLE_MASK = 5 };
enum { SV_K_CONV3X3 = 1, SV_K_CONV3X3P = 2, SV_K_CONV3X3M = 4, SV_K_CONV3X3W = 8, SV_K_CONV3X3X = 16,
       SV_K_WGRAD3X3 = 32, SV_K_WGRAD3X3W = 64, SV_K_IGEMM_KV2 = 128, SV_K_HALO = 256, SV_K_HALOP = 512, SV_K_HWGRAD = 1024, SV_K_IGEMM_BIG = 2048, SV_K_WGRAD_WIDE = 4096, SV_K_IGEMM_ALIGNED = 8192, SV_K_IGEMM_DMA = 16384, SV_K_WGRAD_INCR = 32768, SV_K_WGRAD3X3M = 65536, SV_K_TCONVR = 131072, SV_K_TCONVR_EX = 262144, SV_K_SCONV = 524288, SV_K_PCONV = 8388608, SV_K_THCONV = 16777216, SV_K_THWGRAD = 67108864, SV_K_S2WGRAD = 134217728,
       SV_K_MAP4 = 268435456,      /* wgrad3x3 on 4 x 4 maps (ON by default: 236 against 405 us at 512 -> 512, 4 x 512 images) */
       SV_K_MAP4_CONV = 536870912, /* conv3x3 (forward / data gradient) on 4 x 4 maps: OFF by default (SV_OPT_ENABLE_MASK) -- measured
                                      224 against 235 us forward (inside the run-to-run spread), 191 against 161 us data gradient */
       SV_K_PIXGEMM = 1073741824   /* per-pixel GEMMs for ConvTranspose2d(4, 2, 1) on maps <= 4 x 4 and its data gradient (pixgemm.hip) */ };
int sv_set_option(int key, int value);
int sv_get_option(int key);          /* -1 for an unknown key */

/* Stream fork: everything enqueued on `from` so far happens-before whatever is enqueued on `to` afterwards (the step's weight
 * gradients run on a side stream beside the data gradients).  hipEventRecord + hipStreamWaitEvent on an event from a pool the
 * library owns; light != 0 creates the events with hipEventDisableSystemFence: the two streams are on one device, the
 * system-scope release an ordinary event performs in `from` (cache writeback + an idle gap in front of the next kernel, ~6 us per
 * fork on MI355X) is not needed for them.  Works under stream capture (the record becomes a graph edge).                  */
int sv_stream_fork(void* from, void* to, int light);
/* The device-side form of the fork (sv_igemm_args::start_flag).  sv_stream_flag_next: the flag word the library keeps for
 * `stream` (device memory, allocated and zeroed at the first call -- not inside a stream capture) and the next value of its
 * sequence; the caller passes both to the launch that is to signal and to sv_stream_wait_flag on the other stream.
 * sv_stream_wait_flag: enqueues a one-wave kernel on `stream` that returns once (int32)(*flag - value) >= 0; it gives up after
 * ~3 s (a signalling launch that never ran) and counts that in a STICKY counter in host-mapped memory: sv_flag_timeouts()
 * reads it without a copy or a synchronisation, so the host layer checks it on every step and raises (a weight gradient that
 * ran behind a failed wait read unfinished operands; the step is invalid).  sv_flag_timeouts_reset() clears it once the
 * caller has handled the condition (e.g. switched to sv_stream_fork).
 * NOT for environments that serialise kernel dispatch across streams (rocprofv3 --pmc, AMD_SERIALIZE_KERNEL,
 * HIP_LAUNCH_BLOCKING): the waiting kernel may then be dispatched in front of the one it waits for -- fork with
 * sv_stream_fork there (the Python host layer checks the environment).                                                     */
int sv_stream_flag_next(void* stream, uint32_t** flag, uint32_t* value);
int sv_stream_wait_flag(void* stream, const uint32_t* flag, uint32_t value);
int sv_flag_timeouts(void);
int sv_flag_timeouts_reset(void);

int sv_version(void);
const char* sv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
