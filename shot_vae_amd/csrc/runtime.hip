// Host-side runtime glue of libshotvae_hip.so: error reporting and in-situ kernel timing.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include <mutex>

#include "common.h"

static thread_local char g_err[512] = "";

void sv_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int sv_check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        sv_set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
        return SV_E_HIP;
    }
    return SV_OK;
}

int sv_lds_optin_set(const void* kernel, int bytes, const char* name) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) return SV_OK;
    char what[64];
    snprintf(what, sizeof(what), "hipFuncSetAttribute(%s)", name);
    return sv_check_launch(what);
}

namespace {
int g_disable_mask = 0;
int g_wide_min_blocks = 256;
int g_halo_all = 0;
int g_persistent_blocks = 512;
int g_deterministic = 0;
int g_enable_mask = 0;
thread_local int* tl_query_blocks = nullptr;
}  // namespace
bool sv_in_query() { return tl_query_blocks != nullptr; }
bool sv_deterministic() { return g_deterministic == 1; }
bool sv_det_stats() { return g_deterministic != 0; }

// Deterministic mode: per-block partial results of the two-pass reductions (sv_colsum, the loss sums, sv_pool_bwd, the replica
// pre-pass of sv_bn_bwd_apply) live in a ring the library owns -- 32 MB, allocated at the first use, which therefore has to be
// outside a stream capture (the warm-up iterations any capture needs anyway).  A slice is reused once the ring has wrapped:
// a single call takes at most a few MB, two kernels that are in flight together on different streams are never that many
// calls apart.
namespace {
float* g_det_ring = nullptr;
size_t g_det_off = 0;
constexpr size_t DET_RING_FLOATS = (size_t)8 << 20;
}  // namespace
float* sv_det_scratch(size_t floats) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    floats = (floats + 63) / 64 * 64;
    // (bound: no single request above a quarter of the ring, so at least four calls lie between a slice and its reuse -- the
    //  side stream lags the main stream by at most the few weight gradients in flight, each of which takes at most one slice)
    if (floats > DET_RING_FLOATS / 4) {
        sv_set_error("deterministic mode: a reduction asks for %zu floats of scratch (limit: a quarter of the %zu-float ring)", floats, DET_RING_FLOATS);
        return nullptr;
    }
    if (!g_det_ring) {
        void* p = nullptr;
        if (hipMalloc(&p, DET_RING_FLOATS * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            sv_set_error("deterministic mode: cannot allocate the scratch ring (first use inside a stream capture? run one step before capturing)");
            return nullptr;
        }
        g_det_ring = static_cast<float*>(p);
    }
    if (g_det_off + floats > DET_RING_FLOATS) g_det_off = 0;
    float* r = g_det_ring + g_det_off;
    g_det_off += floats;
    return r;
}
// BatchNorm finalisation folded into an sv_igemm launch (sv_igemm_args::fold_*): sv_igemm announces it (sv_fold_begin); a
// launcher whose kernel derives the coefficients itself claims it (sv_fold_claim); for every other kernel the launch gate
// (sv_dry_run, in front of every launch of the family) runs sv_bn_finalize first.
namespace {
thread_local const sv_igemm_args* tl_fold = nullptr;
thread_local const sv_geom* tl_fold_g = nullptr;
thread_local void* tl_fold_stream = nullptr;
}  // namespace
void sv_fold_begin(const sv_geom* g, const sv_igemm_args* a, void* stream) { tl_fold = a; tl_fold_g = g; tl_fold_stream = stream; }
void sv_fold_end() { tl_fold = nullptr; }
bool sv_fold_claim(bool can) {
    if (!tl_fold || !can) return false;
    tl_fold = nullptr;
    return true;
}
int sv_prof_nested_scope(int enter, int kind);
static int sv_fold_materialize() {
    const sv_igemm_args* a = tl_fold;
    tl_fold = nullptr;
    // (in-situ timing: this launch is filed under its own tag -- sv_prof_nested_tag -- or not at all, never as a second launch
    //  of the layer whose sv_igemm issued it)
    struct Nested { Nested() { sv_prof_nested_scope(1, 0); } ~Nested() { sv_prof_nested_scope(0, 0); } } nested;
    return sv_bn_finalize(a->fold_stats, a->fold_replicas, tl_fold_g->Cin, a->fold_count, a->fold_gamma, a->fold_beta, a->fold_eps, 0.f,
                          nullptr, nullptr, const_cast<float*>(a->pro_scale), const_cast<float*>(a->pro_shift), a->fold_mean,
                          a->fold_rstd, sv_ngroups(a->groups), tl_fold_stream);
}
bool sv_dry_run(int grid_x, const sv_igemm_args* a, int* rc) {
    if (tl_fold && !tl_query_blocks) {           // nobody claimed the fold: this kernel reads finished coefficients
        const int r = sv_fold_materialize();
        if (r != SV_OK) { *rc = r; return true; }
    }
    if (tl_query_blocks) {
        *tl_query_blocks = grid_x;
        *rc = SV_OK;
        return true;
    }
    if (a && (a->flags & SV_FLAG_DET) && (a->stats || a->ex) && (int64_t)a->replicas < 4 * (int64_t)grid_x) {
        sv_set_error("sv_igemm: deterministic mode needs replicas >= 4 * blocks = %d (got %d): size the accumulators with "
                     "sv_igemm_query_blocks", 4 * grid_x, a->replicas);
        *rc = SV_E_ARG;
        return true;
    }
    return false;
}
static thread_local const char* tl_last_kernel = "";
void sv_note_kernel(const char* label) { tl_last_kernel = label; }
extern "C" int sv_debug_last_kernel(char* buf, int len) {
    SV_REQUIRE(buf && len > 0, SV_E_ARG, "sv_debug_last_kernel: no buffer");
    snprintf(buf, (size_t)len, "%s", tl_last_kernel);
    return SV_OK;
}
struct SvQueryScope {
    explicit SvQueryScope(int* out) { tl_query_blocks = out; }
    ~SvQueryScope() { tl_query_blocks = nullptr; }
};
extern "C" int sv_igemm_query_blocks(const sv_geom* g, int dtype, const sv_igemm_args* a, int* blocks) {
    SV_REQUIRE(blocks, SV_E_ARG, "sv_igemm_query_blocks: null argument");
    *blocks = 0;
    SvQueryScope scope(blocks);
    return sv_igemm(g, dtype, a, nullptr);
}
static thread_local int tl_block_budget = 0;      // per-launch override, set for the duration of one entry-point call
SvBudgetScope::SvBudgetScope(int budget) : old(tl_block_budget) { tl_block_budget = budget > 0 ? budget : 0; }
SvBudgetScope::~SvBudgetScope() { tl_block_budget = old; }
int sv_persistent_blocks() { return tl_block_budget > 0 ? tl_block_budget : g_persistent_blocks; }
bool sv_halo_all() { return g_halo_all != 0; }
bool sv_disabled(int kernel_bit) {
    // (deterministic mode: conv3x3w / conv3x3x keep per-wave channel sums that the block adds in a fixed order -- it is the only
    //  adder of its replica, sv_igemm_query_blocks sizes the accumulators; the wide weight gradient writes per-split slabs)
    return (g_disable_mask & kernel_bit) != 0;
}
int sv_wide_min_blocks() { return g_wide_min_blocks; }
bool sv_enabled(int kernel_bit) { return (g_enable_mask & kernel_bit) != 0; }

namespace {
struct Rec { hipEvent_t a, b; int tag; bool closed; };
int g_prof_on = 0, g_tag = 0, g_nested_tag[2] = {-1, -1};     // nested kinds: 0 = folded BatchNorm finalisation, 1 = materialised prologue
std::vector<Rec> g_recs;
std::vector<Rec> g_pool;
constexpr size_t kMaxRecs = 1 << 17;
}  // namespace

// Scopes nest (an entry point that times itself and calls other timed entry points: sv_shot_loss_step2): only the OUTERMOST
// scope owns a record -- an inner begin / end pair must neither open one of its own nor close the outer one early (its end
// event would stay unrecorded, or stale from the pool: a negative time in the table).
namespace { int g_prof_depth = 0; long g_prof_open = -1; }
void sv_prof_begin(hipStream_t s) {
    if (g_prof_depth++ > 0) return;
    g_prof_open = -1;
    if (!g_prof_on || g_recs.size() >= kMaxRecs) return;
    Rec r;
    if (!g_pool.empty()) {
        r = g_pool.back();
        g_pool.pop_back();
    } else {
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    }
    r.tag = g_tag;
    r.closed = false;
    (void)hipEventRecord(r.a, s);
    g_prof_open = (long)g_recs.size();
    g_recs.push_back(r);
}

void sv_prof_end(hipStream_t s) {
    if (g_prof_depth > 0 && --g_prof_depth > 0) return;
    if (g_prof_open < 0 || (size_t)g_prof_open >= g_recs.size()) return;
    (void)hipEventRecord(g_recs[g_prof_open].b, s);
    g_recs[g_prof_open].closed = true;
    g_prof_open = -1;
}

// launches the library issues on its own inside an entry point (the BatchNorm finalisation of a folded launch): timed under
// g_nested_tag, or not at all when none is set
int sv_prof_nested_scope(int enter, int kind) {
    static thread_local int saved_tag = 0, saved_on = 0;
    if (enter) {
        saved_tag = g_tag;
        saved_on = g_prof_on;
        if (g_nested_tag[kind] >= 0) g_tag = g_nested_tag[kind];
        else g_prof_on = 0;
    } else {
        g_tag = saved_tag;
        g_prof_on = saved_on;
    }
    return 0;
}

extern "C" {

int sv_prof_enable(int on) {
    g_prof_on = on ? 1 : 0;
    return SV_OK;
}

int sv_prof_tag(int tag) {
    g_tag = tag;
    return SV_OK;
}

int sv_prof_nested_tag(int tag) {
    g_nested_tag[0] = tag;
    return SV_OK;
}

int sv_prof_nested_tag_kind(int kind, int tag) {
    SV_REQUIRE(kind == 0 || kind == 1, SV_E_ARG, "sv_prof_nested_tag_kind: kind=%d", kind);
    g_nested_tag[kind] = tag;
    return SV_OK;
}

int sv_prof_collect(int max_tags, double* ms, int* count) {
    if (hipDeviceSynchronize() != hipSuccess) return sv_check_launch("sv_prof_collect");
    for (int i = 0; i < max_tags; ++i) { ms[i] = 0.0; count[i] = 0; }
    for (Rec& r : g_recs) {
        float t = 0.f;
        if (r.closed && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess && t >= 0.f && r.tag >= 0 && r.tag < max_tags) {
            ms[r.tag] += t;
            count[r.tag] += 1;
        }
        g_pool.push_back(r);
    }
    g_recs.clear();
    (void)hipGetLastError();
    return SV_OK;
}

int sv_set_option(int key, int value) {
    switch (key) {
        case SV_OPT_DISABLE_MASK: g_disable_mask = value; return SV_OK;
        case SV_OPT_WIDE_MIN_BLOCKS:
            SV_REQUIRE(value >= 1, SV_E_ARG, "sv_set_option: SV_OPT_WIDE_MIN_BLOCKS=%d", value);
            g_wide_min_blocks = value;
            return SV_OK;
        case SV_OPT_HALO_ALL: g_halo_all = value; return SV_OK;
        case SV_OPT_PERSISTENT_BLOCKS:
            SV_REQUIRE(value >= 8, SV_E_ARG, "sv_set_option: SV_OPT_PERSISTENT_BLOCKS=%d", value);
            g_persistent_blocks = value;
            return SV_OK;
        case SV_OPT_DETERMINISTIC:
            SV_REQUIRE(value >= 0 && value <= 2, SV_E_ARG, "sv_set_option: SV_OPT_DETERMINISTIC=%d (0, 1 or 2)", value);
            g_deterministic = value;
            return SV_OK;
        case SV_OPT_ENABLE_MASK: g_enable_mask = value; return SV_OK;
    }
    sv_set_error("sv_set_option: unknown key %d", key);
    return SV_E_ARG;
}

int sv_get_option(int key) {
    switch (key) {
        case SV_OPT_DISABLE_MASK: return g_disable_mask;
        case SV_OPT_WIDE_MIN_BLOCKS: return g_wide_min_blocks;
        case SV_OPT_HALO_ALL: return g_halo_all;
        case SV_OPT_PERSISTENT_BLOCKS: return g_persistent_blocks;
        case SV_OPT_DETERMINISTIC: return g_deterministic;
        case SV_OPT_ENABLE_MASK: return g_enable_mask;
    }
    return -1;
}

namespace {
constexpr int FORK_POOL = 128;
hipEvent_t g_fork_ev[2][FORK_POOL];
int g_fork_n[2] = {0, 0}, g_fork_i[2] = {0, 0};
std::mutex g_fork_mu;
}  // namespace
int sv_stream_fork(void* from, void* to, int light) {
    const int k = light ? 1 : 0;
    hipEvent_t e;
    {
        std::lock_guard<std::mutex> lk(g_fork_mu);
        if (g_fork_n[k] < FORK_POOL) {
            const unsigned flags = hipEventDisableTiming | (light ? hipEventDisableSystemFence : 0u);
            if (hipEventCreateWithFlags(&g_fork_ev[k][g_fork_n[k]], flags) != hipSuccess) return sv_check_launch("sv_stream_fork: event");
            ++g_fork_n[k];
        }
        // (an event is re-recorded FORK_POOL forks later: a wait captures the record that preceded it, later records do not move it)
        e = g_fork_ev[k][g_fork_i[k]++ % g_fork_n[k]];
    }
    if (hipEventRecord(e, (hipStream_t)from) != hipSuccess || hipStreamWaitEvent((hipStream_t)to, e, 0) != hipSuccess)
        return sv_check_launch("sv_stream_fork");
    return SV_OK;
}

// ---- device-side fork: flag words + the kernel that waits for one --------------------------------------------------------
// A wait that gives up (the signalling launch did not start within ~3 s: dispatch serialised by a tool, a pre-empted queue)
// must never pass silently -- the weight gradient behind it would read operands that are not written yet.  The kernel bumps
// a STICKY counter in host-mapped pinned memory (system-scope atomic): the host reads it without a copy or a sync
// (sv_flag_timeouts), Engine._join_side / FlatSGD.step / dp.all_reduce check it on every step and raise.
namespace {
constexpr int FLAG_WORDS = 1024;                 // one flag per stream
uint32_t* g_flags = nullptr;
uint32_t* g_flag_err = nullptr;                  // host-mapped: [0] time-out counter
struct FlagSlot { void* stream; uint32_t next; };
std::vector<FlagSlot> g_flag_slots;

__global__ void wait_flag_kernel(const uint32_t* flag, uint32_t value, uint32_t* timeouts) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = wall_clock64();          // 100 MHz
    while ((int32_t)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - value) < 0) {
        __builtin_amdgcn_s_sleep(32);
        if (wall_clock64() - t0 > 300000000ull) {        // ~3 s: the signalling launch never ran
            __hip_atomic_fetch_add(timeouts, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
    }
}
}  // namespace
int sv_stream_flag_next(void* stream, uint32_t** flag, uint32_t* value) {
    SV_REQUIRE(flag && value, SV_E_ARG, "sv_stream_flag_next: null argument");
    std::lock_guard<std::mutex> lk(g_fork_mu);
    if (!g_flags) {
        void* p = nullptr;
        void* h = nullptr;
        if (hipMalloc(&p, FLAG_WORDS * sizeof(uint32_t)) != hipSuccess || hipMemset(p, 0, FLAG_WORDS * sizeof(uint32_t)) != hipSuccess ||
            hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess)
            return sv_check_launch("sv_stream_flag_next: flag memory (first use inside a stream capture?)");
        memset(h, 0, 64);
        g_flag_err = static_cast<uint32_t*>(h);
        g_flags = static_cast<uint32_t*>(p);
    }
    size_t i = 0;
    while (i < g_flag_slots.size() && g_flag_slots[i].stream != stream) ++i;
    if (i == g_flag_slots.size()) {
        SV_REQUIRE((int)i < FLAG_WORDS, SV_E_ARG, "sv_stream_flag_next: more than %d streams", FLAG_WORDS);
        g_flag_slots.push_back(FlagSlot{stream, 0u});
    }
    *flag = g_flags + i;
    *value = ++g_flag_slots[i].next;
    return SV_OK;
}
int sv_stream_wait_flag(void* stream, const uint32_t* flag, uint32_t value) {
    SV_REQUIRE(flag && g_flags, SV_E_ARG, "sv_stream_wait_flag: no flag (sv_stream_flag_next first)");
    hipLaunchKernelGGL(wait_flag_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flag, value, g_flag_err);
    return sv_check_launch("sv_stream_wait_flag");
}
// sticky count of waits that gave up; no copy, no synchronisation (the word lives in host-mapped memory)
int sv_flag_timeouts(void) {
    if (!g_flag_err) return 0;
    return (int)__atomic_load_n(g_flag_err, __ATOMIC_ACQUIRE);
}
// (tests: the caller has handled the condition -- e.g. switched to event forks -- and starts over)
int sv_flag_timeouts_reset(void) {
    if (g_flag_err) __atomic_store_n(g_flag_err, 0u, __ATOMIC_RELEASE);
    return SV_OK;
}

int sv_version(void) { return SV_ABI_VERSION; }

const char* sv_last_error(void) { return g_err; }

}  // extern "C"
