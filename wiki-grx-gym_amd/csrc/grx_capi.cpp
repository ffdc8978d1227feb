// grx_capi.cpp -- host side of the C ABI declared in include/grx.h (compiled with hipcc into
// libgrx_hip.so together with grx_kernels.hip).  No torch, no Python: plain C entry points.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <memory>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/grx.h"
#include "grx_device.h"
#include "grx_rng.h"

extern "C" {
// the kernel families' table lookups (grx_device.h, "the step kernels' tables") and, where a kernel's argument types are private to its
// translation unit, the family's typed launch
const FusedStepRow* grx_step_row(int terrain, int waves, int base, int dbg, int* envs_per_block);        // lane pairs (grx_kernels.hip)
const FusedStepRow* grx_step_row_quad(int terrain, int waves, int base, int dbg, int* envs_per_block);   // lane quads (grx_quad.hip)
int grx_tree_row(int terrain, int base, int waves, int nb, int nlc, int nchain, int nsph, const StepRow** row, const StepRow** dbg_row, int* envs_per_block, int* lds_bytes);
void grx_launch_step_tree(const StepRow* row, const KParams* dP, const void* tree_tab, const void* gen_tab, int nblocks, int waves, int lds_bytes, const float* actions,
                          float delay, long long common_step, const float* noise, float* obs_out, float* pri_out, const StepSeq* sq, const float* dbg, hipStream_t stream);
// csrc/grx_tree16.hip: the tree kernel with a 16-lane group per env (four envs per wave)
int grx_tree_row16(int terrain, int base, int waves, int nb, int nlc, int nchain, int nsph, const StepRow** row, const StepRow** dbg_row, int* envs_per_block, int* lds_bytes);
void grx_launch_step_tree16(const StepRow* row, const KParams* dP, const void* tree_tab, const void* gen_tab, int nblocks, int waves, int lds_bytes, const float* actions,
                            float delay, long long common_step, const float* noise, float* obs_out, float* pri_out, const StepSeq* sq, const float* dbg, hipStream_t stream);
int grx_generic_row(int terrain, int base, int lds_bytes, const StepRow** row);
void grx_launch_step_generic(const StepRow* row, const KParams* dP, const void* tables, float* ws, int nblocks, int epb, int lds_bytes, const float* actions, float delay,
                             long long common_step, const float* noise, float* obs_out, float* pri_out, long long seq, hipStream_t stream);
void grx_launch_reset_all_generic(const KParams* dP, const void* tables, int nblocks, int epb, uint32_t step, long long seq, uint8_t* mask, hipStream_t stream);
int grx_generic_ws_floats_per_env(int nb, int nlc);
void grx_launch_finalize(const KParams* dP, long long seq, long long* progress, long long ticket, hipStream_t stream);
void grx_launch_ticket(long long* progress, long long ticket, hipStream_t stream);
void grx_launch_reset_all(const KParams* dP, int N, uint32_t step, const StepSeq* sq, uint8_t* mask, hipStream_t stream);
void grx_launch_mark(const int32_t* env_ids, int n, int N, uint8_t* mask, hipStream_t stream);
void grx_launch_set_state(const KParams* dP, int N, const float* root, const float* q, const float* qd, const int32_t* env_ids, int n, hipStream_t stream);
void grx_launch_refresh_heights(const KParams* dP, int N, int nh, hipStream_t stream);
void grx_launch_debug_terrain(const KParams* dP, const float* xy, int n, float* out, hipStream_t stream);
void grx_launch_debug_wall(const KParams* dP, const float* xyzr, int n, float* out, hipStream_t stream);
void grx_launch_refresh_rbs(const KParams* dP, int N, int nlinks, int pushed, hipStream_t stream);
int grx_debug_rows(void);
// ABI 7: the statistics kernels of legged_gym's base reward terms
void grx_launch_base_reset(const KParams* dP, int N, const uint8_t* mask, hipStream_t stream);
void grx_launch_base_stats(const KParams* dP, long long seq, int nb, hipStream_t stream);
void grx_launch_curriculum(const KParams* dP, int nb, uint32_t step, float* obs, int nobs, float* pri, int npri, hipStream_t stream);
int grx_debug_row_of(int what);   // 0: torques, 1: last_last_actions, 2: termination contact, 3: apply_reset
int grx_set_spin_word(unsigned long long* p);
int grx_set_spin_word_quad(unsigned long long* p);
}

namespace {
constexpr int NT = GRX_NUM_REWARD_TERMS;
constexpr int NSTAT = GRX_NSTAT;
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
}  // namespace

// the pure table builders: ahead of the handle's definition, so that none of them can touch a handle or the HIP runtime
#include "grx_host_tables.h"

namespace {
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(GRX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct Timing {
    bool enabled = false;
    std::deque<std::pair<hipEvent_t, hipEvent_t>> pending;   // at most kMaxPending launches in flight
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    double total_ms = 0;   // launches already drained from `pending`
    int64_t count = 0;
    static constexpr size_t kMaxPending = 64;
    int stride = 1;        // record every stride-th launch (an event pair costs the stream ~7 us of serialisation)
    int64_t tick = 0;
};

// Host run-ahead pacing and completion visibility.  A caller that never synchronises (rollout loops, bench.py) can
// enqueue hundreds of policy steps in a few milliseconds.  On the shared MI355X boxes the HIP runtime's view of
// completed work (hipEventQuery / stream synchronisation) was measured to lag the GPU by 10-80 ms, sporadically, for
// this low-occupancy workload (rocprofv3 kernel traces show the kernels themselves at a steady 75 us).  The library
// therefore keeps its own progress word in host-pinned memory: every step kernel stores, when it STARTS, the ticket of
// the work enqueued before it (complete by stream order: one launch per step, no trailing kernel), and the host reads
// that word directly -- to bound its
// run-ahead (kPaceAhead steps: about 20 ms of queued work, enough to ride out a descheduled host thread) and to let callers spin until everything enqueued so far has really finished
// (grx_wait_idle) without going through the runtime's signal machinery.
struct Pace {
    static constexpr int64_t kPaceAhead = 256;
    volatile int64_t* progress = nullptr;   // host-pinned, device-visible
    long long* d_progress = nullptr;        // device view of the same word
    int64_t issued = 0;                     // ticket of the last step enqueued
    hipStream_t last_stream = nullptr;      // stream of the last ticketed launch (grx_wait_idle sends the closing ticket there)
};

// The layout a handle steps with, resolved ONCE by plan_layout (grx_create): grx_step, grx_reset_*, grx_debug_post_physics, grx_layout and
// state_fingerprint only read it.
enum StepFamily { FAM_PAIR, FAM_QUAD, FAM_TREE, FAM_GENERIC };   // (FAM_TREE: grx_tree.h's 8-lane groups or grx_tree16.hip's 16, by lanes_per_env)
struct StepPlan {
    StepFamily family = FAM_PAIR;
    const StepRow* row = nullptr;    // the family's table rows: the product kernel (its name is what grx_layout reports) ...
    const StepRow* dbg_row = nullptr;   // ... and the DBG instantiation grx_debug_post_physics launches (the generic family has none)
    bool base = false;               // ABI 7: legged_gym's base reward terms active -- the *_base entries of the layout
    int grid = 0, block = 0, dbg_block = 0, lds = 0;   // blocks, threads per block (of the DBG twin's launch: dbg_block), bytes of dynamic LDS
    int lanes_per_env = 2, waves = 1, envs_per_block = 0;
    int stat_cols = 0;               // statistics columns a launch of the base terms writes: one per wave of the step kernel
    // every family's picks as plan_layout made them -- those of the families this handle does not launch too: the snapshot fingerprint hashes them all
    int fused_waves = 1;             // waves per 32-env block of the lane-pair kernels (1, 2, 4 or 8), or per 16-env block of the lane-quad ones (4 or 8)
    int tree_g = GRX_TREE_G;         // lanes per env of the tree kernel: 8, or 16 (grx_tree16.hip) while 16-lane groups still fit the SIMDs in one round
    int tree_waves = 2;              // 8-env waves per block of the tree kernel: 2 while those blocks fit the CUs in one round, else 4 (a whole CU's LDS)
    int gen_epb = 64, gen_lds = 0;   // generic kernel: envs per (single-wave) block; bytes of dynamic LDS when the workspace lives there (0: global memory)
    bool generic() const { return family == FAM_TREE || family == FAM_GENERIC; }   // model outside the fast kernel's lower-limb topology (grx_generic.h, grx_tree.h)
};

struct Alloc { void* p; size_t bytes; };   // dalloc's record of a device buffer: what grx_destroy frees and a snapshot region's size (state_regions)
}  // namespace

struct grx_sim {
    grx_config cfg;
    int device = 0;
    int N = 0;
    StepPlan plan;         // which step kernel this handle launches and how
    int rbs_mode = GRX_PUBLISH_NEVER, heights_mode = GRX_PUBLISH_EVERY_STEP;   // grx_publish_mode of GRX_T_RIGID_BODY_STATES / GRX_T_MEASURED_HEIGHTS
    int nd = GRX_ND;
    void* d_gen = nullptr; // GenTables (device)
    void* d_tree = nullptr; // TreeTab (device): the lane-group tree kernel (grx_tree.h) runs this model
    float* d_ws = nullptr; // generic workspace
    int64_t seq = 0;       // launches of this handle that write statistics rows (steps, resets, debug steps; recorded ones too)
    int64_t eager_seq = 0; // ... the last of them that was launched eagerly (its rows are what grx_flush_stats reduces)
    bool stats_current = true;   // GRX_T_EPISODE_STATS already holds the statistics of the last EAGER launch (grx_flush_stats)
    bool has_recorded = false;   // a launch of this handle was recorded into a graph: replays advance the simulation without passing through the host
                                 // counters below, so grx_refresh no longer trusts them and always launches
    int64_t rbs_seq = -1, heights_seq = -1;   // launch number (seq) the on-demand tensors were last materialised for (grx_refresh)
    int64_t state_epoch = 0, rbs_epoch = -1, heights_epoch = -1;   // ... and the count of state writes outside steps (grx_set_state*, grx_reset_*)
    bool last_pushed = false;    // the last step was a _push_robots step (the base's vx, vy were overwritten after the sub-steps)
    bool prev_recorded = false;  // the last launch in host order was recorded into a graph: its successor must not fold "launch seq - 1"
    uint8_t* d_mask = nullptr;   // grx_reset_idx: per-env flags
    KParams hp;            // launch parameters: host image ...
    KParams* d_hp = nullptr;   // ... and the device copy every kernel reads through the constant address space
    KTables tab;           // host image of the device tables
    std::vector<Alloc> allocs;
    uint32_t reset_count = 0;
    Timing timing;
    Pace pace;
    // tensor table
    grx_tensor_desc desc[GRX_NUM_TENSORS];
    long long* prof_host = nullptr; int prof_blocks = 0;
    bool spin_bounded = false;    // a -DGRX_SPIN_LIMIT build: LDS spins are bounded and report through pace.progress[1]
    float* d_dbg = nullptr;       // grx_debug_post_physics: injected quantities [grx_debug_rows()][N]
    float* d_dbg_actions = nullptr;   // ... and the injected (already clipped) actions, (N, nd) row-major
    size_t ws_floats = 0;         // floats of the generic workspace d_ws
    uint64_t fingerprint = 0;     // grx_save_state / grx_load_state: hash of the creation inputs and the launched layout (state_fingerprint)
};

namespace {

#define GRX_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

template <typename T>
int dalloc(grx_sim* s, T** out, size_t count) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) return fail(GRX_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
    s->allocs.push_back({p, count * sizeof(T)});   // (owned from here on: a failure below frees it with the handle)
    e = hipMemset(p, 0, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) return fail(GRX_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    *out = static_cast<T*>(p);
    return GRX_OK;
}
// dalloc + the host array's contents: every table and constant a handle uploads
template <typename T, typename D>
int upload(grx_sim* s, D** out, const T* host, size_t count) {
    T* d = nullptr;
    GRX_TRY(dalloc(s, &d, count));
    HIP_TRY(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    *out = d;
    return GRX_OK;
}
template <typename T, typename D>
int upload(grx_sim* s, D** out, const std::vector<T>& host) { return upload(s, out, host.data(), host.size()); }
const Alloc* find_alloc(const grx_sim* s, const void* p) {
    for (const Alloc& a : s->allocs) if (a.p == p) return &a;
    return nullptr;
}

void set_desc(grx_tensor_desc* d, void* p, int dtype, int ndim, const int64_t* shape, const int64_t* stride) {
    d->data = p;
    d->dtype = dtype;
    d->ndim = ndim;
    for (int i = 0; i < 4; ++i) { d->shape[i] = i < ndim ? shape[i] : 1; d->stride[i] = i < ndim ? stride[i] : 1; }
}
// SoA [k][N] exposed as (N, k) with strides (1, N)
void desc_soa(grx_sim* s, int id, void* p, int dtype, int64_t k) {
    int64_t shape[2] = {s->N, k}, stride[2] = {1, s->N};
    set_desc(&s->desc[id], p, dtype, 2, shape, stride);
}
void desc_soa3(grx_sim* s, int id, void* p, int64_t a, int64_t b) {  // [a*b][N] as (N, a, b)
    int64_t shape[3] = {s->N, a, b}, stride[3] = {1, b * (int64_t)s->N, s->N};
    set_desc(&s->desc[id], p, GRX_F32, 3, shape, stride);
}
void desc_vec(grx_sim* s, int id, void* p, int dtype, int64_t n) {
    int64_t shape[1] = {n}, stride[1] = {1};
    set_desc(&s->desc[id], p, dtype, 1, shape, stride);
}
void desc_rows(grx_sim* s, int id, void* p, int64_t rows, int64_t cols) {  // row-major
    int64_t shape[2] = {rows, cols}, stride[2] = {cols, 1};
    set_desc(&s->desc[id], p, GRX_F32, 2, shape, stride);
}

// The generic path's tables: GenTables (device, s->d_gen) with the workspace, and -- G > 0 -- the tree kernel's TreeTab for G lanes per env into
// `tree` (host; left empty when the model does not fit a lane group: the one-lane generic kernel runs it)
int build_generic(grx_sim* s, const grx_config& c, int G, std::unique_ptr<TreeTab>& tree) {
    std::unique_ptr<GenTables> T(new GenTables());
    std::vector<int> pos_of;
    GRX_TRY(build_gen_tables(c, *T, pos_of));
    GRX_TRY(upload(s, &s->d_gen, T.get(), 1));
    s->ws_floats = (size_t)grx_generic_ws_floats_per_env(T->nb, T->nlc) * (size_t)s->N;
    GRX_TRY(dalloc(s, &s->d_ws, s->ws_floats));
    if (G > 0) GRX_TRY(build_tree_tab(c, *T, pos_of, G, tree));
    return GRX_OK;
}

// Which step kernel the handle launches, and how: ALL of the layout policy, device properties read once.  generic: the model is outside the
// fused kernels' lower-limb topology (grx_create); a generic model's tables are built and uploaded on the way (the tree kernel takes a model
// only if its tables fit a lane group).  A key without a row in its family's table is refused here, not at launch time.
int plan_layout(grx_sim* s, const grx_config& c, bool generic, bool base) {
    StepPlan& L = s->plan;
    const int N = c.num_envs;
    // the tables' terrain key: 0 plane, 1 the raster as a heightfield, 2 mesh_type 'trimesh' (the *_trimesh kernels: the reference's corrected mesh)
    const int terrain = c.terrain_type == GRX_TERRAIN_HEIGHTFIELD ? (c.vertical_faces ? 2 : 1) : 0;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, s->device));
    L.base = base;
    bool quad = false;     // four waves, a lane quad per env, 16 envs per block (grx_quad.hip): while the blocks fit the CUs in one round
    int pair_epb = 0, quad_epb = 0;
    grx_step_row(terrain, 1, 0, 0, &pair_epb); grx_step_row_quad(terrain, 8, 0, 0, &quad_epb);
    const int nblocks = (N + pair_epb - 1) / pair_epb;
    {   // waves per block: the step kernel needs a SIMD per wave (512 registers/lane).  Four waves per block while the
        // blocks fit the device's SIMDs in at most TWO rounds (measured on MI355X, rough terrain: 16384 envs = 2 rounds of
        // the four-wave layout 131 us, two-wave layout 152 us, one-wave layout 170 us; 20480 envs: 192 / 276 / 171 us),
        // one wave per block beyond; the two-wave layout is never the fastest any more (kept: GRX_WAVES_PER_BLOCK, tests)
        const int simds = prop.multiProcessorCount * 4;
        L.fused_waves = nblocks * 4 <= 2 * simds ? 8 : 1;   // (the pipeline with eight waves per block, two per SIMD: +3 % over four at 8192 envs, +1 % at 16384)
        if (const char* w = getenv("GRX_WAVES_PER_BLOCK")) {
            const int v = atoi(w);
            if (v == 1 || v == 2 || v == 4 || v == 8) L.fused_waves = v;
        }
        // a lane QUAD per env, 16 envs per block: one block per CU needs all of the CU (four SIMDs' registers, 100+ KB of LDS),
        // so this layout pays exactly while its blocks fit the device in ONE round -- half the CUs would otherwise idle
        const int qblocks = (N + quad_epb - 1) / quad_epb;
        quad = !generic && L.fused_waves >= 4 && qblocks <= prop.multiProcessorCount && !getenv("GRX_WAVES_PER_BLOCK");
        if (const char* q = getenv("GRX_LANES_PER_ENV")) quad = !generic && atoi(q) == 4;   // tests / A-B runs: 2 or 4
        if (quad) { L.fused_waves = 8; if (const char* w = getenv("GRX_QUAD_WAVES")) L.fused_waves = atoi(w) == 4 ? 4 : 8; }   // eight waves (two per SIMD) unless a test asks for the four-role pipeline
        // control_type 'V' / 'T' and heading_command (ABI 5; off in every registered task) live in the general one-wave layout only:
        // the wave pipelines keep the registered tasks' code path
        if (c.control_type != GRX_CONTROL_P || c.heading_command) { quad = false; L.fused_waves = 1; }
        // so do legged_gym's base reward terms (ABI 7), in entries of their own
        if (base) { quad = false; L.fused_waves = 1; }
    }
    if (!generic) {
        L.family = quad ? FAM_QUAD : FAM_PAIR; L.lanes_per_env = quad ? 4 : 2; L.waves = L.fused_waves;
        L.row = (quad ? grx_step_row_quad : grx_step_row)(terrain, L.waves, base, 0, &L.envs_per_block);
        L.dbg_row = (quad ? grx_step_row_quad : grx_step_row)(terrain, L.waves, base, 1, &L.envs_per_block);
        L.stat_cols = nblocks;   // (the fused one-wave entry: a wave per 32-env block)
    } else {
        // generic kernel: the per-body workspace goes to LDS when 16 envs' rows fit (155 KB for the 33-body robot: LDS round
        // trips are ~5x shorter than global ones and the kernel is bound by exactly those); else 64 envs per block over the
        // global workspace.  GRX_GENERIC_EPB = 16 / 32 / 64 forces a block size over the GLOBAL workspace (A/B runs).
        const size_t per_env = (size_t)grx_generic_ws_floats_per_env(c.model.num_bodies, GEN_MAXLC) * sizeof(float);
        // one such block fills a CU's LDS, so this only pays while all blocks run in ONE round (<= 16 envs per CU:
        // 4096 envs on an MI355X; measured 1.9 ms vs 3.2 ms at 4096 envs, but 7.5 ms vs 3.7 ms at 16384)
        if (per_env * 16 + 1024 <= 159 * 1024 && (N + 15) / 16 <= prop.multiProcessorCount) { L.gen_epb = 16; L.gen_lds = (int)(per_env * 16); }
        if (const char* ev = getenv("GRX_GENERIC_EPB")) { const int v = atoi(ev); if (v == 16 || v == 32 || v == 64) { L.gen_epb = v; L.gen_lds = 0; } }
        // the lane-group tree kernel unless GRX_TREE=0.  Lanes per env: 8 (eight envs per wave), or 16 (four envs per wave: the passes are bound by
        // the tree's depth levels whatever the group size, but twice the waves) while those waves still have a SIMD each -- 4096 envs on an
        // MI355X, BASELINE.json config 5's per-GPU size
        const char* tv_ = getenv("GRX_TREE");
        const bool try_tree = !(tv_ && atoi(tv_) == 0);
        if (try_tree) {
            if ((long long)N * GRX_TREE_GMAX <= 64ll * 4 * prop.multiProcessorCount) L.tree_g = GRX_TREE_GMAX;
            if (const char* g_ = getenv("GRX_TREE_G")) { const int v = atoi(g_); if (v == GRX_TREE_G || v == GRX_TREE_GMAX) L.tree_g = v; }
        }
        std::unique_ptr<TreeTab> tree;
        GRX_TRY(build_generic(s, c, try_tree ? L.tree_g : 0, tree));
        L.family = FAM_GENERIC;
        if (tree) {
            const TreeTab& K = *tree;
            int refused = 0, epb = 0, lds = 0;
            auto look = [&](int waves) { refused = (K.g == GRX_TREE_GMAX ? grx_tree_row16 : grx_tree_row)(terrain, base, waves, K.nb, K.nlc, K.nchain, K.nsph, &L.row, &L.dbg_row, &epb, &lds); };
            // waves per block: two while those blocks fit the device's CUs in one round (every wave still has a SIMD to itself and the CU's
            // LDS bandwidth is shared by two), else four -- a whole CU's LDS, one wave on every SIMD.  GRX_TREE_WAVES overrides (A/B runs).
            look(2);
            L.tree_waves = (N + epb - 1) / epb <= prop.multiProcessorCount ? 2 : 4;
            if (const char* tw_ = getenv("GRX_TREE_WAVES")) { const int v = atoi(tw_); if (v == 1 || v == 2 || v == 4) L.tree_waves = v; }
            look(L.tree_waves);
            while (lds > 160 * 1024 - 1024 && L.tree_waves > 1) { L.tree_waves /= 2; look(L.tree_waves); }
            if (lds <= 160 * 1024 - 1024) {   // (else the workspace of one wave does not fit a CU's LDS)
                if (refused) return fail(GRX_ERR_HIP, "grx_create: cannot raise the dynamic LDS limit of the tree kernel");
                GRX_TRY(upload(s, &s->d_tree, &K, 1));
                L.family = FAM_TREE; L.lanes_per_env = K.g; L.waves = L.tree_waves; L.envs_per_block = epb; L.lds = lds;
            }
        }
        if (L.family == FAM_GENERIC) {
            L.dbg_row = nullptr;
            if (grx_generic_row(terrain, base, L.gen_lds, &L.row)) return fail(GRX_ERR_HIP, "grx_create: cannot raise the dynamic LDS limit of the generic kernel");
            L.lanes_per_env = 1; L.waves = 1; L.envs_per_block = L.gen_epb; L.lds = L.gen_lds;
        }
    }
    if (!L.row || (!L.dbg_row && L.family != FAM_GENERIC)) return fail(GRX_ERR_UNSUPPORTED_MODEL, "grx_create: no step kernel for this layout (terrain " + std::to_string(terrain) + ", " + std::to_string(L.waves) + " waves per block)");
    L.grid = (N + L.envs_per_block - 1) / L.envs_per_block;
    L.block = L.family == FAM_GENERIC ? L.gen_epb : 64 * L.waves;   // (the one-lane kernel: a thread per env)
    if (L.dbg_row) L.dbg_block = 64 * (L.dbg_row->waves ? L.dbg_row->waves : L.waves);
    if (generic) L.stat_cols = L.family == FAM_TREE ? L.grid * L.waves : L.grid;
    return GRX_OK;
}
}  // namespace

// ---- grx_save_state / grx_load_state (include/grx.h): what a snapshot holds and how it is checked
namespace {
constexpr uint64_t kStateMagic = 0x3154415453585247ull;   // "GRXSTAT1"
constexpr int32_t kStateFormat = 1;

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
template <typename T> uint64_t fnv_val(uint64_t h, const T& v) { return fnv1a(h, &v, sizeof v); }

// the creation inputs a snapshot is only valid for: grx_config (its two host pointers cleared) with the model, N, env_offset and seed in it;
// the raster and the terrain origins behind those pointers; the layout grx_create picked (grx_layout, environment overrides included) and
// the launch parameters environment variables can change
uint64_t state_fingerprint(grx_sim* s, const grx_config& c) {
    uint64_t h = 0xcbf29ce484222325ull;
    h = fnv1a(h, &s->cfg, sizeof s->cfg);   // (height_samples / terrain_origins are nullptr in the handle's copy)
    if (c.terrain_type == GRX_TERRAIN_HEIGHTFIELD) {
        h = fnv1a(h, c.height_samples, (size_t)c.hf_rows * c.hf_cols * sizeof(int16_t));
        h = fnv1a(h, c.terrain_origins, (size_t)c.num_terrain_rows * c.num_terrain_cols * 3 * sizeof(float));
    }
    grx_layout_info li;
    if (grx_layout(s, &li) == GRX_OK) h = fnv1a(h, &li, sizeof li);
    const KParams& P = s->hp;
    const StepPlan& L = s->plan;
    for (int32_t v : {s->N, s->nd, (int)L.generic(), (int)(L.family == FAM_QUAD), (int)L.base, L.stat_cols, L.fused_waves, L.tree_g, L.tree_waves, L.gen_epb, L.gen_lds,
                      (int)(L.family == FAM_TREE), s->rbs_mode, s->heights_mode, P.self_collisions, P.publish_debug, P.publish_rbs, P.publish_heights,
                      P.stash_pre_reset, P.stat_stride, (int32_t)P.base_active})
        h = fnv_val(h, v);
    h = fnv_val(h, P.bounce_threshold);
    return h;
}

struct StateRegion { void* p; size_t bytes; };

// every device buffer of the handle that is state: written by a launch and read by a later one, or exposed through grx_tensor.  A region is a
// whole allocation: its size is the one dalloc recorded.  A buffer named here that dalloc does not know (a pointer into an allocation, memory
// from elsewhere) is an error, not a shorter snapshot
int state_regions(const grx_sim* s, std::vector<StateRegion>& r) {
    const KParams& P = s->hp;
    bool unknown = false;
    auto add = [&](const void* p, size_t bytes) { if (p && bytes) r.push_back({const_cast<void*>(p), bytes}); };
    auto one = [&](const void* p) {   // (nullptr: a buffer this handle does not have -- the workspace of a fused-kernel handle)
        const Alloc* a = p ? find_alloc(s, p) : nullptr;
        if (a) add(p, a->bytes);
        unknown = unknown || (p && !a);
    };
    auto whole = [&](auto... p) { (one(p), ...); };
    whole(P.q, P.qd, P.root, P.anchors);
    whole(P.last_actions, P.last_dof_vel, P.actions, P.torques);
    whole(P.commands, P.origins, P.levels, P.types);
    whole(P.air_time, P.land_time, P.feet_contact);
    whole(P.feet_height, P.avg_force, P.feet_force, P.contact_forces);
    whole(P.feet_pos, P.avg_speed, P.avg_speed_rpy);
    whole(P.base_heights_offset, P.ep_len, P.rew, P.reset, P.time_out, P.term_contact);
    whole(P.base_lin_vel, P.base_ang_vel, P.proj_grav);
    whole(P.episode_sums, P.reward_terms, P.heights);
    whole(P.obs, P.pri_obs);
    whole(P.stat_partial, P.stat_nblocks);
    whole(P.stat_hist, P.stats);
    if (s->plan.base) whole(P.base_episode_sums, P.base_reward_terms, P.base_stat_partial, P.base_stats, P.base_stat_hist);
    if (s->rbs_mode != GRX_PUBLISH_NEVER) whole(P.rbs);
    if (P.stash_pre_reset) whole(P.pre_q, P.pre_qd, P.pre_root, P.pre_push_vel);
    whole(s->d_mask, s->d_ws);
    // the command ranges the kernels draw from live in the device copy of KParams (the curriculum kernel widens them there)
    add(reinterpret_cast<char*>(s->d_hp) + offsetof(KParams, cmd_lin_vel_x), 6 * sizeof(float));
    if (unknown) return fail(GRX_ERR_HIP, "snapshot: a state buffer is not a whole allocation of this handle");
    return GRX_OK;
}

// the host counters that shape the next launch (statistics parity and folding, the reset draws' step number, the refresh of a push step)
struct StateCounters {
    int64_t seq, eager_seq;
    uint32_t reset_count;
    uint8_t stats_current, last_pushed, prev_recorded, pad;
};

struct StateHeader {
    uint64_t magic;
    int32_t abi_version, format;
    int64_t bytes;          // the whole blob, header included
    uint64_t fingerprint;   // state_fingerprint of the handle that wrote it
    uint64_t checksum;      // FNV-1a of everything behind the header
    StateCounters counters;
};

size_t state_payload_bytes(const std::vector<StateRegion>& r) {
    size_t n = 0;
    for (const StateRegion& x : r) n += x.bytes;
    return n;
}

// pinned staging for one copy in either direction, freed on every path
struct PinnedBuffer {
    void* p = nullptr;
    ~PinnedBuffer() { if (p) hipHostFree(p); }
};

// ---- the stages of grx_create that allocate and upload (the contents: grx_host_tables.h)
struct HandleRelease { void operator()(grx_sim* s) const { grx_destroy(s); } };   // grx_create's owner: whatever a half-built handle holds goes with it

// the state and output buffers, zeroed (those the per-env constants fill: upload_env_constants).  generic / base: the handle's class (grx_create).
// Reads from the handle: cfg, N, nd, hp.nh, and the publish modes (rbs_mode, hp.stash_pre_reset), which size the on-demand buffers
int alloc_state(grx_sim* s, bool generic, bool base) {
    const grx_config& c = s->cfg;
    KParams& P = s->hp;
    const size_t N = (size_t)s->N;
    const int nd = s->nd, nh = P.nh;
#define DA(field, count) GRX_TRY(dalloc(s, &P.field, (count)))
    DA(qd, nd * N); DA(anchors, 24 * N);
    DA(last_actions, nd * N); DA(last_dof_vel, nd * N); DA(actions, nd * N); DA(torques, nd * N);
    DA(commands, 3 * N);
    DA(air_time, 2 * N); DA(land_time, 2 * N); DA(feet_contact, 2 * N);
    DA(feet_height, 2 * N); DA(avg_force, 2 * N); DA(feet_force, 6 * N); DA(contact_forces, 3 * GRX_MAX_LINKS * N); DA(feet_pos, 6 * N); DA(avg_speed, 6 * N); DA(avg_speed_rpy, 6 * N);
    DA(base_heights_offset, N); DA(ep_len, N); DA(rew, N); DA(time_out, N); DA(term_contact, N);
    DA(base_lin_vel, 3 * N); DA(base_ang_vel, 3 * N); DA(proj_grav, 3 * N);
    DA(episode_sums, NT * N); DA(reward_terms, NT * N); DA(heights, (size_t)(nh > 0 ? nh : 1) * N);
    DA(obs, (size_t)c.num_obs * N + 64); DA(pri_obs, (size_t)c.num_pri_obs * N + 64);
    const int nblocks = (c.num_envs + GRX_PAIR_EPB - 1) / GRX_PAIR_EPB;
    // a column per block of the writing kernel: 16-env blocks at the least for the fused kernels (lane quads) and the one-lane generic kernel;
    // the tree kernel goes down to one four-env wave per block (16 lanes per env, GRX_TREE_WAVES=1)
    P.stat_stride = (generic ? 8 : 2) * nblocks + 1;
    DA(stat_partial, (size_t)2 * NSTAT * P.stat_stride); DA(stat_nblocks, 2); DA(stat_hist, (size_t)GRX_STATS_HISTORY * NSTAT);
    DA(stats, NSTAT); DA(prof, (size_t)std::max(2 * nblocks, 64) * GRX_PROF_SLOTS);   // (16-env blocks in the quad layout; the tree kernel stamps blocks 0..63 whatever their size)
    if (base) {
        constexpr int NB = GRX_NUM_BASE_REWARD_TERMS;
        DA(base_episode_sums, NB * N); DA(base_reward_terms, NB * N);
        DA(base_stat_partial, (size_t)(NB + 1) * P.stat_stride); DA(base_stats, NB); DA(base_stat_hist, (size_t)GRX_STATS_HISTORY * NB);
    }
    GRX_TRY(dalloc(s, &s->d_mask, N));
    DA(rbs, s->rbs_mode != GRX_PUBLISH_NEVER ? (size_t)13 * GRX_MAX_LINKS * N : 1);
    DA(pre_q, P.stash_pre_reset ? nd * N : 1); DA(pre_qd, P.stash_pre_reset ? nd * N : 1); DA(pre_root, P.stash_pre_reset ? 13 * N : 1);
    DA(pre_push_vel, P.stash_pre_reset ? 2 * N : 1);
#undef DA
    return GRX_OK;
}

// link frames: the refresh kernel's joint tree, every link by carrying body, and -- rbs: the fused kernels' per-lane lists (nullptr: a generic model)
int upload_model_tables(grx_sim* s, const grx_model& m, const RbsTables* rbs) {
    KParams& P = s->hp;
    if (s->rbs_mode == GRX_PUBLISH_ON_REFRESH) {   // grx_refresh: the joint tree as the model holds it (built only for the handles that refresh link
        // frames; a tree deeper than the refresh kernel walks -- such models run on the one-lane generic kernel -- loses the tensor, not the handle)
        std::unique_ptr<RefreshTab> rt(new RefreshTab());
        if (!build_refresh_tab(m, *rt)) s->rbs_mode = GRX_PUBLISH_NEVER;   // (desc[GRX_T_RIGID_BODY_STATES].data is cleared with the other NEVER handles: fill_tensor_table)
        else GRX_TRY(upload(s, &P.refresh_tab, rt.get(), 1));
    }
    std::unique_ptr<LinkTab> lt(new LinkTab());
    build_link_tab(m, *lt);
    GRX_TRY(upload(s, &P.link_tab, lt.get(), 1));
    if (rbs) GRX_TRY(upload(s, &P.rbs_tab, rbs, 1));
    return GRX_OK;
}

// a heightfield terrain: the raster, its per-cell tables, the coarse max map and the terrain origins
int upload_terrain_tables(grx_sim* s, const grx_config& c) {
    KParams& P = s->hp;
    GRX_TRY(upload(s, &P.hf, c.height_samples, (size_t)c.hf_rows * c.hf_cols));
    const TerrainTables t = build_terrain_tables(c);
    uint32_t* cells = nullptr;
    GRX_TRY(upload(s, &cells, t.cells));
    P.hf_cells = reinterpret_cast<const uint2*>(cells); P.tm_off = (int32_t)t.tm_off;
    GRX_TRY(upload(s, &P.hf_max4, t.max4));
    GRX_TRY(upload(s, &P.coarse_max, t.coarse));
    P.coarse_rows = t.coarse_rows; P.coarse_cols = t.coarse_cols;
    GRX_TRY(upload(s, &P.terrain_origins, c.terrain_origins, (size_t)c.num_terrain_rows * c.num_terrain_cols * 3));
    return GRX_OK;
}

// the per-env constants and the initial state
int upload_env_constants(grx_sim* s, const grx_config& c, float** base_mass_com) {
    KParams& P = s->hp;
    const EnvConstants e = build_env_constants(c);
    GRX_TRY(upload(s, &P.motor_strength, e.motor_strength)); GRX_TRY(upload(s, &P.base_m, e.base_m)); GRX_TRY(upload(s, &P.base_c, e.base_c));
    GRX_TRY(upload(s, &P.base_I, e.base_I)); GRX_TRY(upload(s, &P.friction, e.friction)); GRX_TRY(upload(s, &P.restitution, e.restitution));
    GRX_TRY(upload(s, &P.origins, e.origins)); GRX_TRY(upload(s, &P.levels, e.levels)); GRX_TRY(upload(s, &P.types, e.types));
    GRX_TRY(upload(s, &P.q, e.q)); GRX_TRY(upload(s, &P.root, e.root)); GRX_TRY(upload(s, &P.reset, e.reset));
    GRX_TRY(upload(s, base_mass_com, e.base_mass_com));
    return GRX_OK;
}

// ---- tensor table
void fill_tensor_table(grx_sim* s, bool base, float* base_mass_com) {
    const grx_config& c = s->cfg;
    const KParams& P = s->hp;
    const int64_t Ni = c.num_envs;
    const int nd = s->nd, nh = P.nh;
    desc_rows(s, GRX_T_OBS, P.obs, Ni, c.num_obs);
    desc_rows(s, GRX_T_PRI_OBS, P.pri_obs, Ni, c.num_pri_obs);
    desc_vec(s, GRX_T_REW, P.rew, GRX_F32, Ni);
    desc_vec(s, GRX_T_RESET, P.reset, GRX_U8, Ni);
    desc_vec(s, GRX_T_TIME_OUT, P.time_out, GRX_U8, Ni);
    desc_vec(s, GRX_T_EPISODE_LENGTH, P.ep_len, GRX_I64, Ni);
    desc_soa(s, GRX_T_DOF_POS, P.q, GRX_F32, nd);
    desc_soa(s, GRX_T_DOF_VEL, P.qd, GRX_F32, nd);
    desc_soa(s, GRX_T_TORQUES, P.torques, GRX_F32, nd);
    desc_soa(s, GRX_T_ACTIONS, P.actions, GRX_F32, nd);
    desc_soa(s, GRX_T_LAST_ACTIONS, P.last_actions, GRX_F32, nd);
    desc_soa(s, GRX_T_LAST_DOF_VEL, P.last_dof_vel, GRX_F32, nd);
    desc_soa(s, GRX_T_COMMANDS, P.commands, GRX_F32, 3);
    desc_soa(s, GRX_T_ROOT_STATES, P.root, GRX_F32, 13);
    desc_soa(s, GRX_T_BASE_LIN_VEL, P.base_lin_vel, GRX_F32, 3);
    desc_soa(s, GRX_T_BASE_ANG_VEL, P.base_ang_vel, GRX_F32, 3);
    desc_soa(s, GRX_T_PROJECTED_GRAVITY, P.proj_grav, GRX_F32, 3);
    desc_soa3(s, GRX_T_FEET_CONTACT_FORCE, P.feet_force, 2, 3);
    desc_soa3(s, GRX_T_FEET_POS, P.feet_pos, 2, 3);
    desc_soa(s, GRX_T_FEET_HEIGHT, P.feet_height, GRX_F32, 2);
    desc_soa(s, GRX_T_FEET_AIR_TIME, P.air_time, GRX_F32, 2);
    desc_soa(s, GRX_T_FEET_LAND_TIME, P.land_time, GRX_F32, 2);
    desc_soa(s, GRX_T_FEET_CONTACT, P.feet_contact, GRX_U8, 2);
    desc_soa(s, GRX_T_AVG_FEET_FORCE, P.avg_force, GRX_F32, 2);
    desc_soa3(s, GRX_T_AVG_FEET_SPEED, P.avg_speed, 2, 3);
    desc_soa3(s, GRX_T_AVG_FEET_SPEED_RPY, P.avg_speed_rpy, 2, 3);
    desc_soa(s, GRX_T_MEASURED_HEIGHTS, P.heights, GRX_F32, nh);
    desc_vec(s, GRX_T_BASE_HEIGHTS_OFFSET, P.base_heights_offset, GRX_F32, Ni);
    desc_rows(s, GRX_T_EPISODE_SUMS, P.episode_sums, NT, Ni);
    desc_rows(s, GRX_T_REWARD_TERMS, P.reward_terms, NT, Ni);
    desc_vec(s, GRX_T_TERRAIN_LEVELS, P.levels, GRX_I32, Ni);
    desc_vec(s, GRX_T_TERRAIN_TYPES, P.types, GRX_I32, Ni);
    desc_soa(s, GRX_T_ENV_ORIGINS, P.origins, GRX_F32, 3);
    desc_soa(s, GRX_T_MOTOR_STRENGTH, P.motor_strength, GRX_F32, nd);
    desc_vec(s, GRX_T_FRICTION, P.friction, GRX_F32, Ni);
    desc_rows(s, GRX_T_BASE_MASS_COM, base_mass_com, Ni, 4);
    desc_vec(s, GRX_T_TERM_CONTACT, P.term_contact, GRX_U8, Ni);
    desc_vec(s, GRX_T_EPISODE_STATS, P.stats, GRX_F32, NSTAT);
    desc_rows(s, GRX_T_EPISODE_STATS_HISTORY, P.stat_hist, GRX_STATS_HISTORY, NSTAT);
    if (base) {   // (ABI 7; a handle without base terms has no such tensors: data stays NULL, grx_tensor refuses them)
        desc_rows(s, GRX_T_BASE_EPISODE_SUMS, P.base_episode_sums, GRX_NUM_BASE_REWARD_TERMS, Ni);
        desc_rows(s, GRX_T_BASE_REWARD_TERMS, P.base_reward_terms, GRX_NUM_BASE_REWARD_TERMS, Ni);
        desc_vec(s, GRX_T_BASE_EPISODE_STATS, P.base_stats, GRX_F32, GRX_NUM_BASE_REWARD_TERMS);
        desc_rows(s, GRX_T_BASE_EPISODE_STATS_HISTORY, P.base_stat_hist, GRX_STATS_HISTORY, GRX_NUM_BASE_REWARD_TERMS);
    }
    desc_soa3(s, GRX_T_ANCHORS, P.anchors, 8, 3);
    desc_soa3(s, GRX_T_CONTACT_FORCES, P.contact_forces, GRX_MAX_LINKS, 3);
    desc_soa3(s, GRX_T_RIGID_BODY_STATES, P.rbs, GRX_MAX_LINKS, 13);
    if (s->rbs_mode == GRX_PUBLISH_NEVER) s->desc[GRX_T_RIGID_BODY_STATES].data = nullptr;
}

// the host-pinned progress word (Pace) and the bounded-spin builds' report word behind it
int start_pace(grx_sim* s) {
    void* hp_ = nullptr;
    HIP_TRY(hipHostMalloc(&hp_, 2 * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent));   // [0] progress, [1] spin report
    s->pace.progress = static_cast<volatile int64_t*>(hp_);
    s->pace.progress[0] = 0; s->pace.progress[1] = 0;
    void* dp_ = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dp_, hp_, 0));
    s->pace.d_progress = static_cast<long long*>(dp_);
    // -DGRX_SPIN_LIMIT builds: an expired LDS spin stores its code in word [1] before it traps (grx_flags.h)
    s->spin_bounded = grx_set_spin_word(reinterpret_cast<unsigned long long*>(s->pace.d_progress + 1)) == 1;
    grx_set_spin_word_quad(reinterpret_cast<unsigned long long*>(s->pace.d_progress + 1));
    return GRX_OK;
}
}  // namespace

extern "C" {

int grx_create(const grx_config* cfg, int device_id, grx_handle* out) {
    // ---- the arguments
    if (!cfg || !out) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: null argument");
    if (cfg->abi_version != GRX_ABI_VERSION || cfg->struct_size != (int)sizeof(grx_config))
        return fail(GRX_ERR_ABI_MISMATCH, "grx_create: grx_config ABI mismatch (header " + std::to_string(sizeof(grx_config)) + " B, caller " + std::to_string(cfg->struct_size) + " B)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GRX_ERR_NO_DEVICE, "grx_create: no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= ndev) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: bad device id");
    HIP_TRY(hipSetDevice(device_id));
    const grx_config& c = *cfg;
    const grx_model& m = c.model;
    if (c.num_envs < 1) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: num_envs < 1");
    // (the step kernels form a column element's byte offset in 32 bits -- GCOL, grx_kernels.hip: rows * N * 4 < 4 GiB for the tallest column
    //  table, the height scan's GRX_MAX_HEIGHT_POINTS rows: 8.4 M envs, ~30 x what fits one MI355X)
    if ((long long)c.num_envs * GRX_MAX_HEIGHT_POINTS * 4 >= (1ll << 32)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: num_envs too large for 32-bit column offsets");
    // ---- the model's class: fused or generic, base reward terms
    // the lower-limb topology runs on the fused lane-pair kernel; every other tree on the generic-tree kernel
    const int topology = check_topology(m);
    bool armature = false;   // (the fused lower-limb kernels carry no armature term: such a model runs on the tree kernel)
    for (int j = 0; j + 1 < m.num_bodies && j < GRX_MAX_DOFS; ++j) {
        if (!(m.dof_armature[j] >= 0.f)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: negative joint armature");
        armature = armature || m.dof_armature[j] != 0.f;
    }
    bool generic = topology != GRX_OK || armature || getenv("GRX_FORCE_GENERIC") != nullptr;
    // ABI 7: legged_gym's base reward terms and the command curriculum (which reads tracking_lin_vel) live in the one-wave lower-limb entries only
    if (c.command_curriculum && c.base_reward_scale[GRX_BREW_TRACKING_LIN_VEL] == 0.f)
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: command_curriculum needs the tracking_lin_vel reward term (the reference raises KeyError without it)");
    bool base = false;
    for (int t = 0; t < GRX_NUM_BASE_REWARD_TERMS; ++t) base = base || c.base_reward_scale[t] != 0.f;
    if (base && !(c.tracking_sigma > 0.f)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: base reward terms need tracking_sigma > 0");
    // control_type outside {P, V, T}: the reference raises (legged_robot.py:707); a C caller gets the status code (the Python host raises NameError before)
    if (c.control_type != GRX_CONTROL_P && c.control_type != GRX_CONTROL_V && c.control_type != GRX_CONTROL_T)
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: control_type must be GRX_CONTROL_P, _V or _T");
    // the fused lower-limb kernels hold fixed-size shape / pair tables: a lower-limb model that overflows them (say, more base-lump spheres near
    // the thighs than GRX_MAX_BC) is not refused -- it runs on the tree kernel like every other model
    std::unique_ptr<KTables> side_tab(new KTables());
    uint32_t side_ll = 0; uint64_t side_sp = 0;
    if (!generic) {
        const int rs = build_side_tables(c, *side_tab, &side_ll, &side_sp);
        if (rs == GRX_ERR_UNSUPPORTED_MODEL) generic = true;
        else if (rs) return rs;
    }
    g_err.clear();
    const int nd = m.num_bodies - 1;
    if (nd < 1 || m.num_bodies > GRX_MAX_BODIES) return fail(GRX_ERR_UNSUPPORTED_MODEL, "grx_create: unsupported body count");
    const int nh = c.measure_heights ? c.num_height_points : 0;
    if (c.num_obs != 9 + 3 * nd) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: num_obs must be 9 + 3 * num_dofs");
    if (c.num_pri_obs != c.num_obs + 8 + nh || (!generic && c.num_pri_obs > GRX_MAX_PRI)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: num_pri_obs mismatch");
    if (nh > GRX_MAX_HEIGHT_POINTS) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: too many height points");
    if (!generic && ((c.ankle_left_mask >> GRX_LEG) || (c.ankle_right_mask & 31u))) return fail(GRX_ERR_UNSUPPORTED_MODEL, "ankle masks must be split left/right");
    if (c.terrain_type == GRX_TERRAIN_HEIGHTFIELD && (!c.height_samples || !c.terrain_origins))
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: heightfield terrain needs height_samples and terrain_origins");
    if (c.publish_rigid_body_states < 0 || c.publish_rigid_body_states > 2 || c.publish_measured_heights < 0 || c.publish_measured_heights > 2)
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: publish_* must be a grx_publish_mode");
    if (m.num_links < 0 || m.num_links > GRX_MAX_LINKS) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_model.num_links out of range");
    for (int l = 0; l < m.num_links; ++l)
        if (m.link_body[l] < 0 || m.link_body[l] >= m.num_bodies) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_model.link_body out of range");
    RbsTables rbs_tab;
    if (!generic) GRX_TRY(build_rbs_tables(m, rbs_tab));
    if (c.num_terrain_rows > 255) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: more than 255 terrain levels");
    const bool heightfield = c.terrain_type == GRX_TERRAIN_HEIGHTFIELD;
    if (heightfield && c.vertical_faces && (size_t)c.hf_rows * c.hf_cols > (size_t)0x0fffffff) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_create: trimesh raster too large");

    // ---- the handle: owned here until the last line, so every exit below releases what was built so far
    std::unique_ptr<grx_sim, HandleRelease> owner(new grx_sim());
    grx_sim* s = owner.get();
    s->cfg = c;
    s->cfg.height_samples = nullptr;
    s->cfg.terrain_origins = nullptr;
    s->device = device_id;
    s->N = c.num_envs;
    s->nd = nd;
    KParams& P = s->hp;
    fill_params(c, P);
    memcpy(s->tab.height_points, c.height_points, sizeof s->tab.height_points);
    if (!generic) { memcpy(s->tab.side, side_tab->side, sizeof s->tab.side); P.ll_mask = side_ll; P.sp_mask = side_sp; }
    s->rbs_mode = c.publish_rigid_body_states;
    s->heights_mode = c.publish_measured_heights == GRX_PUBLISH_ON_REFRESH ? GRX_PUBLISH_ON_REFRESH : GRX_PUBLISH_EVERY_STEP;
    P.publish_rbs = s->rbs_mode == GRX_PUBLISH_EVERY_STEP;   // (the one-lane generic fallback does not publish link frames: cleared below)
    P.publish_heights = s->heights_mode == GRX_PUBLISH_EVERY_STEP;
    P.stash_pre_reset = s->rbs_mode == GRX_PUBLISH_ON_REFRESH || s->heights_mode == GRX_PUBLISH_ON_REFRESH;
    // ---- device memory: state (sized by what was set above: fill_params' nh, rbs_mode, stash_pre_reset), then the model's, the terrain's and the envs' tables
    GRX_TRY(alloc_state(s, generic, base));
    GRX_TRY(upload_model_tables(s, m, generic ? nullptr : &rbs_tab));
    if (heightfield) GRX_TRY(upload_terrain_tables(s, c));
    float* base_mass_com = nullptr;
    GRX_TRY(upload_env_constants(s, c, &base_mass_com));
    GRX_TRY(upload(s, &P.tables, &s->tab, 1));
    static_assert(sizeof(KParams) <= 4096, "KParams must fit the kernarg segment");
    fill_tensor_table(s, base, base_mass_com);
    // ---- the layout, and what the kernel it picked cannot publish
    GRX_TRY(plan_layout(s, c, generic, base));
    s->prof_host = P.prof; s->prof_blocks = s->plan.family == FAM_QUAD ? s->plan.grid : (c.num_envs + GRX_PAIR_EPB - 1) / GRX_PAIR_EPB;
    if (generic) {
        if (s->plan.stat_cols > s->hp.stat_stride) return fail(GRX_ERR_UNSUPPORTED_MODEL, "grx_create: more statistics columns than the table holds");
        if (s->plan.family == FAM_GENERIC) {   // the one-lane generic kernel (trees with more than eight chains): no link frames, neither every step nor on refresh (it does not stash the state before a reset)
            s->hp.publish_rbs = 0;
            if (s->rbs_mode == GRX_PUBLISH_EVERY_STEP) { s->rbs_mode = GRX_PUBLISH_NEVER; s->desc[GRX_T_RIGID_BODY_STATES].data = nullptr; }
            // (it reads the raw heights back from memory: always materialised there; it neither stashes the state before a reset)
            s->hp.publish_heights = 1; s->heights_mode = GRX_PUBLISH_EVERY_STEP;
            if (s->rbs_mode == GRX_PUBLISH_ON_REFRESH) { s->rbs_mode = GRX_PUBLISH_NEVER; s->desc[GRX_T_RIGID_BODY_STATES].data = nullptr; }
            s->hp.stash_pre_reset = 0;
        }
    }
    GRX_TRY(start_pace(s));
    {   // the parameter block is immutable from here on -- but for the command ranges of a curriculum handle (grx_curriculum_kernel): upload it once
        GRX_TRY(upload(s, &s->d_hp, &s->hp, 1));
        if (s->hp.command_curriculum) {   // the ranges the kernels draw from ARE the device copy's (the curriculum kernel widens them there)
            grx_tensor_desc& d = s->desc[GRX_T_COMMAND_RANGES];
            d.data = reinterpret_cast<char*>(s->d_hp) + offsetof(KParams, cmd_lin_vel_x);
            d.dtype = GRX_F32; d.ndim = 2; d.shape[0] = 3; d.shape[1] = 2; d.stride[0] = 2; d.stride[1] = 1;
            static_assert(offsetof(KParams, cmd_lin_vel_y) == offsetof(KParams, cmd_lin_vel_x) + 2 * sizeof(float) &&
                          offsetof(KParams, cmd_ang_vel_yaw) == offsetof(KParams, cmd_lin_vel_x) + 4 * sizeof(float), "the three ranges must be one (3, 2) block");
        }
    }
    s->fingerprint = state_fingerprint(s, c);
    *out = owner.release();
    return GRX_OK;
}

int grx_destroy(grx_handle s) {
    if (!s) return GRX_OK;
    hipSetDevice(s->device);
    for (const Alloc& a : s->allocs) hipFree(a.p);
    for (auto& pr : s->timing.pending) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto& pr : s->timing.pool) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    if (s->pace.progress) hipHostFree((void*)s->pace.progress);
    delete s;
    return GRX_OK;
}

// Spin on the pinned progress word until it reaches `target`, WITH a way out: a GPU fault (or steps that were recorded into
// a graph and never run) would otherwise hang the host forever.  The HIP runtime is polled every few thousand reads and a
// deadline (GRX_SPIN_TIMEOUT_S, default 60 s -- a step takes microseconds) bounds the wait.
static int spin_until(grx_sim* s, int64_t target, const char* who) {
    static const double limit_s = [] { const char* e = getenv("GRX_SPIN_TIMEOUT_S"); return e ? atof(e) : 60.0; }();
    if (*s->pace.progress >= target) return GRX_OK;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t it = 1;; ++it) {
        if (*s->pace.progress >= target) return GRX_OK;
        if ((it & 0x3fff) == 0) {
            const hipError_t e = hipPeekAtLastError();
            if (e != hipSuccess && e != hipErrorNotReady)
                return fail(GRX_ERR_HIP, std::string(who) + ": device error while waiting for enqueued steps: " + hipGetErrorString(e));
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s)
                return fail(GRX_ERR_HIP, std::string(who) + ": enqueued steps did not finish within GRX_SPIN_TIMEOUT_S");
        }
    }
}

// true while `st` records into a graph: a recorded step runs later (or never), so it neither paces nor takes a ticket
static bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

// place of the next launch in the handle's sequence: statistics parity / history row, and -- unless the stream is recording a
// graph -- the ticket of the work before it, which that launch publishes when it starts
static StepSeq next_seq(grx_sim* s, hipStream_t st, bool capturing) {
    StepSeq q;
    q.seq = ++s->seq;
    q.progress = capturing ? nullptr : s->pace.d_progress;
    q.ticket_done = s->pace.issued;
    // a recorded launch runs later, any number of times, or never: neither it nor the first eager launch behind it may fold the rows of
    // "launch seq - 1" (an eager step after a captured-but-never-replayed one folded partials of a launch that had not run)
    q.fold_prev = (capturing || s->prev_recorded) ? 0 : 1;
    q.pad = 0;
    s->prev_recorded = capturing;
    if (!capturing) { ++s->pace.issued; s->pace.last_stream = st; s->stats_current = false; s->eager_seq = q.seq; }   // (recorded work changes nothing until it is replayed)
    return q;
}

// Stream capture starts from reduced statistics: the rows of the last EAGER launch cannot be reduced by a recorded kernel (replayed later,
// between other launches, it would reduce some other launch's rows of that parity and overwrite a history row that is not its own).
static int capture_needs_flushed_stats(grx_sim* s, const char* who) {
    if (s->stats_current) return GRX_OK;
    return fail(GRX_ERR_INVALID_ARGUMENT, std::string(who) + ": call grx_flush_stats() on this stream BEFORE stream capture begins (the episode statistics of the last eager "
                "launch are still unreduced, and a recorded kernel cannot reduce them)");
}

// BaseTask.reset()'s reset_idx(all envs) (mask == nullptr) or reset_idx(env_ids) of the envs flagged in mask: one statistics-writing launch
static int reset_envs(grx_sim* s, uint8_t* mask, const int32_t* env_ids, int32_t n, hipStream_t st, const char* who) {
    // extras["episode"] of a full reset: mean of the running episode sums over all envs
    // (legged_robot.py:420-424); computed by the stats path with every env flagged.
    const StepPlan& L = s->plan;
    const bool capturing = stream_is_capturing(st);
    if (capturing) s->has_recorded = true;
    if (capturing) if (int rc = capture_needs_flushed_stats(s, who)) return rc;
    ++s->state_epoch;
    uint32_t step = 0x80000000u + (s->reset_count++);
    // (the generic reset kernel does not fold its predecessor's statistics: reduce them now)
    if (L.generic() && !s->stats_current) grx_launch_finalize(s->d_hp, s->eager_seq, nullptr, 0, st);
    const StepSeq q = next_seq(s, st, capturing);
    if (mask) grx_launch_mark(env_ids, n, s->N, mask, st);
    if (L.base) grx_launch_base_reset(s->d_hp, s->N, mask, st);   // ABI 7: the base terms' sums of the finished episodes (every layout; before the reset kernel consumes the flags)
    if (L.generic()) {
        grx_launch_reset_all_generic(s->d_hp, s->d_gen, (s->N + L.gen_epb - 1) / L.gen_epb, L.gen_epb, step, q.seq, mask, st);
        grx_launch_finalize(s->d_hp, q.seq, q.progress, q.progress ? s->pace.issued : 0, st);
        if (!capturing) s->stats_current = true;
    } else {
        grx_launch_reset_all(s->d_hp, s->N, step, &q, mask, st);
        if (capturing) grx_launch_finalize(s->d_hp, q.seq, nullptr, 0, st);   // recorded into a graph: carries its own reduction, see grx_step
    }
    if (L.base) grx_launch_base_stats(s->d_hp, q.seq, (s->N + 63) / 64, st);
    HIP_TRY(hipGetLastError());
    return GRX_OK;
}

int grx_reset_all(grx_handle s, void* stream) {
    if (!s) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_reset_all: null handle");
    return reset_envs(s, nullptr, nullptr, 0, (hipStream_t)stream, "grx_reset_all");
}

int grx_reset_idx(grx_handle s, const int32_t* env_ids, int32_t n, void* stream) {
    if (!s || (n > 0 && !env_ids)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_reset_idx: null argument");
    if (n <= 0) return GRX_OK;   // legged_robot.py:387-388
    return reset_envs(s, s->d_mask, env_ids, n, (hipStream_t)stream, "grx_reset_idx");
}

int grx_step(grx_handle s, grx_step_args* a, void* stream) {
    if (!s || !a) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_step: null argument");
    hipStream_t st = (hipStream_t)stream;
    static const bool no_pace = getenv("GRX_DEBUG_NO_PACE") != nullptr;
    const bool capturing = stream_is_capturing(st);
    if (capturing) s->has_recorded = true;
    if (!no_pace && !capturing)   // (the progress word trails the GPU by one launch: a step publishes its predecessor's ticket)
        if (int rc = spin_until(s, s->pace.issued - Pace::kPaceAhead, "grx_step")) return rc;
    std::pair<hipEvent_t, hipEvent_t> ev;
    const bool timed = !capturing && s->timing.enabled && (s->timing.tick++ % s->timing.stride) == 0;
    if (timed) {
        if (s->timing.pending.size() >= Timing::kMaxPending) {   // bound the event population (and the host's run-ahead)
            auto pr = s->timing.pending.front();
            s->timing.pending.pop_front();
            hipError_t qe;
            while ((qe = hipEventQuery(pr.second)) == hipErrorNotReady) {}   // spin: see Pace (any other error ends it)
            if (qe != hipSuccess) return fail(GRX_ERR_HIP, std::string("grx_step: timing event: ") + hipGetErrorString(qe));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
            s->timing.total_ms += ms; ++s->timing.count;
            s->timing.pool.push_back(pr);
        }
        if (!s->timing.pool.empty()) { ev = s->timing.pool.back(); s->timing.pool.pop_back(); }
        else { HIP_TRY(hipEventCreate(&ev.first)); HIP_TRY(hipEventCreate(&ev.second)); }
        HIP_TRY(hipEventRecord(ev.first, st));
    }
    // A step recorded into a graph may be replayed any number of times: its predecessor in execution order is then not launch
    // seq - 1, so it must not fold that launch's statistics rows (it would re-publish stale means and lose its own partials:
    // ADVICE r3).  Recorded steps therefore carry their statistics reduction with them, right behind the step: every replay leaves
    // GRX_T_EPISODE_STATS and its row of the history ring current.  The rows of the last EAGER launch must have been reduced before
    // the capture began (grx_flush_stats; ADVICE r4: recorded, that reduction ran at replay time on whatever launch then held the parity).
    if (capturing) if (int rc = capture_needs_flushed_stats(s, "grx_step")) return rc;
    const StepSeq q = next_seq(s, st, capturing);
    a->stats_slot = q.seq & (GRX_STATS_HISTORY - 1);
    a->stats_seq = q.seq;
    s->last_pushed = s->cfg.push_robots && s->cfg.push_interval > 0 && ((uint32_t)a->common_step_counter % (uint32_t)s->cfg.push_interval) == 0;
    const StepPlan& L = s->plan;
    const long long csc = (long long)a->common_step_counter;
    if (L.family == FAM_TREE)
        (L.lanes_per_env == GRX_TREE_GMAX ? grx_launch_step_tree16 : grx_launch_step_tree)(L.row, s->d_hp, s->d_tree, s->d_gen, L.grid, L.waves, L.lds, a->actions, a->delay_substeps, csc,
                                                                                           a->noise_uniform, a->obs_out, a->pri_obs_out, &q, nullptr, st);
    else if (L.family == FAM_GENERIC)
        grx_launch_step_generic(L.row, s->d_hp, s->d_gen, s->d_ws, L.grid, L.block, L.lds, a->actions, a->delay_substeps, csc, a->noise_uniform, a->obs_out, a->pri_obs_out, q.seq, st);
    else
        hipLaunchKernelGGL(static_cast<const FusedStepRow*>(L.row)->fn, dim3(L.grid), dim3(L.block), 0, st, s->d_hp, a->actions, a->delay_substeps, csc, a->noise_uniform,
                           (const float*)nullptr, a->obs_out, a->pri_obs_out, q);
    if (L.base) {   // the base terms' episode statistics right behind the step, then the command curriculum (one block; returns at once on a step without resets)
        grx_launch_base_stats(s->d_hp, q.seq, L.stat_cols, st);
        if (s->hp.command_curriculum)
            grx_launch_curriculum(s->d_hp, L.stat_cols, (uint32_t)a->common_step_counter, a->obs_out ? a->obs_out : s->hp.obs, s->cfg.num_obs,
                                  a->pri_obs_out ? a->pri_obs_out : s->hp.pri_obs, s->cfg.num_pri_obs, st);
    }
    if (timed) {
        HIP_TRY(hipEventRecord(ev.second, st));
        s->timing.pending.push_back(ev);
    }
    if (L.family == FAM_GENERIC || capturing) {   // the one-lane generic kernel does not fold its predecessor's statistics: its own small kernel, with the step's ticket
        grx_launch_finalize(s->d_hp, q.seq, q.progress, q.progress ? s->pace.issued : 0, st);
        if (!capturing) s->stats_current = true;
    }
    HIP_TRY(hipGetLastError());
    return GRX_OK;
}

int grx_flush_stats(grx_handle s, void* stream) {
    if (!s) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_flush_stats: null handle");
    if (s->stats_current) return GRX_OK;
    if (stream_is_capturing((hipStream_t)stream)) return capture_needs_flushed_stats(s, "grx_flush_stats");
    // (the last launch in host order may be a recorded one that has not run: the rows to reduce are those of the last EAGER launch)
    grx_launch_finalize(s->d_hp, s->eager_seq, nullptr, 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    s->stats_current = true;
    return GRX_OK;
}

int grx_refresh(grx_handle s, int id, void* stream) {
    if (!s) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_refresh: null handle");
    if (id < 0 || id >= GRX_NUM_TENSORS) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_refresh: unknown tensor id");
    if (!s->desc[id].data) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_refresh: this handle does not publish that tensor (grx_config.publish_*)");
    hipStream_t st = (hipStream_t)stream;
    if (id == GRX_T_RIGID_BODY_STATES && s->rbs_mode == GRX_PUBLISH_ON_REFRESH) {
        if (s->rbs_seq == s->seq && s->rbs_epoch == s->state_epoch && !s->has_recorded && !stream_is_capturing(st)) return GRX_OK;   // current
        grx_launch_refresh_rbs(s->d_hp, s->N, s->cfg.model.num_links, s->last_pushed ? 1 : 0, st);
        HIP_TRY(hipGetLastError());
        if (!stream_is_capturing(st)) { s->rbs_seq = s->seq; s->rbs_epoch = s->state_epoch; }
    } else if (id == GRX_T_MEASURED_HEIGHTS && s->heights_mode == GRX_PUBLISH_ON_REFRESH) {
        if (s->heights_seq == s->seq && s->heights_epoch == s->state_epoch && !s->has_recorded && !stream_is_capturing(st)) return GRX_OK;
        grx_launch_refresh_heights(s->d_hp, s->N, s->hp.nh, st);
        HIP_TRY(hipGetLastError());
        if (!stream_is_capturing(st)) { s->heights_seq = s->seq; s->heights_epoch = s->state_epoch; }
    }
    return GRX_OK;
}

int grx_tensor(grx_handle s, int id, grx_tensor_desc* out) {
    if (!s || !out) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_tensor: null argument");
    if (id < 0 || id >= GRX_NUM_TENSORS) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_tensor: unknown tensor id");
    if (id == GRX_T_COMMAND_RANGES && !s->hp.command_curriculum) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_tensor: GRX_T_COMMAND_RANGES exists on handles with command_curriculum only");
    if (id >= GRX_T_BASE_EPISODE_SUMS && !s->plan.base) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_tensor: the base reward term tensors exist on handles with base reward terms only");
    *out = s->desc[id];
    return GRX_OK;
}

int grx_set_state(grx_handle s, const float* root, const float* q, const float* qd, void* stream) {
    if (!s) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_set_state: null handle");
    if (stream_is_capturing((hipStream_t)stream)) s->has_recorded = true;
    ++s->state_epoch;
    grx_launch_set_state(s->d_hp, s->N, root, q, qd, nullptr, 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return GRX_OK;
}

int grx_set_state_indexed(grx_handle s, const int32_t* env_ids, int32_t n, const float* root, const float* q, const float* qd, void* stream) {
    if (!s || (n > 0 && !env_ids)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_set_state_indexed: null argument");
    if (n <= 0) return GRX_OK;
    if (stream_is_capturing((hipStream_t)stream)) s->has_recorded = true;
    ++s->state_epoch;
    grx_launch_set_state(s->d_hp, s->N, root, q, qd, env_ids, n, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return GRX_OK;
}

int grx_episode_stats(grx_handle s, float* host_out, void* stream) {
    if (!s || !host_out) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_episode_stats: null argument");
    if (int rc = grx_flush_stats(s, stream)) return rc;
    HIP_TRY(hipMemcpyAsync(host_out, s->hp.stats, NSTAT * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return GRX_OK;
}

// tests / tools: 0 = no spin of the wave pipelines has expired; else 'SP' << 48 | block << 32 | LDS address of the flag << 16 | value
// waited for (-DGRX_SPIN_LIMIT builds; *bounded = whether this library is one).  Readable after the kernel has trapped: the word
// is host memory.
int grx_debug_spin_report(grx_handle s, uint64_t* code, int* bounded) {
    if (!s || !code) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_debug_spin_report: null argument");
    *code = (uint64_t)s->pace.progress[1];
    if (bounded) *bounded = s->spin_bounded ? 1 : 0;
    return GRX_OK;
}

int grx_stats_seq(grx_handle s, int64_t* out) {
    if (!s || !out) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_stats_seq: null argument");
    *out = s->seq;
    return GRX_OK;
}

int grx_layout(grx_handle s, grx_layout_info* out) {
    if (!s || !out) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_layout: null argument");
    memset(out, 0, sizeof *out);
    const StepPlan& L = s->plan;
    out->lanes_per_env = L.lanes_per_env; out->waves_per_block = L.waves; out->envs_per_block = L.envs_per_block; out->num_blocks = L.grid;
    snprintf(out->kernel, sizeof out->kernel, "%s", L.row->name);   // the table row's name IS the kernel grx_step launches
    return GRX_OK;
}

int grx_kernel_time_ms(grx_handle s, int enable, float* avg_ms, int64_t* launches) {
    if (!s) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_kernel_time_ms: null handle");
    double tot = s->timing.total_ms;
    int64_t n = s->timing.count;
    s->timing.total_ms = 0; s->timing.count = 0;
    for (auto& pr : s->timing.pending) {
        HIP_TRY(hipEventSynchronize(pr.second));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        tot += ms;
        ++n;
        s->timing.pool.push_back(pr);
    }
    s->timing.pending.clear();
    s->timing.enabled = enable != 0;
    s->timing.stride = enable > 1 ? enable : 1;
    s->timing.tick = 0;
    if (avg_ms) *avg_ms = n ? (float)(tot / n) : 0.f;
    if (launches) *launches = n;
    return GRX_OK;
}

// tools only (GRX_PROFILE_SECTIONS builds): copy the per-block section stamps to the host
int grx_debug_profile(grx_handle s, long long* out, int max_blocks) {
    if (!s || !out) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_debug_profile: null argument");
    int nb = s->prof_blocks < max_blocks ? s->prof_blocks : max_blocks;
    HIP_TRY(hipMemcpy(out, s->prof_host, (size_t)nb * GRX_PROF_SLOTS * sizeof(long long), hipMemcpyDeviceToHost));
    return nb;
}

// TEST-ONLY: post_physics_step of every env on injected state (include/grx.h).  Uploads the records into the SoA state
// buffers + the debug rows, then launches the DBG instantiation (no sub-steps) of the step kernel this handle runs.
int grx_debug_post_physics(grx_handle s, const grx_pipeline_state* ps, int apply_reset, const grx_step_args* a, void* stream) {
    if (!s || !ps || !a) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_debug_post_physics: null argument");
    const StepPlan& L = s->plan;
    if (L.family == FAM_GENERIC) return fail(GRX_ERR_UNSUPPORTED_MODEL, "grx_debug_post_physics: the fused kernels or the tree kernel only (this model runs on the one-lane generic kernel)");
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)s->N;
    const int nd = s->nd, rows = grx_debug_rows(), r_tor = grx_debug_row_of(0), r_lla = grx_debug_row_of(1), r_term = grx_debug_row_of(2), r_apply = grx_debug_row_of(3);
    if (!s->d_dbg_actions) {   // (set last: a failure between the two allocations is resumed by the next call, never skipped)
        if (!s->d_dbg) GRX_TRY(dalloc(s, &s->d_dbg, (size_t)rows * N));
        GRX_TRY(dalloc(s, &s->d_dbg_actions, (size_t)nd * N));
    }
    std::vector<float> q(nd * N), qd(nd * N), root(13 * N), la(nd * N), lqd(nd * N), cmd(3 * N), air(2 * N), land(2 * N), bho(N), dbg((size_t)rows * N), act(nd * N);
    std::vector<uint8_t> fc(2 * N);
    std::vector<long long> ep(N);
    for (size_t i = 0; i < N; ++i) {
        const grx_pipeline_state& p = ps[i];
        for (int j = 0; j < nd; ++j) {
            q[j * N + i] = p.q[j]; qd[j * N + i] = p.qd[j]; la[j * N + i] = p.last_actions[j]; lqd[j * N + i] = p.last_dof_vel[j];
            act[i * nd + j] = p.actions[j];
            dbg[(r_tor + j) * N + i] = p.torques[j]; dbg[(r_lla + j) * N + i] = p.last_last_actions[j];
        }
        for (int k = 0; k < 13; ++k) root[k * N + i] = p.root[k];
        for (int k = 0; k < 3; ++k) cmd[k * N + i] = p.commands[k];
        for (int f = 0; f < 2; ++f) {
            air[f * N + i] = p.air_time[f]; land[f * N + i] = p.land_time[f]; fc[f * N + i] = p.contact_last[f] ? 1 : 0;
            dbg[(12 + f) * N + i] = p.avg_force[f];
            for (int k = 0; k < 3; ++k) {
                dbg[(0 + f * 3 + k) * N + i] = p.feet_force[f][k]; dbg[(6 + f * 3 + k) * N + i] = p.feet_pos[f][k];
                dbg[(14 + f * 3 + k) * N + i] = p.avg_speed[f][k];
            }
        }
        bho[i] = p.base_heights_offset; ep[i] = p.episode_length;
        dbg[(size_t)r_term * N + i] = p.term_contact ? 1.f : 0.f; dbg[(size_t)r_apply * N + i] = apply_reset ? 1.f : 0.f;
    }
    const KParams& P = s->hp;
#define UPS(dst, vec) HIP_TRY(hipMemcpyAsync(dst, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st))
    UPS(P.q, q); UPS(P.qd, qd); UPS(P.root, root); UPS(P.last_actions, la); UPS(P.last_dof_vel, lqd); UPS(P.commands, cmd);
    UPS(P.air_time, air); UPS(P.land_time, land); UPS(P.feet_contact, fc); UPS(P.base_heights_offset, bho); UPS(P.ep_len, ep);
    UPS(s->d_dbg, dbg); UPS(s->d_dbg_actions, act);
#undef UPS
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors go out of scope
    const StepSeq sq = next_seq(s, st, false);
    // the post-physics half of the kernel this handle steps with: the DBG row of its key (lane pairs: 1 / 4 / 8 waves; lane quads: 4 / 8; GRX_FORCE_GENERIC: the tree kernel)
    if (L.family == FAM_TREE)
        (L.lanes_per_env == GRX_TREE_GMAX ? grx_launch_step_tree16 : grx_launch_step_tree)(L.dbg_row, s->d_hp, s->d_tree, s->d_gen, L.grid, L.waves, L.lds, s->d_dbg_actions, 0.f,
                                                                                           (long long)a->common_step_counter, a->noise_uniform, nullptr, nullptr, &sq, s->d_dbg, st);
    else
        hipLaunchKernelGGL(static_cast<const FusedStepRow*>(L.dbg_row)->fn, dim3(L.grid), dim3(L.dbg_block), 0, st, s->d_hp, s->d_dbg_actions, 0.f, (long long)a->common_step_counter,
                           a->noise_uniform, s->d_dbg, (float*)nullptr, (float*)nullptr, sq);
    if (L.base) grx_launch_base_stats(s->d_hp, sq.seq, L.stat_cols, st);
    HIP_TRY(hipGetLastError());
    return GRX_OK;
}

// TEST-ONLY queries of the step kernels' terrain code: n host records of `width` floats -> `launch` -> n host records of 3 floats
// (inside extern "C" like spin_until: the function pointer type must have the C linkage of grx_launch_debug_*)
typedef void (*DebugQuery)(const KParams* dP, const float* in, int n, float* out, hipStream_t stream);
static int debug_query(grx_sim* s, DebugQuery launch, const std::string& who, const float* in, int width, int32_t n, float* out, void* stream) {
    if (!s || (n > 0 && (!in || !out))) return fail(GRX_ERR_INVALID_ARGUMENT, who + ": null argument");
    if (n <= 0) return GRX_OK;
    hipStream_t st = (hipStream_t)stream;
    float *din = nullptr, *dout = nullptr;
    HIP_TRY(hipMalloc(&din, (size_t)n * width * sizeof(float)));
    if (hipMalloc(&dout, (size_t)n * 3 * sizeof(float)) != hipSuccess) { hipFree(din); return fail(GRX_ERR_OUT_OF_MEMORY, who + ": out of device memory"); }
    hipError_t e = hipMemcpyAsync(din, in, (size_t)n * width * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) { launch(s->d_hp, din, n, dout, st); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(din); hipFree(dout);
    if (e != hipSuccess) return fail(GRX_ERR_HIP, who + ": " + hipGetErrorString(e));
    return GRX_OK;
}

// TEST-ONLY: the step kernels' physics terrain query at n host points (x, y) -> host (height, dh/dx, dh/dy) each (include/grx.h)
int grx_debug_terrain(grx_handle s, const float* xy, int32_t n, float* out, void* stream) {
    return debug_query(s, grx_launch_debug_terrain, "grx_debug_terrain", xy, 2, n, out, stream);
}

// TEST-ONLY, host only (no device needed): the per-cell tables grx_create builds for mesh_type 'trimesh' (build_trimesh_tables) -- ground int16[rows * cols][6],
// walls int16[rows * cols][8] (include/grx.h); the CPU test tier compares them with the oracle's own (gro_debug_trimesh_tables)
int grx_debug_trimesh_tables(const grx_config* cfg, int16_t* ground, int16_t* walls) {
    if (!cfg || !ground || !walls) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_debug_trimesh_tables: null argument");
    if (cfg->terrain_type != GRX_TERRAIN_HEIGHTFIELD || !cfg->height_samples || cfg->hf_rows < 2 || cfg->hf_cols < 2)
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_debug_trimesh_tables: a heightfield raster is needed");
    const TrimeshTables tm = build_trimesh_tables(*cfg);
    memcpy(ground, tm.ground.data(), tm.ground.size() * sizeof(int16_t));
    memcpy(walls, tm.walls.data(), tm.walls.size() * sizeof(int16_t));
    return GRX_OK;
}

// TEST-ONLY: mesh_type 'trimesh', spheres at rest (x, y, z, r) against the vertical faces next to them -> host (overlap * unit direction) each (include/grx.h)
int grx_debug_wall(grx_handle s, const float* xyzr, int32_t n, float* out, void* stream) {
    return debug_query(s, grx_launch_debug_wall, "grx_debug_wall", xyzr, 4, n, out, stream);
}

// spin until every step enqueued through this handle has finished on the GPU (reads the pinned progress word: the last
// step's own ticket is published by a one-thread kernel behind it)
int grx_wait_idle(grx_handle s) {
    if (!s) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_wait_idle: null handle");
    if ((int64_t)*s->pace.progress < s->pace.issued) {
        grx_launch_ticket(s->pace.d_progress, (long long)s->pace.issued, s->pace.last_stream);
        HIP_TRY(hipGetLastError());
    }
    return spin_until(s, s->pace.issued, "grx_wait_idle");
}

int grx_state_bytes(grx_handle s, int64_t* bytes) {
    if (!s || !bytes) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_state_bytes: null argument");
    std::vector<StateRegion> regions;
    GRX_TRY(state_regions(s, regions));
    *bytes = (int64_t)(sizeof(StateHeader) + state_payload_bytes(regions));
    return GRX_OK;
}

int grx_save_state(grx_handle s, void* host_dst, int64_t bytes, void* stream) {
    if (!s || !host_dst) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_save_state: null argument");
    std::vector<StateRegion> regions;
    GRX_TRY(state_regions(s, regions));
    const size_t payload = state_payload_bytes(regions);
    if (bytes != (int64_t)(sizeof(StateHeader) + payload))
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_save_state: bytes must equal grx_state_bytes() (" + std::to_string(sizeof(StateHeader) + payload) + ")");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_save_state: the stream is recording a graph");
    PinnedBuffer stage;
    HIP_TRY(hipHostMalloc(&stage.p, payload, hipHostMallocDefault));
    size_t off = 0;
    for (const StateRegion& x : regions) {
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(stage.p) + off, x.p, x.bytes, hipMemcpyDeviceToHost, st));
        off += x.bytes;
    }
    HIP_TRY(hipStreamSynchronize(st));
    StateHeader hd;
    memset(&hd, 0, sizeof hd);
    hd.magic = kStateMagic; hd.abi_version = GRX_ABI_VERSION; hd.format = kStateFormat; hd.bytes = bytes; hd.fingerprint = s->fingerprint;
    hd.checksum = fnv1a(0xcbf29ce484222325ull, stage.p, payload);
    hd.counters.seq = s->seq; hd.counters.eager_seq = s->eager_seq; hd.counters.reset_count = s->reset_count;
    hd.counters.stats_current = s->stats_current ? 1 : 0; hd.counters.last_pushed = s->last_pushed ? 1 : 0; hd.counters.prev_recorded = s->prev_recorded ? 1 : 0;
    memcpy(host_dst, &hd, sizeof hd);
    memcpy(static_cast<char*>(host_dst) + sizeof hd, stage.p, payload);
    return GRX_OK;
}

int grx_load_state(grx_handle s, const void* host_src, int64_t bytes, void* stream) {
    if (!s || !host_src) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: null argument");
    std::vector<StateRegion> regions;
    GRX_TRY(state_regions(s, regions));
    const size_t payload = state_payload_bytes(regions);
    if (bytes < (int64_t)sizeof(StateHeader)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: blob shorter than its header");
    StateHeader hd;
    memcpy(&hd, host_src, sizeof hd);
    if (hd.magic != kStateMagic || hd.format != kStateFormat) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: not a grx_save_state blob");
    if (hd.abi_version != GRX_ABI_VERSION) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: blob written by ABI " + std::to_string(hd.abi_version));
    if (hd.bytes != bytes || bytes != (int64_t)(sizeof(StateHeader) + payload))
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: blob of " + std::to_string(bytes) + " B, this handle's state has " + std::to_string(sizeof(StateHeader) + payload) + " B");
    if (hd.fingerprint != s->fingerprint)
        return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: the blob was written by a handle created from other inputs (config, model, envs, seed, terrain or layout)");
    const char* body = static_cast<const char*>(host_src) + sizeof hd;
    if (hd.checksum != fnv1a(0xcbf29ce484222325ull, body, payload)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: checksum mismatch (corrupted blob)");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st)) return fail(GRX_ERR_INVALID_ARGUMENT, "grx_load_state: the stream is recording a graph");
    PinnedBuffer stage;
    HIP_TRY(hipHostMalloc(&stage.p, payload, hipHostMallocDefault));
    memcpy(stage.p, body, payload);
    size_t off = 0;
    for (const StateRegion& x : regions) {
        HIP_TRY(hipMemcpyAsync(x.p, static_cast<const char*>(stage.p) + off, x.bytes, hipMemcpyHostToDevice, st));
        off += x.bytes;
    }
    HIP_TRY(hipStreamSynchronize(st));
    s->seq = hd.counters.seq; s->eager_seq = hd.counters.eager_seq; s->reset_count = hd.counters.reset_count;
    s->stats_current = hd.counters.stats_current != 0; s->last_pushed = hd.counters.last_pushed != 0; s->prev_recorded = hd.counters.prev_recorded != 0;
    s->rbs_seq = s->heights_seq = -1;   // the on-demand tensors are materialised anew
    ++s->state_epoch;
    return GRX_OK;
}

const char* grx_last_error(void) { return g_err.c_str(); }
int grx_abi_version(void) { return GRX_ABI_VERSION; }

int grx_sizeof(int id) {
    switch (id) {
        case GRX_STRUCT_CONFIG: return (int)sizeof(grx_config);
        case GRX_STRUCT_STEP_ARGS: return (int)sizeof(grx_step_args);
        case GRX_STRUCT_TENSOR_DESC: return (int)sizeof(grx_tensor_desc);
        case GRX_STRUCT_PIPELINE_STATE: return (int)sizeof(grx_pipeline_state);
        case GRX_STRUCT_LAYOUT_INFO: return (int)sizeof(grx_layout_info);
        case GRX_STRUCT_MODEL: return (int)sizeof(grx_model);
    }
    return -1;
}

const char* grx_reward_term_name(int t) {
    static const char* names[NT] = {
        "action_diff", "action_diff_diff", "action_diff_knee", "cmd_diff_ang_vel_pitch", "cmd_diff_ang_vel_roll",
        "cmd_diff_ang_vel_yaw", "cmd_diff_base_height", "cmd_diff_base_orient", "cmd_diff_forehead_orient",
        "cmd_diff_lin_vel_x", "cmd_diff_lin_vel_y", "cmd_diff_lin_vel_z", "cmd_diff_torso_orient", "collision",
        "dof_acc_new", "dof_tor_ankle_feet_lift_up", "dof_tor_new", "dof_tor_new_hip_roll", "dof_vel_new",
        "dof_vel_new_knee", "feet_air_force", "feet_air_height", "feet_air_time", "feet_land_time",
        "feet_speed_xy_close_to_ground", "feet_speed_z_close_to_height_target", "feet_stumble", "limits_actions",
        "limits_dof_pos", "limits_dof_tor", "limits_dof_vel", "on_the_air", "pose_offset", "pose_offset_hip_yaw",
        "stand_still", "termination"};
    return (t >= 0 && t < NT) ? names[t] : "";
}

const char* grx_base_reward_term_name(int t) {
    static const char* names[GRX_NUM_BASE_REWARD_TERMS] = {
        "action_rate", "ang_vel_xy", "base_height", "dof_acc", "dof_pos_limits", "dof_vel", "dof_vel_limits", "feet_contact_forces",
        "lin_vel_z", "orientation", "stumble", "torque_limits", "torques", "tracking_ang_vel", "tracking_lin_vel"};
    return (t >= 0 && t < GRX_NUM_BASE_REWARD_TERMS) ? names[t] : nullptr;
}

}  // extern "C"
