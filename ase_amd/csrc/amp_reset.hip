// HumanoidAMP / HumanoidAMPGetup resets: state initialisation of the environments that just terminated and
// the refill of their AMP observation history, as ONE launch over the (reset row, history slot) items - no intermediate
// tensor in HBM.  Follows env/tasks/humanoid_amp.py:141-246,257-275 and env/tasks/humanoid_amp_getup.py:105-129
// of the reference.  The sampler and the frame builder are the device functions of amp_frames.h, the
// ones ase_hip_motion_state and ase_hip_build_amp_obs run.
//
// Two entries share one kernel body.  ase_hip_amp_reset (ids mode) reads a plan from global memory.  ase_hip_amp_reset_due
//  runs over every environment: phase 0 makes the due test and the row's draws (philox.h, environment e's
// draws depend on seed, stream position and e only) into a plan in LDS, which the same phases then read; the three
// environment buffers and the recovery counter are reset in the same launch.
#include "amp_frames.h"
#include "philox.h"

namespace {

constexpr int kMaxSteps = 64;               // history slots: all slots of a row sit in one block
constexpr int kItemsPerBlock = 32;          // (row, slot) items a block aims at (a row of more slots has a block of its own):
                                            // 512 threads, three blocks per CU beside each other at 75 registers
                                            // (ids mode: 75 VGPRs; due mode: 79 VGPRs, the same three blocks per CU -
                                            // 6 waves per SIMD; no scratch in either; from the build's resource remarks)
constexpr int kLanesPerItem = 16;           // an item's joints, root and key bodies are spread over 16 lanes
constexpr int kMaxThreads = kMaxSteps * kLanesPerItem;

struct AmpResetArgs {
    MotionClips c;
    const int32_t *env_ids, *kind, *motion_ids, *src_rows;
    const float* motion_times;
    const float *tab_root, *tab_dof_pos, *tab_dof_vel;       // [n_tab, 13] [n_tab, D] x2
    float *root_states, *dof_pos, *dof_vel;                  // row strides ld_root / ld_dof, dof element stride dof_stride
    const float *body_pos, *body_rot, *body_vel, *body_ang_vel;
    float* hist;                                             // [n_envs, S, F]
    int64_t ld_root, ld_dof, dof_stride;
    float neg_dt;                                            // (float)(-env_dt)
    int n_ids, n_envs, n_tab, S, F, rows_per_block, kinds;
    int local_root, root_height;
};

// what ase_hip_amp_reset_due adds: the due test, the draws and the book-keeping of the launch
struct AmpDueArgs {
    const uint64_t* rng;                                     // {seed, offset}
    int64_t *progress, *reset, *terminate;                   // [n_envs]; progress / terminate may be NULL
    int32_t* recovery_counter;                               // get-up options only
    const uint32_t* cdf;                                     // [n_clips]: clip m is drawn for v in [cdf[m - 1], cdf[m])
    int32_t *env_ids_out, *kind_out, *motion_ids_out, *src_rows_out;     // the exported plan, all or none
    float* motion_times_out;
    float recovery_prob, fall_prob, hybrid_prob;
    int state_init, getup, recovery_steps, n_fall, n_clips;
};
struct AmpNoDue {};

// The decision of environment e (include/ase_hip.h, the draw table of ase_hip_amp_reset_due): element 8 e + j of the stream
// is draw j.  -> kind; mid / t / src are those of the kind, 0 where it has none.
__device__ __forceinline__ int draw_reset_row(const AmpResetArgs& a, const AmpDueArgs& d, int e, int& mid, float& t, int& src) {
    const uint64_t seed = d.rng[0], off = d.rng[1], e8 = 8 * (uint64_t)e;
    mid = 0; t = 0.f; src = 0;
    if (d.getup) {
        if (philox_uniform(seed, off, e8) < d.recovery_prob && d.terminate[e] == 1) return ASE_RESET_FRAME;
        if (philox_uniform(seed, off, e8 + 1) < d.fall_prob) {
            // multiply-shift: exact, never reaches n_fall
            src = a.n_envs + (int)(((uint64_t)philox_word0(seed, off, e8 + 2) * (uint64_t)(uint32_t)d.n_fall) >> 32);
            return ASE_RESET_TABLE;
        }
    }
    bool motion = d.state_init == ASE_INIT_START || d.state_init == ASE_INIT_RANDOM;
    if (d.state_init == ASE_INIT_HYBRID) motion = philox_uniform(seed, off, e8 + 3) < d.hybrid_prob;
    if (!motion) {
        src = e;
        return ASE_RESET_TABLE;
    }
    // the first m with v < cdf[m]; cdf[n_clips - 1] = 2^24 > v
    const uint32_t v = philox_word<2>(seed, off, e8 + 4) >> 8;
    int lo = 0, hi = d.n_clips - 1;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (v < d.cdf[m]) hi = m; else lo = m + 1;
    }
    mid = lo;
    if (d.state_init != ASE_INIT_START) t = philox_uniform(seed, off, e8 + 5) * a.c.lengths[mid];
    return ASE_RESET_MOTION;
}

// One lane per (item, part): a motion state and a frame are ~200 dependent transcendental calls, one lane per item would
// make the launch as slow as that chain.  Lanes 0-14 of an item take its joints, lane 15 the root; key bodies and copies are
// spread over all 16.  Phase 1: state initialisation (slot 0) and the motion states of the history slots; phase 2: the frames.
// LDS: per item a frame [F] and the sampler's scratch (dof positions [D], key body positions [3 K], root state [13]); pitch
// odd.  Then per row of the block: the environment (-1: skip the row) and its kind.
// Due: a row is an environment, and the rest of its plan (motion, time, table row) follows in LDS.  Phase 0: the first lane
// of a row tests reset_buf and draws; the barrier hands the plan to the row's other lanes, and a block without a due row
// leaves behind it (the exit is the same for the whole block).  The same lane resets the row's buffers at the end.
template <bool Due, class DueArgs>
__device__ __forceinline__ void amp_reset_body(const AmpResetArgs& a, const DueArgs& d) {
    extern __shared__ float tile[];
    const int F = a.F, S = a.S, D = a.c.D, K = a.c.K, J = a.c.J, B = a.c.B, R = a.rows_per_block;
    const int pitch = (F + D + 3 * K + 13) | 1;
    int* env_s = (int*)(tile + R * S * pitch);
    int* kind_s = env_s + R;
    [[maybe_unused]] int* mid_s = kind_s + R;
    [[maybe_unused]] int* src_s = mid_s + R;
    [[maybe_unused]] float* time_s = (float*)(src_s + R);
    const int tid = threadIdx.x;
    const int item = tid / kLanesPerItem, sub = tid - item * kLanesPerItem;
    const int r = item / S, s = item - r * S;                // the item's row within the block and its history slot
    const int row = blockIdx.x * R + r;
    const bool live = r < R && row < a.n_ids;
    int env = -1, kd = -1;
    [[maybe_unused]] int counter = 0;                        // Due, the row's first lane: what the recovery counter becomes
    if constexpr (Due) {
        if (live && s == 0 && sub == 0) {
            const bool due = d.reset[row] != 0;
            int mid = 0, src = 0;
            float t = 0.f;
            const int k = due ? draw_reset_row(a, d, row, mid, t, src) : 0;
            // a recovery or a fall episode.  Decided here, from registers: the same test at the end of the kernel, on the kind
            // and the table row read back from LDS, came out of hipcc (ROCm 7.2) without its select - fall rows stored 0
            if (k == ASE_RESET_FRAME || src >= a.n_envs) counter = d.recovery_steps;
            env_s[r] = due ? row : -1; kind_s[r] = k; mid_s[r] = mid; src_s[r] = src; time_s[r] = t;
            if (d.env_ids_out) {
                d.env_ids_out[row] = due ? row : -1; d.kind_out[row] = k; d.motion_ids_out[row] = mid;
                d.src_rows_out[row] = src; d.motion_times_out[row] = t;
            }
        }
        __syncthreads();
        bool any = false;                                    // the same value in every lane: the block leaves as a whole
        for (int i = 0, n = min(R, a.n_ids - (int)blockIdx.x * R); i < n; ++i) any |= env_s[i] >= 0;
        if (!any) return;
        if (live) { env = env_s[r]; kd = kind_s[r]; }
    } else if (live) {
        env = a.env_ids[row];
        kd = a.kind[row];
        // an id outside the buffers, an unknown kind, a kind whose operands were not given or a table row outside the
        // table: the row is skipped, never dereferenced
        bool ok = env >= 0 && env < a.n_envs && kd >= 0 && kd <= ASE_RESET_MOTION;
        if (kd == ASE_RESET_TABLE) ok = ok && (a.kinds & 1) && a.src_rows[row] >= 0 && a.src_rows[row] < a.n_tab;
        if (kd == ASE_RESET_MOTION) ok = ok && (a.kinds & 2);
        if (!ok) env = -1;
        if (s == 0 && sub == 0) { env_s[r] = env; kind_s[r] = kd; }
    }
    // the rest of the row's plan
    const auto plan_src = [&]() -> int { if constexpr (Due) return src_s[r]; else return a.src_rows[row]; };
    const auto plan_motion = [&]() -> int { if constexpr (Due) return mid_s[r]; else return a.motion_ids[row]; };
    const auto plan_time = [&]() -> float { if constexpr (Due) return time_s[r]; else return a.motion_times[row]; };
    const bool work = live && env >= 0;
    const bool framed = work && (s == 0 || kd == ASE_RESET_MOTION);          // the item computes a frame of its own
    float* o = tile + (work ? item : 0) * pitch;
    float* sdp = o + F;                                      // scratch: dof positions, key body positions, root state
    float* skp = sdp + D;
    float* srt = skp + 3 * K;
    const int od = 13 + 6 * J;
    // the environment's state rows (slot 0 writes them) and where a slot's frame reads its dof state and root from
    float* rs = a.root_states + (int64_t)(work ? env : 0) * a.ld_root;
    float* gdp = a.dof_pos + (int64_t)(work ? env : 0) * a.ld_dof;
    float* gdv = a.dof_vel + (int64_t)(work ? env : 0) * a.ld_dof;
    // ---- phase 1
    if (work && s == 0 && kd == ASE_RESET_TABLE) {           // _reset_default / _reset_fall_episode
        const int64_t src = plan_src();
        for (int c = sub; c < 13; c += kLanesPerItem) rs[c] = a.tab_root[src * 13 + c];
        for (int d = sub; d < D; d += kLanesPerItem) {
            gdp[d * a.dof_stride] = a.tab_dof_pos[src * D + d];
            gdv[d * a.dof_stride] = a.tab_dof_vel[src * D + d];
        }
    } else if (work && kd == ASE_RESET_MOTION) {
        // slot 0: _reset_ref_state_init + _set_env_state, into the environment's state; slot k: the pose k steps before the
        // sampled time (_init_amp_obs_ref), into the scratch - its dof velocities, a copy of a clip row, go straight to
        // their columns of the frame
        const float t = s == 0 ? plan_time() : plan_time() + a.neg_dt * (float)s;
        const FrameBlend fb = motion_blend(a.c, plan_motion(), t);
        float* dp = s == 0 ? gdp : sdp;
        float* dv = s == 0 ? gdv : o + od;
        const int64_t ds = s == 0 ? a.dof_stride : 1;
        if (sub == kLanesPerItem - 1) {
            float* root = s == 0 ? rs : srt;
            motion_root(a.c, fb, root, root + 3, root + 7, root + 10);
        } else {
            for (int j = sub; j < J; j += kLanesPerItem - 1) motion_joint(a.c, fb, j, dp, ds);
        }
        for (int d = sub; d < D; d += kLanesPerItem) dv[d * ds] = a.c.dvs[fb.f0 * D + d];
        if (s > 0)
            for (int k = sub; k < K; k += kLanesPerItem) motion_key(a.c, fb, k, skp + 3 * k);
    }
    __syncthreads();       // (the state rows written above are read below by other lanes of the block)
    // ---- phase 2: the frames.  Slot 0 is the current frame: rigid-body tensors (root = body 0) and the dof state as phase 1
    // left it; slot k of a motion row is the frame of the scratch pose.
    if (framed) {
        const FrameDims dims{D, K, J, a.local_root, a.root_height};
        const int64_t b0 = (int64_t)env * B;
        const float* bp = a.body_pos + b0 * 3;
        const float* rp = s == 0 ? bp : srt;
        const float* rq = s == 0 ? a.body_rot + b0 * 4 : srt + 3;
        const float* dp = s == 0 ? gdp : sdp;
        const int64_t ds = s == 0 ? a.dof_stride : 1;
        if (sub == kLanesPerItem - 1) {
            frame_root(dims, rp, rq, s == 0 ? a.body_vel + b0 * 3 : srt + 7, s == 0 ? a.body_ang_vel + b0 * 3 : srt + 10, o);
        } else {
            for (int j = sub; j < J; j += kLanesPerItem - 1) frame_joint(a.c.dof_off, j, dp, ds, o);
        }
        if (s == 0)
            for (int d = sub; d < D; d += kLanesPerItem) o[od + d] = gdv[d * a.dof_stride];
        if (sub < K) {
            const Q4 hq = heading_quat_inv(load_q(rq));
            for (int k = sub; k < K; k += kLanesPerItem)
                frame_key(hq, rp, s == 0 ? bp + 3 * a.c.key_body[k] : skp + 3 * k, o + od + D + 3 * k);
        }
    }
    __syncthreads();
    // rows leave row-contiguous: lanes walk the feature columns of every (row, slot) of the block.  A table row's history
    // is its current frame (_init_amp_obs_default); a frame-only row keeps its history.
    const int rows = min(R, a.n_ids - blockIdx.x * R);
    for (int i = 0; i < rows; ++i) {
        const int e = env_s[i], k = kind_s[i];
        if (e < 0) continue;
        const int n = (k == ASE_RESET_FRAME ? 1 : S) * F;
        float* h = a.hist + (int64_t)e * S * F;
        for (int x = tid; x < n; x += (int)blockDim.x) {
            const int sl = x / F, f = x - sl * F;
            h[x] = tile[(i * S + (k == ASE_RESET_MOTION ? sl : 0)) * pitch + f];
        }
    }
    if constexpr (Due) {
        // _reset_env_tensors (humanoid.py:165-167) and the recovery counter (humanoid_amp_getup.py:101,106,114), by the lane
        // that read reset_buf and terminate_buf in phase 0
        if (work && s == 0 && sub == 0) {
            if (d.progress) d.progress[env] = 0;
            d.reset[env] = 0;
            if (d.terminate) d.terminate[env] = 0;
            if (d.getup) d.recovery_counter[env] = counter;
        }
    }
}

__global__ __launch_bounds__(kMaxThreads) void amp_reset_kernel(AmpResetArgs a) { amp_reset_body<false>(a, AmpNoDue{}); }
__global__ __launch_bounds__(kMaxThreads) void amp_reset_due_kernel(AmpResetArgs a, AmpDueArgs d) { amp_reset_body<true>(a, d); }

// the clip, skeleton and state operands of both entries
struct AmpResetOperands {
    const float *gts, *grs, *lrs, *grvs, *gravs, *dvs;
    int n_bodies;
    const float* lengths;
    const int32_t* num_frames;
    const float* dt;
    const int32_t *length_starts, *dof_body_ids, *dof_offsets;
    int n_joints;
    const int32_t* key_body_ids;
    int n_key;
    const float *tab_root_states, *tab_dof_pos, *tab_dof_vel;
    int n_tab;
    float* root_states;
    int64_t ld_root;
    float *dof_pos, *dof_vel;
    int64_t ld_dof;
    int dof_stride;
    const float *body_pos, *body_rot, *body_vel, *body_ang_vel;
    int n_envs, local_root_obs, root_height_obs;
    float env_dt;
    float* hist;
    int n_steps;
};

// The checks and the launch geometry the two entries share: fills a (the plan and n_ids stay with the entry).  plan_words: the
// 4-byte words per row of the block behind the staging tile.
int amp_reset_setup(const char* name, const AmpResetOperands& o, bool table, bool motion, int plan_words, AmpResetArgs& a,
                    int& threads, int& lds) {
    ASE_CHECK_ARG(o.root_states && o.dof_pos && o.dof_vel && o.body_pos && o.body_rot && o.body_vel && o.body_ang_vel && o.hist &&
                      o.dof_offsets && (o.key_body_ids || o.n_key == 0),
                  "%s: null operand", name);
    ASE_CHECK_ARG(o.n_envs > 0 && o.n_bodies >= 1, "%s: bad sizes (envs %d, bodies %d)", name, o.n_envs, o.n_bodies);
    ASE_CHECK_ARG(o.n_steps >= 1 && o.n_steps <= kMaxSteps, "%s: n_steps %d (1-%d history slots)", name, o.n_steps, kMaxSteps);
    ASE_CHECK_ARG(o.n_joints >= 1 && o.n_joints <= kMaxJoints && o.n_key >= 0 && o.n_key <= kMaxJoints,
                  "%s: %d joints, %d key bodies (at most %d each)", name, o.n_joints, o.n_key, kMaxJoints);
    ASE_CHECK_ARG(o.dof_stride == 1 || o.dof_stride == 2, "%s: dof_stride %d (1: plain tensors, 2: interleaved position / velocity)",
                  name, o.dof_stride);
    MotionClips& c = a.c;
    c.gts = o.gts; c.grs = o.grs; c.lrs = o.lrs; c.grvs = o.grvs; c.gravs = o.gravs; c.dvs = o.dvs;
    c.lengths = o.lengths; c.dt = o.dt; c.num_frames = o.num_frames; c.length_starts = o.length_starts;
    c.B = o.n_bodies; c.J = o.n_joints; c.K = o.n_key; c.D = o.dof_offsets[o.n_joints];
    for (int j = 0; j <= o.n_joints; ++j) c.dof_off[j] = o.dof_offsets[j];
    ASE_CHECK_ARG(o.dof_offsets[0] == 0 && c.D >= 1, "%s: dof_offsets do not cover the dofs", name);
    for (int j = 0; j < o.n_joints; ++j) {
        const int sz = o.dof_offsets[j + 1] - o.dof_offsets[j];
        ASE_CHECK_ARG(sz == 1 || sz == 3, "%s: joint %d has %d dofs (1 or 3 supported)", name, j, sz);
        if (motion) {
            ASE_CHECK_ARG(o.dof_body_ids[j] >= 0 && o.dof_body_ids[j] < o.n_bodies, "%s: joint %d on body %d of %d", name, j,
                          o.dof_body_ids[j], o.n_bodies);
            c.dof_body[j] = o.dof_body_ids[j];
        }
    }
    for (int k = 0; k < o.n_key; ++k) {
        ASE_CHECK_ARG(o.key_body_ids[k] >= 0 && o.key_body_ids[k] < o.n_bodies, "%s: key body %d out of range", name, o.key_body_ids[k]);
        c.key_body[k] = o.key_body_ids[k];
    }
    ASE_CHECK_ARG(o.ld_root >= 13 && o.ld_dof >= (int64_t)(c.D - 1) * o.dof_stride + 1,
                  "%s: row strides %lld / %lld do not hold 13 root columns / %d dofs at element stride %d", name, (long long)o.ld_root,
                  (long long)o.ld_dof, c.D, o.dof_stride);
    a.tab_root = o.tab_root_states; a.tab_dof_pos = o.tab_dof_pos; a.tab_dof_vel = o.tab_dof_vel;
    a.root_states = o.root_states; a.dof_pos = o.dof_pos; a.dof_vel = o.dof_vel;
    a.body_pos = o.body_pos; a.body_rot = o.body_rot; a.body_vel = o.body_vel; a.body_ang_vel = o.body_ang_vel; a.hist = o.hist;
    a.ld_root = o.ld_root; a.ld_dof = o.ld_dof; a.dof_stride = o.dof_stride;
    a.neg_dt = (float)(-o.env_dt);
    a.n_envs = o.n_envs; a.n_tab = o.n_tab; a.S = o.n_steps;
    a.kinds = (table ? ASE_RESET_HAS_TABLE : 0) | (motion ? ASE_RESET_HAS_MOTION : 0);
    a.F = 13 + 6 * o.n_joints + c.D + 3 * o.n_key;
    a.rows_per_block = o.n_steps >= kItemsPerBlock ? 1 : kItemsPerBlock / o.n_steps;
    threads = (a.rows_per_block * o.n_steps * kLanesPerItem + 63) / 64 * 64;
    a.local_root = o.local_root_obs != 0; a.root_height = o.root_height_obs != 0;
    const int pitch = (a.F + c.D + 3 * o.n_key + 13) | 1;
    lds = (a.rows_per_block * o.n_steps * pitch + plan_words * a.rows_per_block) * (int)sizeof(float);
    ASE_CHECK_ARG(lds <= 64 * 1024, "%s: frame of %d floats does not fit the staging tile", name, a.F);
    return ASE_OK;
}

}  // namespace

extern "C" int ase_hip_amp_reset(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                                 const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames,
                                 const float* dt, const int32_t* length_starts, const int32_t* dof_body_ids,
                                 const int32_t* dof_offsets, int n_joints, const int32_t* key_body_ids, int n_key,
                                 const int32_t* env_ids, const int32_t* kind, const int32_t* motion_ids,
                                 const float* motion_times, const int32_t* src_rows, int n_ids, int kinds,
                                 const float* tab_root_states, const float* tab_dof_pos, const float* tab_dof_vel, int n_tab,
                                 float* root_states, int64_t ld_root, float* dof_pos, float* dof_vel, int64_t ld_dof,
                                 int dof_stride, const float* body_pos, const float* body_rot, const float* body_vel,
                                 const float* body_ang_vel, int n_envs, int local_root_obs, int root_height_obs, float env_dt,
                                 float* hist, int n_steps, void* stream) {
    ASE_CHECK_ARG(env_ids && kind, "amp_reset: null operand");
    ASE_CHECK_ARG(n_ids >= 0, "amp_reset: bad sizes (ids %d)", n_ids);
    ASE_CHECK_ARG(kinds >= 0 && kinds <= 3, "amp_reset: kinds %d is not a mask of ASE_RESET_HAS_TABLE | ASE_RESET_HAS_MOTION", kinds);
    const bool table = kinds & ASE_RESET_HAS_TABLE, motion = kinds & ASE_RESET_HAS_MOTION;
    ASE_CHECK_ARG(!table || (tab_root_states && tab_dof_pos && tab_dof_vel && src_rows && n_tab >= 1),
                  "amp_reset: rows of kind 1 need the state table and src_rows (kinds %d)", kinds);
    ASE_CHECK_ARG(!motion || (gts && grs && lrs && grvs && gravs && dvs && lengths && num_frames && dt && length_starts &&
                              dof_body_ids && motion_ids && motion_times),
                  "amp_reset: rows of kind 2 need the clip tensors, motion_ids and motion_times (kinds %d)", kinds);
    const AmpResetOperands o = {gts, grs, lrs, grvs, gravs, dvs, n_bodies, lengths, num_frames, dt, length_starts, dof_body_ids,
                                dof_offsets, n_joints, key_body_ids, n_key, tab_root_states, tab_dof_pos, tab_dof_vel, n_tab,
                                root_states, ld_root, dof_pos, dof_vel, ld_dof, dof_stride, body_pos, body_rot, body_vel,
                                body_ang_vel, n_envs, local_root_obs, root_height_obs, env_dt, hist, n_steps};
    AmpResetArgs a = {};
    int threads = 0, lds = 0;
    if (const int rc = amp_reset_setup("amp_reset", o, table, motion, 2, a, threads, lds)) return rc;
    a.env_ids = env_ids; a.kind = kind; a.motion_ids = motion_ids; a.src_rows = src_rows; a.motion_times = motion_times;
    a.n_ids = n_ids;
    if (n_ids == 0) return ASE_OK;                   // an empty plan: nothing to write
    ASE_LAUNCH(amp_reset_kernel, dim3((n_ids + a.rows_per_block - 1) / a.rows_per_block), dim3(threads), lds,
               (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("amp_reset");
    return ASE_OK;
}

extern "C" int ase_hip_amp_reset_due(const float* gts, const float* grs, const float* lrs, const float* grvs, const float* gravs,
                                     const float* dvs, int n_bodies, const float* lengths, const int32_t* num_frames,
                                     const float* dt, const int32_t* length_starts, const int32_t* dof_body_ids,
                                     const int32_t* dof_offsets, int n_joints, const int32_t* key_body_ids, int n_key,
                                     const uint32_t* cdf, int n_clips, const float* tab_root_states, const float* tab_dof_pos,
                                     const float* tab_dof_vel, int n_tab, int state_init, double hybrid_init_prob, int getup,
                                     double recovery_episode_prob, double fall_init_prob, int recovery_steps,
                                     uint64_t* rng_state, int advance, int64_t* progress_buf, int64_t* reset_buf,
                                     int64_t* terminate_buf, int32_t* recovery_counter, int32_t* env_ids_out, int32_t* kind_out,
                                     int32_t* motion_ids_out, float* motion_times_out, int32_t* src_rows_out, float* root_states,
                                     int64_t ld_root, float* dof_pos, float* dof_vel, int64_t ld_dof, int dof_stride,
                                     const float* body_pos, const float* body_rot, const float* body_vel,
                                     const float* body_ang_vel, int n_envs, int local_root_obs, int root_height_obs, float env_dt,
                                     float* hist, int n_steps, void* stream) {
    ASE_CHECK_ARG(reset_buf, "amp_reset_due: null reset_buf");
    ASE_CHECK_ARG(rng_state, "amp_reset_due: null rng_state");
    ASE_CHECK_ARG(state_init >= ASE_INIT_DEFAULT && state_init <= ASE_INIT_HYBRID, "amp_reset_due: unknown state_init %d", state_init);
    const auto prob = [](double p) { return p >= 0.0 && p <= 1.0; };             // (false for a NaN)
    ASE_CHECK_ARG(prob(hybrid_init_prob), "amp_reset_due: hybrid_init_prob %g outside [0, 1]", hybrid_init_prob);
    ASE_CHECK_ARG(!getup || prob(recovery_episode_prob), "amp_reset_due: recovery_episode_prob %g outside [0, 1]", recovery_episode_prob);
    ASE_CHECK_ARG(!getup || prob(fall_init_prob), "amp_reset_due: fall_init_prob %g outside [0, 1]", fall_init_prob);
    ASE_CHECK_ARG(!getup || terminate_buf, "amp_reset_due: the get-up options need terminate_buf");
    ASE_CHECK_ARG(!getup || recovery_counter, "amp_reset_due: the get-up options need recovery_counter");
    ASE_CHECK_ARG(!getup || recovery_steps >= 0, "amp_reset_due: recovery_steps %d is negative", recovery_steps);
    const bool falls = getup && fall_init_prob > 0.0;
    const bool table = state_init == ASE_INIT_DEFAULT || state_init == ASE_INIT_HYBRID || falls;
    const bool motion = state_init != ASE_INIT_DEFAULT;
    const char* const init_names[4] = {"Default", "Start", "Random", "Hybrid"};
    ASE_CHECK_ARG(!table || (tab_root_states && tab_dof_pos && tab_dof_vel),
                  "amp_reset_due: state_init %s%s needs the state table (tab_root_states, tab_dof_pos, tab_dof_vel)",
                  init_names[state_init], falls ? " with fall episodes" : "");
    ASE_CHECK_ARG(!table || n_tab >= n_envs, "amp_reset_due: n_tab %d below n_envs %d (the initial state has a row per environment)",
                  n_tab, n_envs);
    ASE_CHECK_ARG(!falls || n_tab > n_envs, "amp_reset_due: fall_init_prob %g without fall rows (n_tab %d, n_envs %d)", fall_init_prob,
                  n_tab, n_envs);
    ASE_CHECK_ARG(!motion || (gts && grs && lrs && grvs && gravs && dvs && lengths && num_frames && dt && length_starts && dof_body_ids),
                  "amp_reset_due: %s needs the clip tensors and dof_body_ids", init_names[state_init]);
    ASE_CHECK_ARG(!motion || (cdf && n_clips >= 1), "amp_reset_due: %s needs cdf (n_clips %d)", init_names[state_init], n_clips);
    const int n_out = (env_ids_out != nullptr) + (kind_out != nullptr) + (motion_ids_out != nullptr) + (motion_times_out != nullptr) +
                      (src_rows_out != nullptr);
    ASE_CHECK_ARG(n_out == 0 || n_out == 5,
                  "amp_reset_due: the plan export (env_ids_out, kind_out, motion_ids_out, motion_times_out, src_rows_out) comes all "
                  "or none (%d of 5 given)", n_out);
    const AmpResetOperands o = {gts, grs, lrs, grvs, gravs, dvs, n_bodies, lengths, num_frames, dt, length_starts, dof_body_ids,
                                dof_offsets, n_joints, key_body_ids, n_key, tab_root_states, tab_dof_pos, tab_dof_vel, n_tab,
                                root_states, ld_root, dof_pos, dof_vel, ld_dof, dof_stride, body_pos, body_rot, body_vel,
                                body_ang_vel, n_envs, local_root_obs, root_height_obs, env_dt, hist, n_steps};
    AmpResetArgs a = {};
    int threads = 0, lds = 0;
    if (const int rc = amp_reset_setup("amp_reset_due", o, table, motion, 5, a, threads, lds)) return rc;
    a.n_ids = n_envs;                                // a row per environment
    AmpDueArgs d = {};
    d.rng = rng_state; d.progress = progress_buf; d.reset = reset_buf; d.terminate = terminate_buf;
    d.recovery_counter = getup ? recovery_counter : nullptr; d.cdf = cdf;
    d.env_ids_out = env_ids_out; d.kind_out = kind_out; d.motion_ids_out = motion_ids_out; d.src_rows_out = src_rows_out;
    d.motion_times_out = motion_times_out;
    d.recovery_prob = (float)recovery_episode_prob; d.fall_prob = (float)fall_init_prob; d.hybrid_prob = (float)hybrid_init_prob;
    d.state_init = state_init; d.getup = getup != 0; d.recovery_steps = recovery_steps;
    d.n_fall = falls ? n_tab - n_envs : 0; d.n_clips = n_clips;
    ASE_LAUNCH(amp_reset_due_kernel, dim3((n_envs + a.rows_per_block - 1) / a.rows_per_block), dim3(threads), lds,
               (hipStream_t)stream, a, d);
    if (advance) ASE_LAUNCH(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng_state);    // a call is one stream position
    ASE_CHECK_LAUNCH("amp_reset_due");
    return ASE_OK;
}
