// HumanoidAMP / HumanoidAMPGetup resets: state initialisation of the environments that just terminated and
// the refill of their AMP observation history, as ONE launch over the (reset row, history slot) items - no intermediate
// tensor in HBM.  Follows env/tasks/humanoid_amp.py:141-246,257-275 and env/tasks/humanoid_amp_getup.py:105-129
// of the reference.  The sampler and the frame builder are the device functions of amp_frames.h, the
// ones ase_hip_motion_state and ase_hip_build_amp_obs run.
#include "amp_frames.h"

namespace {

constexpr int kMaxSteps = 64;               // history slots: all slots of a row sit in one block
constexpr int kItemsPerBlock = 32;          // (row, slot) items a block aims at (a row of more slots has a block of its own):
                                            // 512 threads, three blocks per CU beside each other at 75 registers
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

// One lane per (item, part): a motion state and a frame are ~200 dependent transcendental calls, one lane per item would
// make the launch as slow as that chain.  Lanes 0-14 of an item take its joints, lane 15 the root; key bodies and copies are
// spread over all 16.  Phase 1: state initialisation (slot 0) and the motion states of the history slots; phase 2: the frames.
// LDS: per item a frame [F] and the sampler's scratch (dof positions [D], key body positions [3 K], root state [13]); pitch
// odd.  Then per row of the block: the environment (-1: skip the row) and its kind.
__global__ __launch_bounds__(kMaxThreads) void amp_reset_kernel(AmpResetArgs a) {
    extern __shared__ float tile[];
    const int F = a.F, S = a.S, D = a.c.D, K = a.c.K, J = a.c.J, B = a.c.B, R = a.rows_per_block;
    const int pitch = (F + D + 3 * K + 13) | 1;
    int* env_s = (int*)(tile + R * S * pitch);
    int* kind_s = env_s + R;
    const int tid = threadIdx.x;
    const int item = tid / kLanesPerItem, sub = tid - item * kLanesPerItem;
    const int r = item / S, s = item - r * S;                // the item's row within the block and its history slot
    const int row = blockIdx.x * R + r;
    const bool live = r < R && row < a.n_ids;
    int env = -1, kd = -1;
    if (live) {
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
        const int64_t src = a.src_rows[row];
        for (int c = sub; c < 13; c += kLanesPerItem) rs[c] = a.tab_root[src * 13 + c];
        for (int d = sub; d < D; d += kLanesPerItem) {
            gdp[d * a.dof_stride] = a.tab_dof_pos[src * D + d];
            gdv[d * a.dof_stride] = a.tab_dof_vel[src * D + d];
        }
    } else if (work && kd == ASE_RESET_MOTION) {
        // slot 0: _reset_ref_state_init + _set_env_state, into the environment's state; slot k: the pose k steps before the
        // sampled time (_init_amp_obs_ref), into the scratch - its dof velocities, a copy of a clip row, go straight to
        // their columns of the frame
        const float t = s == 0 ? a.motion_times[row] : a.motion_times[row] + a.neg_dt * (float)s;
        const FrameBlend fb = motion_blend(a.c, a.motion_ids[row], t);
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
    ASE_CHECK_ARG(env_ids && kind && root_states && dof_pos && dof_vel && body_pos && body_rot && body_vel && body_ang_vel &&
                      hist && dof_offsets && (key_body_ids || n_key == 0),
                  "amp_reset: null operand");
    ASE_CHECK_ARG(n_ids >= 0 && n_envs > 0 && n_bodies >= 1, "amp_reset: bad sizes (ids %d, envs %d, bodies %d)", n_ids, n_envs,
                  n_bodies);
    ASE_CHECK_ARG(n_steps >= 1 && n_steps <= kMaxSteps, "amp_reset: n_steps %d (1-%d history slots)", n_steps, kMaxSteps);
    ASE_CHECK_ARG(n_joints >= 1 && n_joints <= kMaxJoints && n_key >= 0 && n_key <= kMaxJoints,
                  "amp_reset: %d joints, %d key bodies (at most %d each)", n_joints, n_key, kMaxJoints);
    ASE_CHECK_ARG(dof_stride == 1 || dof_stride == 2, "amp_reset: dof_stride %d (1: plain tensors, 2: interleaved position / velocity)",
                  dof_stride);
    ASE_CHECK_ARG(kinds >= 0 && kinds <= 3, "amp_reset: kinds %d is not a mask of ASE_RESET_HAS_TABLE | ASE_RESET_HAS_MOTION", kinds);
    const bool table = kinds & ASE_RESET_HAS_TABLE, motion = kinds & ASE_RESET_HAS_MOTION;
    ASE_CHECK_ARG(!table || (tab_root_states && tab_dof_pos && tab_dof_vel && src_rows && n_tab >= 1),
                  "amp_reset: rows of kind 1 need the state table and src_rows (kinds %d)", kinds);
    ASE_CHECK_ARG(!motion || (gts && grs && lrs && grvs && gravs && dvs && lengths && num_frames && dt && length_starts &&
                              dof_body_ids && motion_ids && motion_times),
                  "amp_reset: rows of kind 2 need the clip tensors, motion_ids and motion_times (kinds %d)", kinds);
    AmpResetArgs a = {};
    MotionClips& c = a.c;
    c.gts = gts; c.grs = grs; c.lrs = lrs; c.grvs = grvs; c.gravs = gravs; c.dvs = dvs;
    c.lengths = lengths; c.dt = dt; c.num_frames = num_frames; c.length_starts = length_starts;
    c.B = n_bodies; c.J = n_joints; c.K = n_key; c.D = dof_offsets[n_joints];
    for (int j = 0; j <= n_joints; ++j) c.dof_off[j] = dof_offsets[j];
    ASE_CHECK_ARG(dof_offsets[0] == 0 && c.D >= 1, "amp_reset: dof_offsets do not cover the dofs");
    for (int j = 0; j < n_joints; ++j) {
        const int sz = dof_offsets[j + 1] - dof_offsets[j];
        ASE_CHECK_ARG(sz == 1 || sz == 3, "amp_reset: joint %d has %d dofs (1 or 3 supported)", j, sz);
        if (motion) {
            ASE_CHECK_ARG(dof_body_ids[j] >= 0 && dof_body_ids[j] < n_bodies, "amp_reset: joint %d on body %d of %d", j,
                          dof_body_ids[j], n_bodies);
            c.dof_body[j] = dof_body_ids[j];
        }
    }
    for (int k = 0; k < n_key; ++k) {
        ASE_CHECK_ARG(key_body_ids[k] >= 0 && key_body_ids[k] < n_bodies, "amp_reset: key body %d out of range", key_body_ids[k]);
        c.key_body[k] = key_body_ids[k];
    }
    ASE_CHECK_ARG(ld_root >= 13 && ld_dof >= (int64_t)(c.D - 1) * dof_stride + 1,
                  "amp_reset: row strides %lld / %lld do not hold 13 root columns / %d dofs at element stride %d", (long long)ld_root,
                  (long long)ld_dof, c.D, dof_stride);
    a.env_ids = env_ids; a.kind = kind; a.motion_ids = motion_ids; a.src_rows = src_rows; a.motion_times = motion_times;
    a.tab_root = tab_root_states; a.tab_dof_pos = tab_dof_pos; a.tab_dof_vel = tab_dof_vel;
    a.root_states = root_states; a.dof_pos = dof_pos; a.dof_vel = dof_vel;
    a.body_pos = body_pos; a.body_rot = body_rot; a.body_vel = body_vel; a.body_ang_vel = body_ang_vel; a.hist = hist;
    a.ld_root = ld_root; a.ld_dof = ld_dof; a.dof_stride = dof_stride;
    a.neg_dt = (float)(-env_dt);
    a.n_ids = n_ids; a.n_envs = n_envs; a.n_tab = n_tab; a.S = n_steps; a.kinds = kinds;
    a.F = 13 + 6 * n_joints + c.D + 3 * n_key;
    a.rows_per_block = n_steps >= kItemsPerBlock ? 1 : kItemsPerBlock / n_steps;
    const int threads = (a.rows_per_block * n_steps * kLanesPerItem + 63) / 64 * 64;
    a.local_root = local_root_obs != 0; a.root_height = root_height_obs != 0;
    const int pitch = (a.F + c.D + 3 * n_key + 13) | 1;
    const int lds = (a.rows_per_block * n_steps * pitch + 2 * a.rows_per_block) * (int)sizeof(float);
    ASE_CHECK_ARG(lds <= 64 * 1024, "amp_reset: frame of %d floats does not fit the staging tile", a.F);
    if (n_ids == 0) return ASE_OK;                   // an empty plan: nothing to write
    ASE_LAUNCH(amp_reset_kernel, dim3((n_ids + a.rows_per_block - 1) / a.rows_per_block), dim3(threads), lds,
               (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("amp_reset");
    return ASE_OK;
}
