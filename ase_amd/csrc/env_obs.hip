// Environment-side tensor functions: the policy observation of the humanoid, the termination test and the
// task observations / rewards of the four HRL tasks, from the simulator's rigid-body state tensors.  All of it is a few
// dozen f32 operations per element over a few MB: bandwidth- and launch-bound, so each reference function is ONE launch.
// Follows env/tasks/humanoid.py:385-413,592-672, humanoid_heading.py:231-289, humanoid_location.py:169-232,
// humanoid_reach.py:174-198 and humanoid_strike.py:193-297 (reference, /root/reference/ase).
#include "common.h"
#include "quat.h"

namespace {

// ---- compute_humanoid_observations_max (humanoid.py:592-636) -----------------------------------------------------------
constexpr int kObsEnvPerBlock = 16;
constexpr int kObsThreads = 256;

struct HumanoidObsArgs {
    const float *pos, *rot, *vel, *ang_vel;      // [n_envs, B, 3 | 4]
    const int32_t* ids;                          // rows to produce (nullable: all)
    float* obs;                                  // row r of the output starts at obs + r * ld
    int64_t ld;
    int n_envs, n_rows, B, F, local_root, root_height;
};

__device__ __forceinline__ V3 load_v(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void store_v(float* o, const V3& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// One lane per (environment, body).  The block's rows are staged in LDS ([kObsEnvPerBlock][F + 1]: F = 15 B - 2 is odd for
// the 17-body humanoid and the rows of obs are not 16-byte aligned) and leave as row-contiguous stores.
__global__ __launch_bounds__(kObsThreads) void humanoid_obs_max_kernel(HumanoidObsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int F = a.F, B = a.B, pitch = F + 1;
    float* hq_s = tile + kObsEnvPerBlock * pitch;                 // [kObsEnvPerBlock][4]: inverse heading rotation
    int* env_s = (int*)(hq_s + 4 * kObsEnvPerBlock);              // [kObsEnvPerBlock]: environment of the row, -1: none
    const int tid = threadIdx.x, r0 = blockIdx.x * kObsEnvPerBlock;
    const int live = min(kObsEnvPerBlock, a.n_rows - r0);
    if (tid < live) {
        int env = a.ids ? a.ids[r0 + tid] : r0 + tid;
        if (env < 0 || env >= a.n_envs) env = -1;                 // an id outside the buffers is skipped, never dereferenced
        env_s[tid] = env;
        if (env >= 0) {
            const Q4 hq = heading_quat_inv(load_q(a.rot + (int64_t)env * B * 4));
            hq_s[4 * tid] = hq.x; hq_s[4 * tid + 1] = hq.y; hq_s[4 * tid + 2] = hq.z; hq_s[4 * tid + 3] = hq.w;
        }
    }
    __syncthreads();
    const int o_rot = 1 + 3 * (B - 1), o_vel = o_rot + 6 * B, o_ang = o_vel + 3 * B;
    for (int i = tid; i < live * B; i += kObsThreads) {
        const int e = i / B, b = i - e * B, env = env_s[e];
        if (env < 0) continue;
        float* o = tile + e * pitch;
        const Q4 hq = load_q(hq_s + 4 * e);
        const int64_t body = (int64_t)env * B + b;
        const float* root = a.pos + (int64_t)env * B * 3;
        const Q4 q = load_q(a.rot + body * 4);
        if (b == 0) {
            o[0] = a.root_height ? root[2] : 0.f;
            // local_root_obs TRUE overwrites the root's columns with the tangent / normal of the RAW root rotation
            // (humanoid.py:620-622), false leaves the heading-local one
            tan_norm(a.local_root ? q : mul(hq, q), o + o_rot);
        } else {
            const V3 p = load_v(a.pos + body * 3);
            store_v(o + 1 + 3 * (b - 1), rot(hq, V3{p.x - root[0], p.y - root[1], p.z - root[2]}));
            tan_norm(mul(hq, q), o + o_rot + 6 * b);
        }
        store_v(o + o_vel + 3 * b, rot(hq, load_v(a.vel + body * 3)));
        store_v(o + o_ang + 3 * b, rot(hq, load_v(a.ang_vel + body * 3)));
    }
    __syncthreads();
    for (int e = 0; e < live; ++e) {
        const int env = env_s[e];
        if (env < 0) continue;
        float* o = a.obs + (int64_t)env * a.ld;
        for (int f = tid; f < F; f += kObsThreads) o[f] = tile[e * pitch + f];
    }
}

// ---- compute_humanoid_reset (humanoid.py:645-672; strike form humanoid_strike.py:255-297) -------------------------------
struct ResetArgs {
    const int64_t* progress;
    const float *contact, *pos, *heights, *tar_contact;      // [n, B, 3] [n, B, 3] [B] [n, 3] (strike form only)
    int64_t *reset, *terminated;
    uint64_t contact_mask, strike_mask;                      // bit b: body b is a contact / strike body
    float max_len;
    int n, B, early, strike;
};

__global__ __launch_bounds__(64) void humanoid_reset_kernel(ResetArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int64_t progress = a.progress[i];
    int64_t terminated = 0;
    if (a.early) {
        bool fall_contact = false, fall_height = false, other_contact = false;
        const float* c = a.contact + (int64_t)i * a.B * 3;
        const float* p = a.pos + (int64_t)i * a.B * 3;
        for (int b = 0; b < a.B; ++b) {
            if ((a.contact_mask >> b) & 1) continue;                                   // masked_contact_buf[:, contact_body_ids] = 0
            const float m = fmaxf(fmaxf(fabsf(c[3 * b]), fabsf(c[3 * b + 1])), fabsf(c[3 * b + 2]));
            fall_contact |= m > 0.1f;                                                  // humanoid.py:653
            fall_height |= p[3 * b + 2] < a.heights[b];
            if (!((a.strike_mask >> b) & 1)) other_contact |= m > 1.0f;                // contact_force_threshold, humanoid_strike.py:259
        }
        bool failed = fall_contact && fall_height;
        if (a.strike) {
            const float* t = a.tar_contact + 3 * (int64_t)i;
            const bool tar_contact = fabsf(t[0]) > 1.0f || fabsf(t[1]) > 1.0f;         // tar_contact_forces[..., 0:2]
            failed |= tar_contact && other_contact;
        }
        terminated = (failed && progress > 1) ? 1 : 0;      // the first steps can still carry contact forces
    }
    a.terminated[i] = terminated;
    a.reset[i] = ((float)progress >= a.max_len - 1.f) ? 1 : terminated;
}

// ---- task observations ----------------------------------------------------------------------------------------------
struct TaskArgs {
    const float *root_states, *prev_root_pos, *tar_a, *tar_b, *tar_speed, *tar_states, *body_pos;
    const int32_t* ids;
    float* out;              // observations: row r at out + r * ld; rewards: [n]
    int64_t ld;
    float tar_speed_scalar, dt;
    int n_envs, n_rows, kind, body_stride, body_off;
};

__global__ __launch_bounds__(64) void task_obs_kernel(TaskArgs a) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_rows) return;
    const int env = a.ids ? a.ids[r] : r;
    if (env < 0 || env >= a.n_envs) return;
    const float* rs = a.root_states + 13 * (int64_t)env;
    const Q4 hq = heading_quat_inv(load_q(rs + 3));
    float* o = a.out + (int64_t)env * a.ld;
    switch (a.kind) {
    case ASE_TASK_HEADING: {       // compute_heading_observations, humanoid_heading.py:231-250
        const float* d = a.tar_a + 2 * (int64_t)env;
        const float* f = a.tar_b + 2 * (int64_t)env;
        const V3 ld = rot(hq, V3{d[0], d[1], 0.f}), lf = rot(hq, V3{f[0], f[1], 0.f});
        o[0] = ld.x; o[1] = ld.y; o[2] = a.tar_speed[env]; o[3] = lf.x; o[4] = lf.y;
    } break;
    case ASE_TASK_LOCATION: {      // compute_location_observations, humanoid_location.py:169-183
        const float* t = a.tar_a + 2 * (int64_t)env;
        const V3 l = rot(hq, V3{t[0] - rs[0], t[1] - rs[1], 0.f - rs[2]});
        o[0] = l.x; o[1] = l.y;
    } break;
    case ASE_TASK_REACH:           // compute_location_observations, humanoid_reach.py:174-182
        store_v(o, rot(hq, load_v(a.tar_a + 3 * (int64_t)env)));
        break;
    default: {                     // compute_strike_observations, humanoid_strike.py:193-219
        const float* ts = a.tar_states + 13 * (int64_t)env;
        store_v(o, rot(hq, V3{ts[0] - rs[0], ts[1] - rs[1], ts[2]}));        // the target's height stays absolute
        tan_norm(mul(hq, load_q(ts + 3)), o + 3);
        store_v(o + 9, rot(hq, load_v(ts + 7)));
        store_v(o + 12, rot(hq, load_v(ts + 10)));
    } break;
    }
}

// ---- task rewards: every constant below is the reference's literal ----------------------------------------------------
// torch.nn.functional.normalize of a 2-vector (eps 1e-12)
__device__ __forceinline__ void normalize2(float& x, float& y) {
    const float n = fmaxf(sqrtf(x * x + y * y), 1e-12f);
    x = x / n; y = y / n;
}
// the root's speed towards (dx, dy): (root_pos - prev_root_pos) / dt projected on the direction
__device__ __forceinline__ float dir_speed(const float* rs, const float* prev, float dt, float dx, float dy, float& vx, float& vy) {
    vx = (rs[0] - prev[0]) / dt; vy = (rs[1] - prev[1]) / dt;
    return dx * vx + dy * vy;
}
// the heading direction: calc_heading_quat + quat_rotate of the x axis (utils/torch_utils.py:131-141)
__device__ __forceinline__ V3 facing_dir(const float* rs) { return rot(heading_quat(load_q(rs + 3)), V3{1.f, 0.f, 0.f}); }

__global__ __launch_bounds__(64) void task_reward_kernel(TaskArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_envs) return;
    // (the reach reward has no root operands: offsets are only applied where the kind's operands exist)
    const float* rs = a.root_states ? a.root_states + 13 * (int64_t)i : nullptr;
    const float* prev = a.prev_root_pos ? a.prev_root_pos + 3 * (int64_t)i : nullptr;
    float reward, vx, vy;
    switch (a.kind) {
    case ASE_TASK_HEADING: {       // compute_heading_reward, humanoid_heading.py:252-289
        const float vel_err_scale = 0.25f, tangent_err_w = 0.1f, dir_reward_w = 0.7f, facing_reward_w = 0.3f;   // :255-259
        const float* d = a.tar_a + 2 * (int64_t)i;
        const float* f = a.tar_b + 2 * (int64_t)i;
        const float speed = dir_speed(rs, prev, a.dt, d[0], d[1], vx, vy);
        const float tangent = (vx - speed * d[0]) + (vy - speed * d[1]);
        const float err = a.tar_speed[i] - speed;
        float dir_reward = expf(-vel_err_scale * (err * err + tangent_err_w * tangent * tangent));
        if (speed <= 0.f) dir_reward = 0.f;
        const V3 fd = facing_dir(rs);
        const float facing_reward = fmaxf(f[0] * fd.x + f[1] * fd.y, 0.f);
        reward = dir_reward_w * dir_reward + facing_reward_w * facing_reward;
    } break;
    case ASE_TASK_LOCATION: {      // compute_location_reward, humanoid_location.py:185-232
        const float dist_threshold = 0.5f, pos_err_scale = 0.5f, vel_err_scale = 4.0f;                          // :188-191
        const float pos_reward_w = 0.5f, vel_reward_w = 0.4f, face_reward_w = 0.1f;                             // :193-195
        const float* t = a.tar_a + 2 * (int64_t)i;
        float dx = t[0] - rs[0], dy = t[1] - rs[1];
        const float pos_err = dx * dx + dy * dy;
        const float pos_reward = expf(-pos_err_scale * pos_err);
        normalize2(dx, dy);
        const float speed = dir_speed(rs, prev, a.dt, dx, dy, vx, vy);
        const float err = fmaxf(a.tar_speed_scalar - speed, 0.f);
        float vel_reward = expf(-vel_err_scale * (err * err));
        if (speed <= 0.f) vel_reward = 0.f;
        const V3 fd = facing_dir(rs);
        float facing_reward = fmaxf(dx * fd.x + dy * fd.y, 0.f);
        if (pos_err < dist_threshold) { facing_reward = 1.f; vel_reward = 1.f; }
        reward = pos_reward_w * pos_reward + vel_reward_w * vel_reward + face_reward_w * facing_reward;
    } break;
    case ASE_TASK_REACH: {         // compute_reach_reward, humanoid_reach.py:184-196
        const float pos_err_scale = 4.0f;                                                                        // :187
        const float* t = a.tar_a + 3 * (int64_t)i;
        const float* p = a.body_pos + (int64_t)i * a.body_stride + a.body_off;
        const float dx = t[0] - p[0], dy = t[1] - p[1], dz = t[2] - p[2];
        reward = expf(-pos_err_scale * (dx * dx + dy * dy + dz * dz));
    } break;
    default: {                     // compute_strike_reward, humanoid_strike.py:221-252
        const float tar_speed = 1.0f, vel_err_scale = 4.0f, tar_rot_w = 0.6f, vel_reward_w = 0.4f;               // :224-228
        const float* ts = a.tar_states + 13 * (int64_t)i;
        const float tar_rot_err = rot(load_q(ts + 3), V3{0.f, 0.f, 1.f}).z;       // <up, target's up>
        const float tar_rot_r = fmaxf(1.0f - tar_rot_err, 0.f);
        float dx = ts[0] - rs[0], dy = ts[1] - rs[1];
        normalize2(dx, dy);
        const float speed = dir_speed(rs, prev, a.dt, dx, dy, vx, vy);
        const float err = fmaxf(tar_speed - speed, 0.f);
        float vel_reward = expf(-vel_err_scale * (err * err));
        if (speed <= 0.f) vel_reward = 0.f;
        reward = tar_rot_w * tar_rot_r + vel_reward_w * vel_reward;
        if (tar_rot_err < 0.2f) reward = 1.f;                                      // :249
    } break;
    }
    a.out[i] = reward;
}

// operands of a task entry: which a kind needs (all others must be NULL)
enum { kRoot = 1, kPrev = 2, kTarA = 4, kTarB = 8, kSpeed = 16, kTarStates = 32, kBody = 64 };
constexpr int kObsNeeds[4] = {kRoot | kTarA | kTarB | kSpeed, kRoot | kTarA, kRoot | kTarA, kRoot | kTarStates};
constexpr int kRewardNeeds[4] = {kRoot | kPrev | kTarA | kTarB | kSpeed, kRoot | kPrev | kTarA, kTarA | kBody,
                                 kRoot | kPrev | kTarStates};
constexpr int kTaskCols[4] = {5, 2, 3, 15};
const char* const kOperandNames[7] = {"root_states", "prev_root_pos", "tar_a", "tar_b", "tar_speed", "tar_states", "body_pos"};

int check_task_operands(const char* entry, int kind, const int* needs, const void* const* ops) {
    ASE_CHECK_ARG(kind >= 0 && kind < 4, "%s: unknown task kind %d", entry, kind);
    for (int k = 0; k < 7; ++k) {
        const bool need = (needs[kind] >> k) & 1;
        ASE_CHECK_ARG(!need || ops[k], "%s: task kind %d needs %s", entry, kind, kOperandNames[k]);
        ASE_CHECK_ARG(need || !ops[k], "%s: task kind %d does not use %s (must be NULL)", entry, kind, kOperandNames[k]);
    }
    return ASE_OK;
}

int body_mask(const char* entry, const int32_t* ids, int n, int n_bodies, uint64_t* mask) {
    *mask = 0;
    for (int k = 0; k < n; ++k) {
        ASE_CHECK_ARG(ids[k] >= 0 && ids[k] < n_bodies, "%s: body id %d out of range (%d bodies)", entry, ids[k], n_bodies);
        *mask |= (uint64_t)1 << ids[k];
    }
    return ASE_OK;
}

}  // namespace

extern "C" int ase_hip_humanoid_obs_max(const float* body_pos, const float* body_rot, const float* body_vel,
                                        const float* body_ang_vel, int n_envs, int n_bodies, int local_root_obs,
                                        int root_height_obs, const int32_t* env_ids, int n_ids, float* obs, int64_t ld_obs,
                                        int col_offset, void* stream) {
    ASE_CHECK_ARG(body_pos && body_rot && body_vel && body_ang_vel && obs, "humanoid_obs_max: null operand");
    ASE_CHECK_ARG(n_envs > 0 && n_bodies >= 1 && n_bodies <= 64, "humanoid_obs_max: bad sizes (envs %d, bodies %d; 1-64 bodies)",
                  n_envs, n_bodies);
    ASE_CHECK_ARG(env_ids ? n_ids >= 0 : n_ids == 0, "humanoid_obs_max: n_ids %d %s env_ids", n_ids, env_ids ? "with" : "without");
    HumanoidObsArgs a;
    a.F = 15 * n_bodies - 2;                         // 1 + 3 (B - 1) + 6 B + 3 B + 3 B
    ASE_CHECK_ARG(col_offset >= 0 && ld_obs >= (int64_t)col_offset + a.F,
                  "humanoid_obs_max: %d columns at offset %d do not fit a leading dimension of %lld", a.F, col_offset, (long long)ld_obs);
    a.pos = body_pos; a.rot = body_rot; a.vel = body_vel; a.ang_vel = body_ang_vel; a.ids = env_ids;
    a.obs = obs + col_offset; a.ld = ld_obs;
    a.n_envs = n_envs; a.n_rows = env_ids ? n_ids : n_envs; a.B = n_bodies;
    a.local_root = local_root_obs != 0; a.root_height = root_height_obs != 0;
    if (a.n_rows == 0) return ASE_OK;                // an empty env_ids list: nothing to write
    const int lds = (kObsEnvPerBlock * (a.F + 1) + 5 * kObsEnvPerBlock) * (int)sizeof(float);
    ASE_LAUNCH(humanoid_obs_max_kernel, dim3((a.n_rows + kObsEnvPerBlock - 1) / kObsEnvPerBlock), dim3(kObsThreads), lds,
               (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("humanoid_obs_max");
    return ASE_OK;
}

extern "C" int ase_hip_humanoid_reset(const int64_t* progress_buf, const float* contact_forces, const float* body_pos,
                                      const float* termination_heights, const int32_t* contact_body_ids, int n_contact,
                                      const float* tar_contact_forces, const int32_t* strike_body_ids, int n_strike,
                                      int n_envs, int n_bodies, float max_episode_length, int enable_early_termination,
                                      int64_t* reset, int64_t* terminated, void* stream) {
    ASE_CHECK_ARG(progress_buf && contact_forces && body_pos && termination_heights && reset && terminated,
                  "humanoid_reset: null operand");
    ASE_CHECK_ARG(n_envs > 0 && n_bodies >= 1 && n_bodies <= 64, "humanoid_reset: bad sizes (envs %d, bodies %d; 1-64 bodies)",
                  n_envs, n_bodies);
    ASE_CHECK_ARG(n_contact >= 0 && (contact_body_ids || n_contact == 0), "humanoid_reset: %d contact bodies without ids", n_contact);
    ASE_CHECK_ARG((tar_contact_forces != nullptr) == (strike_body_ids != nullptr),
                  "humanoid_reset: the strike form needs tar_contact_forces AND strike_body_ids");
    ASE_CHECK_ARG(strike_body_ids ? n_strike >= 1 : n_strike == 0, "humanoid_reset: n_strike %d %s strike_body_ids", n_strike,
                  strike_body_ids ? "with" : "without");
    ResetArgs a;
    if (int rc = body_mask("humanoid_reset", contact_body_ids, n_contact, n_bodies, &a.contact_mask)) return rc;
    if (int rc = body_mask("humanoid_reset", strike_body_ids, n_strike, n_bodies, &a.strike_mask)) return rc;
    a.progress = progress_buf; a.contact = contact_forces; a.pos = body_pos; a.heights = termination_heights;
    a.tar_contact = tar_contact_forces; a.reset = reset; a.terminated = terminated;
    a.max_len = max_episode_length; a.n = n_envs; a.B = n_bodies;
    a.early = enable_early_termination != 0; a.strike = strike_body_ids != nullptr;
    ASE_LAUNCH(humanoid_reset_kernel, dim3((n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("humanoid_reset");
    return ASE_OK;
}

extern "C" int ase_hip_task_obs(int kind, const float* root_states, const float* tar_a, const float* tar_b,
                                const float* tar_speed, const float* tar_states, int n_envs, const int32_t* env_ids,
                                int n_ids, float* obs, int64_t ld_obs, int col_offset, void* stream) {
    const void* ops[7] = {root_states, nullptr, tar_a, tar_b, tar_speed, tar_states, nullptr};
    if (int rc = check_task_operands("task_obs", kind, kObsNeeds, ops)) return rc;
    ASE_CHECK_ARG(obs, "task_obs: null output");
    ASE_CHECK_ARG(n_envs > 0, "task_obs: bad size (envs %d)", n_envs);
    ASE_CHECK_ARG(env_ids ? n_ids >= 0 : n_ids == 0, "task_obs: n_ids %d %s env_ids", n_ids, env_ids ? "with" : "without");
    ASE_CHECK_ARG(col_offset >= 0 && ld_obs >= (int64_t)col_offset + kTaskCols[kind],
                  "task_obs: %d columns at offset %d do not fit a leading dimension of %lld", kTaskCols[kind], col_offset,
                  (long long)ld_obs);
    TaskArgs a = {};
    a.root_states = root_states; a.tar_a = tar_a; a.tar_b = tar_b; a.tar_speed = tar_speed; a.tar_states = tar_states;
    a.ids = env_ids; a.out = obs + col_offset; a.ld = ld_obs;
    a.n_envs = n_envs; a.n_rows = env_ids ? n_ids : n_envs; a.kind = kind;
    if (a.n_rows == 0) return ASE_OK;
    ASE_LAUNCH(task_obs_kernel, dim3((a.n_rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("task_obs");
    return ASE_OK;
}

extern "C" int ase_hip_task_reward(int kind, const float* root_states, const float* prev_root_pos, const float* tar_a,
                                   const float* tar_b, const float* tar_speed, float tar_speed_scalar,
                                   const float* tar_states, const float* body_pos, int n_bodies, int body_id, float dt,
                                   int n_envs, float* reward, void* stream) {
    const void* ops[7] = {root_states, prev_root_pos, tar_a, tar_b, tar_speed, tar_states, body_pos};
    if (int rc = check_task_operands("task_reward", kind, kRewardNeeds, ops)) return rc;
    ASE_CHECK_ARG(reward, "task_reward: null output");
    ASE_CHECK_ARG(n_envs > 0, "task_reward: bad size (envs %d)", n_envs);
    ASE_CHECK_ARG(kind == ASE_TASK_REACH || dt > 0.f, "task_reward: dt %g must be positive", (double)dt);
    ASE_CHECK_ARG(!body_pos || (n_bodies >= 1 && body_id >= 0 && body_id < n_bodies), "task_reward: reach body %d of %d bodies",
                  body_id, n_bodies);
    TaskArgs a = {};
    a.root_states = root_states; a.prev_root_pos = prev_root_pos; a.tar_a = tar_a; a.tar_b = tar_b; a.tar_speed = tar_speed;
    a.tar_states = tar_states; a.body_pos = body_pos; a.out = reward;
    a.tar_speed_scalar = tar_speed_scalar; a.dt = dt; a.n_envs = n_envs; a.kind = kind;
    a.body_stride = 3 * n_bodies; a.body_off = 3 * body_id;
    ASE_LAUNCH(task_reward_kernel, dim3((n_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("task_reward");
    return ASE_OK;
}
