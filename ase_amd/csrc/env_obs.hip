// Environment-side tensor functions: the policy observation of the humanoid, the termination test and the
// task observations / rewards of the four HRL tasks, from the simulator's rigid-body state tensors.  All of it is a few
// dozen f32 operations per element over a few MB: bandwidth- and launch-bound, so each reference function is ONE launch.
// Follows env/tasks/humanoid.py:385-413,592-672, humanoid_heading.py:231-289, humanoid_location.py:169-232,
// humanoid_reach.py:174-198 and humanoid_strike.py:193-297 (reference, /root/reference/ase).
// The per-row arithmetic lives in env_funcs.h, which env_step.hip calls too.
#include "env_funcs.h"

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
    for (int i = tid; i < live * B; i += kObsThreads) {
        const int e = i / B, b = i - e * B, env = env_s[e];
        if (env < 0) continue;
        const int64_t body = (int64_t)env * B + b;
        humanoid_obs_body(b, B, a.local_root, a.root_height, load_q(hq_s + 4 * e), a.pos + (int64_t)env * B * 3, a.pos + body * 3,
                          a.rot + body * 4, a.vel + body * 3, a.ang_vel + body * 3, tile + e * pitch);
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
    const float *contact, *pos, *tar_contact;                // [n, B, 3] [n, B, 3] [n, 3] (strike form only)
    int64_t *reset, *terminated;
    ResetRule rule;
    int n;
};

__global__ __launch_bounds__(64) void humanoid_reset_kernel(ResetArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    int64_t terminated;
    const int B = a.rule.B;
    a.reset[i] = humanoid_reset_row(a.rule, a.progress[i], a.contact + (int64_t)i * B * 3, 3, a.pos + (int64_t)i * B * 3, 3,
                                    a.rule.strike ? a.tar_contact + 3 * (int64_t)i : nullptr, terminated);
    a.terminated[i] = terminated;
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
    // (offsets are only applied where the kind's operands exist)
    const int wa = a.kind == ASE_TASK_REACH ? 3 : 2;
    task_obs_row(a.kind, a.root_states + 13 * (int64_t)env, a.tar_a ? a.tar_a + wa * (int64_t)env : nullptr,
                 a.tar_b ? a.tar_b + 2 * (int64_t)env : nullptr, a.tar_speed ? a.tar_speed[env] : 0.f,
                 a.tar_states ? a.tar_states + 13 * (int64_t)env : nullptr, a.out + (int64_t)env * a.ld);
}

__global__ __launch_bounds__(64) void task_reward_kernel(TaskArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_envs) return;
    // (the reach reward has no root operands: offsets are only applied where the kind's operands exist)
    const int wa = a.kind == ASE_TASK_REACH ? 3 : 2;
    a.out[i] = task_reward_row(a.kind, a.root_states ? a.root_states + 13 * (int64_t)i : nullptr,
                               a.prev_root_pos ? a.prev_root_pos + 3 * (int64_t)i : nullptr,
                               a.tar_a ? a.tar_a + wa * (int64_t)i : nullptr, a.tar_b ? a.tar_b + 2 * (int64_t)i : nullptr,
                               a.tar_speed ? a.tar_speed[i] : a.tar_speed_scalar, a.tar_states ? a.tar_states + 13 * (int64_t)i : nullptr,
                               a.body_pos ? a.body_pos + (int64_t)i * a.body_stride + a.body_off : nullptr, a.dt);
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
    if (int rc = body_mask("humanoid_reset", contact_body_ids, n_contact, n_bodies, &a.rule.contact_mask)) return rc;
    if (int rc = body_mask("humanoid_reset", strike_body_ids, n_strike, n_bodies, &a.rule.strike_mask)) return rc;
    a.progress = progress_buf; a.contact = contact_forces; a.pos = body_pos; a.rule.heights = termination_heights;
    a.tar_contact = tar_contact_forces; a.reset = reset; a.terminated = terminated;
    a.rule.max_len = max_episode_length; a.n = n_envs; a.rule.B = n_bodies;
    a.rule.early = enable_early_termination != 0; a.rule.strike = strike_body_ids != nullptr;
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
