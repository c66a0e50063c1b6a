// One environment step's tensor work as ONE launch per side of the physics step, on simulator-layout state:
//   ase_hip_env_pre_step    the pre_physics_step chain: action clamp and copy, PD targets or forces, the previous root position
//                           of the tasks that use it, the get-up task's recovery counter
//                           (env/tasks/base/vec_task.py:90-96, humanoid.py:361-366,479-481, humanoid_heading.py:81-85,
//                           humanoid_amp_getup.py:63-66,131-134 of the reference)
//   ase_hip_env_post_step   Humanoid.post_physics_step + HumanoidAMP.post_physics_step (humanoid.py:368-383,
//                           humanoid_amp.py:50-59, humanoid_amp_getup.py:136-142): progress, observation (humanoid + task
//                           columns, clipped as VecTaskPython.step does), reward, reset / terminate with the recovery mask,
//                           AMP history shift and the new frame
// Every per-body / per-dof state operand is a base pointer with an environment stride and an element stride (floats): windows of
// the simulator's packed [n, bodies_per_env, 13] rigid-body tensor and [n, D, 2] dof tensor are read in place.  The arithmetic
// is the device functions of env_funcs.h and amp_frames.h - the ones env_obs.hip and amp_obs.hip launch on contiguous tensors -
// so the outputs are bitwise those entries'.  Fixed grids, no atomics, no host decision: both entries record in a launch
// program.  Compiled without a * b + c contraction (Makefile NOFMA).
#include "amp_frames.h"
#include "env_funcs.h"

namespace {

constexpr int kStepEnvs = 16;          // environments per block: the staging tile is [kStepEnvs][max(F_obs, F_amp) + 1]
constexpr int kStepThreads = 256;
constexpr int kTaskPitch = 16;         // >= the widest task observation (15)

// element (environment e, item b) of a state operand sits at p + e * se + b * sb
struct View {
    const float* p;
    int64_t se, sb;
    __device__ __forceinline__ const float* at(int e, int b) const { return p + (int64_t)e * se + (int64_t)b * sb; }
};

struct EnvPostArgs {
    View pos, rot, vel, ang, contact, dof_pos, dof_vel;
    float *obs, *task_out;                   // row e at + e * ld_obs (column offsets applied); task_out NULL: no task columns
    int64_t ld_obs;
    float clip_obs;
    const float *root_states, *tar_states;   // actor e at + e * rs_stride / ts_stride
    int64_t rs_stride, ts_stride;
    const float *prev_root_pos, *tar_a, *tar_b, *tar_speed, *reach_pos;   // reach_pos: body reach_body of pos (or NULL)
    float tar_speed_scalar, dt;
    float* reward;
    int64_t* progress;
    const float* tar_contact;                // environment e at + e * tc_stride
    int64_t tc_stride;
    const int32_t* recovery;
    int64_t *reset, *terminated;
    ResetRule rule;
    float* hist;                             // [n, S, F_amp] or NULL
    int n, B, F_obs, F_amp, pitch, kind, local_root, root_height, S, D, K, J;
    int dof_off[kMaxJoints + 1], key_body[kMaxJoints];
};

__device__ __forceinline__ float clip_nan(float x, float c) { return ceil_nan(floor_nan(x, -c), c); }

__global__ __launch_bounds__(kStepThreads) void env_post_step_kernel(EnvPostArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int pitch = a.pitch, B = a.B;
    float* hq_s = tile + kStepEnvs * pitch;                  // [kStepEnvs][4]: inverse heading rotation of the root body
    float* tobs_s = hq_s + 4 * kStepEnvs;                    // [kStepEnvs][kTaskPitch]: the task observation
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, e0 = blockIdx.x * kStepEnvs;
    const int live = min(kStepEnvs, a.n - e0);
    const int wa = a.kind == ASE_TASK_REACH ? 3 : 2;
    // ---- the per-environment scalars, one job per wave, one lane per environment
    if (lane < live) {
        const int env = e0 + lane;
        const float* rs = a.root_states ? a.root_states + env * a.rs_stride : nullptr;
        const float* ta = a.tar_a ? a.tar_a + (int64_t)wa * env : nullptr;
        const float* tb = a.tar_b ? a.tar_b + 2 * (int64_t)env : nullptr;
        const float* ts = a.tar_states ? a.tar_states + env * a.ts_stride : nullptr;
        if (wave == 0) {
            const Q4 hq = heading_quat_inv(load_q(a.rot.at(env, 0)));
            hq_s[4 * lane] = hq.x; hq_s[4 * lane + 1] = hq.y; hq_s[4 * lane + 2] = hq.z; hq_s[4 * lane + 3] = hq.w;
        } else if (wave == 1) {
            // progress_buf += 1 comes first: the reset test sees the incremented value (humanoid.py:368-372)
            const int64_t progress = a.progress[env] + 1;
            a.progress[env] = progress;
            int64_t terminated;
            int64_t reset = humanoid_reset_row(a.rule, progress, a.contact.at(env, 0), a.contact.sb, a.pos.at(env, 0), a.pos.sb,
                                               a.rule.strike ? a.tar_contact + env * a.tc_stride : nullptr, terminated);
            if (a.recovery && a.recovery[env] > 0) { reset = 0; terminated = 0; }          // humanoid_amp_getup.py:136-142
            a.reset[env] = reset;
            a.terminated[env] = terminated;
        } else if (wave == 2) {
            float r = 1.0f;                                                                 // compute_humanoid_reward
            if (a.kind >= 0)
                r = task_reward_row(a.kind, rs, a.prev_root_pos ? a.prev_root_pos + 3 * (int64_t)env : nullptr, ta, tb,
                                    a.tar_speed ? a.tar_speed[env] : a.tar_speed_scalar, ts,
                                    a.reach_pos ? a.reach_pos + env * a.pos.se : nullptr, a.dt);
            a.reward[env] = r;
        } else if (a.task_out) {
            task_obs_row(a.kind, rs, ta, tb, a.tar_speed ? a.tar_speed[env] : 0.f, ts, tobs_s + kTaskPitch * lane);
        }
    }
    __syncthreads();
    // ---- the humanoid observation: one lane per (environment, body) into the tile
    for (int i = tid; i < live * B; i += kStepThreads) {
        const int e = i / B, b = i - e * B, env = e0 + e;
        humanoid_obs_body(b, B, a.local_root, a.root_height, load_q(hq_s + 4 * e), a.pos.at(env, 0), a.pos.at(env, b), a.rot.at(env, b),
                          a.vel.at(env, b), a.ang.at(env, b), tile + e * pitch);
    }
    __syncthreads();
    const float clip = a.clip_obs;
    for (int e = 0; e < live; ++e) {
        float* o = a.obs + (int64_t)(e0 + e) * a.ld_obs;
        for (int f = tid; f < a.F_obs; f += kStepThreads) o[f] = clip_nan(tile[e * pitch + f], clip);
    }
    if (a.task_out) {
        const int cols = kTaskCols[a.kind];
        for (int i = tid; i < live * cols; i += kStepThreads) {
            const int e = i / cols, c = i - e * cols;
            a.task_out[(int64_t)(e0 + e) * a.ld_obs + c] = clip_nan(tobs_s[kTaskPitch * e + c], clip);
        }
    }
    if (!a.hist) return;
    __syncthreads();                                         // the tile is free for the frame
    // ---- AMP history: every lane walks its own column from the oldest slot down, so a slot is read before it is overwritten;
    // slot 0 is read here and written only behind the next barrier
    const int F = a.F_amp;
    for (int i = tid; i < live * F; i += kStepThreads) {
        const int e = i / F, f = i - e * F;
        float* h = a.hist + (int64_t)(e0 + e) * a.S * F + f;
        for (int s = a.S - 2; s >= 0; --s) h[(int64_t)(s + 1) * F] = h[(int64_t)s * F];
    }
    // the new frame in its parts: root, one joint, one key body per lane; root and key bodies come from the rigid-body operands
    const FrameDims d{a.D, a.K, a.J, a.local_root, a.root_height};
    const int parts = 1 + a.J + a.K, od = 13 + 6 * a.J;
    for (int i = tid; i < live * parts; i += kStepThreads) {
        const int e = i / parts, part = i - e * parts, env = e0 + e;
        float* o = tile + e * pitch;
        if (part == 0) {
            frame_root(d, a.pos.at(env, 0), a.rot.at(env, 0), a.vel.at(env, 0), a.ang.at(env, 0), o);
        } else if (part <= a.J) {
            frame_joint(a.dof_off, part - 1, a.dof_pos.at(env, 0), a.dof_pos.sb, o);
        } else {
            const int k = part - 1 - a.J;
            frame_key(load_q(hq_s + 4 * e), a.pos.at(env, 0), a.pos.at(env, a.key_body[k]), o + od + a.D + 3 * k);
        }
    }
    for (int i = tid; i < live * a.D; i += kStepThreads) {
        const int e = i / a.D, j = i - e * a.D;
        tile[e * pitch + od + j] = *a.dof_vel.at(e0 + e, j);
    }
    __syncthreads();
    for (int e = 0; e < live; ++e) {
        float* h = a.hist + (int64_t)(e0 + e) * a.S * F;
        for (int f = tid; f < F; f += kStepThreads) h[f] = tile[e * pitch + f];
    }
}

struct EnvPreArgs {
    const float* in;
    float *actions, *targets;
    int64_t ld_in, ld_act, ld_t;
    const float *offset, *scale, *efforts, *root_states;
    int64_t rs_stride;
    float* prev_root_pos;
    int32_t* recovery;
    float clip, power_scale;
    int n, D, pd;
};

// one lane per (environment, dof); the lane of dof 0 also does the environment's own two jobs
__global__ __launch_bounds__(256) void env_pre_step_kernel(EnvPreArgs a) {
    const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (i >= (int64_t)a.n * a.D) return;
    const int e = (int)(i / a.D), j = (int)(i - (int64_t)e * a.D);
    const float x = clip_nan(a.in[e * a.ld_in + j], a.clip);
    a.actions[e * a.ld_act + j] = x;
    float t;
    if (a.pd) {
        const float p = a.scale[j] * x;                      // _action_to_pd_targets: the product, then the sum
        t = a.offset[j] + p;
    } else {
        const float f = x * a.efforts[j];                    // actions * motor_efforts * power_scale, left to right
        t = f * a.power_scale;
    }
    a.targets[e * a.ld_t + j] = t;
    if (j != 0) return;
    if (a.prev_root_pos) {
        const float* rs = a.root_states + e * a.rs_stride;
        float* p = a.prev_root_pos + 3 * (int64_t)e;
        p[0] = rs[0]; p[1] = rs[1]; p[2] = rs[2];
    }
    if (a.recovery) a.recovery[e] = max(a.recovery[e] - 1, 0);
}

// an operand's strides: the element stride covers the element, the environment stride the environment's items
inline bool view_ok(const View& v, int items, int elem) { return v.sb >= elem && v.se >= (int64_t)(items - 1) * v.sb + elem; }

}  // namespace

extern "C" int ase_hip_env_pre_step(const float* actions_in, int64_t ld_in, float clip_actions, float* actions, int64_t ld_actions,
                                    float* targets, int64_t ld_targets, int pd_control, const float* pd_offset,
                                    const float* pd_scale, const float* motor_efforts, float power_scale,
                                    const float* root_states, int64_t root_stride, float* prev_root_pos,
                                    int32_t* recovery_counter, int n_envs, int n_dof, void* stream) {
    ASE_CHECK_ARG(actions_in && actions && targets, "env_pre_step: null actions_in / actions / targets");
    ASE_CHECK_ARG(n_envs >= 1 && n_dof >= 1, "env_pre_step: bad sizes (envs %d, dofs %d)", n_envs, n_dof);
    ASE_CHECK_ARG(ld_in >= n_dof && ld_actions >= n_dof && ld_targets >= n_dof, "env_pre_step: a pitch below the %d dofs", n_dof);
    ASE_CHECK_ARG(clip_actions >= 0.f, "env_pre_step: clip_actions %g", (double)clip_actions);
    ASE_CHECK_ARG(pd_control ? (pd_offset && pd_scale) : motor_efforts != nullptr,
                  "env_pre_step: %s", pd_control ? "PD control needs pd_offset and pd_scale" : "torque control needs motor_efforts");
    ASE_CHECK_ARG(!prev_root_pos || (root_states && root_stride >= 3), "env_pre_step: prev_root_pos needs root_states at a stride >= 3");
    EnvPreArgs a = {};
    a.in = actions_in; a.actions = actions; a.targets = targets; a.ld_in = ld_in; a.ld_act = ld_actions; a.ld_t = ld_targets;
    a.offset = pd_offset; a.scale = pd_scale; a.efforts = motor_efforts; a.root_states = root_states; a.rs_stride = root_stride;
    a.prev_root_pos = prev_root_pos; a.recovery = recovery_counter; a.clip = clip_actions; a.power_scale = power_scale;
    a.n = n_envs; a.D = n_dof; a.pd = pd_control != 0;
    const int64_t blocks = ((int64_t)n_envs * n_dof + 255) / 256;
    ASE_LAUNCH(env_pre_step_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("env_pre_step");
    return ASE_OK;
}

extern "C" int ase_hip_env_post_step(
    const float* body_pos, int64_t pos_se, int64_t pos_sb, const float* body_rot, int64_t rot_se, int64_t rot_sb,
    const float* body_vel, int64_t vel_se, int64_t vel_sb, const float* body_ang_vel, int64_t ang_se, int64_t ang_sb,
    const float* contact_forces, int64_t cf_se, int64_t cf_sb, const float* dof_pos, int64_t dp_se, int64_t dp_sd,
    const float* dof_vel, int64_t dv_se, int64_t dv_sd, int n_envs, int n_bodies, int n_dof, int local_root_obs,
    int root_height_obs, float* obs, int64_t ld_obs, int col_offset, float clip_obs, int task_kind, int enable_task_obs,
    int task_col_offset, const float* root_states, int64_t root_stride, const float* prev_root_pos, const float* tar_a,
    const float* tar_b, const float* tar_speed, float tar_speed_scalar, const float* tar_states, int64_t tar_stride,
    int reach_body_id, float dt, float* reward, int64_t* progress_buf, const float* termination_heights,
    const int32_t* contact_body_ids, int n_contact, const float* tar_contact_forces, int64_t tar_contact_stride,
    const int32_t* strike_body_ids, int n_strike, float max_episode_length, int enable_early_termination,
    const int32_t* recovery_counter, int64_t* reset, int64_t* terminated, float* hist, int n_steps, const int32_t* dof_offsets,
    int n_joints, const int32_t* key_body_ids, int n_key, void* stream) {
    const char* me = "env_post_step";
    ASE_CHECK_ARG(body_pos && body_rot && body_vel && body_ang_vel && contact_forces && obs && reward && progress_buf &&
                      termination_heights && reset && terminated,
                  "env_post_step: null operand");
    ASE_CHECK_ARG(n_envs >= 1 && n_bodies >= 1 && n_bodies <= 64, "env_post_step: bad sizes (envs %d, bodies %d; 1-64 bodies)", n_envs,
                  n_bodies);
    EnvPostArgs a = {};
    a.pos = View{body_pos, pos_se, pos_sb}; a.rot = View{body_rot, rot_se, rot_sb}; a.vel = View{body_vel, vel_se, vel_sb};
    a.ang = View{body_ang_vel, ang_se, ang_sb}; a.contact = View{contact_forces, cf_se, cf_sb};
    a.dof_pos = View{dof_pos, dp_se, dp_sd}; a.dof_vel = View{dof_vel, dv_se, dv_sd};
    ASE_CHECK_ARG(view_ok(a.pos, n_bodies, 3) && view_ok(a.rot, n_bodies, 4) && view_ok(a.vel, n_bodies, 3) &&
                      view_ok(a.ang, n_bodies, 3) && view_ok(a.contact, n_bodies, 3),
                  "env_post_step: a body operand's element stride is smaller than the element, or its environment stride than %d bodies",
                  n_bodies);
    // ---- observation
    a.F_obs = 15 * n_bodies - 2;
    ASE_CHECK_ARG(col_offset >= 0 && ld_obs >= (int64_t)col_offset + a.F_obs,
                  "env_post_step: %d columns at offset %d do not fit a leading dimension of %lld", a.F_obs, col_offset, (long long)ld_obs);
    ASE_CHECK_ARG(clip_obs >= 0.f, "env_post_step: clip_obs %g", (double)clip_obs);
    a.obs = obs + col_offset; a.ld_obs = ld_obs; a.clip_obs = clip_obs;
    a.local_root = local_root_obs != 0; a.root_height = root_height_obs != 0;
    // ---- task
    a.kind = -1;
    if (task_kind >= 0) {
        const void* ops[7] = {root_states, prev_root_pos, tar_a, tar_b, tar_speed, tar_states, task_kind == ASE_TASK_REACH ? body_pos : nullptr};
        int needs[4];
        for (int k = 0; k < 4; ++k) needs[k] = kRewardNeeds[k] | (enable_task_obs ? kObsNeeds[k] : 0);
        if (int rc = check_task_operands(me, task_kind, needs, ops)) return rc;
        ASE_CHECK_ARG(task_kind == ASE_TASK_REACH || dt > 0.f, "env_post_step: dt %g must be positive", (double)dt);
        ASE_CHECK_ARG(!root_states || root_stride >= 13, "env_post_step: root_states stride %lld below 13", (long long)root_stride);
        ASE_CHECK_ARG(!tar_states || tar_stride >= 13, "env_post_step: tar_states stride %lld below 13", (long long)tar_stride);
        a.kind = task_kind;
        if (task_kind == ASE_TASK_REACH) {
            ASE_CHECK_ARG(reach_body_id >= 0 && reach_body_id < n_bodies, "env_post_step: reach body %d of %d bodies", reach_body_id, n_bodies);
            a.reach_pos = body_pos + reach_body_id * pos_sb;
        }
        if (enable_task_obs) {
            ASE_CHECK_ARG(task_col_offset >= 0 && ld_obs >= (int64_t)task_col_offset + kTaskCols[task_kind],
                          "env_post_step: %d task columns at offset %d do not fit a leading dimension of %lld", kTaskCols[task_kind],
                          task_col_offset, (long long)ld_obs);
            a.task_out = obs + task_col_offset;
        }
    } else {
        ASE_CHECK_ARG(!enable_task_obs, "env_post_step: enable_task_obs without a task");
    }
    a.root_states = root_states; a.rs_stride = root_stride; a.tar_states = tar_states; a.ts_stride = tar_stride;
    a.prev_root_pos = prev_root_pos; a.tar_a = tar_a; a.tar_b = tar_b; a.tar_speed = tar_speed;
    a.tar_speed_scalar = tar_speed_scalar; a.dt = dt; a.reward = reward;
    // ---- reset
    ASE_CHECK_ARG(n_contact >= 0 && (contact_body_ids || n_contact == 0), "env_post_step: %d contact bodies without ids", n_contact);
    ASE_CHECK_ARG((tar_contact_forces != nullptr) == (strike_body_ids != nullptr),
                  "env_post_step: the strike form needs tar_contact_forces AND strike_body_ids");
    ASE_CHECK_ARG(strike_body_ids ? n_strike >= 1 : n_strike == 0, "env_post_step: n_strike %d %s strike_body_ids", n_strike,
                  strike_body_ids ? "with" : "without");
    ASE_CHECK_ARG(!tar_contact_forces || tar_contact_stride >= 3, "env_post_step: tar_contact_forces stride %lld below 3",
                  (long long)tar_contact_stride);
    if (int rc = body_mask(me, contact_body_ids, n_contact, n_bodies, &a.rule.contact_mask)) return rc;
    if (int rc = body_mask(me, strike_body_ids, n_strike, n_bodies, &a.rule.strike_mask)) return rc;
    a.rule.heights = termination_heights; a.rule.max_len = max_episode_length; a.rule.B = n_bodies;
    a.rule.early = enable_early_termination != 0; a.rule.strike = strike_body_ids != nullptr;
    a.progress = progress_buf; a.tar_contact = tar_contact_forces; a.tc_stride = tar_contact_stride;
    a.recovery = recovery_counter; a.reset = reset; a.terminated = terminated;
    // ---- AMP history
    a.hist = hist;
    if (hist) {
        ASE_CHECK_ARG(dof_pos && dof_vel && dof_offsets && (key_body_ids || n_key == 0), "env_post_step: the AMP history needs dof_pos, "
                      "dof_vel, dof_offsets and key_body_ids");
        ASE_CHECK_ARG(n_dof >= 1 && n_steps >= 1 && n_joints >= 1 && n_joints <= kMaxJoints && n_key >= 0 && n_key <= kMaxJoints,
                      "env_post_step: bad sizes (dofs %d, steps %d, joints %d, key bodies %d)", n_dof, n_steps, n_joints, n_key);
        ASE_CHECK_ARG(view_ok(a.dof_pos, n_dof, 1) && view_ok(a.dof_vel, n_dof, 1),
                      "env_post_step: a dof operand's element stride is smaller than the element, or its environment stride than %d dofs", n_dof);
        a.F_amp = 13 + 6 * n_joints + n_dof + 3 * n_key;
        ASE_CHECK_ARG(a.F_amp <= 255, "env_post_step: AMP frame of %d floats does not fit the staging tile (F <= 255)", a.F_amp);
        for (int j = 0; j <= n_joints; ++j) {
            a.dof_off[j] = dof_offsets[j];
            if (j > 0) {
                const int sz = dof_offsets[j] - dof_offsets[j - 1];
                ASE_CHECK_ARG(sz == 1 || sz == 3, "env_post_step: joint %d has %d dofs (1 or 3 supported)", j - 1, sz);
            }
        }
        ASE_CHECK_ARG(dof_offsets[0] == 0 && dof_offsets[n_joints] == n_dof, "env_post_step: dof_offsets do not cover the dofs");
        for (int k = 0; k < n_key; ++k) {
            ASE_CHECK_ARG(key_body_ids[k] >= 0 && key_body_ids[k] < n_bodies, "env_post_step: key body %d out of range", key_body_ids[k]);
            a.key_body[k] = key_body_ids[k];
        }
        a.S = n_steps; a.D = n_dof; a.K = n_key; a.J = n_joints;
    }
    a.n = n_envs; a.B = n_bodies;
    a.pitch = (a.F_obs > a.F_amp ? a.F_obs : a.F_amp) + 1;
    const int lds = (kStepEnvs * a.pitch + (4 + kTaskPitch) * kStepEnvs) * (int)sizeof(float);      // <= 62.7 KB at 64 bodies
    ASE_LAUNCH(env_post_step_kernel, dim3((n_envs + kStepEnvs - 1) / kStepEnvs), dim3(kStepThreads), lds, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("env_post_step");
    return ASE_OK;
}
