// The per-row device functions of the environment side, shared by env_obs.hip (one launch per reference function on contiguous
// tensors) and env_step.hip (the whole post-physics tail in one launch on simulator-layout state): one body's columns of
// compute_humanoid_observations_max (env/tasks/humanoid.py:592-636), compute_humanoid_reset (humanoid.py:645-672; strike form
// humanoid_strike.py:255-297) and the four tasks' observations and rewards (humanoid_heading.py:231-289,
// humanoid_location.py:169-232, humanoid_reach.py:174-198, humanoid_strike.py:193-297).  Every function takes pointers to the
// row's own elements, so the caller owns the layout.  Both files compile with -ffp-contract=off.
#pragma once
#include "common.h"
#include "quat.h"

namespace {

__device__ __forceinline__ V3 load_v(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void store_v(float* o, const V3& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// ---- compute_humanoid_observations_max: the columns of body b in the row o[15 B - 2] --------------------------------------
// hq = heading_quat_inv(root rotation); root: the root's position; p, qp, v, w: body b's position, rotation and velocities
__device__ __forceinline__ void humanoid_obs_body(int b, int B, int local_root, int root_height, const Q4& hq, const float* root,
                                                  const float* p, const float* qp, const float* v, const float* w, float* o) {
    const int o_rot = 1 + 3 * (B - 1), o_vel = o_rot + 6 * B, o_ang = o_vel + 3 * B;
    const Q4 q = load_q(qp);
    if (b == 0) {
        o[0] = root_height ? root[2] : 0.f;
        // local_root_obs TRUE overwrites the root's columns with the tangent / normal of the RAW root rotation
        // (humanoid.py:620-622), false leaves the heading-local one
        tan_norm(local_root ? q : mul(hq, q), o + o_rot);
    } else {
        const V3 pp = load_v(p);
        store_v(o + 1 + 3 * (b - 1), rot(hq, V3{pp.x - root[0], pp.y - root[1], pp.z - root[2]}));
        tan_norm(mul(hq, q), o + o_rot + 6 * b);
    }
    store_v(o + o_vel + 3 * b, rot(hq, load_v(v)));
    store_v(o + o_ang + 3 * b, rot(hq, load_v(w)));
}

// ---- compute_humanoid_reset: one environment -> reset, terminated ---------------------------------------------------------
// c, p: the environment's contact forces and body positions, body b at [b * c_sb], [b * p_sb]; t: the strike target's contact
// force (strike form only)
struct ResetRule {
    const float* heights;                                    // [B]
    uint64_t contact_mask, strike_mask;                      // bit b: body b is a contact / strike body
    float max_len;
    int B, early, strike;
};
__device__ __forceinline__ int64_t humanoid_reset_row(const ResetRule& a, int64_t progress, const float* c, int64_t c_sb,
                                                      const float* p, int64_t p_sb, const float* t, int64_t& terminated) {
    terminated = 0;
    if (a.early) {
        bool fall_contact = false, fall_height = false, other_contact = false;
        for (int b = 0; b < a.B; ++b) {
            if ((a.contact_mask >> b) & 1) continue;                                   // masked_contact_buf[:, contact_body_ids] = 0
            const float* cb = c + b * c_sb;
            // fmaxf on purpose: the reference asks torch.any over the components, so a NaN beside a loud component does not hide it
            const float m = fmaxf(fmaxf(fabsf(cb[0]), fabsf(cb[1])), fabsf(cb[2]));
            fall_contact |= m > 0.1f;                                                  // humanoid.py:653
            fall_height |= p[b * p_sb + 2] < a.heights[b];
            if (!((a.strike_mask >> b) & 1)) other_contact |= m > 1.0f;                // contact_force_threshold, humanoid_strike.py:259
        }
        bool failed = fall_contact && fall_height;
        if (a.strike) {
            const bool tar_contact = fabsf(t[0]) > 1.0f || fabsf(t[1]) > 1.0f;         // tar_contact_forces[..., 0:2]
            failed |= tar_contact && other_contact;
        }
        terminated = (failed && progress > 1) ? 1 : 0;      // the first steps can still carry contact forces
    }
    return ((float)progress >= a.max_len - 1.f) ? 1 : terminated;
}

// ---- task observations: one environment's columns (5 / 2 / 3 / 15) --------------------------------------------------------
// rs: the root state [13]; ta, tb: the environment's rows of tar_a / tar_b; speed: its tar_speed (heading); ts: the target's
// state [13] (strike)
__device__ __forceinline__ void task_obs_row(int kind, const float* rs, const float* ta, const float* tb, float speed,
                                             const float* ts, float* o) {
    const Q4 hq = heading_quat_inv(load_q(rs + 3));
    switch (kind) {
    case ASE_TASK_HEADING: {       // compute_heading_observations, humanoid_heading.py:231-250
        const V3 ld = rot(hq, V3{ta[0], ta[1], 0.f}), lf = rot(hq, V3{tb[0], tb[1], 0.f});
        o[0] = ld.x; o[1] = ld.y; o[2] = speed; o[3] = lf.x; o[4] = lf.y;
    } break;
    case ASE_TASK_LOCATION: {      // compute_location_observations, humanoid_location.py:169-183
        const V3 l = rot(hq, V3{ta[0] - rs[0], ta[1] - rs[1], 0.f - rs[2]});
        o[0] = l.x; o[1] = l.y;
    } break;
    case ASE_TASK_REACH:           // compute_location_observations, humanoid_reach.py:174-182
        store_v(o, rot(hq, load_v(ta)));
        break;
    default: {                     // compute_strike_observations, humanoid_strike.py:193-219
        store_v(o, rot(hq, V3{ts[0] - rs[0], ts[1] - rs[1], ts[2]}));        // the target's height stays absolute
        tan_norm(mul(hq, load_q(ts + 3)), o + 3);
        store_v(o + 9, rot(hq, load_v(ts + 7)));
        store_v(o + 12, rot(hq, load_v(ts + 10)));
    } break;
    }
}

// ---- task rewards: every constant below is the reference's literal ----------------------------------------------------
// The reference clamps with torch.clamp_min, which keeps a NaN: every clamp here is floor_nan (fmaxf would turn the NaN of a
// simulator state that has blown up into 0 and hand the agent a plausible finite reward).  A NaN operand that reaches a
// reward's arithmetic gives NaN; the two overrides (location: pos_err < 0.5, strike: tar_rot_err < 0.2) replace what they
// replace in the reference, NaN included, and no comparison with a NaN is true.
// torch.nn.functional.normalize of a 2-vector (eps 1e-12).  Both components enter every sum they are used in, so a NaN norm
// gives a NaN result whether the bound keeps it (clamp_min) or not (fmaxf)
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

// rs, prev: the root state [13] and the previous root position [3] (unused by reach); ta, tb: the environment's rows of tar_a /
// tar_b; speed: its tar_speed (heading) or the task's scalar (location); ts: the target's state [13] (strike); p: the reach
// body's position [3]
__device__ __forceinline__ float task_reward_row(int kind, const float* rs, const float* prev, const float* ta, const float* tb,
                                                 float speed_tar, const float* ts, const float* p, float dt) {
    float reward, vx, vy;
    switch (kind) {
    case ASE_TASK_HEADING: {       // compute_heading_reward, humanoid_heading.py:252-289
        const float vel_err_scale = 0.25f, tangent_err_w = 0.1f, dir_reward_w = 0.7f, facing_reward_w = 0.3f;   // :255-259
        const float speed = dir_speed(rs, prev, dt, ta[0], ta[1], vx, vy);
        const float tangent = (vx - speed * ta[0]) + (vy - speed * ta[1]);
        const float err = speed_tar - speed;
        float dir_reward = expf(-vel_err_scale * (err * err + tangent_err_w * tangent * tangent));
        if (speed <= 0.f) dir_reward = 0.f;
        const V3 fd = facing_dir(rs);
        const float facing_reward = floor_nan(tb[0] * fd.x + tb[1] * fd.y, 0.f);
        reward = dir_reward_w * dir_reward + facing_reward_w * facing_reward;
    } break;
    case ASE_TASK_LOCATION: {      // compute_location_reward, humanoid_location.py:185-232
        const float dist_threshold = 0.5f, pos_err_scale = 0.5f, vel_err_scale = 4.0f;                          // :188-191
        const float pos_reward_w = 0.5f, vel_reward_w = 0.4f, face_reward_w = 0.1f;                             // :193-195
        float dx = ta[0] - rs[0], dy = ta[1] - rs[1];
        const float pos_err = dx * dx + dy * dy;
        const float pos_reward = expf(-pos_err_scale * pos_err);
        normalize2(dx, dy);
        const float speed = dir_speed(rs, prev, dt, dx, dy, vx, vy);
        const float err = floor_nan(speed_tar - speed, 0.f);
        float vel_reward = expf(-vel_err_scale * (err * err));
        if (speed <= 0.f) vel_reward = 0.f;
        const V3 fd = facing_dir(rs);
        float facing_reward = floor_nan(dx * fd.x + dy * fd.y, 0.f);
        if (pos_err < dist_threshold) { facing_reward = 1.f; vel_reward = 1.f; }
        reward = pos_reward_w * pos_reward + vel_reward_w * vel_reward + face_reward_w * facing_reward;
    } break;
    case ASE_TASK_REACH: {         // compute_reach_reward, humanoid_reach.py:184-196
        const float pos_err_scale = 4.0f;                                                                        // :187
        const float dx = ta[0] - p[0], dy = ta[1] - p[1], dz = ta[2] - p[2];
        reward = expf(-pos_err_scale * (dx * dx + dy * dy + dz * dz));
    } break;
    default: {                     // compute_strike_reward, humanoid_strike.py:221-252
        const float tar_speed = 1.0f, vel_err_scale = 4.0f, tar_rot_w = 0.6f, vel_reward_w = 0.4f;               // :224-228
        const float tar_rot_err = rot(load_q(ts + 3), V3{0.f, 0.f, 1.f}).z;       // <up, target's up>
        const float tar_rot_r = floor_nan(1.0f - tar_rot_err, 0.f);
        float dx = ts[0] - rs[0], dy = ts[1] - rs[1];
        normalize2(dx, dy);
        const float speed = dir_speed(rs, prev, dt, dx, dy, vx, vy);
        const float err = floor_nan(tar_speed - speed, 0.f);
        float vel_reward = expf(-vel_err_scale * (err * err));
        if (speed <= 0.f) vel_reward = 0.f;
        reward = tar_rot_w * tar_rot_r + vel_reward_w * vel_reward;
        if (tar_rot_err < 0.2f) reward = 1.f;                                      // :249
    } break;
    }
    return reward;
}

// operands of a task entry: which a kind needs (all others must be NULL)
enum { kRoot = 1, kPrev = 2, kTarA = 4, kTarB = 8, kSpeed = 16, kTarStates = 32, kBody = 64 };
constexpr int kObsNeeds[4] = {kRoot | kTarA | kTarB | kSpeed, kRoot | kTarA, kRoot | kTarA, kRoot | kTarStates};
constexpr int kRewardNeeds[4] = {kRoot | kPrev | kTarA | kTarB | kSpeed, kRoot | kPrev | kTarA, kTarA | kBody,
                                 kRoot | kPrev | kTarStates};
constexpr int kTaskCols[4] = {5, 2, 3, 15};
const char* const kOperandNames[7] = {"root_states", "prev_root_pos", "tar_a", "tar_b", "tar_speed", "tar_states", "body_pos"};

inline int check_task_operands(const char* entry, int kind, const int* needs, const void* const* ops) {
    ASE_CHECK_ARG(kind >= 0 && kind < 4, "%s: unknown task kind %d", entry, kind);
    for (int k = 0; k < 7; ++k) {
        const bool need = (needs[kind] >> k) & 1;
        ASE_CHECK_ARG(!need || ops[k], "%s: task kind %d needs %s", entry, kind, kOperandNames[k]);
        ASE_CHECK_ARG(need || !ops[k], "%s: task kind %d does not use %s (must be NULL)", entry, kind, kOperandNames[k]);
    }
    return ASE_OK;
}

inline int body_mask(const char* entry, const int32_t* ids, int n, int n_bodies, uint64_t* mask) {
    *mask = 0;
    for (int k = 0; k < n; ++k) {
        ASE_CHECK_ARG(ids[k] >= 0 && ids[k] < n_bodies, "%s: body id %d out of range (%d bodies)", entry, ids[k], n_bodies);
        *mask |= (uint64_t)1 << ids[k];
    }
    return ASE_OK;
}

}  // namespace
