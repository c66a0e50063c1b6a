// The projectile launches of the perturbation task: HumanoidPerturb._update_proj as ONE launch with one lane per
// environment (or per id) and no intermediate tensor.  The schedule test runs inside the kernel on progress_buf[0] - the
// reference's semantics: environment 0's counter decides for all - so there is no host read, no nonzero and no where.
// Follows env/tasks/humanoid_perturb.py:172-213 of the reference, operation by operation in f32 (the file compiles with
// -ffp-contract=off).
#include "philox.h"

namespace {

constexpr float kTwoPi = 6.2831855f;   // (float)(2 * np.pi): the scalar of the reference's in-place f32 product

struct ProjLaunchArgs {
    const int64_t* progress;         // due mode: progress_buf, of which element 0 is read; NULL: explicit slot
    const int32_t* timesteps;        // due mode: cumulative step counts [n_slots]
    const int32_t* ids;              // explicit mode: the rows; NULL: every environment
    const float *u, *eps;            // passed-in draws [rows, 4] / [rows, 3]; NULL: device draws from rng
    const uint64_t* rng;
    const float *root, *body_pos, *body_vel;      // body_pos / body_vel: the target body's row of environment 0
    float* proj;
    int32_t *slot_out, *ids_out;
    float* draws_out;
    int64_t ld_root, pos_se, vel_se, ld_env, ld_slot;
    float dist_lo, dist_span, h_lo, h_span, speed_lo, speed_span, noise;
    int n_envs, n_rows, n_slots, slot;
};

__global__ __launch_bounds__(64) void proj_launch_kernel(ProjLaunchArgs a) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    int slot = a.slot;
    if (a.progress) {                // _update_proj: curr_timestep % (perturb_timesteps[-1] + 1), the first equal entry
        slot = -1;
        const int64_t period = (int64_t)a.timesteps[a.n_slots - 1] + 1;
        const int64_t p0 = a.progress[0];
        if (period > 0) {
            const int64_t t = ((p0 % period) + period) % period;     // numpy's %: the sign of the divisor
            for (int k = a.n_slots - 1; k >= 0; --k)
                if ((int64_t)a.timesteps[k] == t) slot = k;
        }
    }
    if (r == 0 && a.slot_out) a.slot_out[0] = slot;
    if (r >= a.n_rows) return;
    const int e = a.ids ? a.ids[r] : r;
    if (e < 0 || e >= a.n_envs) return;                  // an id outside the buffers is skipped, never dereferenced
    if (a.ids_out) a.ids_out[e] = slot >= 0 ? e : -1;
    if (slot < 0) return;
    float d[7];                                          // theta, distance, height, noise x 3, speed
    if (a.u) {
        const float* ur = a.u + 4 * (int64_t)r;
        const float* er = a.eps + 3 * (int64_t)r;
        d[0] = ur[0]; d[1] = ur[1]; d[2] = ur[2]; d[3] = er[0]; d[4] = er[1]; d[5] = er[2]; d[6] = ur[3];
    } else {
        // the draws of environment e depend on (seed, offset, e) only: draw j is element 8 e + j
        const uint64_t seed = a.rng[0], off = a.rng[1], e8 = 8 * (uint64_t)e;
        for (int j = 0; j < 3; ++j) d[j] = philox_uniform(seed, off, e8 + j);
        for (int j = 3; j < 6; ++j) d[j] = philox_normal(seed, off, e8 + j);
        d[6] = philox_uniform(seed, off, e8 + 6);
    }
    if (a.draws_out)
        for (int j = 0; j < 7; ++j) a.draws_out[7 * (int64_t)e + j] = d[j];
    const float* rs = a.root + (int64_t)e * a.ld_root;
    const float* bp = a.body_pos + (int64_t)e * a.pos_se;
    const float* bv = a.body_vel + (int64_t)e * a.vel_se;
    float* t = a.proj + (int64_t)e * a.ld_env + (int64_t)slot * a.ld_slot;
    const float theta = d[0] * kTwoPi;
    const float dist = a.dist_span * d[1] + a.dist_lo;
    const float px = rs[0] + dist * cosf(theta);
    const float py = rs[1] + (-dist) * sinf(theta);
    const float pz = a.h_span * d[2] + a.h_lo;
    // launch_dir = target - position, += 0.1 * randn, F.normalize (max(norm, 1e-12) that keeps a NaN)
    const float dx = (bp[0] - px) + a.noise * d[3];
    const float dy = (bp[1] - py) + a.noise * d[4];
    const float dz = (bp[2] - pz) + a.noise * d[5];
    const float nrm = floor_nan(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
    const float speed = a.speed_span * d[6] + a.speed_lo;
    t[0] = px; t[1] = py; t[2] = pz;
    t[3] = 0.f; t[4] = 0.f; t[5] = 0.f; t[6] = 1.f;
    t[7] = speed * (dx / nrm) + bv[0];
    t[8] = speed * (dy / nrm) + bv[1];
    t[9] = speed * (dz / nrm);
    t[10] = 0.f; t[11] = 0.f; t[12] = 0.f;
}

}  // namespace

extern "C" int ase_hip_proj_launch(const int64_t* progress_buf, const int32_t* timesteps, int n_slots, int slot,
                                   const int32_t* env_ids, int n_ids, const float* u, const float* eps, uint64_t* rng_state,
                                   int advance, const float* root_states, int64_t ld_root, const float* body_pos, int64_t pos_se,
                                   int64_t pos_sb, const float* body_vel, int64_t vel_se, int64_t vel_sb, int n_bodies,
                                   int tar_body, float* proj_states, int64_t ld_env, int64_t ld_slot, double dist_min,
                                   double dist_max, double h_min, double h_max, double speed_min, double speed_max, double noise,
                                   int32_t* slot_out, int32_t* ids_out, float* draws_out, int n_envs, void* stream) {
    ASE_CHECK_ARG(n_envs > 0, "proj_launch: bad size (envs %d)", n_envs);
    ASE_CHECK_ARG(n_slots >= 1 && n_slots <= 32, "proj_launch: n_slots %d outside 1 .. 32", n_slots);
    ASE_CHECK_ARG(root_states && body_pos && body_vel && proj_states,
                  "proj_launch: needs root_states, body_pos, body_vel and proj_states");
    const bool due = slot < 0;
    ASE_CHECK_ARG(slot >= -1 && slot < n_slots, "proj_launch: slot %d outside -1 (due mode) .. %d", slot, n_slots - 1);
    ASE_CHECK_ARG(due ? (progress_buf && timesteps) : (!progress_buf && !timesteps),
                  "proj_launch: progress_buf and timesteps come with due mode (slot -1), and only then");
    ASE_CHECK_ARG(env_ids ? n_ids >= 0 : n_ids == 0, "proj_launch: n_ids %d %s env_ids", n_ids, env_ids ? "with" : "without");
    ASE_CHECK_ARG(!env_ids || !due, "proj_launch: due mode launches for every environment (env_ids NULL)");
    ASE_CHECK_ARG(!env_ids || !ids_out, "proj_launch: ids_out is the export of the modes without env_ids");
    ASE_CHECK_ARG((u != nullptr) != (rng_state != nullptr), "proj_launch: exactly one draw source, u or rng_state (%s given)",
                  u ? "both" : "none");
    ASE_CHECK_ARG((u != nullptr) == (eps != nullptr), "proj_launch: eps comes with u, and only then");
    ASE_CHECK_ARG(ld_root >= 13, "proj_launch: root_states row stride %lld below 13", (long long)ld_root);
    ASE_CHECK_ARG(ld_env >= 13 && ld_slot >= 13, "proj_launch: proj_states strides (%lld per environment, %lld per slot) below 13",
                  (long long)ld_env, (long long)ld_slot);
    ASE_CHECK_ARG(n_bodies >= 1 && tar_body >= 0 && tar_body < n_bodies, "proj_launch: tar_body %d outside the %d bodies", tar_body,
                  n_bodies);
    ASE_CHECK_ARG(pos_se >= 3 && vel_se >= 3 && pos_sb >= 3 && vel_sb >= 3,
                  "proj_launch: body_pos / body_vel strides (%lld, %lld per environment, %lld, %lld per body) below 3",
                  (long long)pos_se, (long long)vel_se, (long long)pos_sb, (long long)vel_sb);
    ProjLaunchArgs a = {};
    a.progress = progress_buf; a.timesteps = timesteps; a.ids = env_ids; a.u = u; a.eps = eps; a.rng = rng_state;
    a.root = root_states; a.body_pos = body_pos + (int64_t)tar_body * pos_sb; a.body_vel = body_vel + (int64_t)tar_body * vel_sb;
    a.proj = proj_states; a.slot_out = slot_out; a.ids_out = ids_out; a.draws_out = draws_out;
    a.ld_root = ld_root; a.pos_se = pos_se; a.vel_se = vel_se; a.ld_env = ld_env; a.ld_slot = ld_slot;
    // the ranges are Python numbers in the reference: a difference of two of them is taken in f64 and rounded once
    a.dist_lo = (float)dist_min; a.dist_span = (float)(dist_max - dist_min);
    a.h_lo = (float)h_min; a.h_span = (float)(h_max - h_min);
    a.speed_lo = (float)speed_min; a.speed_span = (float)(speed_max - speed_min);
    a.noise = (float)noise;
    a.n_envs = n_envs; a.n_rows = env_ids ? n_ids : n_envs; a.n_slots = n_slots; a.slot = slot;
    const bool bump = rng_state && advance;          // a call is one position of the stream, whether or not a launch was due
    if (a.n_rows == 0 && !bump && !slot_out) return ASE_OK;
    if (a.n_rows > 0 || slot_out)
        ASE_LAUNCH(proj_launch_kernel, dim3(a.n_rows > 0 ? (a.n_rows + 63) / 64 : 1), dim3(64), 0, (hipStream_t)stream, a);
    if (bump) ASE_LAUNCH(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng_state);
    ASE_CHECK_LAUNCH("proj_launch");
    return ASE_OK;
}
