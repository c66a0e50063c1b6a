// The view-motion task: HumanoidViewMotion's per-step logic as ONE launch with one lane per environment on a
// fixed grid, no host read and no intermediate tensor.  Mode SYNC is _compute_reset + _motion_sync (env/tasks/
// humanoid_view_motion.py:44-77,91-97 of the reference): the clip time from the step counter, the strict end-of-clip test, the
// sampled pose written in place into the simulator's root and dof tensors with zero velocities.  Mode RESET is
// _reset_env_tensors (lines 82-89) with the due test inside the kernel.  The sampler is amp_frames.h's - the functions
// motion_state_kernel runs - and the file compiles with -ffp-contract=off like amp_obs.hip, so the poses are its bits.
#include "amp_frames.h"

namespace {

struct MotionSyncArgs {
    MotionClips c;
    int32_t* motion_ids;
    int64_t *progress, *reset, *terminate;
    const int32_t* ids;              // RESET: the rows (-1: skip); NULL: every environment with reset != 0
    int32_t* ids_out;
    float *root, *dof_pos, *dof_vel, *body_pos, *body_rot, *body_vel, *body_ang_vel;
    int64_t ld_root, dp_se, dp_sd, dv_se, dv_sd, bp_se, bp_sb, br_se, br_sb, bv_se, bv_sb, ba_se, ba_sb;
    float motion_dt;
    int n_envs, n_ids, num_motions;
};

__global__ __launch_bounds__(64) void motion_sync_kernel(MotionSyncArgs a) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.n_envs) return;
    const int mid = a.motion_ids[e];
    if (mid < 0 || mid >= a.num_motions) return;         // an id outside the library: the row is left as it is
    // motion_times = progress_buf * motion_dt: the counter rounded to f32, times the f32 rounding of the step
    const float t = (float)a.progress[e] * a.motion_dt;
    a.reset[e] = t > a.c.lengths[mid] ? 1 : 0;
    a.terminate[e] = 0;
    const FrameBlend fb = motion_blend(a.c, mid, t);
    float* rs = a.root + (int64_t)e * a.ld_root;
    motion_body(a.c, fb, 0, rs);
    motion_body_rot(a.c, fb, 0, rs + 3);
#pragma unroll
    for (int c = 7; c < 13; ++c) rs[c] = 0.f;
    float* dp = a.dof_pos + (int64_t)e * a.dp_se;
    float* dv = a.dof_vel + (int64_t)e * a.dv_se;
    for (int j = 0; j < a.c.J; ++j) motion_joint(a.c, fb, j, dp, a.dp_sd);
    for (int d = 0; d < a.c.D; ++d) dv[d * a.dv_sd] = 0.f;
    for (int b = 0; b < a.c.B; ++b) {
        if (a.body_pos) motion_body(a.c, fb, b, a.body_pos + (int64_t)e * a.bp_se + b * a.bp_sb);
        if (a.body_rot) motion_body_rot(a.c, fb, b, a.body_rot + (int64_t)e * a.br_se + b * a.br_sb);
        if (a.body_vel) {
            float* v = a.body_vel + (int64_t)e * a.bv_se + b * a.bv_sb;
            v[0] = 0.f; v[1] = 0.f; v[2] = 0.f;
        }
        if (a.body_ang_vel) {
            float* w = a.body_ang_vel + (int64_t)e * a.ba_se + b * a.ba_sb;
            w[0] = 0.f; w[1] = 0.f; w[2] = 0.f;
        }
    }
}

__global__ __launch_bounds__(64) void motion_advance_kernel(MotionSyncArgs a) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_envs) return;
    int e = r;
    bool due;
    if (a.ids) {                                         // row r of the list; -1 and ids outside the buffers are skipped
        if (r >= a.n_ids) return;
        e = a.ids[r];
        due = e >= 0 && e < a.n_envs;
    } else {
        due = a.reset[e] != 0;
    }
    int mid = 0;
    if (due) {
        mid = a.motion_ids[e];
        due = mid >= 0 && mid < a.num_motions;           // an id outside the library: the row is left as it is
    }
    if (a.ids_out) a.ids_out[r] = due ? e : -1;          // (not with a list: r is the environment)
    if (!due) return;
    a.motion_ids[e] = (int32_t)(((int64_t)mid + a.n_envs) % a.num_motions);
    a.progress[e] = 0;
    a.reset[e] = 0;
    a.terminate[e] = 0;
}

}  // namespace

extern "C" int ase_hip_motion_sync(int mode, const float* gts, const float* grs, const float* lrs, int n_bodies,
                                   const float* lengths, const int32_t* num_frames, const float* dt,
                                   const int32_t* length_starts, int num_motions, const int32_t* dof_body_ids,
                                   const int32_t* dof_offsets, int n_joints, int32_t* motion_ids, int64_t* progress_buf,
                                   double motion_dt, int64_t* reset_buf, int64_t* terminate_buf, float* root_states,
                                   int64_t ld_root, float* dof_pos, int64_t dp_se, int64_t dp_sd, float* dof_vel,
                                   int64_t dv_se, int64_t dv_sd, float* body_pos, int64_t bp_se, int64_t bp_sb,
                                   float* body_rot, int64_t br_se, int64_t br_sb, float* body_vel, int64_t bv_se,
                                   int64_t bv_sb, float* body_ang_vel, int64_t ba_se, int64_t ba_sb, const int32_t* env_ids,
                                   int n_ids, int32_t* ids_out, int n_envs, void* stream) {
    ASE_CHECK_ARG(mode == ASE_MOTION_SYNC || mode == ASE_MOTION_RESET, "motion_sync: mode %d (ASE_MOTION_SYNC or ASE_MOTION_RESET)", mode);
    ASE_CHECK_ARG(n_envs > 0, "motion_sync: bad size (envs %d)", n_envs);
    ASE_CHECK_ARG(num_motions >= 1, "motion_sync: num_motions %d below 1", num_motions);
    ASE_CHECK_ARG(motion_ids && progress_buf && reset_buf && terminate_buf,
                  "motion_sync: needs motion_ids, progress_buf, reset_buf and terminate_buf");
    MotionSyncArgs a = {};
    a.motion_ids = motion_ids; a.progress = progress_buf; a.reset = reset_buf; a.terminate = terminate_buf;
    a.n_envs = n_envs; a.num_motions = num_motions;
    const dim3 grid((n_envs + 63) / 64), block(64);
    if (mode == ASE_MOTION_RESET) {
        ASE_CHECK_ARG(env_ids ? n_ids >= 0 && n_ids <= n_envs : n_ids == 0, "motion_sync: n_ids %d %s env_ids (0 .. n_envs = %d)", n_ids,
                      env_ids ? "with" : "without", n_envs);
        ASE_CHECK_ARG(!env_ids || !ids_out, "motion_sync: ids_out is the export of the due test (env_ids NULL)");
        ASE_CHECK_ARG(!root_states && !dof_pos && !dof_vel && !body_pos && !body_rot && !body_vel && !body_ang_vel,
                      "motion_sync: ASE_MOTION_RESET writes no state (every state operand NULL)");
        a.ids = env_ids; a.n_ids = n_ids; a.ids_out = ids_out;
        if (env_ids && n_ids == 0) return ASE_OK;
        ASE_LAUNCH(motion_advance_kernel, grid, block, 0, (hipStream_t)stream, a);
        ASE_CHECK_LAUNCH("motion_sync");
        return ASE_OK;
    }
    ASE_CHECK_ARG(!env_ids && n_ids == 0 && !ids_out, "motion_sync: ASE_MOTION_SYNC runs on every environment (env_ids, ids_out NULL)");
    ASE_CHECK_ARG(gts && grs && lrs && lengths && num_frames && dt && length_starts && dof_body_ids && dof_offsets,
                  "motion_sync: null clip operand");
    ASE_CHECK_ARG(root_states && dof_pos && dof_vel, "motion_sync: needs root_states, dof_pos and dof_vel");
    ASE_CHECK_ARG(n_bodies >= 1 && n_bodies <= ASE_MOTION_SYNC_MAX_BODIES && n_joints >= 1 && n_joints <= kMaxJoints,
                  "motion_sync: bad sizes (bodies %d of at most %d, joints %d of at most %d)", n_bodies, ASE_MOTION_SYNC_MAX_BODIES,
                  n_joints, kMaxJoints);
    ASE_CHECK_ARG(dof_offsets[0] == 0, "motion_sync: dof_offsets do not cover the dofs (first offset %d)", dof_offsets[0]);
    MotionClips& c = a.c;
    c.gts = gts; c.grs = grs; c.lrs = lrs; c.lengths = lengths; c.dt = dt; c.num_frames = num_frames; c.length_starts = length_starts;
    c.B = n_bodies; c.J = n_joints; c.K = 0; c.D = dof_offsets[n_joints];
    for (int j = 0; j <= n_joints; ++j) c.dof_off[j] = dof_offsets[j];
    for (int j = 0; j < n_joints; ++j) {
        const int sz = dof_offsets[j + 1] - dof_offsets[j];
        ASE_CHECK_ARG((sz == 1 || sz == 3) && dof_body_ids[j] >= 0 && dof_body_ids[j] < n_bodies,
                      "motion_sync: joint %d: %d dofs on body %d", j, sz, dof_body_ids[j]);
        c.dof_body[j] = dof_body_ids[j];
    }
    const int64_t D = c.D, B = n_bodies;
    ASE_CHECK_ARG(ld_root >= 13, "motion_sync: root_states row stride %lld below 13", (long long)ld_root);
    ASE_CHECK_ARG(dp_sd >= 1 && dv_sd >= 1 && dp_se >= (D - 1) * dp_sd + 1 && dv_se >= (D - 1) * dv_sd + 1,
                  "motion_sync: dof_pos / dof_vel strides (%lld, %lld per environment, %lld, %lld per element) do not cover %lld dofs",
                  (long long)dp_se, (long long)dv_se, (long long)dp_sd, (long long)dv_sd, (long long)D);
    ASE_CHECK_ARG((!body_pos || (bp_sb >= 3 && bp_se >= (B - 1) * bp_sb + 3)) && (!body_rot || (br_sb >= 4 && br_se >= (B - 1) * br_sb + 4)) &&
                      (!body_vel || (bv_sb >= 3 && bv_se >= (B - 1) * bv_sb + 3)) &&
                      (!body_ang_vel || (ba_sb >= 3 && ba_se >= (B - 1) * ba_sb + 3)),
                  "motion_sync: body strides do not cover %lld bodies (pos %lld / %lld, rot %lld / %lld, vel %lld / %lld, ang_vel %lld / %lld)",
                  (long long)B, (long long)bp_se, (long long)bp_sb, (long long)br_se, (long long)br_sb, (long long)bv_se,
                  (long long)bv_sb, (long long)ba_se, (long long)ba_sb);
    a.root = root_states; a.dof_pos = dof_pos; a.dof_vel = dof_vel; a.body_pos = body_pos; a.body_rot = body_rot;
    a.body_vel = body_vel; a.body_ang_vel = body_ang_vel;
    a.ld_root = ld_root; a.dp_se = dp_se; a.dp_sd = dp_sd; a.dv_se = dv_se; a.dv_sd = dv_sd;
    a.bp_se = bp_se; a.bp_sb = bp_sb; a.br_se = br_se; a.br_sb = br_sb; a.bv_se = bv_se; a.bv_sb = bv_sb; a.ba_se = ba_se; a.ba_sb = ba_sb;
    a.motion_dt = (float)motion_dt;                  // the Python float of the product enters it as its f32 rounding
    ASE_LAUNCH(motion_sync_kernel, grid, block, 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("motion_sync");
    return ASE_OK;
}
