// AMP observation production: one frame of the 140-float (per character: 1 + 6 + 3 + 3 + 6 J + D + 3 K)
// discriminator observation from the simulator state, pushed into the per-env history [N, S, F] whose flattened rows
// are the amp_obs the update path consumes.  HBM-light quaternion arithmetic: one lane per environment, the frame is
// staged through LDS so that both the history shift and the new slot are row-contiguous accesses.
// Follows env/tasks/humanoid_amp.py:248-266,280-316 and env/tasks/humanoid.py:523-552 (reference, /root/reference/ase).
#include "amp_frames.h"

namespace {

constexpr int kEnvPerBlock = 64;

struct AmpObsArgs {
    const float *root_pos, *root_rot, *root_vel, *root_ang_vel, *dof_pos, *dof_vel, *key_pos;
    float* hist;            // [N, S, F]
    int N, D, K, J, S, F;
    int local_root, root_height, shift;
    int dof_off[kMaxJoints + 1];
};

__global__ __launch_bounds__(kEnvPerBlock) void amp_obs_kernel(AmpObsArgs a) {
    extern __shared__ float tile[];                       // [kEnvPerBlock][F + 1]
    const int F = a.F, pitch = F + 1;
    const int e0 = blockIdx.x * kEnvPerBlock, n = e0 + threadIdx.x;
    const int live = min(kEnvPerBlock, a.N - e0);
    if (n < a.N) {
        const float* kp = a.key_pos + (int64_t)a.K * 3 * n;
        const FrameDims d{a.D, a.K, a.J, a.local_root, a.root_height};
        amp_frame(d, a.dof_off, a.root_pos + 3 * (int64_t)n, a.root_rot + 4 * (int64_t)n, a.root_vel + 3 * (int64_t)n,
                  a.root_ang_vel + 3 * (int64_t)n, a.dof_pos + (int64_t)a.D * n, a.dof_vel + (int64_t)a.D * n, 1,
                  [kp](int k) { return kp + 3 * k; }, tile + threadIdx.x * pitch);
    }
    __syncthreads();
    // the new frame takes slot 0 (the shift kernel has already moved the past): threads walk feature columns of the
    // block's environments, so the stores are row-contiguous
    for (int e = 0; e < live; ++e) {
        float* h = a.hist + (int64_t)(e0 + e) * a.S * F;
        for (int f = threadIdx.x; f < F; f += kEnvPerBlock) h[f] = tile[e * pitch + f];
    }
}

// history slots move one step into the past (oldest dropped): one thread per (env, feature) walks its column from the
// oldest slot down, lanes cover consecutive features -> every access is a contiguous row segment
__global__ __launch_bounds__(256) void amp_hist_shift_kernel(float* __restrict__ hist, int64_t n_cols, int S, int F) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_cols) return;
    const int64_t e = i / F;
    const int f = (int)(i - e * F);
    float* h = hist + e * S * F + f;
    for (int s = S - 2; s >= 0; --s) h[(int64_t)(s + 1) * F] = h[(int64_t)s * F];
}

// ---- motion clip sampler (utils/motion_lib.py:122-172,263-272,296-325; utils/torch_utils.py:7-28,94-118) -------------
struct MotionArgs {
    MotionClips c;
    const int32_t* motion_ids;
    const float* times;
    float *root_pos, *root_rot, *dof_pos, *root_vel, *root_ang_vel, *dof_vel, *key_pos;
    int n;
};

__global__ __launch_bounds__(64) void motion_state_kernel(MotionArgs a) {
    const int64_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    motion_state_at(a.c, a.motion_ids[i], a.times[i], a.root_pos + 3 * i, a.root_rot + 4 * i, a.dof_pos + a.c.D * i,
                    a.root_vel + 3 * i, a.root_ang_vel + 3 * i, a.dof_vel + a.c.D * i, 1, a.key_pos + i * a.c.K * 3);
}

}  // namespace

extern "C" int ase_hip_build_amp_obs(const float* root_pos, const float* root_rot, const float* root_vel,
                                     const float* root_ang_vel, const float* dof_pos, const float* dof_vel,
                                     const float* key_body_pos, int n_envs, int n_dof, int n_key,
                                     const int32_t* dof_offsets, int n_joints, int local_root_obs, int root_height_obs,
                                     float* hist, int n_steps, int shift, void* stream) {
    ASE_CHECK_ARG(root_pos && root_rot && root_vel && root_ang_vel && dof_pos && dof_vel && (key_body_pos || n_key == 0) && hist &&
                      dof_offsets,
                  "build_amp_obs: null operand");
    ASE_CHECK_ARG(n_envs > 0 && n_dof > 0 && n_key >= 0 && n_steps >= 1 && n_joints >= 1 && n_joints <= kMaxJoints,
                  "build_amp_obs: bad sizes (envs %d, dofs %d, joints %d)", n_envs, n_dof, n_joints);
    AmpObsArgs a;
    a.F = 13 + 6 * n_joints + n_dof + 3 * n_key;
    ASE_CHECK_ARG(kEnvPerBlock * (a.F + 1) * (int)sizeof(float) <= 64 * 1024,
                  "build_amp_obs: frame of %d floats does not fit the staging tile", a.F);
    a.root_pos = root_pos; a.root_rot = root_rot; a.root_vel = root_vel; a.root_ang_vel = root_ang_vel;
    a.dof_pos = dof_pos; a.dof_vel = dof_vel; a.key_pos = key_body_pos; a.hist = hist;
    a.N = n_envs; a.D = n_dof; a.K = n_key; a.J = n_joints; a.S = n_steps;
    a.local_root = local_root_obs; a.root_height = root_height_obs; a.shift = shift;
    for (int j = 0; j <= n_joints; ++j) {
        a.dof_off[j] = dof_offsets[j];
        if (j > 0) {
            const int sz = dof_offsets[j] - dof_offsets[j - 1];
            ASE_CHECK_ARG(sz == 1 || sz == 3, "build_amp_obs: joint %d has %d dofs (1 or 3 supported)", j - 1, sz);
        }
    }
    ASE_CHECK_ARG(dof_offsets[0] == 0 && dof_offsets[n_joints] == n_dof, "build_amp_obs: dof_offsets do not cover the dofs");
    const int lds = kEnvPerBlock * (a.F + 1) * (int)sizeof(float);
    if (shift && n_steps > 1) {
        const int64_t cols = (int64_t)n_envs * a.F;
        ASE_LAUNCH(amp_hist_shift_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, (hipStream_t)stream, hist,
                           cols, n_steps, a.F);
    }
    ASE_LAUNCH(amp_obs_kernel, dim3((n_envs + kEnvPerBlock - 1) / kEnvPerBlock), dim3(kEnvPerBlock), lds,
                       (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("build_amp_obs");
    return ASE_OK;
}

extern "C" int ase_hip_motion_state(const float* gts, const float* grs, const float* lrs, const float* grvs,
                                    const float* gravs, const float* dvs, int n_bodies, const float* lengths,
                                    const int32_t* num_frames, const float* dt, const int32_t* length_starts,
                                    const int32_t* motion_ids, const float* times, int n, const int32_t* dof_body_ids,
                                    const int32_t* dof_offsets, int n_joints, const int32_t* key_body_ids, int n_key,
                                    float* root_pos, float* root_rot, float* dof_pos, float* root_vel,
                                    float* root_ang_vel, float* dof_vel, float* key_pos, void* stream) {
    ASE_CHECK_ARG(gts && grs && lrs && grvs && gravs && dvs && lengths && num_frames && dt && length_starts && motion_ids &&
                      times && dof_body_ids && dof_offsets && root_pos && root_rot && dof_pos && root_vel && root_ang_vel &&
                      dof_vel && (key_pos || n_key == 0) && (key_body_ids || n_key == 0),
                  "motion_state: null operand");
    ASE_CHECK_ARG(n > 0 && n_bodies > 0 && n_joints >= 1 && n_joints <= kMaxJoints && n_key >= 0 && n_key <= kMaxJoints,
                  "motion_state: bad sizes (n %d, bodies %d, joints %d, key bodies %d)", n, n_bodies, n_joints, n_key);
    ASE_CHECK_ARG(dof_offsets[0] == 0, "motion_state: dof_offsets do not cover the dofs (first offset %d)", dof_offsets[0]);
    MotionArgs a;
    MotionClips& c = a.c;
    c.gts = gts; c.grs = grs; c.lrs = lrs; c.grvs = grvs; c.gravs = gravs; c.dvs = dvs;
    c.lengths = lengths; c.dt = dt; c.num_frames = num_frames; c.length_starts = length_starts;
    a.motion_ids = motion_ids; a.times = times;
    a.root_pos = root_pos; a.root_rot = root_rot; a.dof_pos = dof_pos; a.root_vel = root_vel;
    a.root_ang_vel = root_ang_vel; a.dof_vel = dof_vel; a.key_pos = key_pos;
    a.n = n; c.B = n_bodies; c.J = n_joints; c.K = n_key; c.D = dof_offsets[n_joints];
    for (int j = 0; j <= n_joints; ++j) c.dof_off[j] = dof_offsets[j];
    for (int j = 0; j < n_joints; ++j) {
        const int sz = dof_offsets[j + 1] - dof_offsets[j];
        ASE_CHECK_ARG((sz == 1 || sz == 3) && dof_body_ids[j] >= 0 && dof_body_ids[j] < n_bodies,
                      "motion_state: joint %d: %d dofs on body %d", j, sz, dof_body_ids[j]);
        c.dof_body[j] = dof_body_ids[j];
    }
    for (int k = 0; k < n_key; ++k) {
        ASE_CHECK_ARG(key_body_ids[k] >= 0 && key_body_ids[k] < n_bodies, "motion_state: key body %d out of range", key_body_ids[k]);
        c.key_body[k] = key_body_ids[k];
    }
    ASE_LAUNCH(motion_state_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("motion_state");
    return ASE_OK;
}
