// Target draws and resets of the four HRL tasks: _reset_task of the heading, location and reach tasks,
// HumanoidStrike._reset_target and the per-step _update_task, as ONE launch with one lane per environment (or per id) and no
// intermediate tensor.  The due test of _update_task runs inside the kernel, so there is no nonzero and no host round trip.
// Follows env/tasks/humanoid_heading.py:147-174, humanoid_location.py:107-125, humanoid_reach.py:111-130 and
// humanoid_strike.py:108-128 of the reference, operation by operation in f32 (the file compiles with -ffp-contract=off).
#include "philox.h"
#include "quat.h"

namespace {

// uniforms per row: the reference's torch.rand calls, in order
__device__ __forceinline__ int draws_of(int kind) { return kind == ASE_TASK_LOCATION ? 2 : kind == ASE_TASK_STRIKE ? 4 : 3; }
constexpr float kTwoPi = 6.2831855f, kPi = 3.1415927f;   // (float)(2 * np.pi), (float)np.pi: the scalars of the reference's f32 products

struct TaskResetArgs {
    const int32_t* ids;              // ids mode; NULL: due mode
    const float* u;                  // passed-in draws [n_ids, U]; NULL: device draws from rng
    const int64_t* steps;            // passed-in change steps [n_ids]
    const uint64_t* rng;
    const int64_t* progress;
    int64_t* change;
    const float* root;
    float *tar_a, *tar_b, *tar_speed, *target;
    int64_t ld_root, ld_target, steps_low;
    uint32_t steps_span;             // steps_high - steps_low
    float lo, span;                  // heading: speed range; reach: height range; strike: tar_dist_min, tar_dist_max
    float dist_max, near_dist, near_prob;
    int n_envs, n_rows, kind, rand_heading;
};

__global__ __launch_bounds__(64) void task_reset_kernel(TaskResetArgs a) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= a.n_rows) return;
    const int e = a.ids ? a.ids[r] : r;
    if (e < 0 || e >= a.n_envs) return;                  // an id outside the buffers is skipped, never dereferenced
    int64_t progress = 0;
    if (a.kind != ASE_TASK_STRIKE) {
        progress = a.progress[e];
        if (!a.ids && progress < a.change[e]) return;    // _update_task: progress_buf >= change_steps
    }
    const int U = draws_of(a.kind);
    float u[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t steps = 0;
    if (a.u) {
        for (int j = 0; j < U; ++j) u[j] = a.u[(int64_t)r * U + j];
        if (a.steps) steps = a.steps[r];
    } else {
        // the draws of environment e depend on (seed, offset, e) only: uniform j is element 4 e + j, the change steps come
        // from word 0 of element 4 e + 3 by multiply-shift (exact, never reaches steps_high)
        const uint64_t seed = a.rng[0], off = a.rng[1], e4 = 4 * (uint64_t)e;
        for (int j = 0; j < U; ++j) u[j] = philox_uniform(seed, off, e4 + j);
        if (a.kind != ASE_TASK_STRIKE)
            steps = a.steps_low + (int64_t)(((uint64_t)philox_word0(seed, off, e4 + 3) * (uint64_t)a.steps_span) >> 32);
    }
    switch (a.kind) {
    case ASE_TASK_HEADING: {       // humanoid_heading.py:154-174
        const float theta = a.rand_heading ? kTwoPi * u[0] - kPi : 0.f;
        const float face = a.rand_heading ? kTwoPi * u[1] - kPi : 0.f;
        a.tar_speed[e] = a.span * u[2] + a.lo;
        a.tar_a[2 * (int64_t)e] = cosf(theta); a.tar_a[2 * (int64_t)e + 1] = sinf(theta);
        a.tar_b[2 * (int64_t)e] = cosf(face); a.tar_b[2 * (int64_t)e + 1] = sinf(face);
    } break;
    case ASE_TASK_LOCATION: {      // humanoid_location.py:114-125
        const float* rs = a.root + (int64_t)e * a.ld_root;
        a.tar_a[2 * (int64_t)e] = rs[0] + a.dist_max * (2.0f * u[0] - 1.0f);
        a.tar_a[2 * (int64_t)e + 1] = rs[1] + a.dist_max * (2.0f * u[1] - 1.0f);
    } break;
    case ASE_TASK_REACH: {         // humanoid_reach.py:118-130
        float* t = a.tar_a + 3 * (int64_t)e;
        t[0] = a.dist_max * (2.0f * u[0] - 1.0f);
        t[1] = a.dist_max * (2.0f * u[1] - 1.0f);
        t[2] = a.span * u[2] + a.lo;
    } break;
    default: {                     // _reset_target, humanoid_strike.py:108-128
        const float* rs = a.root + (int64_t)e * a.ld_root;
        float* t = a.target + (int64_t)e * a.ld_target;
        const float dist_max = u[0] < a.near_prob ? a.near_dist : a.span;
        const float dist = (dist_max - a.lo) * u[1] + a.lo;
        const float theta = kTwoPi * u[2];
        const float x = dist * cosf(theta) + rs[0], y = dist * sinf(theta) + rs[1];
        const Q4 q = from_angle_axis(kTwoPi * u[3], V3{0.f, 0.f, 1.f});
        t[0] = x; t[1] = y; t[2] = 0.9f;
        t[3] = q.x; t[4] = q.y; t[5] = q.z; t[6] = q.w;
        for (int c = 7; c < 13; ++c) t[c] = 0.f;
    } break;
    }
    if (a.kind != ASE_TASK_STRIKE) a.change[e] = progress + steps;
}

// operands of the entry: which a kind uses (all others must be NULL)
enum { kProgress = 1, kChange = 2, kRoot = 4, kTarA = 8, kTarB = 16, kSpeed = 32, kTarget = 64 };
constexpr int kNeeds[4] = {kProgress | kChange | kTarA | kTarB | kSpeed, kProgress | kChange | kRoot | kTarA,
                           kProgress | kChange | kTarA, kRoot | kTarget};
const char* const kNames[7] = {"progress_buf", "change_steps", "root_states", "tar_a", "tar_b", "tar_speed", "target_states"};

}  // namespace

extern "C" int ase_hip_task_reset(int kind, const int32_t* env_ids, int n_ids, const float* u, const int64_t* steps,
                                  uint64_t* rng_state, int advance, const int64_t* progress_buf, int64_t* change_steps,
                                  int64_t steps_low, int64_t steps_high, const float* root_states, int64_t ld_root,
                                  float* tar_a, float* tar_b, float* tar_speed, float* target_states, int64_t ld_target,
                                  double tar_speed_min, double tar_speed_max, double tar_dist_min, double tar_dist_max,
                                  double tar_height_min, double tar_height_max, double near_dist, double near_prob,
                                  int enable_rand_heading, int n_envs, void* stream) {
    ASE_CHECK_ARG(kind >= 0 && kind < 4, "task_reset: unknown task kind %d", kind);
    const void* ops[7] = {progress_buf, change_steps, root_states, tar_a, tar_b, tar_speed, target_states};
    for (int k = 0; k < 7; ++k) {
        const bool need = (kNeeds[kind] >> k) & 1;
        ASE_CHECK_ARG(!need || ops[k], "task_reset: task kind %d needs %s", kind, kNames[k]);
        ASE_CHECK_ARG(need || !ops[k], "task_reset: task kind %d does not use %s (must be NULL)", kind, kNames[k]);
    }
    const bool strike = kind == ASE_TASK_STRIKE;
    ASE_CHECK_ARG(n_envs > 0, "task_reset: bad size (envs %d)", n_envs);
    ASE_CHECK_ARG(env_ids ? n_ids >= 0 : n_ids == 0, "task_reset: n_ids %d %s env_ids", n_ids, env_ids ? "with" : "without");
    ASE_CHECK_ARG(env_ids || !strike, "task_reset: the strike task has no change steps, so no due mode (env_ids NULL)");
    ASE_CHECK_ARG((u != nullptr) != (rng_state != nullptr), "task_reset: exactly one draw source, u or rng_state (%s given)",
                  u ? "both" : "none");
    ASE_CHECK_ARG(!u || env_ids, "task_reset: due mode (env_ids NULL) draws on the device, u must be NULL");
    ASE_CHECK_ARG(u && !strike ? steps != nullptr : steps == nullptr,
                  "task_reset: steps comes with u for the tasks that have change steps, and only then");
    ASE_CHECK_ARG(strike || (steps_high > steps_low && steps_high - steps_low <= (int64_t)0xFFFFFFFF),
                  "task_reset: change steps in [%lld, %lld): high must exceed low by 1 .. 2^32 - 1", (long long)steps_low,
                  (long long)steps_high);
    ASE_CHECK_ARG(!root_states || ld_root >= 13, "task_reset: root_states row stride %lld below 13", (long long)ld_root);
    ASE_CHECK_ARG(!target_states || ld_target >= 13, "task_reset: target_states row stride %lld below 13", (long long)ld_target);
    TaskResetArgs a = {};
    a.ids = env_ids; a.u = u; a.steps = steps; a.rng = rng_state; a.progress = progress_buf; a.change = change_steps;
    a.root = root_states; a.tar_a = tar_a; a.tar_b = tar_b; a.tar_speed = tar_speed; a.target = target_states;
    a.ld_root = ld_root; a.ld_target = ld_target;
    a.steps_low = steps_low; a.steps_span = strike ? 0u : (uint32_t)(steps_high - steps_low);
    // the ranges are Python floats in the reference: a difference of two of them is taken in f64 and rounded once
    if (kind == ASE_TASK_HEADING) { a.lo = (float)tar_speed_min; a.span = (float)(tar_speed_max - tar_speed_min); }
    if (kind == ASE_TASK_REACH) { a.lo = (float)tar_height_min; a.span = (float)(tar_height_max - tar_height_min); }
    if (strike) { a.lo = (float)tar_dist_min; a.span = (float)tar_dist_max; }      // (dist_max - tar_dist_min is a tensor operation)
    a.dist_max = (float)tar_dist_max; a.near_dist = (float)near_dist; a.near_prob = (float)near_prob;
    a.n_envs = n_envs; a.n_rows = env_ids ? n_ids : n_envs; a.kind = kind; a.rand_heading = enable_rand_heading != 0;
    const bool bump = rng_state && advance;          // a call is one position of the stream, an empty env_ids list included
    if (a.n_rows == 0 && !bump) return ASE_OK;
    if (a.n_rows > 0)
        ASE_LAUNCH(task_reset_kernel, dim3((a.n_rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
    if (bump) ASE_LAUNCH(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng_state);
    ASE_CHECK_LAUNCH("task_reset");
    return ASE_OK;
}
