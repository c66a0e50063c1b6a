// Renewals of the ASE agent's per-environment latents: _reset_latents + _reset_latent_step_count of env_reset,
// the per-step _update_latents and the copy of all latents into the experience slot, as ONE launch with one wave per
// environment (or per id) and no intermediate tensor.  The due test of _update_latents runs inside the kernel, so there is
// no nonzero and no host round trip.  Follows learning/ase_agent.py:310-379 and learning/ase_network_builder.py:221-225 of
// the reference, operation by operation in f32 (the file compiles with -ffp-contract=off).
#include "latent_row.h"

namespace {

struct LatentRenewArgs {
    const int32_t* ids;              // ids mode; NULL: due mode
    const float* eps;                // passed-in normals [n_ids, ld_eps]; NULL: device draws from rng
    const int32_t* steps;            // passed-in steps [n_ids]
    const uint64_t* rng;
    const void* progress;            // int32 or int64 [n_envs], due mode
    int32_t* reset_steps;            // NULL: no steps bookkeeping
    float* z;
    void* z2;                        // due mode: every environment's latent after the decision
    int64_t ld_eps, ld_z, ld_z2, steps_low;
    uint32_t steps_span;             // steps_high - steps_low
    int n_envs, n_rows, dim, progress_i64, steps_add, z2_dtype;
};

// one wave per row, dim <= 128
__global__ __launch_bounds__(256) void latent_renew_kernel(LatentRenewArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.n_rows) return;
    const int e = a.ids ? a.ids[r] : r;
    if (e < 0 || e >= a.n_envs) return;                  // an id outside the buffers is skipped, never dereferenced
    bool renew = true;                                   // the same for every lane of the wave
    if (!a.ids) {                                        // _update_latents: _latent_reset_steps <= progress_buf
        const int64_t progress = a.progress_i64 ? reinterpret_cast<const int64_t*>(a.progress)[e]
                                                : (int64_t)reinterpret_cast<const int32_t*>(a.progress)[e];
        renew = (int64_t)a.reset_steps[e] <= progress;
    }
    float* zrow = a.z + (int64_t)e * a.ld_z;
    float v[2] = {0.f, 0.f};
    if (renew) {
        if (a.eps) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int j = lane + 64 * q;
                if (j < a.dim) v[q] = a.eps[(int64_t)r * a.ld_eps + j];
            }
        } else {
            // the draws of environment e depend on (seed, offset, e) only: row e of sample_latents(n_envs, dim)
            latent_row_normals(a.rng[0], a.rng[1], (uint64_t)e * a.dim, a.dim, lane, v);
        }
        latent_row_normalize(v);
        if (a.reset_steps && lane == 0) {
            // word 3 of the row's first element by multiply-shift (exact, never reaches steps_high)
            const int32_t s = a.steps ? a.steps[r]
                                      : (int32_t)(a.steps_low + (int64_t)(((uint64_t)philox_word<3>(a.rng[0], a.rng[1], (uint64_t)e * a.dim) *
                                                                           (uint64_t)a.steps_span) >> 32));
            a.reset_steps[e] = a.steps_add ? a.reset_steps[e] + s : s;
        }
    } else if (a.z2) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int j = lane + 64 * q;
            if (j < a.dim) v[q] = zrow[j];
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = lane + 64 * q;
        if (j < a.dim) {
            if (renew) zrow[j] = v[q];
            if (a.z2) latent_store_as(a.z2, a.z2_dtype, (int64_t)e * a.ld_z2 + j, v[q]);
        }
    }
}

}  // namespace

extern "C" int ase_hip_latent_renew(const int32_t* env_ids, int n_ids, const float* eps, int64_t ld_eps, const int32_t* steps,
                                    uint64_t* rng_state, int advance, const void* progress_buf, int progress_i64,
                                    int32_t* reset_steps, int steps_add, int64_t steps_low, int64_t steps_high, float* latents,
                                    int64_t ld_z, void* z2, int64_t ld_z2, int z2_dtype, int n_envs, int dim, void* stream) {
    const bool due = env_ids == nullptr;
    ASE_CHECK_ARG(latents, "latent_renew: null latents");
    ASE_CHECK_ARG(dim >= 1 && dim <= 128, "latent_renew: dim %d outside 1 .. 128", dim);
    ASE_CHECK_ARG(ld_z >= dim, "latent_renew: ld_z %lld below dim %d", (long long)ld_z, dim);
    ASE_CHECK_ARG(n_envs > 0, "latent_renew: bad size (n_envs %d)", n_envs);
    ASE_CHECK_ARG(env_ids ? n_ids >= 0 : n_ids == 0, "latent_renew: n_ids %d %s env_ids", n_ids, env_ids ? "with" : "without");
    ASE_CHECK_ARG((eps != nullptr) != (rng_state != nullptr), "latent_renew: exactly one draw source, eps or rng_state (%s given)",
                  eps ? "both" : "none");
    ASE_CHECK_ARG(!eps || !due, "latent_renew: due mode (env_ids NULL) draws on the device, eps must be NULL");
    ASE_CHECK_ARG(!eps || ld_eps >= dim, "latent_renew: ld_eps %lld below dim %d", (long long)ld_eps, dim);
    ASE_CHECK_ARG(eps && reset_steps ? steps != nullptr : steps == nullptr,
                  "latent_renew: steps comes with eps when reset_steps is given, and only then");
    ASE_CHECK_ARG(!due || progress_buf, "latent_renew: due mode (env_ids NULL) needs progress_buf");
    ASE_CHECK_ARG(!due || reset_steps, "latent_renew: due mode (env_ids NULL) needs reset_steps");
    ASE_CHECK_ARG(!due || steps_add, "latent_renew: due mode (env_ids NULL) adds the steps, steps_add must be set");
    ASE_CHECK_ARG(due || !progress_buf, "latent_renew: ids mode does not use progress_buf (must be NULL)");
    ASE_CHECK_ARG(due || !z2, "latent_renew: ids mode does not use z2 (must be NULL)");
    ASE_CHECK_ARG(!z2 || z2_dtype == ASE_F32 || z2_dtype == ASE_F16 || z2_dtype == ASE_BF16, "latent_renew: unknown z2_dtype %d", z2_dtype);
    ASE_CHECK_ARG(!z2 || ld_z2 >= dim, "latent_renew: ld_z2 %lld below dim %d", (long long)ld_z2, dim);
    const bool draws_steps = rng_state && reset_steps;
    ASE_CHECK_ARG(!draws_steps || (steps_high > steps_low && steps_high - steps_low <= (int64_t)0xFFFFFFFF),
                  "latent_renew: steps in [steps_low %lld, steps_high %lld): high must exceed low by 1 .. 2^32 - 1",
                  (long long)steps_low, (long long)steps_high);
    ASE_CHECK_ARG(!draws_steps || (steps_low >= INT32_MIN && steps_high - 1 <= INT32_MAX),
                  "latent_renew: steps in [steps_low %lld, steps_high %lld) do not fit the int32 reset_steps", (long long)steps_low,
                  (long long)steps_high);
    LatentRenewArgs a = {};
    a.ids = env_ids; a.eps = eps; a.steps = steps; a.rng = rng_state; a.progress = progress_buf; a.reset_steps = reset_steps;
    a.z = latents; a.z2 = z2; a.ld_eps = ld_eps; a.ld_z = ld_z; a.ld_z2 = ld_z2;
    a.steps_low = steps_low; a.steps_span = draws_steps ? (uint32_t)(steps_high - steps_low) : 0u;
    a.n_envs = n_envs; a.n_rows = due ? n_envs : n_ids; a.dim = dim; a.progress_i64 = progress_i64 != 0;
    a.steps_add = steps_add != 0; a.z2_dtype = z2_dtype;
    const bool bump = rng_state && advance;          // a call is one position of the stream, an empty env_ids list included
    if (a.n_rows == 0 && !bump) return ASE_OK;
    if (a.n_rows > 0)
        ASE_LAUNCH(latent_renew_kernel, dim3((a.n_rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
    if (bump) ASE_LAUNCH(rng_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, rng_state);
    ASE_CHECK_LAUNCH("latent_renew");
    return ASE_OK;
}
