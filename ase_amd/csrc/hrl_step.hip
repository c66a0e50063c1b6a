// The glue of the HRL agent's inner loop (learning/hrl_agent.py:45-82,89-93,231-240 of the reference): one
// high-level step wraps llc_steps simulator steps around the frozen low-level controller.  Three entries, contracts in
// include/ase_hip.h:
//   ase_hip_hrl_latent      once per high-level step   z = normalize(clamp(action, -1, 1)), also into the style chain's input
//   ase_hip_hrl_llc_action  once per inner step        padded head output -> the action the environment gets
//   ase_hip_hrl_accum       once per inner step        task reward, discriminator reward, done / terminate counts; the finals
// Fixed grids, no host decision, no atomics, no intermediate tensor: each is one launch a launch program can hold.  The file is
// compiled without a * b + c contraction (Makefile NOFMA), which the bitwise contracts rest on.
#include "latent_row.h"

namespace {

// one wave per row, dim <= 128: normalize_rows_kernel's arithmetic (latent_row_normalize) behind the clamp
__global__ __launch_bounds__(256) void hrl_latent_kernel(const float* __restrict__ actions, int64_t ld_a, float* __restrict__ z,
                                                         int64_t ld_z, void* __restrict__ z2, int64_t ld_z2, int z2_dtype, int n,
                                                         int dim) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = lane + 64 * q;
        if (j < dim) v[q] = ceil_nan(floor_nan(actions[(int64_t)r * ld_a + j], -1.0f), 1.0f);
    }
    latent_row_normalize(v);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = lane + 64 * q;
        if (j < dim) {
            if (z) z[(int64_t)r * ld_z + j] = v[q];
            if (z2) latent_store_as(z2, z2_dtype, (int64_t)r * ld_z2 + j, v[q]);
        }
    }
}

// one lane per element of [n, act]
__global__ __launch_bounds__(256) void hrl_llc_action_kernel(const float* __restrict__ mu, int64_t ld_mu,
                                                             const float* __restrict__ low, const float* __restrict__ high,
                                                             float* __restrict__ out, int64_t ld_out, int n, int act, int clip) {
    const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (i >= (int64_t)n * act) return;
    const int e = (int)(i / act), j = (int)(i - (int64_t)e * act);
    float m = mu[(int64_t)e * ld_mu + j];
    if (clip) {
        // rl_games rescale_actions on the clamped mu: d and m of the bounds, then a multiply and an add, each rounded
        const float d = (high[j] - low[j]) / 2.0f;
        const float c = (high[j] + low[j]) / 2.0f;
        const float p = ceil_nan(floor_nan(m, -1.0f), 1.0f) * d;
        m = p + c;
    }
    out[(int64_t)e * ld_out + j] = m;
}

struct HrlAccumArgs {
    const float* rewards;
    const void* dones;
    const void* terminate;
    const float* logit;
    float* acc;
    float* rewards_out;
    float* disc_out;
    float* dones_out;
    float* terminate_out;
    int64_t ld_l, acc_stride;
    float disc_scale, steps;
    int dones_kind, terminate_kind, first, last, n;
};

// acc = (first ? 0.0f : acc) + x: the reference starts every sum from the float 0.0
__device__ __forceinline__ float hrl_fold(float* acc, int first, float x) {
    const float s = (first ? 0.0f : *acc) + x;
    *acc = s;
    return s;
}

// one lane per environment
__global__ __launch_bounds__(256) void hrl_accum_kernel(HrlAccumArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    bool set;
    const float r = hrl_fold(a.acc + e, a.first, a.rewards[e]);
    const float d = hrl_fold(a.acc + 2 * a.acc_stride + e, a.first, flag_value(a.dones, a.dones_kind, e, set));
    float dr = 0.f, t = 0.f;
    if (a.logit) dr = hrl_fold(a.acc + a.acc_stride + e, a.first, disc_reward_of(a.logit[(int64_t)e * a.ld_l], a.disc_scale));
    if (a.terminate) t = hrl_fold(a.acc + 3 * a.acc_stride + e, a.first, flag_value(a.terminate, a.terminate_kind, e, set));
    if (!a.last) return;
    a.rewards_out[e] = r / a.steps;
    a.dones_out[e] = d > 0.f ? 1.0f : 0.0f;                  // a NaN count: 0, as the reference's (count > 0) mask
    if (a.logit) a.disc_out[e] = dr / a.steps;
    if (a.terminate) a.terminate_out[e] = t > 0.f ? 1.0f : 0.0f;
}

inline bool storage_ok(int dtype) { return dtype == ASE_F32 || dtype == ASE_BF16 || dtype == ASE_F16; }

}  // namespace

extern "C" int ase_hip_hrl_latent(const float* actions, int64_t ld_a, float* z, int64_t ld_z, void* z2, int64_t ld_z2,
                                  int z2_dtype, int n, int dim, void* stream) {
    ASE_CHECK_ARG(actions, "hrl_latent: null actions");
    ASE_CHECK_ARG(z || z2, "hrl_latent: neither z nor z2");
    ASE_CHECK_ARG(dim >= 1 && dim <= 128, "hrl_latent: dim %d outside [1, 128]", dim);
    ASE_CHECK_ARG(ld_a >= dim && (!z || ld_z >= dim) && (!z2 || ld_z2 >= dim), "hrl_latent: a pitch below dim %d", dim);
    ASE_CHECK_ARG(!z2 || storage_ok(z2_dtype), "hrl_latent: z2 dtype %d (ASE_F32 / ASE_BF16 / ASE_F16)", z2_dtype);
    ASE_CHECK_ARG(n >= 1, "hrl_latent: n %d", n);
    ASE_LAUNCH(hrl_latent_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, actions, ld_a, z, ld_z, z2, ld_z2,
               z2_dtype, n, dim);
    ASE_CHECK_LAUNCH("hrl_latent");
    return ASE_OK;
}

extern "C" int ase_hip_hrl_llc_action(const float* mu, int64_t ld_mu, const float* low, const float* high, float* out,
                                      int64_t ld_out, int n, int act, int clip, void* stream) {
    ASE_CHECK_ARG(mu && out, "hrl_llc_action: null mu / out");
    ASE_CHECK_ARG(!clip || (low && high), "hrl_llc_action: clip without low / high");
    ASE_CHECK_ARG(act >= 1 && act <= 128, "hrl_llc_action: act %d outside [1, 128]", act);
    ASE_CHECK_ARG(ld_mu >= act && ld_out >= act, "hrl_llc_action: a pitch below act %d", act);
    ASE_CHECK_ARG(n >= 1, "hrl_llc_action: n %d", n);
    const int64_t blocks = ((int64_t)n * act + 255) / 256;
    ASE_LAUNCH(hrl_llc_action_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mu, ld_mu, low, high, out,
               ld_out, n, act, clip);
    ASE_CHECK_LAUNCH("hrl_llc_action");
    return ASE_OK;
}

extern "C" int ase_hip_hrl_accum(const float* rewards, const void* dones, int dones_kind, const void* terminate,
                                 int terminate_kind, const float* logit, int64_t ld_l, float disc_scale, float* acc,
                                 int64_t acc_stride, int first, int last, int llc_steps, float* rewards_out, float* disc_out,
                                 float* dones_out, float* terminate_out, int n, void* stream) {
    ASE_CHECK_ARG(rewards && dones && acc, "hrl_accum: null rewards / dones / acc");
    ASE_CHECK_ARG(kind_ok(dones_kind), "hrl_accum: dones kind %d (ASE_KIND_U8 / I32 / I64 / F32)", dones_kind);
    ASE_CHECK_ARG(!terminate || kind_ok(terminate_kind), "hrl_accum: terminate kind %d (ASE_KIND_U8 / I32 / I64 / F32)",
                  terminate_kind);
    ASE_CHECK_ARG(terminate || !terminate_out, "hrl_accum: partial terminate group (terminate_out without terminate)");
    ASE_CHECK_ARG(logit || !disc_out, "hrl_accum: partial discriminator group (disc_out without logit)");
    ASE_CHECK_ARG(!logit || ld_l >= 1, "hrl_accum: logit pitch %lld", (long long)ld_l);
    ASE_CHECK_ARG(llc_steps >= 1, "hrl_accum: llc_steps %d", llc_steps);
    ASE_CHECK_ARG(!last || (rewards_out && dones_out), "hrl_accum: last without rewards_out / dones_out");
    ASE_CHECK_ARG(!last || !terminate || terminate_out, "hrl_accum: partial terminate group (last, terminate without "
                  "terminate_out)");
    ASE_CHECK_ARG(!last || !logit || disc_out, "hrl_accum: partial discriminator group (last, logit without disc_out)");
    ASE_CHECK_ARG(acc_stride >= n, "hrl_accum: acc_stride %lld below n %d", (long long)acc_stride, n);
    ASE_CHECK_ARG(n >= 1, "hrl_accum: n %d", n);
    HrlAccumArgs a = {};
    a.rewards = rewards; a.dones = dones; a.dones_kind = dones_kind; a.terminate = terminate; a.terminate_kind = terminate_kind;
    a.logit = logit; a.ld_l = ld_l; a.disc_scale = disc_scale; a.acc = acc; a.acc_stride = acc_stride;
    a.first = first; a.last = last; a.steps = (float)llc_steps;
    a.rewards_out = rewards_out; a.disc_out = disc_out; a.dones_out = dones_out; a.terminate_out = terminate_out; a.n = n;
    ASE_LAUNCH(hrl_accum_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    ASE_CHECK_LAUNCH("hrl_accum");
    return ASE_OK;
}
