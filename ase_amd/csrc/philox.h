// The library's random stream (rollout.hip, task_reset.hip, latent_renew.hip): counter-based Philox4x32-10 on the counter {elem lo, elem hi,
// offset lo, offset hi} with the key {seed lo, seed hi}; rng_state is u64[2] = {seed, offset} on the device, read by the
// drawing kernel and advanced behind it by rng_advance_kernel.  tests/ref_rollout.py states the stream word for word.
#pragma once
#include "common.h"

namespace {

// Philox4x32-10
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k[0], n1 = lo1, n2 = hi0 ^ c[3] ^ k[1], n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
}

__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t offset, uint64_t elem) {
    uint32_t c[4] = {(uint32_t)elem, (uint32_t)(elem >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int i = 0; i < 10; ++i) philox_round(c, k);
    const float u1 = ((float)c[0] + 1.0f) * 2.3283064365386963e-10f;  // (0, 1]
    const float u2 = (float)c[1] * 2.3283064365386963e-10f;
    return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t offset, uint64_t elem) {
    uint32_t c[4] = {(uint32_t)elem, (uint32_t)(elem >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int i = 0; i < 10; ++i) philox_round(c, k);
    // 24 bits: exact in f32 and < 1.  (float)c[2] * 2^-32 rounds every word >= 0xFFFFFF80 to 1.0, and Bernoulli(1.0) then draws 0
    return (float)(c[2] >> 8) * 5.9604644775390625e-08f;             // [0, 1)
}

// output word W of an element, for integer draws.  The normal of an element uses words 0 and 1, its keep-uniform word 2: word 3
// of an element is independent of every float the element gives.
template <int W> __device__ __forceinline__ uint32_t philox_word(uint64_t seed, uint64_t offset, uint64_t elem) {
    uint32_t c[4] = {(uint32_t)elem, (uint32_t)(elem >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
    uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
    for (int i = 0; i < 10; ++i) philox_round(c, k);
    return c[W];
}
__device__ __forceinline__ uint32_t philox_word0(uint64_t seed, uint64_t offset, uint64_t elem) { return philox_word<0>(seed, offset, elem); }

__global__ void rng_advance_kernel(uint64_t* rng) { rng[1] += 1; }

}  // namespace
