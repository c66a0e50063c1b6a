// NT matrix-core kernels of the dense layers (gfx950 / CDNA4): C = mask(act(alpha * A·Bᵀ + bias)) - forward, data-gradient,
// gradient-penalty chain.  Templates only; each storage type is instantiated in its own translation unit
// (gemm_nt_<type>.hip -> ase_nt::dispatch_nt_<type>) so that the library builds in parallel.
//
// Storage types: bf16 / f16 (v_mfma_f32_32x32x16_{bf16,f16}, f32 accumulate), exact f32 (v_mfma_f32_32x32x2_f32), f32 multiplied
// as three bf16 MFMAs on a hi/lo split (f32s_t) and f32 multiplied as three f16 MFMAs on a hi/lo split of SCALED operands
// (f32h_t).  Wave64, XCD-aware tile order (8 XCDs, private L2s).
//   Staging: tiles go HBM -> LDS directly with global_load_lds_dwordx4 (no staging VGPRs, no ds_write pass); LDS rows
//       are 128 bytes, unpadded (the DMA writes lane-linear), with the 16-byte chunks of row r stored at slot
//       chunk ^ ((r >> 1) & 7): the permutation is applied to the per-lane SOURCE address and again on the fragment
//       read, which makes every ds_read_b128 lane group hit 16 distinct bank slots.
//   Kernels: gemm_nt_kernel (64 / 128 / 256 tiles, S-stage ring, one barrier per K-tile, every wave in lock-step) and
//       gemm_nt8_kernel (16-bit storage, 256 x 256: four phases per K-tile, two wave groups one barrier apart, counted
//       vmcnt) - see the comment blocks in front of each; nt_choice() picks per shape.
#pragma once
#include "gemm_nt.h"
#include <stdlib.h>
#include <utility>

namespace {

using namespace ase_nt;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index can be a template argument
template <int N, typename F, int... I> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl<N>(f, std::make_integer_sequence<int, N>{}); }

template <typename T> struct Mma;

template <typename T> struct Mma16 {
    typedef typename V16<T>::x8 x8;
    // one staged row = RB/2 k-values = RB/32 steps of 16
    // SW: D = B-fragment x A-fragment (transposed accumulator block: a lane owns one output row, see nt_epilogue_rows)
    template <int FM, int FN, int RB, bool SW = false>
    static __device__ __forceinline__ void tile(const char* sA, const char* sB, int lane, f32x16 (&acc)[FM][FN]) {
        const int r = lane & 31, h = lane >> 5, sw = lds_swz<RB>(r);
#pragma unroll
        for (int ks = 0; ks < RB / 32; ++ks) {
            x8 a[FM], b[FN];
            const int off = r * RB + (((ks * 2 + h) ^ sw) << 4);
#pragma unroll
            for (int i = 0; i < FM; ++i)
                a[i] = *reinterpret_cast<const x8*>(sA + i * 32 * RB + off);
#pragma unroll
            for (int j = 0; j < FN; ++j)
                b[j] = *reinterpret_cast<const x8*>(sB + j * 32 * RB + off);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    if constexpr (SW) acc[i][j] = mfma16<T>(b[j], a[i], acc[i][j]);
                    else acc[i][j] = mfma16<T>(a[i], b[j], acc[i][j]);
                }
        }
    }
};
template <> struct Mma<bf16_t> : Mma16<bf16_t> {};
template <> struct Mma<f16_t> : Mma16<f16_t> {};

template <> struct Mma<float> {
    // one staged row = RB/4 k-values = RB/32 blocks of 8; within a block lane-half h holds k = 4h..4h+3
    // and MFMA j multiplies element j of both operands (any k order is fine if A and B agree).
    template <int FM, int FN, int RB>
    static __device__ __forceinline__ void tile(const char* sA, const char* sB, int lane, f32x16 (&acc)[FM][FN]) {
        const int r = lane & 31, h = lane >> 5, sw = lds_swz<RB>(r);
#pragma unroll
        for (int kb = 0; kb < RB / 32; ++kb) {
            f32x4 a[FM], b[FN];
            const int off = r * RB + (((kb * 2 + h) ^ sw) << 4);
#pragma unroll
            for (int i = 0; i < FM; ++i)
                a[i] = *reinterpret_cast<const f32x4*>(sA + i * 32 * RB + off);
#pragma unroll
            for (int j = 0; j < FN; ++j)
                b[j] = *reinterpret_cast<const f32x4*>(sB + j * 32 * RB + off);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < FM; ++i)
#pragma unroll
                    for (int j = 0; j < FN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
        }
    }
};

__device__ __forceinline__ void split_bf16(const f32x4& x0, const f32x4& x1, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        hi[q] = (bf16_t)x0[q];
        hi[q + 4] = (bf16_t)x1[q];
        lo[q] = (bf16_t)(x0[q] - (float)hi[q]);
        lo[q + 4] = (bf16_t)(x1[q] - (float)hi[q + 4]);
    }
}

template <> struct Mma<f32s_t> {
    // f32 rows (RB/4 k-values = RB/64 steps of 16): a lane needs 8 consecutive k per step = 2 chunks.
    template <int FM, int FN, int RB>
    static __device__ __forceinline__ void tile(const char* sA, const char* sB, int lane, f32x16 (&acc)[FM][FN]) {
        const int r = lane & 31, h = lane >> 5, sw = lds_swz<RB>(r);
#pragma unroll
        for (int ks = 0; ks < RB / 64; ++ks) {
            bf16x8 ah[FM], al[FM], bh[FN], bl[FN];
            const int c0 = ks * 4 + h * 2;
            const int o0 = r * RB + ((c0 ^ sw) << 4), o1 = r * RB + (((c0 + 1) ^ sw) << 4);
#pragma unroll
            for (int i = 0; i < FM; ++i)
                split_bf16(*reinterpret_cast<const f32x4*>(sA + i * 32 * RB + o0),
                           *reinterpret_cast<const f32x4*>(sA + i * 32 * RB + o1), ah[i], al[i]);
#pragma unroll
            for (int j = 0; j < FN; ++j)
                split_bf16(*reinterpret_cast<const f32x4*>(sB + j * 32 * RB + o0),
                           *reinterpret_cast<const f32x4*>(sB + j * 32 * RB + o1), bh[j], bl[j]);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
    }
};

// f32h_t (ASE_F32H3): f32-sized storage whose products run as three f16 MFMAs on hi / lo splits of power-of-two SCALED operands.
//   A (activations, chain values: f32 in HBM and LDS) is split in registers:  sx = x * sa (exact), hi = half(sx), lo = half(sx - hi).
//     With |sx| >= 2^-2 both parts are normal halves and hi + lo carries 22 significant bits of x; smaller values degrade gracefully
//     (lo subnormal: absolute error 2^-25 of the scaled range); |sx| > 65504 overflows to inf and the launch's output is NaN - loud
//     on purpose (the caller's scale exponent was wrong), never a silently saturated value.
//   B (weights) arrives PRE-SPLIT: ase_hip_refresh_shadow(dtype = ASE_F32H3 | eb << 16) writes the shadows in the packed format
//     [8 hi halves | 8 lo halves] per group of 8 consecutive k (32 bytes, the footprint of 8 floats), already scaled by 2^eb.  A B
//     element is needed by every row tile of the launch (64 of them at 4096 rows): splitting it once per optimisation step instead
//     of once per tile removes two thirds of the kernel's VALU work, which is what bounded it (round 5: 5 VALU operations per
//     element and fragment against 3 MFMAs of 32 cycles per fragment pair).
//   The split of two elements is four instructions, written out because the compiler reaches this form for a quarter of the elements
//     only (the rest it converts back to f32 and SLP-packs into v_pk_mul_f32 / v_pk_fma_f32, the costliest VALU form beside MFMAs):
//       hi = half(sa x)       v_fma_mix{lo,hi}_f16: f32 sources, ONE rounding, into the low / high half of the packed register
//       lo = half(sa x - hi)  the same, hi read back as a half source (op_sel / op_sel_hi of source 2)
//     and equals half(f32(sa x)), half(f32(f32(sa x) - hi)) bit for bit: sa is a power of two, so sa x is exact in f32 (or inf in both
//     forms), and sa x - hi is a multiple of the f32 ulp of sa x no larger than half an ulp of hi, hence exact in f32 as well
//     (tests/test_h3_split_rounding.py).  Two differences no output can see: sa x = -0 gives hi = +0 (the fma adds +0), lo = -0; a
//     finite x whose sa x leaves f32's range gives lo = -inf where inf - inf gave NaN - with hi = inf the products sum to NaN either way.
__device__ __forceinline__ void split_f16_pair(float x0, float x1, float sa, uint32_t& hi, uint32_t& lo) {
    asm("v_fma_mixlo_f16 %0, %4, %2, 0\n\t"
        "v_fma_mixhi_f16 %0, %4, %3, 0\n\t"
        "v_fma_mixlo_f16 %1, %4, %2, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %4, %3, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(hi), "=&v"(lo)
        : "v"(x0), "v"(x1), "s"(sa));
}
// the two wait states between a VALU write inside an asm statement and an MFMA that reads the register as an operand (the compiler
// pads nothing it cannot see); naming the registers keeps every MFMA that reads them below it
__device__ __forceinline__ void split_f16_fence(u32x4& hi, u32x4& lo) { asm("s_nop 1" : "+v"(hi), "+v"(lo)); }

template <> struct Mma<f32h_t> {
    // rows of 128 / 64 bytes = 32 / 16 k-values; per k-step of 16 a lane (r, h) owns the 8 k-values of group 2 ks + h = two
    // 16-byte chunks: A - 8 floats to split; B - its 8 hi halves and its 8 lo halves.
    //   Schedule of one K-tile (pinned with sched_barrier: the split is asm the scheduler cannot weigh):
    //     read A(0), B(0) | split A(0) under B(0)'s latency | read A(1), B(1) | MFMAs(0) with the split of A(1) spread between them |
    //     MFMAs(1).   Every wait is the compiler's counted lgkmcnt of reads issued in order.  Tiles of more than four accumulators
    //     read B(1) after MFMAs(0) instead (PF: their fragments would not fit the registers twice).
    //   MFMA order per accumulator and k-step: al bh, ah bl, ah bh, k ascending - the order of every earlier version (bitwise results).
    //   Addresses: fa / fb = the lane's byte offsets of its two chunks per k-step in the A / B part of ring buffer 0 (frag_offsets: loop
    //     invariant), sbuf = the K-tile's ring buffer as a scalar byte offset: one add per chunk, the fragment index is the ds_read's
    //     immediate offset.
    template <int RB>
    static __device__ __forceinline__ void frag_offsets(int lane, uint32_t a0, uint32_t b0, uint32_t (&fa)[RB / 64][2], uint32_t (&fb)[RB / 64][2]) {
        const int r = lane & 31, h = lane >> 5, sw = lds_swz<RB>(r);
#pragma unroll
        for (int ks = 0; ks < RB / 64; ++ks)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t o = r * RB + (((ks * 4 + h * 2 + c) ^ sw) << 4);
                fa[ks][c] = a0 + o;
                fb[ks][c] = b0 + o;
                asm volatile("" : "+v"(fa[ks][c]), "+v"(fb[ks][c]));      // kept whole: eight registers, not a sum re-formed per K-tile
            }
    }
    template <int FM, int FN, int RB>
    static __device__ __forceinline__ void tile(const char* smem, uint32_t sbuf, const uint32_t (&fa)[RB / 64][2], const uint32_t (&fb)[RB / 64][2],
                                                f32x16 (&acc)[FM][FN], float sa) {
        constexpr int KS = RB / 64, NM = FM * FN * 3, NP = FM * 4;
        constexpr bool PF = FM * FN <= 4;
        f32x4 ax[2][FM][2];
        u32x4 ah[2][FM], al[2][FM];
        f16x8 bh[2][FN], bl[2][FN];
        auto read_a = [&](int ks) {
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int c = 0; c < 2; ++c) ax[ks & 1][i][c] = *reinterpret_cast<const f32x4*>(smem + (fa[ks][c] + sbuf) + i * 32 * RB);
        };
        auto read_b = [&](int ks) {
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                bh[PF ? ks & 1 : 0][j] = *reinterpret_cast<const f16x8*>(smem + (fb[ks][0] + sbuf) + j * 32 * RB);
                bl[PF ? ks & 1 : 0][j] = *reinterpret_cast<const f16x8*>(smem + (fb[ks][1] + sbuf) + j * 32 * RB);
            }
        };
        // pair q of k-step ks = packed register q & 3 of row fragment q >> 2: elements 0, 1 or 2, 3 of chunk (q >> 1) & 1
        auto split_pair = [&](int ks, int q) {
            const int i = q >> 2, c = (q >> 1) & 1, e = (q & 1) * 2;
            uint32_t hi, lo;
            split_f16_pair(ax[ks & 1][i][c][e], ax[ks & 1][i][c][e + 1], sa, hi, lo);
            ah[ks & 1][i][c * 2 + (q & 1)] = hi;
            al[ks & 1][i][c * 2 + (q & 1)] = lo;
        };
        auto fence = [&](int ks) {
#pragma unroll
            for (int i = 0; i < FM; ++i) split_f16_fence(ah[ks & 1][i], al[ks & 1][i]);
        };
        read_a(0);
        read_b(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NP; ++q) split_pair(0, q);
        fence(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bool more = ks + 1 < KS;
            if (more) {
                read_a(ks + 1);
                if constexpr (PF) read_b(ks + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j)
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        const f16x8 a = __builtin_bit_cast(f16x8, t == 0 ? al[ks & 1][i] : ah[ks & 1][i]);
                        const f16x8 b = (t == 1) ? bl[PF ? ks & 1 : 0][j] : bh[PF ? ks & 1 : 0][j];
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[i][j], 0, 0, 0);
                        if (more) {                      // the next k-step's NP pairs, spread evenly behind this one's NM MFMAs
                            const int m = (i * FN + j) * 3 + t;
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int q = 0; q < NP; ++q)
                                if (q * NM >= m * NP && q * NM < (m + 1) * NP) split_pair(ks + 1, q);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
            if (more) {
                fence(ks + 1);
                if constexpr (!PF) read_b(ks + 1);
            }
        }
    }
};

// HBM -> LDS DMA of one operand tile: pass i moves rows [RPP i, RPP i + RPP) (RPP = 8 rows per wave); wave w of the
// pass owns the 8 rows RPP i + 8 w .. + 7 = one 1-KiB lane-linear LDS piece (M0 = wave-uniform base, lane l lands at
// base + 16 l).
template <int PASSES, int RPP, int RB>
__device__ __forceinline__ void nt_stage(const char* const (&src)[PASSES], int64_t koff, char* lds_wave_base) {
#pragma unroll
    for (int i = 0; i < PASSES; ++i)
        __builtin_amdgcn_global_load_lds((gptr_t*)(src[i] + koff), (lptr_t*)(lds_wave_base + i * RPP * RB), 16, 0, 0);
}
// ---- epilogue of the NT kernels.  C/D layout of the 32x32 MFMA: col = lane & 31, row = (e&3) + 8*(e>>2) + 4*(lane>>5),
// i.e. a lane owns ONE column: storing from registers would be 2-byte scattered stores.  Phase 1 applies bias +
// activation (per-column bias = per-lane scalar) and transposes FMC x FNC fragments of the wave's sub-tile through a
// wave-private f32 LDS slab [FMC*32][FNC*32] (row pitch 64 dwords: ds_write_b32 and ds_read_b128 are both
// conflict-free); phase 2 lets every lane pick up 4 consecutive columns of a row, applies the derivative mask,
// issues 8/16-byte row-contiguous stores (full 128-byte lines per row) and keeps per-column partial sums for the bias
// gradient.  The caller guarantees that nobody still reads the staging ring (barrier).
//   The mask operand (AUXK = 1: the activation itself, 8/16 bytes per lane and row; AUXK = 2: its bit matrix, one word)
// is loaded a whole chunk AHEAD of its use - all rows of a chunk at once, the next chunk's before the current chunk's
// LDS transposition: left inside the row loop the loads cost one exposed HBM round trip per 4 rows (+10 us on a
// 256 x 256 tile, measured, whatever their width).
template <typename T, int AUXK> struct AuxReg;
template <typename T> struct AuxReg<T, 0> { char v; };
template <> struct AuxReg<bf16_t, 1> { bf16x4 v; };
template <> struct AuxReg<f16_t, 1> { f16x4 v; };
template <> struct AuxReg<float, 1> { f32x4 v; };
template <> struct AuxReg<f32s_t, 1> { f32x4 v; };
template <> struct AuxReg<f32h_t, 1> { f32x4 v; };
template <typename T> struct AuxReg<T, 2> { uint32_t v; };

// OR over aligned groups of 8 lanes with DPP only (no LDS round trip): xor 1, xor 2, then the half-row mirror
__device__ __forceinline__ uint32_t or8_dpp(uint32_t x) {
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true);   // row_half_mirror
    return x;
}

// mask operand of chunk ch (jc-major) of a wave's sub-tile: one AuxReg per row iteration
template <typename T, int FM, int FN, int FMC, int FNC, int AUXK>
__device__ __forceinline__ void nt_aux_load(const NTParams& p, int ch, int lane, int mrow0, int ncol0,
                                            AuxReg<T, AUXK> (&dst)[(FMC * 32) / (64 / (FNC * 8))]) {
    constexpr int ELPR = FNC * 8, RPI = 64 / ELPR, NIT = (FMC * 32) / RPI;
    if constexpr (AUXK != 0) {
        const int c4 = lane % ELPR, rsub = lane / ELPR;
        const int jc = (ch / (FM / FMC)) * FNC, ic = (ch % (FM / FMC)) * FMC;
        const int n0 = ncol0 + jc * 32 + c4 * 4;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int m = mrow0 + ic * 32 + it * RPI + rsub;
            if (n0 < p.N && m < p.M) {
                const int ma = (m >= p.aux_split) ? m - p.aux_delta : m;
                if constexpr (AUXK == 2)
                    dst[it].v = *reinterpret_cast<const uint32_t*>(p.aux + (int64_t)ma * p.ldaux + (n0 >> 5) * 4);
                else
                    dst[it].v = *reinterpret_cast<const decltype(dst[it].v)*>(p.aux + (int64_t)ma * p.ldaux + (int64_t)n0 * sizeof(T));
            }
        }
    }
}

// PRE: chunk 0 of the mask operand was loaded by the caller (before its main loop) into pre[]
// FUSE (f32h_t storage, ase_hip_gemm_nt_ex): the duties that were launches of their own around the gradient penalty's value path -
// the seed s w_logit[n] [h > 0] in place of the activation (ase_hip_gp_seed), a 16-bit twin of the stored value (the conversion launch,
// ase_hip_gather_multi) and the sum of the stored values' squares (ase_hip_sqnorm; returned per lane, the kernel reduces it) - each by
// the helper's own expression on the 4 columns the lane holds anyway.
template <typename T, int FM, int FN, int FMC, int FNC, int AUXK, bool PRE = false, bool FUSE = false>
__device__ __forceinline__ double nt_epilogue_impl(const NTParams& p, f32x16 (&acc)[FM][FN], float* slab, int lane,
                                                   int mrow0, int ncol0,
                                                   AuxReg<T, AUXK> (*pre)[(FMC * 32) / (64 / (FNC * 8))] = nullptr) {
    constexpr int WCOLS = FNC * 32, WROWS = FMC * 32;
    const int col_in = lane & 31, row_hi = (lane >> 5) * 4;
    constexpr int ELPR = WCOLS / 4;                // lanes per row (4 columns each)
    constexpr int RPI = 64 / ELPR;                 // rows per iteration
    constexpr int NIT = WROWS / RPI;               // row iterations per chunk
    constexpr int NCH = (FN / FNC) * (FM / FMC);   // chunks, jc-major
    constexpr bool AHEAD = AUXK != 0 && sizeof(AuxReg<T, AUXK>) <= 8;   // 16-byte f32 masks: current chunk only
    const int c4 = lane % ELPR, rsub = lane / ELPR;
    AuxReg<T, AUXK> areg[AHEAD ? 2 : 1][NIT];
    bool bad = false;                              // an element this lane stored overflowed (scale records, common.h)
    double sq = 0.0;                               // FUSE: this lane's share of the sum of squares

    auto load_aux = [&](int ch, AuxReg<T, AUXK> (&dst)[NIT]) {
        nt_aux_load<T, FM, FN, FMC, FNC, AUXK>(p, ch, lane, mrow0, ncol0, dst);
    };

    if constexpr (PRE) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) areg[0][it] = (*pre)[it];
    } else if constexpr (AUXK != 0) {
        load_aux(0, areg[0]);
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int jc = (ch / (FM / FMC)) * FNC, ic = (ch % (FM / FMC)) * FMC;
        const int n0 = ncol0 + jc * 32 + c4 * 4;
        if constexpr (AHEAD) {
            if (ch + 1 < NCH) load_aux(ch + 1, areg[(ch + 1) & 1]);
        } else if constexpr (AUXK != 0) {
            if (ch > 0) load_aux(ch, areg[0]);
        }
        AuxReg<T, AUXK> (&cur)[NIT] = areg[AHEAD ? (ch & 1) : 0];
#pragma unroll
        for (int jj = 0; jj < FNC; ++jj) {
            const int j = jc + jj;
            const int n = ncol0 + j * 32 + col_in;
            const float bias = (p.bias && n < p.N) ? p.bias[n] : 0.f;
#pragma unroll
            for (int ii = 0; ii < FMC; ++ii) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float v = p.alpha * acc[ic + ii][j][e] + bias;
                    if (p.act == ASE_ACT_RELU) v = v <= 0.f ? 0.f : v;       // torch.relu: a NaN stays (fmaxf returns 0); -0 -> +0 as fmaxf and the row-per-lane maximum
                    else if (p.act == ASE_ACT_TANH) v = tanhf(v);
                    slab[(ii * 32 + row_hi + (e & 3) + 8 * (e >> 2)) * WCOLS + jj * 32 + col_in] = v;
                }
            }
        }
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4 seed = {0.f, 0.f, 0.f, 0.f};             // FUSE: seed_scale * seed_w of the lane's 4 columns
        if constexpr (FUSE) {
            if (p.seed_w && n0 < p.N) {
#pragma unroll
                for (int q = 0; q < 4; ++q) seed[q] = p.seed_scale * (n0 + q < p.seed_n ? p.seed_w[n0 + q] : 0.f);
            }
        }
        if (n0 < p.N) {                                // N is a multiple of 4 (checked on the host)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int row = it * RPI + rsub;
                const int m = mrow0 + ic * 32 + row;
                if (m >= p.M) continue;
                f32x4 v = *reinterpret_cast<const f32x4*>(slab + row * WCOLS + c4 * 4);
                if (p.act >= ASE_ACT_SILU) {            // smooth activations: the slab holds z; keep it (twin), then activate
                    if (p.pre_out) {
                        if constexpr (sizeof(T) == 2) {
                            typename V16<T>::x4 zt;
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                zt[q] = from_f32<T>(v[q]);
                                bad |= ovf_hit1(zt[q]);
                            }
                            *reinterpret_cast<typename V16<T>::x4*>(p.pre_out + (int64_t)m * p.ldpre + (int64_t)n0 * 2) = zt;
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; ++q) bad |= ovf_hit1(v[q]);
                            *reinterpret_cast<f32x4*>(p.pre_out + (int64_t)m * p.ldpre + (int64_t)n0 * 4) = v;
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = act_apply(p.act, v[q]);
                }
                if constexpr (AUXK == 2) {
                    const uint32_t nib = cur[it].v >> (n0 & 31);
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = ((nib >> q) & 1u) ? v[q] : 0.f;
                } else if constexpr (AUXK == 1) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float a = (float)cur[it].v[q];
                        if (p.aux_mode == ASE_AUX_RELU_MASK) v[q] = a > 0.f ? v[q] : 0.f;
                        else if (p.aux_mode == ASE_AUX_TANH_GRAD) v[q] = v[q] * (1.f - a * a);
                        else v[q] = v[q] * act_grad(p.aux_mode >> 8, a);          // ASE_AUX_PREACT | (activation << 8)
                    }
                }
                if constexpr (FUSE) {
                    f32x4 sv = v;                       // the stored value; v stays the activation (mask_out below)
                    if (p.seed_w) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) sv[q] = seed[q] * (v[q] > 0.f ? 1.f : 0.f);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) bad |= ovf_hit1(sv[q]);
                    if (p.C) *reinterpret_cast<f32x4*>(p.C + (int64_t)m * p.ldc + (int64_t)n0 * 4) = sv;
                    if (p.twin) {
                        char* t = p.twin + (int64_t)m * p.ldtwin + (int64_t)n0 * 2;
                        if (p.twin_dtype == ASE_F16) {
                            f16x4 o;
#pragma unroll
                            for (int q = 0; q < 4; ++q) o[q] = from_f32<f16_t>(sv[q]);
                            *reinterpret_cast<f16x4*>(t) = o;
                        } else {
                            bf16x4 o;
#pragma unroll
                            for (int q = 0; q < 4; ++q) o[q] = from_f32<bf16_t>(sv[q]);
                            *reinterpret_cast<bf16x4*>(t) = o;
                        }
                    }
                    if (p.sq_acc) {                     // as sqnorm_kernel<float, 4>: f32 over the 4 columns (no contraction), then f64
                        float s = 0.f;
#pragma unroll
                        for (int q = 0; q < 4; ++q) s = __fadd_rn(s, __fmul_rn(sv[q], sv[q]));
                        sq += (double)s;
                    }
                } else if (p.out_f32 || sizeof(T) == 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) bad |= ovf_hit1(v[q]);
                    *reinterpret_cast<f32x4*>(p.C + (int64_t)m * p.ldc + (int64_t)n0 * 4) = v;
                } else {
                    typedef typename std::conditional<sizeof(T) == 2, T, bf16_t>::type S;     // (4-byte T: dead branch)
                    typename V16<S>::x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        o[q] = from_f32<S>(v[q]);
                        bad |= ovf_hit1(o[q]);
                        v[q] = (float)o[q];
                    }
                    *reinterpret_cast<typename V16<S>::x4*>(p.C + (int64_t)m * p.ldc + (int64_t)n0 * 2) = o;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) cs[q] += v[q];
                if (p.mask_out) {
                    // nibble of this lane's 4 columns -> OR over the 8 lanes of a 32-column word -> one 4-byte store
                    uint32_t bits = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) bits |= (v[q] > 0.f ? 1u : 0u) << q;
                    bits = or8_dpp(bits << (n0 & 31));
                    if ((c4 & 7) == 0) p.mask_out[(int64_t)m * p.ldmask + (n0 >> 5)] = bits;
                }
            }
        }
        // bias gradient: the chunks of one column group (same jc) follow each other; flush after the last of them
        if (p.colsum) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
#pragma unroll
                for (int o = ELPR; o < 64; o <<= 1) cs[q] += __shfl_xor(cs[q], o, 64);
            }
            if (lane < ELPR) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (n0 + q < p.colsum_n) atomic_add_f32(p.colsum + n0 + q, cs[q]);
            }
        }
    }
    ovf_report(p.alpha_dev, bad);
    return sq;
}

template <typename T, int FM, int FN, int FMC, int FNC, bool FUSE = false>
__device__ __forceinline__ double nt_epilogue(const NTParams& p, f32x16 (&acc)[FM][FN], float* slab, int lane, int mrow0,
                                              int ncol0) {
    if (p.aux_mode == ASE_AUX_NONE) return nt_epilogue_impl<T, FM, FN, FMC, FNC, 0, false, FUSE>(p, acc, slab, lane, mrow0, ncol0);
    if (p.aux_mode == ASE_AUX_RELU_BITS) return nt_epilogue_impl<T, FM, FN, FMC, FNC, 2, false, FUSE>(p, acc, slab, lane, mrow0, ncol0);
    if constexpr (FUSE) return 0.0;                // (the host admits no other mask operand beside the fused duties)
    else return nt_epilogue_impl<T, FM, FN, FMC, FNC, 1>(p, acc, slab, lane, mrow0, ncol0);
}

// ---- row-per-lane epilogue of the lock-step kernels (bf16, swapped MFMA operands): the general FM x FN form of
// nt8_epilogue_rows further down - see there.  acc[i][j]: lane (r = lane & 31, h = lane >> 5) owns output row i*32 + r
// and the columns j*32 + 8 g + 4 h + q.  bits[i][j]: the ReLU mask word of (row, 32-column fragment), loaded by the caller.
template <typename T, int FM, int FN, int AUXK, bool MASK>
__device__ __forceinline__ void nt_epilogue_rows_impl(const NTParams& p, f32x16 (&acc)[FM][FN], int lane, int mrow0, int ncol0,
                                                      const uint32_t (&bits)[FM][FN]) {
    const int r = lane & 31, h = lane >> 5;
    const f32x2 al = {p.alpha, p.alpha};
    const float relu_lo = (p.act == ASE_ACT_RELU) ? 0.f : -__builtin_inff();
    uint32_t ovf = 0;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        f32x4 bias[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (p.bias) bias[g] = *reinterpret_cast<const f32x4*>(p.bias + ncol0 + j * 32 + 8 * g + 4 * h);
            else bias[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int m = mrow0 + i * 32 + r;
            const bool row_ok = m < p.M;
            char* crow = p.C + (int64_t)m * p.ldc + (int64_t)(ncol0 + j * 32) * 2 + h * 16;
            uint32_t pk[4][2];
            const uint32_t mb = rows_frag<T, AUXK, MASK>(acc[i][j], bias, AUXK == 2 ? bits[i][j] >> (4 * h) : 0u, al, relu_lo, h, pk);
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                const auto s0 = __builtin_amdgcn_permlane32_swap(pk[g][0], pk[g + 1][0], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(pk[g][1], pk[g + 1][1], false, false);
                if (row_ok) *reinterpret_cast<uint4*>(crow + 8 * g * 2) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                ovf = ovf_fold(ovf_fold(ovf_fold(ovf_fold(ovf, s0[0]), s1[0]), s0[1]), s1[1]);
            }
            if constexpr (MASK) {
                const auto w = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);   // own 16 bits | the other half-wave's
                if (row_ok && h == 0) p.mask_out[(int64_t)m * p.ldmask + ((ncol0 + j * 32) >> 5)] = w[0] | w[1];
            }
        }
    }
    ovf_report(p.alpha_dev, ovf_hit<T>(ovf));
}

template <typename T, int FM, int FN, int AUXK>
__device__ __forceinline__ void nt_epilogue_rows(const NTParams& p, f32x16 (&acc)[FM][FN], int lane, int mrow0, int ncol0,
                                                 const uint32_t (&bits)[FM][FN]) {
    if (ncol0 >= p.N) return;                                   // wave-uniform: N is a multiple of the wave tile's width
    if (p.mask_out) nt_epilogue_rows_impl<T, FM, FN, AUXK, true>(p, acc, lane, mrow0, ncol0, bits);
    else nt_epilogue_rows_impl<T, FM, FN, AUXK, false>(p, acc, lane, mrow0, ncol0, bits);
}

// The S-stage ring of gemm_nt_kernel (see there) for f32h_t storage, with the loop's address work taken out of the vector unit: the
// fragment reads are a per-lane register plus the ring buffer's scalar offset, and where both operands fit 32-bit byte offsets (the
// phased kernels' launch guard) the DMA pieces go out as lds_dma16 - per-lane offsets that never change, the K-tile's byte offset and
// the LDS destination as scalars; operands beyond that keep their 64-bit per-lane addresses (lds_dma16_global).  Neither is the
// compiler's LDS-DMA builtin, so that the fragment reads' waits come out counted (see lds_dma16_global).
template <int WGM, int WGN, int FM, int FN, int RB, int S, int A_PASSES, int B_PASSES>
__device__ __forceinline__ void nt_h3_loop(const NTParams& p, char* smem, const char* const (&srcA)[A_PASSES], const char* const (&srcB)[B_PASSES],
                                           int lane, int wid, int wm, int wn, int nk, f32x16 (&acc)[FM][FN]) {
    constexpr int BM = WGM * FM * 32, BN = WGN * FN * 32, RPW = 64 / (RB / 16), RPP = WGM * WGN * RPW, P = A_PASSES + B_PASSES;
    constexpr int kBuf = (BM + BN) * RB;
    uint32_t fa[RB / 64][2], fb[RB / 64][2];
    Mma<f32h_t>::template frag_offsets<RB>(lane, (wm * FM * 32) * RB, (BM + wn * FN * 32) * RB, fa, fb);
    const bool fits32 = (int64_t)p.M * p.lda < (int64_t)0x7FFFFFFF && (int64_t)p.N * p.ldb < (int64_t)0x7FFFFFFF;
    const i32x4 rsA = raw_buffer(p.A), rsB = raw_buffer(p.B);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)smem + wid * RPW * RB);      // the wave's piece of pass 0
    uint32_t voffA[A_PASSES], voffB[B_PASSES];
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) voffA[i] = (uint32_t)(srcA[i] - p.A);
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) voffB[i] = (uint32_t)(srcB[i] - p.B);
    auto stage = [&](int t, int b) {                             // K-tile t into ring buffer b
        const uint32_t dst = lds0 + (uint32_t)b * kBuf;
        if (fits32) {
            const uint32_t soff = (uint32_t)t * RB;
            static_for<A_PASSES>([&](auto i) { lds_dma16<i.value * RPP * RB, true>(dst, voffA[i.value], rsA, soff); });
            static_for<B_PASSES>([&](auto i) { lds_dma16<(BM + i.value * RPP) * RB, true>(dst, voffB[i.value], rsB, soff); });
        } else {
            const int64_t koff = (int64_t)t * RB;
            static_for<A_PASSES>([&](auto i) { lds_dma16_global<i.value * RPP * RB>(dst, srcA[i.value] + koff); });
            static_for<B_PASSES>([&](auto i) { lds_dma16_global<(BM + i.value * RPP) * RB>(dst, srcB[i.value] + koff); });
        }
    };
#pragma unroll
    for (int t = 0; t < S - 1; ++t)
        if (t < nk) stage(t, t);
    __builtin_amdgcn_s_waitcnt(0xC07F);                          // lgkmcnt(0): no scalar load is pending inside the loop either
    int buf = 0, prev = S - 1;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + S - 2 < nk) wait_vmcnt<P*(S - 2)>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + S - 1 < nk) stage(kt + S - 1, prev);            // (kt + S - 1) % S = the buffer K-tile kt - 1 occupied
        Mma<f32h_t>::template tile<FM, FN, RB>(smem, (uint32_t)buf * kBuf, fa, fb, acc, p.sa);
        prev = buf;
        buf = (buf + 1 == S) ? 0 : buf + 1;
    }
}

// WPE = minimum waves per SIMD the register allocation must leave room for (k workgroups of T threads per CU <=> k T / 256)
// SW (bf16): swapped MFMA operands + row-per-lane epilogue (16-byte stores from registers, no LDS slab)
// FUSE: the epilogue's fused duties (nt_epilogue_impl), an instantiation of its own so that every other launch keeps its registers
template <typename T, int WGM, int WGN, int FM, int FN, int RB, int S, int WPE = 1, bool SW = false, bool FUSE = false>
__global__ __launch_bounds__(WGM * WGN * 64, WPE) void gemm_nt_kernel(NTParams p) {
    constexpr int BM = WGM * FM * 32, BN = WGN * FN * 32;
    constexpr int BK = RB / (int)sizeof(T);
    constexpr int LPR = RB / 16;                             // lanes (16-byte chunks) per staged row
    constexpr int RPW = 64 / LPR;                            // rows per wave-instruction of the DMA
    constexpr int RPP = WGM * WGN * RPW;                     // tile rows staged per pass
    constexpr int A_PASSES = BM / RPP, B_PASSES = BN / RPP;
    constexpr int P = A_PASSES + B_PASSES;                   // DMA instructions per lane per K-tile
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the rows staged per pass");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kBuf = (BM + BN) * RB;
    if (p.alpha_dev) p.alpha *= *p.alpha_dev;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int nwg = p.tiles_m * p.tiles_n;
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int bm0 = (tile / p.tiles_n) * BM, bn0 = (tile % p.tiles_n) * BN;

    // per-lane DMA sources: tile row RPP i + tid / LPR, LDS slot tid % LPR receives chunk slot ^ swz(row).
    // Rows past M / N are clamped to the last valid row: their products only reach output rows / columns that are
    // never stored.
    const int srow = tid / LPR, sslot = tid % LPR;
    const char* srcA[A_PASSES];
    const char* srcB[B_PASSES];
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
        const int r = i * RPP + srow;
        srcA[i] = p.A + (int64_t)min(bm0 + r, p.M - 1) * p.lda + ((sslot ^ lds_swz<RB>(r)) << 4);
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) {
        const int r = i * RPP + srow;
        srcB[i] = p.B + (int64_t)min(bn0 + r, p.N - 1) * p.ldb + ((sslot ^ lds_swz<RB>(r)) << 4);
    }
    char* const ldsA = smem + (wid * RPW) * RB;
    char* const ldsB = ldsA + BM * RB;

    f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // row-per-lane epilogue: the wave tile's mask words.  With a 2-stage ring every K-tile waits vmcnt(0), so the words
    // can be requested up front (they retire with the first K-tile wherever the compiler places the loads); deeper rings
    // use counted waits and fetch them after the loop.
    uint32_t row_bits[FM][FN];
    auto load_bits = [&]() {
        if (p.aux_mode == ASE_AUX_RELU_BITS && bn0 + wn * FN * 32 < p.N) {
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int m = min(bm0 + wm * FM * 32 + i * 32 + (lane & 31), p.M - 1);
                const int ma = (m >= p.aux_split) ? m - p.aux_delta : m;
                const uint32_t* w = reinterpret_cast<const uint32_t*>(p.aux + (int64_t)ma * p.ldaux) + ((bn0 + wn * FN * 32) >> 5);
#pragma unroll
                for (int j = 0; j < FN; ++j) row_bits[i][j] = w[j];
            }
        }
    };
    if constexpr (SW && S == 2) load_bits();

    // S-stage ring of LDS buffers, DMA prefetch distance S-1 tiles, ONE barrier per K-tile:
    //   wait (counted vmcnt: only the newest S-2 tiles may still be in flight) -> barrier (tile kt has landed for
    //   every wave AND every wave is done reading tile kt-1) -> issue the DMA of tile kt+S-1 into the buffer tile
    //   kt-1 occupied -> MFMAs on tile kt.
    const int nk = p.K / BK;
    if constexpr (std::is_same<T, f32h_t>::value) {
        nt_h3_loop<WGM, WGN, FM, FN, RB, S>(p, smem, srcA, srcB, lane, wid, wm, wn, nk, acc);
    } else {
#pragma unroll
        for (int t = 0; t < S - 1; ++t) {
            if (t < nk) {
                nt_stage<A_PASSES, RPP, RB>(srcA, (int64_t)t * RB, ldsA + t * kBuf);
                nt_stage<B_PASSES, RPP, RB>(srcB, (int64_t)t * RB, ldsB + t * kBuf);
            }
        }
        int buf = 0;
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + S - 2 < nk) wait_vmcnt<P*(S - 2)>();
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            if (kt + S - 1 < nk) {
                const int nb = (buf == 0) ? S - 1 : buf - 1;           // (kt + S - 1) % S
                nt_stage<A_PASSES, RPP, RB>(srcA, (int64_t)(kt + S - 1) * RB, ldsA + nb * kBuf);
                nt_stage<B_PASSES, RPP, RB>(srcB, (int64_t)(kt + S - 1) * RB, ldsB + nb * kBuf);
            }
            const char* sA = smem + buf * kBuf + (wm * FM * 32) * RB;
            const char* sB = smem + buf * kBuf + (BM + wn * FN * 32) * RB;
            if constexpr (SW && sizeof(T) == 2) Mma<T>::template tile<FM, FN, RB, true>(sA, sB, lane, acc);
            else Mma<T>::template tile<FM, FN, RB>(sA, sB, lane, acc);
            buf = (buf + 1 == S) ? 0 : buf + 1;
        }
    }
    if constexpr (SW) {
        if constexpr (S != 2) load_bits();
        if constexpr (sizeof(T) == 2) {
            if (p.aux_mode == ASE_AUX_RELU_BITS) nt_epilogue_rows<T, FM, FN, 2>(p, acc, lane, bm0 + wm * FM * 32, bn0 + wn * FN * 32, row_bits);
            else nt_epilogue_rows<T, FM, FN, 0>(p, acc, lane, bm0 + wm * FM * 32, bn0 + wn * FN * 32, row_bits);
        }
        return;
    }
    __syncthreads();                                   // everyone is done with the ring before it becomes the epilogue slab

    constexpr int FNC = (FN > 2) ? 2 : FN;
    float* slab = reinterpret_cast<float*>(smem) + wid * (FM * 32 * FNC * 32);
    const double sq = nt_epilogue<T, FM, FN, FM, FNC, FUSE>(p, acc, slab, lane, bm0 + wm * FM * 32, bn0 + wn * FN * 32);
    if constexpr (FUSE) {
        if (p.sq_acc) {                                // one f64 atomic per workgroup, as ase_hip_sqnorm (block_sum)
            const double w = wave_sum(sq);
            __syncthreads();                           // every wave is done with its slab
            double* red = reinterpret_cast<double*>(smem);
            if (lane == 0) red[wid] = w;
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
                for (int i = 0; i < WGM * WGN; ++i) t += red[i];
                double scale = p.sq_scale;
                if (p.sq_dyn) scale *= (double)*p.sq_dyn;
                atomic_add_f64(p.sq_acc, t * scale);
            }
        }
    }
}

template <typename T, int WGM, int WGN, int FM, int FN, int RB, int S, int WPE = 1, bool SW = false, bool FUSE = false>
int launch_nt(const NTParams& p0, hipStream_t stream) {
    constexpr int BM = WGM * FM * 32, BN = WGN * FN * 32;
    constexpr int ring = S * (BM + BN) * RB;
    constexpr int slab = WGM * WGN * (FM * 32) * ((FN > 2 ? 2 : FN) * 32) * 4;
    constexpr int lds = ring > slab ? ring : slab;
    static_assert(lds <= 160 * 1024, "LDS budget");
    constexpr auto kern = gemm_nt_kernel<T, WGM, WGN, FM, FN, RB, S, WPE, SW, FUSE>;
    if (const int rc = ase_dynamic_lds<kern>("gemm_nt", lds)) return rc;
    NTParams p = p0;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    ASE_LAUNCH(kern, dim3(p.tiles_m * p.tiles_n), dim3(WGM * WGN * 64), lds, stream, p);
    ASE_CHECK_LAUNCH("gemm_nt");
    return ASE_OK;
}

// ------------------------------------------------------------------------------------------------
// NT, phased 256 x 256 kernel (16-bit storage).  512 threads = 8 waves as 2 (M) x 4 (N); a wave owns 128 x 64 outputs =
// four 64 x 32 quadrants.  One K-tile (64 k-values, 128-byte rows, the swizzle of the kernel above) is FOUR phases, each
//     ds_read the fragments of one quadrant | counted vmcnt | s_barrier | lgkmcnt(0) | 8 MFMAs 32x32x16 with the two
//     global_load_lds of one 16-KiB DMA unit issued among them | s_barrier
// and the two wave groups (waves 0-3 / 4-7: the two waves of every SIMD sit in different groups) run ONE BARRIER
// APART, so that on each SIMD one wave is in its MFMA block while its partner reads LDS.
//   DMA units of K-tile t, in issue order = order of first use:
//     A0 = A rows {0-63, 128-191} (sub-tile 0 of both wave rows)     read in phase 0
//     B0 = B rows {64 c .. 64 c + 31, c = 0..3} (fragment 0 of every wave column)   phase 0 (kept in registers to phase 3)
//     B1 = B rows {64 c + 32 .. 64 c + 63}                            phase 1
//     A1 = A rows {64-127, 192-255}                                   phase 2
//   unit u = 4 t + kind is issued in phase (t', p) with 4 t' + p + 6 = u: six units ahead, into the buffer (t & 1) whose
//   previous occupant (K-tile t - 2) was last read >= 2 phases earlier (the WAR distance two staggered groups need);
//   a unit is read one phase after the counted wait + barrier that retires it (RAW across the stagger).  The DMA of a phase
//   goes out INSIDE its MFMA block (an LDS-DMA instruction costs ~60 issue cycles beside MFMAs - the matrix pipe stays fed
//   by the 32-cycle MFMA issue cadence - but 100-185 cycles in the read half of a phase, where it sat on the critical path
//   of the OTHER wave group's MFMA block): at the counted wait of a phase the newest issued unit is the one of the previous
//   phase, three units may stay in flight.
//   LDS balance (round 5, measured and NOT adopted): the fragment reads are 12 / 4 / 8 / 0 KB per wave over the four phases; reading
//   B fragment 0 of the next K-tile in phase 3 instead (8 / 4 / 8 / 4, 12 more registers) left the main loop where it was - 41831
//   against 41708 shader cycles for 16 K-tiles of 16384 x 1024 x 1024 (profiles/r05_nt8_lds_rebalance.txt): a phase costs ~650
//   cycles for 2 x 256 of MFMA issue, and the ~70 cycles per hand-over between the two wave groups (barrier release, lgkmcnt,
//   priority switch, the DMA issue inside the block) are what is left, not the LDS port.
//   (Round 2-4 ablations of this schedule - no DMA / no reads / no MFMAs / other MFMA shapes / DMA in the read half - lived
//   behind a lab switch in this file up to commit 9f99095; their results are in profiles/r03_lab_*.log, r04_lab_mfma_shape.txt.)
// ------------------------------------------------------------------------------------------------

// (DMA pieces: lds_dma16 in gemm_nt.h, like gemm_nt4.h and the TN twin)
struct NT8Lane {
    uint32_t voff[4][2];       // per-lane byte offset (row * ld + swizzled chunk) of unit kind x piece from its operand's base
    uint32_t dst[4][2];        // wave-uniform LDS byte ADDRESS of the piece in K-tile buffer 0 (buffer 1: + 65536)
    int roff[4];               // per-lane fragment read offsets (row * 128 + swizzled chunk) for the 4 k-steps
    i32x4 rsA, rsB;            // raw buffer descriptors of the two operands (SGPRs)
};

template <int KIND>
__device__ __forceinline__ void nt8_piece(const NT8Lane& L, int g, int tile) {
    constexpr bool isB = (KIND == 1 || KIND == 2);
    lds_dma16(__builtin_amdgcn_readfirstlane(L.dst[KIND][g] + (uint32_t)(tile & 1) * 65536u), L.voff[KIND][g], isB ? L.rsB : L.rsA,
              (uint32_t)tile * 128u);
}

template <int KIND>
__device__ __forceinline__ void nt8_issue(const NT8Lane& L, int tile) {
#pragma unroll
    for (int g = 0; g < 2; ++g) nt8_piece<KIND>(L, g, tile);
}

// fragment registers of one 32-row operand block: 4 k-steps x 16 bytes
__device__ __forceinline__ void nt8_read(i32x4 (&f)[4], const char* base, const NT8Lane& L) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = *reinterpret_cast<const i32x4*>(base + L.roff[ks]);
}

// the 8 MFMAs of a phase with the two DMA pieces of unit KIND (K-tile `tile`) issued among them, and the phase's CLOSING barrier
// in front of the last MFMA pair: every s_barrier of the loop is the end of one wave group's MFMA block and the start of the
// other's, and between the first group's last MFMA issue and the second group's first one lie the barrier's release, an lgkmcnt
// wait and a priority switch (~70 of the ~650 cycles a phase took, round 5's cycle stamps).  With two MFMAs (64 cycles of
// matrix-pipe work) still to issue behind the barrier, the pipe stays fed across the hand-over.  Nothing those two MFMAs touch
// is shared: their operands are in registers since the phase's first barrier.
// NA = 1 (the 192 x 256 tile's third A block): 4 MFMAs of a0 on c0 alone, same DMA / barrier placement; c1 and a1 are not touched.
// (accumulators by reference: handed over as the array and two indices hipcc moved the 256-row kernels' accumulator registers)
template <typename T, int KIND, bool SW, int NA = 2>
__device__ __forceinline__ void nt8_mma_issue(f32x16& c0, f32x16& c1, const i32x4 (&a0)[4], const i32x4 (&a1)[4],
                                              const i32x4 (&b)[4], const NT8Lane& L, int tile, bool live) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        if (ks == 3) NT8_BARRIER();                       // (closes the phase: see above)
        c0 = nt8_mfma<T, SW>(a0[ks], b[ks], c0);
        if constexpr (NA == 2) c1 = nt8_mfma<T, SW>(a1[ks], b[ks], c1);
        if (ks == 0 || ks == 2) {
            __builtin_amdgcn_sched_barrier(0);
            if (live) nt8_piece<KIND>(L, ks >> 1, tile);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
}

// one K-tile = 4 phases.  TAIL = false: every issued unit exists (t + 2 < nk) and the waits are compile-time counts.
// NI = 4: wave tile 128 x 64 (256 x 256 tile); NI = 3: wave tile 96 x 64 (192 x 256 tile) - phases 2 and 3 multiply ONE A block
template <typename T, bool TAIL, bool SW, int NI = 4>
__device__ __forceinline__ void nt8_ktile(int t, int nk, const NT8Lane& L, const char* aP, const char* bP,
                                          f32x16 (&acc)[NI][2], i32x4 (&a0)[4], i32x4 (&a1)[4], i32x4 (&b0)[4],
                                          i32x4 (&b1)[4]) {
    constexpr int RB = 128;
    const int U = 4 * nk;
    const bool l1 = !TAIL || t + 1 < nk, l2 = !TAIL || t + 2 < nk;
    // ---- phase 0: A sub-tile 0, B fragment 0 -> quadrant (0, 0); issues B1 of K-tile t + 1
    nt8_read(b0, bP, L);
    nt8_read(a0, aP, L);
    nt8_read(a1, aP + 32 * RB, L);
    if (!TAIL) wait_dma_units<3>();
    else wait_dma_units_rt(min(U, 4 * t + 6) - (4 * t + 3));
    nt8_sync_in();
    nt8_mma_issue<T, 2, SW>(acc[0][0], acc[1][0], a0, a1, b0, L, t + 1, l1);
    // ---- phase 1: B fragment 1 -> quadrant (0, 1); issues A1 of K-tile t + 1
    nt8_read(b1, bP + 32 * RB, L);
    if (!TAIL) wait_dma_units<3>();
    else wait_dma_units_rt(min(U, 4 * t + 7) - (4 * t + 4));
    nt8_sync_in();
    nt8_mma_issue<T, 3, SW>(acc[0][1], acc[1][1], a0, a1, b1, L, t + 1, l1);
    // ---- phase 2: A sub-tile 1 -> quadrant (1, 1); issues A0 of K-tile t + 2
    nt8_read(a0, aP + 64 * RB, L);
    if constexpr (NI == 4) nt8_read(a1, aP + 96 * RB, L);
    nt8_sync_in();
    nt8_mma_issue<T, 0, SW, NI - 2>(acc[2][1], acc[NI - 1][1], a0, a1, b1, L, t + 2, l2);     // (NI = 3: acc[2] alone)
    // ---- phase 3: quadrant (1, 0); issues B0 of K-tile t + 2; the wait retires A0 / B0 of K-tile t + 1 for the next phase 0
    if (!TAIL) wait_dma_units<3>();
    else if (t + 1 < nk) wait_dma_units_rt(min(U, 4 * t + 9) - (4 * t + 6));
    nt8_sync_in();
    nt8_mma_issue<T, 1, SW, NI - 2>(acc[2][0], acc[NI - 1][0], a0, a1, b0, L, t + 2, l2);
}


// SW: swapped MFMA operands + row-per-lane epilogue (nt8_epilogue_rows), else the LDS-slab epilogue
// BM = 192 (row-per-lane epilogue only): the same schedule on a 192 x 256 tile - wave tile 96 x 64, phases 2 / 3 are 4 MFMAs - for
// row counts whose 256-row tiling leaves a quarter of the CUs idle (12288 x 1024: 192 tiles of 256 rows, 256 tiles of 192).  The
// K-tile buffers keep their 64-KiB stride and B keeps following A (offset BM * 128); unit A1 covers rows 64-95 of BOTH wave rows
// with one piece, its second piece repeats the first (same bytes, same place) so that the counted waits stay what they are.
// STK (SW, 256-row tiles): the stacked form - two row blocks with an epilogue each in one launch.  stack_split is a multiple of the tile's
// 256 rows, so every workgroup lies wholly in one block and takes that block's duties at its entry by rewriting the (scalar) parameter
// fields; nothing further down knows about it, except that the mask operand has M - stack_split rows.  An instantiation of its own:
// every other launch keeps its registers.
template <typename T, bool SW, int BM = 256, bool STK = false>
__global__ __launch_bounds__(512) void gemm_nt8_kernel(NTParams p) {
    static_assert(sizeof(T) == 2, "the phased kernel takes the 16-bit storage types");
    static_assert(BM == 256 || (BM == 192 && SW), "192-row tiles come with the row-per-lane epilogue");
    static_assert(!STK || (SW && BM == 256), "the stacked form comes with the row-per-lane epilogue on 256-row tiles");
    constexpr int RB = 128, BN = 256, BK = 64, WM = BM / 2, NI = WM / 32;
    constexpr int kBuf = 512 * RB;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (!STK) {
        if (p.alpha_dev) p.alpha *= *p.alpha_dev;
    }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3;
    const int nwg = p.tiles_m * p.tiles_n;
    const int tile = xcd_remap(blockIdx.x, nwg);
    const int bm0 = (tile / p.tiles_n) * BM, bn0 = (tile % p.tiles_n) * BN;
    if constexpr (STK) {
        if (bm0 >= p.stack_split) {          // workgroup-uniform: the second block's duties
            p.bias = nullptr;
            p.act = ASE_ACT_NONE;
            p.mask_out = nullptr;
            p.alpha = p.alpha2;
            p.alpha_dev = p.alpha_dev2;
        } else {
            p.aux_mode = ASE_AUX_NONE;       // the mask operand belongs to the second block
        }
        if (p.alpha_dev) p.alpha *= *p.alpha_dev;
    }

    NT_PROF_STAMP(p.prof, tid, blockIdx.x * 4 + 0, false);
    NT8Lane L;
    {
        const int lr = lane >> 3, slot = lane & 7;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int ra = g * WM + wid * 8;                            // A0 piece (A1 of the 256-row tile: + 64)
            const int rb = (g * 2 + (wid >> 2)) * 64 + (wid & 3) * 8;   // B0 piece (B1: + 32)
            const int ra1 = BM == 256 ? ra + 64 : (wid >> 2) * WM + 64 + (wid & 3) * 8;
            const int rows[4] = {ra, rb, rb + 32, ra1};                 // kind 0..3 = A0, B0, B1, A1
#pragma unroll
            for (int kind = 0; kind < 4; ++kind) {
                const int r = rows[kind] + lr;
                const bool isB = (kind == 1 || kind == 2);
                const int64_t grow = isB ? min(bn0 + r, p.N - 1) : min(bm0 + r, p.M - 1);
                L.voff[kind][g] = (uint32_t)(grow * (isB ? p.ldb : p.lda)) + (uint32_t)((slot ^ lds_swz<RB>(r)) << 4);
                L.dst[kind][g] = (uint32_t)(uintptr_t)smem + (isB ? BM * RB : 0) + rows[kind] * RB;
            }
        }
        const int r = lane & 31, h = lane >> 5, sw = lds_swz<RB>(r);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) L.roff[ks] = r * RB + (((ks * 2 + h) ^ sw) << 4);
        // whole operands as raw buffers (rows past M / N are clamped in the per-lane offsets above)
        L.rsA = raw_buffer(p.A);
        L.rsB = raw_buffer(p.B);
    }

    f32x16 acc[NI][2];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // the first chunk's mask words (16 registers) are fetched before anything else: older than every DMA, they retire
    // first and the epilogue finds them in registers instead of waiting an HBM round trip after the last K-tile
    AuxReg<T, 2> pre_bits[16];
    uint32_t row_bits[NI][2];
    if constexpr (!SW) {
        if (p.aux_mode == ASE_AUX_RELU_BITS) nt_aux_load<T, 4, 2, 2, 2, 2>(p, 0, lane, bm0 + wr * WM, bn0 + wc * 64, pre_bits);
    }

    const int nk = p.K / BK;
    // prologue: units 0..5 (K-tile 0 and A0, B0 of K-tile 1); A0 / B0 of K-tile 0 must have landed for phase 0
    nt8_issue<0>(L, 0);
    nt8_issue<1>(L, 0);
    nt8_issue<2>(L, 0);
    nt8_issue<3>(L, 0);
    if (nk > 1) {
        nt8_issue<0>(L, 1);
        nt8_issue<1>(L, 1);
    }
    bool mask_dma = false;
    if constexpr (SW) {
        // row-per-lane epilogue: the mask words of the wave tile (128 rows x 2 words) travel as four 4-byte DMA pieces
        // BEHIND the prologue's units into 1 KiB of LDS per wave past the ring (as ordinary loads in front of the DMA
        // queue they add an exposed HBM round trip to the prologue, 3.1 vs 1.4 us; as ordinary loads behind it their
        // position in the vmcnt queue would be the compiler's choice).  Lane (r, h) fetches word h of row 32 i + r;
        // the first counted wait of the main loop retires them.
        mask_dma = p.aux_mode == ASE_AUX_RELU_BITS && bn0 + wc * 64 < p.N;
        if (mask_dma) {
            char* mlds = smem + 2 * kBuf + wid * 1024;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int m = bm0 + wr * WM + i * 32 + (lane & 31);
                int ma;
                if constexpr (STK) ma = min(m, p.M - 1) - p.stack_split;     // (the mask has M - stack_split rows: clamp FIRST)
                else ma = min((m >= p.aux_split) ? m - p.aux_delta : m, p.M - 1);
                const uint32_t* w = reinterpret_cast<const uint32_t*>(p.aux + (int64_t)ma * p.ldaux) +
                                    ((bn0 + wc * 64) >> 5) + (lane >> 5);
                __builtin_amdgcn_global_load_lds((gptr_t*)w, (lptr_t*)(mlds + i * 256), 4, 0, 0);
            }
        }
    }
    // units 0, 1 (A0 / B0 of K-tile 0) must have landed; the mask pieces (if any) are the NI youngest entries of the queue
    if (nk > 1) {
        if (mask_dma) wait_vmcnt<8 + NI>(); else wait_dma_units<4>();
    } else {
        if (mask_dma) wait_vmcnt<4 + NI>(); else wait_dma_units<2>();
    }
    NT8_BARRIER();
    NT_PROF_STAMP(p.prof, tid, blockIdx.x * 4 + 1, p.prof_clk);
    if (wr == 1) NT8_BARRIER();                  // the second wave group runs one barrier behind

    i32x4 a0[4], a1[4], b0[4], b1[4];
    const int aoff = wr * WM * RB, boff = BM * RB + wc * 64 * RB;
    int t = 0;
    for (; t + 2 < nk; ++t) {
        const char* buf = smem + (t & 1) * kBuf;
        nt8_ktile<T, false, SW, NI>(t, nk, L, buf + aoff, buf + boff, acc, a0, a1, b0, b1);
    }
    for (; t < nk; ++t) {
        const char* buf = smem + (t & 1) * kBuf;
        nt8_ktile<T, true, SW, NI>(t, nk, L, buf + aoff, buf + boff, acc, a0, a1, b0, b1);
    }
    if (wr == 0) NT8_BARRIER();
    __syncthreads();                             // the ring becomes the epilogue slab
    NT_PROF_STAMP(p.prof, tid, blockIdx.x * 4 + 2, p.prof_clk);

    float* slab = reinterpret_cast<float*>(smem) + wid * (64 * 64);
    if constexpr (SW) {
        if (p.aux_mode == ASE_AUX_RELU_BITS) {
            const uint32_t* mw = reinterpret_cast<const uint32_t*>(smem + 2 * kBuf + wid * 1024);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                row_bits[i][0] = mw[i * 64 + (lane & 31)];
                row_bits[i][1] = mw[i * 64 + 32 + (lane & 31)];
            }
            nt8_epilogue_rows<T, 2, 2, NI>(p, acc, lane, bm0 + wr * WM, bn0 + wc * 64, row_bits);
        } else nt8_epilogue_rows<T, 0, 2, NI>(p, acc, lane, bm0 + wr * WM, bn0 + wc * 64, row_bits);
    } else if constexpr (BM == 256) {
        if (p.aux_mode == ASE_AUX_RELU_BITS)
            nt_epilogue_impl<T, 4, 2, 2, 2, 2, true>(p, acc, slab, lane, bm0 + wr * 128, bn0 + wc * 64, &pre_bits);
        else
            nt_epilogue<T, 4, 2, 2, 2>(p, acc, slab, lane, bm0 + wr * 128, bn0 + wc * 64);
    }
    NT_PROF_CLOSE(p.prof, tid, blockIdx.x * 4 + 3);
}

template <typename T, bool SW = false, int BM = 256, bool STK = false> int launch_nt8(const NTParams& p0, hipStream_t stream) {
    constexpr int lds = 2 * 512 * 128 + (SW ? 8 * 1024 : 0);     // ring + (row-per-lane epilogue) 1 KiB of mask words per wave
    constexpr auto kern = gemm_nt8_kernel<T, SW, BM, STK>;
    if (const int rc = ase_dynamic_lds<kern>("gemm_nt8", lds)) return rc;
    NTParams p = p0;
    p.prof = g_nt_prof;
    p.prof_clk = g_nt_prof_clk;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + 255) / 256;
    ASE_LAUNCH(kern, dim3(p.tiles_m * p.tiles_n), dim3(512), lds, stream, p);
    ASE_CHECK_LAUNCH("gemm_nt8");
    return ASE_OK;
}

}  // namespace
#include "gemm_nt4.h"
namespace {

// row-per-lane epilogue (swapped MFMA operands): 16-bit output in whole wave-tile column blocks, no column sums, no tanh,
// mask operand absent or a bit matrix; a mask_out twin only behind ReLU (rows_frag forms its bit from the clamped 16-bit pattern -
// any other activation takes the LDS-slab epilogue, which compares the stored value with 0)
inline bool rows_epi(const NTParams& p, int wave_cols) {
    return !p.out_f32 && p.N % wave_cols == 0 && p.colsum == nullptr && p.act <= ASE_ACT_RELU &&
           (p.mask_out == nullptr || p.act == ASE_ACT_RELU) &&
           (p.aux_mode == ASE_AUX_NONE || p.aux_mode == ASE_AUX_RELU_BITS);
}

template <typename T> int dispatch_nt(const NTParams& p, hipStream_t s) {
    const bool k128 = (p.K * (int)sizeof(T)) % 128 == 0;       // 128-byte staged rows need K in whole 128-byte steps
    // (the phased kernels and the 4-wave kernel address their operands with 32-bit byte offsets from the base: < 2 GiB each)
    const bool fits32 = (int64_t)p.M * p.lda < (int64_t)0x7FFFFFFF && (int64_t)p.N * p.ldb < (int64_t)0x7FFFFFFF;
    int choice = nt_choice(p.M, p.N, p.K, (int)sizeof(T), sizeof(T) == 2);
    if ((choice == 2 || choice == 6) && !fits32) choice = 3;
    if constexpr (std::is_same<T, f32h_t>::value) {
        if (p.seed_w || p.twin || p.sq_acc) {        // the fused epilogue duties: the same tiles, their own instantiations
            switch (choice) {
                case 0: return launch_nt<T, 2, 2, 1, 1, 64, 4, 1, false, true>(p, s);
                case 2: case 3: case 6:
                    if (k128) return launch_nt<T, 4, 2, 2, 4, 128, 2, 1, false, true>(p, s);
                    return launch_nt<T, 4, 2, 2, 4, 64, 4, 1, false, true>(p, s);
                case 4: return launch_nt<T, 2, 2, 1, 2, 128, 2, 2, false, true>(p, s);
                case 5: return launch_nt<T, 2, 2, 1, 1, 128, 4, 2, false, true>(p, s);
                default:
                    // (two workgroups per CU asked for: the plain instantiation gets there by itself, 252 registers)
                    if (k128) return launch_nt<T, 2, 2, 2, 2, 128, 2, 2, false, true>(p, s);
                    return launch_nt<T, 2, 2, 2, 2, 64, 4, 2, false, true>(p, s);
            }
        }
    }
    switch (choice) {
        case 0: return launch_nt<T, 2, 2, 1, 1, 64, 4>(p, s);
        case 6:
            if constexpr (sizeof(T) == 2) if (rows_epi(p, 64)) return launch_nt8<T, true, 192>(p, s);
            [[fallthrough]];
        case 2:
            if constexpr (sizeof(T) == 2) {
                // row-per-lane epilogue (swapped MFMA operands): 16-bit output in whole 64-column wave tiles, no column sums,
                // mask operand absent or a bit matrix; otherwise the LDS-slab epilogue
                // The 4-wave kernel (gemm_nt4.h: whole 128-column wave tiles, operands a 32-bit byte offset reaches) takes the launches of
                // MANY rounds that run with nothing beside them - the epoch tail's reward inference over the whole experience buffer
                // (131072 rows: 324 vs 344 us).  Inside an optimisation step it stays out although it is 4-8 % faster launch by launch
                // (profiles/r06_nt4_lab.txt): its workgroup owns the CU's whole register file (4 waves x 512), the 8-wave kernel leaves
                // 32 registers per SIMD, and in the four-stream step the small HBM-bound kernels of the other branches (<= 32 VGPRs:
                // gathers, conversions, loss heads) run in exactly that space - same-box A/B of the update: 77.5 ms with the 8-wave
                // kernel, 79.3 ms with this one (profiles/r06_nt_policy_ab.txt).
                if (p.M >= 65536 && rows_epi(p, 128)) return launch_nt4<T>(p, s);
                if (rows_epi(p, 64)) return launch_nt8<T, true>(p, s);
                return launch_nt8<T, false>(p, s);
            }
            [[fallthrough]];
        case 3:
            if (k128) return launch_nt<T, 4, 2, 2, 4, 128, 2>(p, s);
            return launch_nt<T, 4, 2, 2, 4, 64, 4>(p, s);                 // 64-byte rows, 4-stage ring (128 KB)
        case 4:
            if constexpr (sizeof(T) == 2) if (rows_epi(p, 64)) return launch_nt<T, 2, 2, 1, 2, 128, 2, 2, true>(p, s);
            return launch_nt<T, 2, 2, 1, 2, 128, 2, 2>(p, s);            // 64 x 128 tile (K in whole 128-byte steps)
        case 5:
            if constexpr (sizeof(T) == 2) if (rows_epi(p, 32)) return launch_nt<T, 2, 2, 1, 1, 128, 4, 2, true>(p, s);
            return launch_nt<T, 2, 2, 1, 1, 128, 4, 2>(p, s);            // 64 x 64 tile, 128-byte rows, 4 stages
        default:
            if constexpr (sizeof(T) == 2) if (k128 && rows_epi(p, 64)) return launch_nt<T, 2, 2, 2, 2, 128, 2, 1, true>(p, s);
            if (k128) return launch_nt<T, 2, 2, 2, 2, 128, 2>(p, s);
            return launch_nt<T, 2, 2, 2, 2, 64, 4>(p, s);                 // 64-byte rows, 4-stage ring (64 KB)
    }
}

// the stacked form as ONE launch (ase_hip_gemm_nt_stacked has checked: kernel 2 of a 16-bit shape, stack_split in whole 256-row tiles,
// operands a 32-bit byte offset reaches, fewer than 65536 rows)
template <typename T> int dispatch_nt_stacked(const NTParams& p, hipStream_t s) { return launch_nt8<T, true, 256, true>(p, s); }

}  // namespace
