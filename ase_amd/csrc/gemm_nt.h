// Pieces of the NT matrix-core kernels (gfx950) kept in a header: tile order, LDS swizzle, launch
// parameters, the MFMA wrapper with swapped operands and the row-per-lane epilogue of the phased kernels.
#pragma once
#include "common.h"
#include "act.h"
#include <type_traits>

namespace ase_nt {


// Bijective XCD-aware remap: workgroup b runs on XCD b % 8; give each XCD a contiguous tile range.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + loc;
}


// LDS rows are RB = 64 or 128 bytes, unpadded; chunk c (16 B) of row r lives at slot c ^ swz(r):
//   RB = 128: swz = (r >> 1) & 7   (a 256-byte bank window holds 2 rows x 8 slots)
//   RB =  64: swz = (r >> 2) & 3   (4 rows x 4 slots)
// either way the 16 rows (distinct mod 16) of a ds_read_b128 lane group land on 16 distinct slots.
template <int RB> __device__ __forceinline__ int lds_swz(int r) { return RB == 128 ? ((r >> 1) & 7) : ((r >> 2) & 3); }

typedef __attribute__((address_space(1))) const void gptr_t;
typedef __attribute__((address_space(3))) void lptr_t;

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

struct NTParams {
    const char* A; int64_t lda;     // leading dims in BYTES
    const char* B; int64_t ldb;
    char* C; int64_t ldc;           // bytes
    const float* bias;
    const char* aux; int64_t ldaux; // bytes
    int aux_split, aux_delta;       // rows m >= aux_split read aux row m - aux_delta (stacked row blocks sharing a mask)
    float* colsum; int colsum_n;
    uint32_t* mask_out; int64_t ldmask;   // nullable: bit (m, n) = stored value > 0, 32 columns per word, ldmask in words
    char* pre_out; int64_t ldpre;         // nullable (smooth activations): the pre-activation z in the storage type, ldpre in bytes
    int M, N, K;                    // K in elements (multiple of 128/sizeof(T))
    int act, aux_mode, out_f32;
    float alpha;
    float* alpha_dev;               // nullable: device record {factor, overflow count} (ase_hip.h "scale records"): factor is multiplied into
                                    // alpha when the launch runs (the dynamic loss scale), and the launch adds to the count when an
                                    // element it stored was non-finite or sat at the storage type's saturation value
    float sa;                       // f32h_t storage: power-of-two scale of the A operand before its half split (B arrives pre-split and
                                    // pre-scaled; alpha undoes both scales)
    int tiles_m, tiles_n;
    unsigned long long* prof;       // debug: per-workgroup phase timestamps (ase_hip_debug_nt_profile), else null
    int prof_clk;                   // debug: stamps 1 and 2 (main loop) in shader clocks instead of the 100 MHz clock
    // ---- fused duties of the f32h_t epilogue (ase_hip_gemm_nt_ex; the FUSE instantiations of gemm_nt_kernel read them, nobody else) ----
    const float* seed_w; int seed_n; float seed_scale;   // nullable: C[m, n] = seed_scale * seed_w[n] * (act(z) > 0 ? 1 : 0) instead of
                                                         // the activation (ase_hip_gp_seed's product; columns >= seed_n: 0)
    char* twin; int64_t ldtwin; int twin_dtype;          // nullable: the stored value once more, from_f32<f16 / bf16> (ldtwin in bytes);
                                                         // with a twin C may be null (no f32 store)
    double* sq_acc; double sq_scale; const float* sq_dyn;   // nullable: *sq_acc += sq_scale * sq_dyn[0] * sum of the stored values' squares
    // ---- stacked form (ase_hip_gemm_nt_stacked; the STK instantiation of gemm_nt8_kernel reads them, nobody else): rows >= stack_split
    // are a second row block with duties of its own - no bias, no activation, no mask_out, alpha2 / alpha_dev2 - and they alone take
    // the mask operand (aux / aux_mode, read at row m - stack_split); bias, act, mask_out, alpha, alpha_dev belong to the first block
    int stack_split;
    float alpha2;
    float* alpha_dev2;
};


typedef __attribute__((ext_vector_type(4))) int i32x4;

// ---- LDS-DMA of the phased kernels and the 4-wave kernel (NT and TN) --------------------------------------------------
// DMA pieces go out as `buffer_load_dwordx4 ... lds` (round 6): an SGPR buffer descriptor per operand, ONE 32-bit offset register per
// piece (the 64-bit per-lane addresses of global_load_lds cost 16 registers and two VALU adds per piece), the K-tile's byte offset as
// the instruction's SGPR offset, M0 = LDS destination.  What it buys is REGISTERS: the kernel's allocation decides how many of the 512
// registers per SIMD its two waves leave to the small HBM-bound kernels of the step's other branches, which run in exactly that space
// (profiles/r06_nt_policy_ab.txt: a matrix kernel that owns the whole file costs the update 2.2 %).
//
// a whole operand as a raw buffer: stride 0, byte extent 2^31 - 1, 32-bit data format (rows past the operand are clamped in the
// callers' per-lane offsets, not by the descriptor)
__device__ __forceinline__ i32x4 raw_buffer(const void* base) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    return i32x4{(int)(uint32_t)a, (int)(uint32_t)(a >> 32), (int)0x7FFFFFFF, 0x00020000};
}
// one DMA piece of 64 lanes x 16 bytes: lane l reads rs base + voff + soff and lands at LDS byte address M0 + 16 l.
// M0 = the wave-uniform lds_s (s_mov_b32), or lds_s + IMM with ADD (s_add_u32, which also writes SCC; ADD with IMM = 0 stays an
// s_add_u32).  M0 is written and read inside ONE statement and declared clobbered: the same kernels fetch their mask words with
// __builtin_amdgcn_global_load_lds, whose M0 the compiler manages itself and may otherwise keep live across this statement.
// (hipcc reserves M0 and warns about the clobber - "may not be preserved across the asm statement", which is exactly what is declared)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define LDS_DMA16_ASM(SET_M0, ...)                                            \
    asm volatile(SET_M0 "\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"          \
                 :                                                              \
                 : "s"(lds_s), "v"(voff), "s"(rs), "s"(soff), "n"(IMM)          \
                 : "memory", "m0", ##__VA_ARGS__)
template <int IMM = 0, bool ADD = (IMM != 0)>
__device__ __forceinline__ void lds_dma16(uint32_t lds_s, uint32_t voff, i32x4 rs, uint32_t soff) {
    if constexpr (ADD) LDS_DMA16_ASM("s_add_u32 m0, %0, %4", "scc");
    else LDS_DMA16_ASM("s_mov_b32 m0, %0");
}
#undef LDS_DMA16_ASM
// the same piece from a 64-bit per-lane address (operands a 32-bit byte offset does not reach): M0 = lds_s + IMM.  As an asm statement
// and not __builtin_amdgcn_global_load_lds, which the compiler books as a flat access of both address spaces - while one is pending by
// its count (the kernels wait for their DMA with vmcnt of their own, which it does not see) every LDS wait it emits is lgkmcnt(0).
template <int IMM>
__device__ __forceinline__ void lds_dma16_global(uint32_t lds_s, const char* src) {
    asm volatile("s_add_u32 m0, %0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(lds_s), "v"(src), "n"(IMM) : "memory", "m0", "scc");
}
#pragma clang diagnostic pop

// SW: operands swapped in the MFMA (D = B-fragment x A-fragment): the accumulator then holds the TRANSPOSED 32 x 32
// block - a lane owns one output ROW and 4 x 4 consecutive columns - which nt8_epilogue_rows stores straight from
// registers (no LDS transposition).
template <typename T, bool SW>
__device__ __forceinline__ f32x16 nt8_mfma(const i32x4& a, const i32x4& b, const f32x16& c) {
    typedef typename V16<T>::x8 x8;
    if constexpr (SW) return mfma16<T>(__builtin_bit_cast(x8, b), __builtin_bit_cast(x8, a), c);
    else return mfma16<T>(__builtin_bit_cast(x8, a), __builtin_bit_cast(x8, b), c);
}


#define NT8_BARRIER()                        \
    do {                                     \
        __builtin_amdgcn_sched_barrier(0);   \
        __builtin_amdgcn_s_barrier();        \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)


// ---- row-per-lane epilogues (swapped MFMA operands): one 32 x 32 accumulator fragment of a lane = 16 outputs of ONE row, the columns
// 8 g + 4 h + q (g = e >> 2, q = e & 3, h = lane >> 5).  Two outputs at a time on the packed instructions of gfx950:
//     v_pk_fma_f32 (alpha * acc + bias) -> [bit-mask operand: v_bfe_i32 + v_and per output] -> v_cvt_pk_{bf16,f16}_f32 ->
//     ReLU as an IEEE-754 maximum, which KEEPS a NaN (torch.relu; v_pk_max_i16 on the packed patterns turned a NaN with the sign set
//     into 0): bf16 v_maximum3_f32 before the conversion, f16 v_pk_minimum3_f16 / v_pk_maximum3_f16 after it (they are its saturation
//     too - the same stored value as from_f32<f16_t> for every non-NaN input, see cvt_relu_pk16) ->
//     [mask_out: "0 < stored <= inf" on the patterns (v_pk_sub_u16, v_pk_sub_u16 clamp, v_pk_min_u16), v_pk_lshlrev_b16 to its bit, v_or]
// i.e. ~4 VALU operations per output (~3 with the integer ReLU, which dropped NaNs) where the scalar form of rounds 2-5 (per output: fma, max, select on the runtime activation
// code, a one-sided cvt_pk + shift + or to pack, compare + select + shift-or for the mask bit) cost 8-10 - with ONE wave per SIMD
// (or two in lock-step) nothing overlaps the epilogue, and at 256 outputs per lane it was 5-6 us of a 35-us launch (round 6).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// max(v, lo) and the conversion of two outputs; lo = 0 (ReLU) or -inf (none).  A NaN stays a NaN in both storage types.
template <typename T> __device__ __forceinline__ uint32_t cvt_relu_pk16(f32x2 v, float lo);
template <> __device__ __forceinline__ uint32_t cvt_relu_pk16<bf16_t>(f32x2 v, float lo) {      // RNE
    const f32x2 l = {lo, lo};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(__builtin_elementwise_maximum(v, l), bf16x2));
}
// RNE, saturating at +-65504: rounding first and clamping the half stores what from_f32<f16_t> (clamp, then round) stores - a value in
// (65504, 65520) rounds to 65504 either way, one from 65520 on rounds to inf and is clamped back
template <> __device__ __forceinline__ uint32_t cvt_relu_pk16<f16_t>(f32x2 v, float lo) {
    const f16_t l16 = (f16_t)__builtin_amdgcn_fmed3f(lo, -65504.f, 65504.f);
    const f16x2 hi = {(f16_t)65504.f, (f16_t)65504.f}, l = {l16, l16};
    const f16x2 c = __builtin_elementwise_maximum(__builtin_elementwise_minimum(__builtin_convertvector(v, f16x2), hi), l);
    return __builtin_bit_cast(uint32_t, c);
}

// ---- overflow detection of the dynamic loss scale, fused into the producers (round 6; rounds 4-5 re-read every half buffer of the step,
// 0.82 GB, with ase_hip_scaler_check): a launch that was given a scale record reports an element it STORED that is non-finite or sits at
// the storage type's saturation value (f16 conversions saturate at +-65504 where autocast would produce inf; bf16 goes to inf).  On the
// packed 16-bit patterns: |x| as an unsigned integer orders like the magnitude, so one v_and + one v_pk_max_u16 per two outputs keep a
// running maximum and ONE comparison per lane at the end of the epilogue decides.
// (as an asm statement: written with __builtin_elementwise_max hipcc re-associated the running maximum of an epilogue into a tree over
//  all of a row block's outputs - 33 more live registers in a kernel whose 217 leave the 64 its co-resident neighbours run in)
__device__ __forceinline__ uint32_t ovf_fold(uint32_t run, uint32_t packed) {
    const uint32_t mag = packed & 0x7FFF7FFFu;
    asm("v_pk_max_u16 %0, %0, %1" : "+v"(run) : "v"(mag));
    return run;
}
template <typename T> __device__ __forceinline__ bool ovf_hit(uint32_t run) {
    return (run & 0xFFFFu) >= ovf_threshold<T>() || (run >> 16) >= ovf_threshold<T>();
}

// bias: the lane's 16 bias values of the fragment as 4 x f32x4 (columns 8 g + 4 h ..); w: the fragment's mask word >> 4 h (AUXK = 2);
// relu_lo: lower bound of the stored value (0 = ReLU, -inf = none); pk[g][0 / 1]: the packed outputs q = 0, 1 / 2, 3;
// returns (MASK) the lane's 16 "stored > 0" bits at their places 8 g + 4 h + q of the fragment's 32-bit mask word
template <typename T, int AUXK, bool MASK>
__device__ __forceinline__ uint32_t rows_frag(const f32x16& c, const f32x4 (&bias)[4], uint32_t w, f32x2 al, float relu_lo, int h,
                                              uint32_t (&pk)[4][2]) {
    uint32_t mlo = 0, mhi = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            f32x2 v = {c[g * 4 + 2 * pr], c[g * 4 + 2 * pr + 1]};
            const f32x2 b = {bias[g][2 * pr], bias[g][2 * pr + 1]};
            v = v * al + b;
            if constexpr (AUXK == 2) {
                // (as ONE vector AND: written per element - v[0] = ..., v[1] = ... - hipcc 7.2 folded the two ANDs into a v_bitop3 that
                //  multiplied element 0 into element 1; caught by the bit-mask tests of round 6)
                const i32x2 keep = {(int)__builtin_amdgcn_sbfe(w, 8 * g + 2 * pr, 1), (int)__builtin_amdgcn_sbfe(w, 8 * g + 2 * pr + 1, 1)};
                v = __builtin_bit_cast(f32x2, __builtin_bit_cast(i32x2, v) & keep);
            }
            pk[g][pr] = cvt_relu_pk16<T>(v, relu_lo);
            if constexpr (MASK) {       // assumes ReLU (a pattern is +0 ... +inf or a NaN): rows_epi() sends every other mask_out launch to the slab
                // 1 where the stored value is > 0, i.e. pattern - 1 < the pattern of +inf (unsigned: +0 wraps; a NaN of either sign is
                // above), as inf - (pattern - 1) saturating at 0, then min with 1
                // (as asm statements: written with __builtin_elementwise_sub_sat / _min hipcc turned the three packed operations into a
                //  compare + select per 16-bit half)
                constexpr uint32_t INF = std::is_same<T, f16_t>::value ? 0x7C007C00u : 0x7F807F80u;
                const u16x2 one = {1, 1};
                const uint32_t d = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, pk[g][pr]) - one);
                uint32_t tw;
                asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(tw) : "s"(INF), "v"(d));
                asm("v_pk_min_u16 %0, %0, %1" : "+v"(tw) : "s"(0x00010001u));
                const u16x2 t = __builtin_bit_cast(u16x2, tw);
                const u16x2 sh = {(unsigned short)((g & 1) * 8 + 2 * pr), (unsigned short)((g & 1) * 8 + 2 * pr + 1)};
                const uint32_t m = __builtin_bit_cast(uint32_t, t << sh);
                if (g < 2) mlo |= m; else mhi |= m;
            }
        }
    if constexpr (MASK) return ((((mlo | (mlo >> 16)) & 0xFFFFu) | ((mhi | (mhi >> 16)) << 16))) << (4 * h);
    else return 0u;
}

// ---- epilogue of the phased kernels with swapped MFMA operands.  acc[i][j] holds the transposed 32 x 32 block: lane
// (r = lane & 31, h = lane >> 5) owns output row i*32 + r and the columns j*32 + 8 g + 4 h + q: four runs of 4 consecutive columns.
// bias + activation + mask in registers (rows_frag), then v_permlane32_swap between the column groups (g, g + 1) of the two half-waves
// gives every lane 8 consecutive columns = ONE 16-byte store (lanes 0-31: columns 8 g .., lanes 32-63: columns 8 (g + 1) ..).
// Mask words: one 32-bit word per (row, 32-column fragment) per lane - fetched by the caller before / during the main loop (bits[]);
// the forward's mask_out word is assembled from the two half-waves' 16 bits each with one more swap.  Needs whole 64-column wave
// tiles (N % 64 == 0), a 16-bit output and act <= ASE_ACT_RELU.
// NJ: 32-column fragments of the wave tile (2: the 8-wave kernel's 128 x 64, 4: the 4-wave kernel's 128 x 128).
// NI: 32-row blocks of the wave tile (4: the 256 x 256 tiles' 128 rows per wave row, 3: the 192 x 256 tile's 96).
template <typename T, int AUXK, bool MASK, int NJ, int NI>
__device__ __forceinline__ void nt8_epilogue_rows_impl(const NTParams& p, f32x16 (&acc)[NI][NJ], int lane, int mrow0, int ncol0,
                                                       const uint32_t (&bits)[NI][NJ]) {
    const int r = lane & 31, h = lane >> 5;
    const f32x2 al = {p.alpha, p.alpha};
    const float relu_lo = (p.act == ASE_ACT_RELU) ? 0.f : -__builtin_inff();
    uint32_t ovf = 0;
    f32x4 bias[NJ][4];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (p.bias) bias[j][g] = *reinterpret_cast<const f32x4*>(p.bias + ncol0 + j * 32 + 8 * g + 4 * h);
            else bias[j][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int m = mrow0 + i * 32 + r;
        const bool row_ok = m < p.M;
        char* crow = p.C + (int64_t)m * p.ldc + (int64_t)ncol0 * 2 + h * 16;
        uint32_t mword[NJ];
        uint4 out[NJ][2];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            uint32_t pk[4][2];
            mword[j] = rows_frag<T, AUXK, MASK>(acc[i][j], bias[j], AUXK == 2 ? bits[i][j] >> (4 * h) : 0u, al, relu_lo, h, pk);
#pragma unroll
            for (int g = 0; g < 4; g += 2) {
                const auto s0 = __builtin_amdgcn_permlane32_swap(pk[g][0], pk[g + 1][0], false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(pk[g][1], pk[g + 1][1], false, false);
                // lanes 0-31: [own g | upper's g] = columns 8 g .. 8 g + 7; lanes 32-63: [lower's g + 1 | own g + 1]
                out[j][g >> 1] = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                // (on the swapped words: they are live until the store anyway - folding pk[] in rows_frag cost 33 registers)
                ovf = ovf_fold(ovf_fold(ovf_fold(ovf_fold(ovf, s0[0]), s1[0]), s0[1]), s1[1]);
            }
        }
        if (row_ok) {                           // (one predicated block per row block: the swaps above need every lane)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int g = 0; g < 4; g += 2) *reinterpret_cast<uint4*>(crow + (j * 32 + 8 * g) * 2) = out[j][g >> 1];
        }
        if constexpr (MASK) {
#pragma unroll
            for (int jp = 0; jp < NJ; jp += 2) {
                // word j of this row = own 16 bits | the other half-wave's 16 bits
                const auto w = __builtin_amdgcn_permlane32_swap(mword[jp], mword[jp + 1], false, false);
                // after the swap: lanes 0-31 hold (own word jp bits, upper's word jp bits); lanes 32-63 (lower's word jp + 1, own)
                const uint32_t full = w[0] | w[1];
                if (row_ok) p.mask_out[(int64_t)m * p.ldmask + (ncol0 >> 5) + jp + h] = full;
            }
        }
    }
    // (rows past M are clamped copies of the last valid row, see the kernels' DMA addressing: they cannot report what a stored row does not)
    ovf_report(p.alpha_dev, ovf_hit<T>(ovf));
}

template <typename T, int AUXK, int NJ = 2, int NI = 4>
__device__ __forceinline__ void nt8_epilogue_rows(const NTParams& p, f32x16 (&acc)[NI][NJ], int lane, int mrow0, int ncol0,
                                                  const uint32_t (&bits)[NI][NJ]) {
    if (ncol0 >= p.N) return;                                   // wave-uniform: N is a multiple of the wave tile's width
    if (p.mask_out) nt8_epilogue_rows_impl<T, AUXK, true, NJ, NI>(p, acc, lane, mrow0, ncol0, bits);
    else nt8_epilogue_rows_impl<T, AUXK, false, NJ, NI>(p, acc, lane, mrow0, ncol0, bits);
}


// ---- counted waits / barriers of the phased kernels (NT and TN share the schedule) ----------------------------------
template <int UNITS> __device__ __forceinline__ void wait_dma_units() { wait_vmcnt<2 * UNITS>(); }
__device__ __forceinline__ void wait_dma_units_rt(int units) {      // wave-uniform runtime count (loop tail)
    if (units >= 4) wait_vmcnt<8>();
    else if (units == 3) wait_vmcnt<6>();
    else if (units == 2) wait_vmcnt<4>();
    else if (units == 1) wait_vmcnt<2>();
    else wait_vmcnt<0>();
}
// end of the read half of a phase: barrier, THEN retire the LDS reads (hipcc puts a vmcnt(0) in front of any LDS read that
// follows a global_load_lds without a barrier in between, so the DMA is always issued after the phase's fragment reads),
// MFMA block at raised priority
__device__ __forceinline__ void nt8_sync_in() {
    NT8_BARRIER();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
}
__device__ __forceinline__ void nt8_sync_out() {                    // end of the MFMA half
    __builtin_amdgcn_s_setprio(0);
    NT8_BARRIER();
}

// ---- debug phase stamps (ase_hip_debug_nt_profile): thread 0 writes prof[slot]; prof null = off.  Stamps 0 - 2 open the prologue, the
// main loop (optionally in shader clocks) and the epilogue; NT_PROF_CLOSE is stamp 3, taken once every store of the workgroup has retired.
// (macros: as inline functions - the same statements - hipcc allocated the scalar registers of all three phased kernels differently)
#define NT_PROF_STAMP(prof, tid, slot, shader_clk)                                                              \
    do {                                                                                                        \
        if ((prof) && (tid) == 0) (prof)[slot] = (shader_clk) ? (unsigned long long)clock64() : wall_clock64(); \
    } while (0)
#define NT_PROF_CLOSE(prof, tid, slot)                         \
    do {                                                       \
        if (prof) {                                            \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   \
            __syncthreads();                                   \
            if ((tid) == 0) (prof)[slot] = wall_clock64();     \
        }                                                      \
    } while (0)

// ---- host side ------------------------------------------------------------------------------------------------------
extern unsigned long long* g_nt_prof;      // tuning aid, see ase_hip_debug_nt_profile (defined in gemm.hip)
extern int g_nt_prof_clk;                  // ... stamps 1, 2 in shader clocks (ase_hip_debug_nt_profile_clock)

// Kernel choice of an NT launch (also reported by ase_hip_gemm_nt_kernel_id):
//   0:  64 x  64 tile, 4 waves   narrow heads (N <= 64): more workgroups
//   1: 128 x 128 tile, 4 waves   grids that would leave a 256 x 256 tiling with a ragged round
//   2: 256 x 256 tile, 8 waves, PHASED (16-bit storage, K in whole 128-byte steps)   192+ tiles in whole rounds
//   3: 256 x 256 tile, 8 waves, lock-step (the 4-byte storage types)
//   4:  64 x 128 tile, 4 waves / 5: 64 x 64 tile, 4 waves   small grids (M = 2048 ... 4096 rows, or N = 512): two workgroups per CU
//   6: 192 x 256 tile, 8 waves, PHASED   grids of 192 ... 255 tiles of 256 x 256 that become <= 256 tiles of 192 x 256 (the
//      discriminator's 12288 rows x 1024: 192 -> 256 workgroups)
int nt_choice(int M, int N, int K, int es, bool b16);

// one translation unit per storage type (gemm_nt_<type>.hip)
int dispatch_nt_bf16(const NTParams& p, hipStream_t s);
int dispatch_nt_f16(const NTParams& p, hipStream_t s);
int dispatch_nt_f32(const NTParams& p, hipStream_t s);
int dispatch_nt_x3(const NTParams& p, hipStream_t s);      // f32s_t: three bf16 MFMAs per product
int dispatch_nt_h3(const NTParams& p, hipStream_t s);      // f32h_t: three f16 MFMAs per product, scaled operands
// stacked form, ONE launch of the phased 256 x 256 kernel (the caller, ase_hip_gemm_nt_stacked, has checked that the shape takes it)
int dispatch_nt_stacked_bf16(const NTParams& p, hipStream_t s);
int dispatch_nt_stacked_f16(const NTParams& p, hipStream_t s);

}  // namespace ase_nt
