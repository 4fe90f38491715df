/* valu_ceiling.hip -- what one gfx950 SIMD sustains per instruction class (cycles per wave64
 * instruction), at 1 / 2 / 4 / 5 / 8 waves per SIMD, alone and with the fused kernel's share of
 * scalar instructions interleaved (0.56 SALU per VALU, and 1.0).
 *
 * Why: the "VALU busy" figure of the bench line priced every vector instruction at 4 cycles
 * (VERDICT r02, weak #2).  MI355X_MICROARCH.md says a wave64 VALU op issues over 2 cycles on the
 * SIMD-32 (4 only for a wave alone); this measures it for the classes the Ascore kernels are made
 * of (i32 add / shift / compare+select, f32, f64 add / fma / compare / convert, 64-bit shifts,
 * multiplies, readlane, DPP moves, LDS reads / atomics / bpermute), so that the busy figure becomes
 * a mix-weighted measured cost.
 *
 * Method: every wave runs `iters` x 64 independent instructions of one class (16 accumulator
 * chains, inline asm so the compiler neither removes nor reorders them) between two s_memtime
 * stamps.  Blocks are 256 threads = one wave per SIMD; w blocks per CU are forced by a dynamic-LDS
 * footprint of floor(160 KB / w) and a grid of 256 x w blocks, so every SIMD holds exactly w waves.
 * Reported: cycles the SIMD spends per wave-instruction = makespan of all waves (first start to last end)
 *           / (w x iters x 64); beside it what the fastest and the slowest wave saw per instruction (waves of
 *           a SIMD are served oldest first, not evenly), the shader clock and the start skew.
 *
 *   hipcc --offload-arch=gfx950 -O2 -o valu_ceiling scripts/valu_ceiling.hip && ./valu_ceiling > out.csv
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                               \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                       \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

/* scalar filler: S0 none, S9 nine per 16 vector instructions (0.56), S16 one per vector instruction */
#define SA(k) "s_add_u32 %[s" #k "], %[s" #k "], 1\n"
#define S0_0
#define S0_1
#define S0_2
#define S0_3
#define S0_4
#define S0_5
#define S0_6
#define S0_7
#define S0_8
#define S0_9
#define S0_10
#define S0_11
#define S0_12
#define S0_13
#define S0_14
#define S0_15
#define S9_0 SA(0)
#define S9_1
#define S9_2 SA(1)
#define S9_3
#define S9_4 SA(2)
#define S9_5 SA(3)
#define S9_6
#define S9_7 SA(0)
#define S9_8
#define S9_9 SA(1)
#define S9_10
#define S9_11 SA(2)
#define S9_12 SA(3)
#define S9_13
#define S9_14 SA(0)
#define S9_15
#define S16_0 SA(0)
#define S16_1 SA(1)
#define S16_2 SA(2)
#define S16_3 SA(3)
#define S16_4 SA(0)
#define S16_5 SA(1)
#define S16_6 SA(2)
#define S16_7 SA(3)
#define S16_8 SA(0)
#define S16_9 SA(1)
#define S16_10 SA(2)
#define S16_11 SA(3)
#define S16_12 SA(0)
#define S16_13 SA(1)
#define S16_14 SA(2)
#define S16_15 SA(3)

#define B16(F, S)                                                                                          \
    F(0) S##_0 F(1) S##_1 F(2) S##_2 F(3) S##_3 F(4) S##_4 F(5) S##_5 F(6) S##_6 F(7) S##_7 F(8) S##_8 F(9) \
        S##_9 F(10) S##_10 F(11) S##_11 F(12) S##_12 F(13) S##_13 F(14) S##_14 F(15) S##_15

#define OPS32                                                                                              \
    [r0] "+v"(r[0]), [r1] "+v"(r[1]), [r2] "+v"(r[2]), [r3] "+v"(r[3]), [r4] "+v"(r[4]), [r5] "+v"(r[5]),   \
        [r6] "+v"(r[6]), [r7] "+v"(r[7]), [r8] "+v"(r[8]), [r9] "+v"(r[9]), [r10] "+v"(r[10]),              \
        [r11] "+v"(r[11]), [r12] "+v"(r[12]), [r13] "+v"(r[13]), [r14] "+v"(r[14]), [r15] "+v"(r[15]),      \
        [m] "+s"(msk), [m2] "+s"(msk2), [s0] "+s"(sa[0]), [s1] "+s"(sa[1]), [s2] "+s"(sa[2]), [s3] "+s"(sa[3])
#define OPSQ                                                                                               \
    , [q0] "+v"(q[0]), [q1] "+v"(q[1]), [q2] "+v"(q[2]), [q3] "+v"(q[3]), [q4] "+v"(q[4]), [q5] "+v"(q[5]),  \
        [q6] "+v"(q[6]), [q7] "+v"(q[7]), [q8] "+v"(q[8]), [q9] "+v"(q[9]), [q10] "+v"(q[10]),              \
        [q11] "+v"(q[11]), [q12] "+v"(q[12]), [q13] "+v"(q[13]), [q14] "+v"(q[14]), [q15] "+v"(q[15])

/* one kernel per (class, scalar share).  T = uint32_t / float / uint64_t / double accumulators;
 * WAIT = a counter wait after every block of 16 (LDS classes). */
#define KERNEL(NAME, T, F, S, WAIT)                                                                        \
    __global__ __launch_bounds__(1024) void k_##NAME##_##S(unsigned long long *out, int iters, T seed,      \
                                                          uint32_t c0) {                                   \
        extern __shared__ unsigned char lds[];                                                             \
        T r[16];                                                                                           \
        uint32_t q[16];                                                                                    \
        for (int i = 0; i < 16; i++) q[i] = threadIdx.x + i;                                               \
        uint32_t sa[4] = {1, 2, 3, 4};                                                                     \
        for (int i = 0; i < 16; i++) r[i] = seed + (T)(threadIdx.x * 16 + i);                              \
        T c = seed;                                                                                        \
        uint32_t ci = (threadIdx.x & 63) * c0;   /* LDS address: lane x access width */                                                        \
        (void)c;                                                                                           \
        unsigned long long msk = 0x5555555555555555ull ^ c0;  unsigned long long msk2 = ~0ull; (void)ci; (void)msk; (void)msk2;                                                                                        \
        unsigned long long t0, t1;                                                                         \
        __syncthreads();                                                                                   \
        const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");                         \
        for (int it = 0; it < iters; it++) {                                                               \
            asm volatile(B16(F, S) WAIT B16(F, S) WAIT B16(F, S) WAIT B16(F, S) WAIT                       \
                         : OPS32 OPSQ                                                                      \
                         : [c] "v"(c), [ci] "v"(ci)                                                      \
                         : "memory", "scc", "vcc");                                                            \
        }                                                                                                  \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");                         \
        T acc = r[0] + (T)(q[0] ^ q[5] ^ q[15]);                                                           \
        for (int i = 1; i < 16; i++) acc = acc + r[i];                                                     \
        if ((threadIdx.x & 63) == 0) {                                                                     \
            const size_t wv = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                         \
            out[wv * 3] = t1 - t0;                                                                         \
            out[wv * 3 + 1] = rt0;                                                                         \
            out[wv * 3 + 2] = __builtin_amdgcn_s_memrealtime();                                            \
        }                                                                                                  \
        if (acc == (T)12345 && sa[0] + sa[1] + sa[2] + sa[3] == 7u) out[0] = 0; /* keeps the chains alive */ \
    }

#define K3(NAME, T, F, WAIT) KERNEL(NAME, T, F, S0, WAIT) KERNEL(NAME, T, F, S9, WAIT) KERNEL(NAME, T, F, S16, WAIT)

#define NOW ""
#define LGKM "s_waitcnt lgkmcnt(0)\n"

/* ---- instruction classes ---- */
#define F_ADD_U32(k) "v_add_u32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_LSHL_B32(k) "v_lshlrev_b32 %[r" #k "], 1, %[r" #k "]\n"
#define F_AND_OR(k) "v_and_or_b32 %[r" #k "], %[r" #k "], %[c], %[c]\n"
#define F_BFE_U32(k) "v_bfe_u32 %[r" #k "], %[r" #k "], 3, 5\n"
#define F_MIN3_I32(k) "v_min3_i32 %[r" #k "], %[r" #k "], %[c], %[c]\n"
#define F_MIN_U32(k) "v_min_u32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_ADD_F32(k) "v_add_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_FMA_F32(k) "v_fma_f32 %[r" #k "], %[r" #k "], %[c], %[c]\n"
#define F_CMP_F32(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\n"
#define F_CNDMASK(k) "v_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_CMP_CND_F32(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_CND_SGPR(k) "v_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\n"
#define F_CMP_CND2(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\nv_cndmask_b32 %[r" #k "], %[c], %[r" #k "], vcc\n"
#define F_CMP_SGPR_CND(k) "v_cmp_lt_f32_e64 %[m], %[r" #k "], %[c]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\n"
#define F_ADD_SUB(k) "v_add_u32 %[r" #k "], %[r" #k "], %[c]\nv_lshlrev_b32 %[r" #k "], 1, %[r" #k "]\n"
/* which reads of a lane mask are cheap: VCC written by the instruction before, VCC written two back, VCC
 * written by the scalar unit, a mask in an SGPR pair */
#define F_X_CMP_CND_CND(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\nv_cndmask_b32 %[q" #k "], %[q" #k "], %[c], vcc\n"
#define F_X_CMP_ADD_CND(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_add_u32 %[q" #k "], %[q" #k "], %[c]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_X_SVCC_CND(k) "s_not_b64 vcc, vcc\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_X_CMPS_CND_CND(k) "v_cmp_lt_f32_e64 %[m], %[r" #k "], %[c]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\nv_cndmask_b32_e64 %[q" #k "], %[q" #k "], %[c], %[m]\n"
#define F_X_ADDCO_ADDC(k) "v_add_co_u32 %[r" #k "], vcc, %[r" #k "], %[c]\nv_addc_co_u32 %[q" #k "], vcc, %[q" #k "], %[c], vcc\n"
#define F_X_CMP_CNDE64VCC(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_add_u32 %[q" #k "], %[q" #k "], %[c]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_X_SSGPR_CND(k) "s_not_b64 %[m], %[m]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\n"
#define F_X_CMPS_SAND_CND(k) "v_cmp_lt_f32_e64 %[m], %[r" #k "], %[c]\ns_and_b64 %[m], %[m], %[m2]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\n"
#define F_X_CMP_SANDVCC_CND(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\ns_and_b64 vcc, vcc, %[m2]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_X_CMPS_SAND_2ADD_CND(k) "v_cmp_lt_f32_e64 %[m], %[r" #k "], %[c]\ns_and_b64 %[m], %[m], %[m2]\nv_add_u32 %[q" #k "], %[q" #k "], %[c]\nv_add_u32 %[q" #k "], %[q" #k "], %[c]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\n"
#define F_X_CMP_CMP_VAND(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\nv_cmp_gt_f32 vcc, %[q" #k "], %[c]\nv_cndmask_b32 %[r" #k "], %[r" #k "], %[c], vcc\n"
#define F_X_SAVEEXEC(k) "v_cmp_lt_u32 vcc, %[q" #k "], %[c]\ns_and_saveexec_b64 %[m], vcc\nv_add_u32 %[r" #k "], %[r" #k "], %[c]\ns_or_b64 exec, exec, %[m]\n"
#define F_X_READLANE_USE(k) "v_readlane_b32 %[s0], %[q" #k "], 3\nv_add_u32 %[r" #k "], %[s0], %[r" #k "]\n"
#define F_X_SADD_USE(k) "s_add_u32 %[s0], %[s0], 1\nv_add_u32 %[r" #k "], %[s0], %[r" #k "]\n"
#define F_X_CMPS_CND(k) "v_cmp_lt_f32_e64 %[m], %[r" #k "], %[c]\nv_cndmask_b32_e64 %[r" #k "], %[r" #k "], %[c], %[m]\n"
#define F_O_SUB_U32(k) "v_sub_u32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_AND_B32(k) "v_and_b32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_OR_B32(k) "v_or_b32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_XOR_B32(k) "v_xor_b32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MAX_U32(k) "v_max_u32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MAX_F32(k) "v_max_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MIN_F32(k) "v_min_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MUL_F32(k) "v_mul_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_SUB_F32(k) "v_sub_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MUL_U32_U24(k) "v_mul_u32_u24 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_LSHRREV_B32(k) "v_lshrrev_b32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_ADD_U32_E64(k) "v_add_u32_e64 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_FMAC_F32(k) "v_fmac_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MAX_F64(k) "v_max_f64 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_ADD_F16(k) "v_add_f16 %[r" #k "], %[r" #k "], %[c]\n"
#define F_O_MOV_B32(k) "v_mov_b32 %[r" #k "], %[c]\n"
#define F_O_LSHL_ADD_U32(k) "v_lshl_add_u32 %[r" #k "], %[r" #k "], 1, %[c]\n"
#define F_O_ADD3_U32(k) "v_add3_u32 %[r" #k "], %[r" #k "], %[c], %[c]\n"
#define F_O_LSHL_OR_B32(k) "v_lshl_or_b32 %[r" #k "], %[r" #k "], 1, %[c]\n"
#define F_O_ADD_CO_U32(k) "v_add_co_u32 %[r" #k "], vcc, %[r" #k "], %[c]\n"
#define F_O_CVT_F32_U32(k) "v_cvt_f32_u32 %[r" #k "], %[r" #k "]\n"
#define F_O_CMP_GT_F32_E64(k) "v_cmp_gt_f32_e64 %[m], %[r" #k "], %[c]\n"
#define F_O_MOV_B64(k) "v_mov_b64 %[r" #k "], %[c]\n"
#define F_O_CVT_F64_F32_ONLY(k) "v_cvt_f64_f32 %[r" #k "], %[ci]\n"
#define F_O_CVT_F32_F64_ONLY(k) "v_cvt_f32_f64 %[q" #k "], %[r" #k "]\n"
#define F_O_ADD_F32_MOV(k) "v_add_f32 %[r" #k "], %[r" #k "], %[c]\nv_lshlrev_b32 %[q" #k "], 1, %[q" #k "]\n"
#define F_O_ADD_U32_ADD_F32(k) "v_add_u32 %[r" #k "], %[r" #k "], %[c]\nv_add_f32 %[q" #k "], %[q" #k "], %[c]\n"
#define F_CMP_U32(k) "v_cmp_lt_u32 vcc, %[r" #k "], %[c]\n"
#define F_CMP_ADDC(k) "v_cmp_lt_f32 vcc, %[r" #k "], %[c]\nv_addc_co_u32 %[r" #k "], vcc, 0, %[r" #k "], vcc\n"
#define F_CVT_U32_F32(k) "v_cvt_u32_f32 %[r" #k "], %[r" #k "]\n"
#define F_MUL_LO(k) "v_mul_lo_u32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_MUL_HI(k) "v_mul_hi_u32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_MAD_U32_U24(k) "v_mad_u32_u24 %[r" #k "], %[r" #k "], %[c], %[c]\n"
#define F_READLANE(k) "v_readlane_b32 %[s" "0" "], %[r" #k "], 5\n"
#define F_READFIRST(k) "v_readfirstlane_b32 %[s" "1" "], %[r" #k "]\n"
#define F_DPP_MOV(k) "v_mov_b32_dpp %[r" #k "], %[r" #k "] row_shr:1 row_mask:0xf bank_mask:0xf\n"
#define F_DPP_ADD(k) "v_add_u32_dpp %[r" #k "], %[r" #k "], %[r" #k "] row_shr:1 row_mask:0xf bank_mask:0xf\n"
#define F_MBCNT(k) "v_mbcnt_lo_u32_b32 %[r" #k "], -1, %[r" #k "]\n"
#define F_BCNT(k) "v_bcnt_u32_b32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_FFBL(k) "v_ffbl_b32 %[r" #k "], %[r" #k "]\n"
/* 64-bit / f64 */
#define F_ADD_F64(k) "v_add_f64 %[r" #k "], %[r" #k "], %[c]\n"
#define F_MUL_F64(k) "v_mul_f64 %[r" #k "], %[r" #k "], %[c]\n"
#define F_FMA_F64(k) "v_fma_f64 %[r" #k "], %[r" #k "], %[c], %[c]\n"
#define F_CMP_F64(k) "v_cmp_lt_f64 vcc, %[r" #k "], %[c]\n"
#define F_FLOOR_F64(k) "v_floor_f64 %[r" #k "], %[r" #k "]\n"
#define F_LSHL_B64(k) "v_lshlrev_b64 %[r" #k "], 1, %[r" #k "]\n"
#define F_LSHR_B64(k) "v_lshrrev_b64 %[r" #k "], %[ci], %[r" #k "]\n"
#define F_MAD_U64(k) "v_mad_u64_u32 %[r" #k "], vcc, %[ci], %[ci], %[r" #k "]\n"
#define F_PK_ADD_F32(k) "v_pk_add_f32 %[r" #k "], %[r" #k "], %[c]\n"
/* the binning kernel's rank count per mate (bin_core.hip.h): float keys with the window in the exponent, "more intense" as a
 * clamped difference.  bk_pk_sub_clamp / bk_sub_f32_e64_clamp: the two instructions alone (the second one is a VOP2 opcode in
 * VOP3 encoding); bk_form_c (two packed instructions per two mates), bk_form_d (two per mate) and bk_form_int (the integer
 * count they replace: subtract, shift, add) with the dependence of the count on the difference */
#define F_BK_PK_SUB_CLAMP(k) "v_pk_add_f32 %[r" #k "], %[r" #k "], %[c] neg_lo:[0,1] neg_hi:[0,1] clamp\n"
#define F_BK_SUB_F32_E64_CLAMP(k) "v_sub_f32_e64 %[r" #k "], %[r" #k "], %[c] clamp\n"
#define F_BK_FORM_C(k) "v_pk_add_f32 %[r" #k "], %[r" #k "], %[c] neg_lo:[0,1] neg_hi:[0,1] clamp\nv_pk_add_f32 %[r" #k "], %[r" #k "], %[c]\n"
#define F_BK_FORM_D(k) "v_sub_f32_e64 %[q" #k "], %[c], %[r" #k "] clamp\nv_add_f32 %[r" #k "], %[r" #k "], %[q" #k "]\n"
#define F_BK_FORM_INT(k) "v_sub_u32 %[q" #k "], %[c], %[r" #k "]\nv_lshrrev_b32 %[q" #k "], 31, %[q" #k "]\nv_add_u32 %[r" #k "], %[r" #k "], %[q" #k "]\n"
#define F_PK_MOV(k) "v_pk_mov_b32 %[r" #k "], %[r" #k "], %[c]\n"
/* LDS (address in ci; conflict-free: lane * 4 / * 8 / * 16 bytes) */
#define F_DS_READ_B32(k) "ds_read_b32 %[r" #k "], %[ci]\n"
#define F_DS_ADD_U32(k) "ds_add_u32 %[ci], %[r" #k "]\n"
#define F_DS_ADD_RTN(k) "ds_add_rtn_u32 %[r" #k "], %[ci], %[r" #k "]\n"
#define F_DS_WRITE_B8(k) "ds_write_b8 %[ci], %[r" #k "]\n"
#define F_DS_WRITE_B32(k) "ds_write_b32 %[ci], %[r" #k "]\n"
#define F_DS_BPERMUTE(k) "ds_bpermute_b32 %[r" #k "], %[ci], %[r" #k "]\n"
#define F_DS_SWIZZLE(k) "ds_swizzle_b32 %[r" #k "], %[r" #k "] offset:0x041f\n"
#define F_DS_READ_B64(k) "ds_read_b64 %[r" #k "], %[ci]\n"
/* scalar alone (the block's "vector" slot holds a scalar op: cost of the scalar unit itself) */
#define F_S_ADD(k) "s_add_u32 %[s0], %[s0], 3\ns_add_u32 %[s1], %[s1], 3\ns_add_u32 %[s2], %[s2], 3\ns_add_u32 %[s3], %[s3], 3\n"
#define F_S_BCNT(k) "s_bcnt1_i32_b32 %[s0], %[s1]\ns_ff1_i32_b32 %[s2], %[s3]\ns_lshl_b32 %[s1], %[s1], 1\ns_and_b32 %[s3], %[s3], %[s2]\n"

K3(add_u32, uint32_t, F_ADD_U32, NOW)
K3(lshl_b32, uint32_t, F_LSHL_B32, NOW)
K3(and_or_b32, uint32_t, F_AND_OR, NOW)
K3(bfe_u32, uint32_t, F_BFE_U32, NOW)
K3(min3_i32, uint32_t, F_MIN3_I32, NOW)
K3(min_u32, uint32_t, F_MIN_U32, NOW)
K3(add_f32, float, F_ADD_F32, NOW)
K3(fma_f32, float, F_FMA_F32, NOW)
K3(cmp_f32, float, F_CMP_F32, NOW)
K3(cndmask, uint32_t, F_CNDMASK, NOW)
K3(cmp_cnd_f32_pair, float, F_CMP_CND_F32, NOW)
K3(cmp_u32, uint32_t, F_CMP_U32, NOW)
K3(o_sub_u32, uint32_t, F_O_SUB_U32, NOW)
K3(o_and_b32, uint32_t, F_O_AND_B32, NOW)
K3(o_or_b32, uint32_t, F_O_OR_B32, NOW)
K3(o_xor_b32, uint32_t, F_O_XOR_B32, NOW)
K3(o_max_u32, uint32_t, F_O_MAX_U32, NOW)
K3(o_max_f32, float, F_O_MAX_F32, NOW)
K3(o_min_f32, float, F_O_MIN_F32, NOW)
K3(o_mul_f32, float, F_O_MUL_F32, NOW)
K3(o_sub_f32, float, F_O_SUB_F32, NOW)
K3(o_mul_u32_u24, uint32_t, F_O_MUL_U32_U24, NOW)
K3(o_lshrrev_b32, uint32_t, F_O_LSHRREV_B32, NOW)
K3(o_add_u32_e64, uint32_t, F_O_ADD_U32_E64, NOW)
K3(o_fmac_f32, float, F_O_FMAC_F32, NOW)
K3(o_max_f64, double, F_O_MAX_F64, NOW)
K3(o_add_f16, uint32_t, F_O_ADD_F16, NOW)
K3(o_mov_b32, uint32_t, F_O_MOV_B32, NOW)
K3(o_lshl_add_u32, uint32_t, F_O_LSHL_ADD_U32, NOW)
K3(o_add3_u32, uint32_t, F_O_ADD3_U32, NOW)
K3(o_lshl_or_b32, uint32_t, F_O_LSHL_OR_B32, NOW)
K3(o_add_co_u32, uint32_t, F_O_ADD_CO_U32, NOW)
K3(o_cvt_f32_u32, uint32_t, F_O_CVT_F32_U32, NOW)
K3(o_cmp_gt_f32_e64, float, F_O_CMP_GT_F32_E64, NOW)
K3(o_mov_b64, uint64_t, F_O_MOV_B64, NOW)
K3(o_cvt_f64_f32_only, double, F_O_CVT_F64_F32_ONLY, NOW)
K3(o_cvt_f32_f64_only, double, F_O_CVT_F32_F64_ONLY, NOW)
K3(o_add_f32_mov, float, F_O_ADD_F32_MOV, NOW)
K3(o_add_u32_add_f32, uint32_t, F_O_ADD_U32_ADD_F32, NOW)
K3(x_ssgpr_cnd, uint32_t, F_X_SSGPR_CND, NOW)
K3(x_cmps_sand_cnd, float, F_X_CMPS_SAND_CND, NOW)
K3(x_cmp_sandvcc_cnd, float, F_X_CMP_SANDVCC_CND, NOW)
K3(x_cmps_sand_2add_cnd, float, F_X_CMPS_SAND_2ADD_CND, NOW)
K3(x_cmp_cnd_cmp_cnd, float, F_X_CMP_CMP_VAND, NOW)
K3(x_saveexec_add_restore, uint32_t, F_X_SAVEEXEC, NOW)
K3(x_readlane_use, uint32_t, F_X_READLANE_USE, NOW)
K3(x_sadd_use, uint32_t, F_X_SADD_USE, NOW)
K3(x_cmps_cnd, float, F_X_CMPS_CND, NOW)
K3(x_cmp_cnd_cnd, float, F_X_CMP_CND_CND, NOW)
K3(x_cmp_add_cnd, float, F_X_CMP_ADD_CND, NOW)
K3(x_svcc_cnd, uint32_t, F_X_SVCC_CND, NOW)
K3(x_cmps_cnd_cnd, float, F_X_CMPS_CND_CND, NOW)
K3(x_addco_addc, uint32_t, F_X_ADDCO_ADDC, NOW)
K3(x_cmp_add_cnde64vcc, float, F_X_CMP_CNDE64VCC, NOW)
K3(cnd_sgpr, uint32_t, F_CND_SGPR, NOW)
K3(cmp_cnd_cnd_triple, float, F_CMP_CND2, NOW)
K3(add_lshl_pair, uint32_t, F_ADD_SUB, NOW)
K3(cmp_addc_pair, float, F_CMP_ADDC, NOW)
K3(cvt_u32_f32, float, F_CVT_U32_F32, NOW)
K3(mul_lo_u32, uint32_t, F_MUL_LO, NOW)
K3(mul_hi_u32, uint32_t, F_MUL_HI, NOW)
K3(mad_u32_u24, uint32_t, F_MAD_U32_U24, NOW)
K3(readlane, uint32_t, F_READLANE, NOW)
K3(readfirstlane, uint32_t, F_READFIRST, NOW)
K3(dpp_mov, uint32_t, F_DPP_MOV, NOW)
K3(dpp_add, uint32_t, F_DPP_ADD, NOW)
K3(mbcnt, uint32_t, F_MBCNT, NOW)
K3(bcnt, uint32_t, F_BCNT, NOW)
K3(ffbl, uint32_t, F_FFBL, NOW)
K3(add_f64, double, F_ADD_F64, NOW)
K3(mul_f64, double, F_MUL_F64, NOW)
K3(fma_f64, double, F_FMA_F64, NOW)
K3(cmp_f64, double, F_CMP_F64, NOW)
K3(floor_f64, double, F_FLOOR_F64, NOW)
K3(lshl_b64, uint64_t, F_LSHL_B64, NOW)
K3(lshr_b64, uint64_t, F_LSHR_B64, NOW)
K3(mad_u64_u32, uint64_t, F_MAD_U64, NOW)
K3(pk_add_f32, uint64_t, F_PK_ADD_F32, NOW)
K3(bk_pk_sub_clamp, uint64_t, F_BK_PK_SUB_CLAMP, NOW)
K3(bk_sub_f32_e64_clamp, float, F_BK_SUB_F32_E64_CLAMP, NOW)
K3(bk_form_c, uint64_t, F_BK_FORM_C, NOW)
K3(bk_form_d, float, F_BK_FORM_D, NOW)
K3(bk_form_int, uint32_t, F_BK_FORM_INT, NOW)
K3(ds_read_b32, uint32_t, F_DS_READ_B32, LGKM)
K3(ds_read_b64, uint64_t, F_DS_READ_B64, LGKM)
K3(ds_add_u32, uint32_t, F_DS_ADD_U32, LGKM)
K3(ds_add_rtn_u32, uint32_t, F_DS_ADD_RTN, LGKM)
K3(ds_write_b8, uint32_t, F_DS_WRITE_B8, LGKM)
K3(ds_write_b32, uint32_t, F_DS_WRITE_B32, LGKM)
K3(ds_bpermute, uint32_t, F_DS_BPERMUTE, LGKM)
K3(ds_swizzle, uint32_t, F_DS_SWIZZLE, LGKM)
K3(s_add_x4, uint32_t, F_S_ADD, NOW)
K3(s_mix_x4, uint32_t, F_S_BCNT, NOW)

/* two conversions need different register widths on the two sides: written out */
__global__ __launch_bounds__(1024) void k_cvt_f64_f32_S0(unsigned long long *out, int iters, float seed, uint32_t) {
    float a[16];
    double d[16];
    for (int i = 0; i < 16; i++) a[i] = seed + (float)(threadIdx.x + i);
    unsigned long long t0, t1;
    __syncthreads();
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int rep = 0; rep < 2; rep++) {
#pragma unroll
            for (int i = 0; i < 16; i++) asm volatile("v_cvt_f64_f32 %0, %1" : "=v"(d[i]) : "v"(a[i]));
#pragma unroll
            for (int i = 0; i < 16; i++) asm volatile("v_cvt_f32_f64 %0, %1" : "=v"(a[i]) : "v"(d[i]));
        }
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
    float acc = 0.f;
    for (int i = 0; i < 16; i++) acc += a[i];
    if ((threadIdx.x & 63) == 0) {
        const size_t wv = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        out[wv * 3] = t1 - t0;
        out[wv * 3 + 1] = rt0;
        out[wv * 3 + 2] = __builtin_amdgcn_s_memrealtime();
    }
    if (acc == 12345.f) out[0] = 0;
}


/* The fused kernel's walk step (pya_score_localize_kernel<true,false>, the loop around look4) as the compiler
 * emits it -- same vector and scalar instructions in the same order with the same dependences, LDS reads
 * replaced by register moves of the same width (their latency is what waves/SIMD hide; their issue is not a
 * VALU slot): 38 vector + 7 scalar instructions per step.  What a SIMD needs per vector instruction of THIS
 * mix is the figure `valu_busy` is priced with. */
__global__ __launch_bounds__(1024) void k_mix_walk_step_S0(unsigned long long *out, int iters, float seed, uint32_t c0) {
    float run = seed, f7 = 0.05f, f19 = 0.125f, f1 = -12.f;
    uint32_t bits = threadIdx.x * 2654435761u, u18 = 255u, v13 = c0, v30 = c0, v21 = 1u;
    double A = 1.007825, B = 0.0;
    float m0 = 57.02f + (threadIdx.x & 7), m1 = m0 + 79.97f;
    float e0 = 300.f, e1 = 301.f, e2 = 302.f, e3 = 303.f;
    uint32_t k0 = 1, k1 = 2, k2 = 3, k3 = 4, acc = 0, v27 = c0;
    unsigned long long t0, t1;
    __syncthreads();
    const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime();
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int rep = 0; rep < 4; rep++) {
            float r16, lo, hi, cellf;
            double d;
            uint32_t cell, idx, ra, rb, rc, rd, best, inc, row;
            asm volatile(
                "v_add_co_u32 %[bits], vcc, %[bits], %[bits]\n"
                "v_cndmask_b32 %[r16], %[m0], %[m1], vcc\n"
                "v_add_f32 %[run], %[run], %[r16]\n"
                "v_cvt_f64_f32 %[d], %[run]\n"
                "v_add_f64 %[d], %[A], %[d]\n"
                "v_add_f64 %[d], %[d], -%[B]\n"
                "v_add_f64 %[d], %[d], %[A]\n"
                "v_cvt_f32_f64 %[hi], %[d]\n"
                "v_sub_f32 %[lo], %[hi], %[f7]\n"
                "v_fma_f32 %[cellf], %[lo], %[f19], %[f1]\n"
                "v_cvt_u32_f32 %[cell], %[cellf]\n"
                "v_add_f32 %[hi], %[f7], %[hi]\n"
                "v_min_u32 %[cell], %[cell], %[u18]\n"
                "v_lshl_add_u32 %[cell], %[cell], 1, 0\n"
                "v_lshlrev_b32 %[idx], 3, %[cell]\n"
                "v_add_u32 %[idx], 0, %[idx]\n"
                "v_cmp_gt_f32 vcc, %[e0], %[lo]\n"
                "v_cmp_lt_f32_e64 s[12:13], %[e0], %[hi]\n"
                "v_cmp_gt_f32_e64 s[14:15], %[e1], %[lo]\n"
                "v_cmp_lt_f32_e64 s[16:17], %[e1], %[hi]\n"
                "s_and_b64 vcc, vcc, s[12:13]\n"
                "s_and_b64 s[12:13], s[14:15], s[16:17]\n"
                "v_cmp_gt_f32_e64 s[18:19], %[e2], %[lo]\n"
                "v_cmp_lt_f32_e64 s[20:21], %[e2], %[hi]\n"
                "v_cndmask_b32 %[ra], 15, %[k0], vcc\n"
                "v_cndmask_b32_e64 %[rb], 15, %[k1], s[12:13]\n"
                "v_cmp_gt_f32 vcc, %[e3], %[lo]\n"
                "v_cmp_lt_f32_e64 s[12:13], %[e3], %[hi]\n"
                "s_and_b64 s[14:15], s[18:19], s[20:21]\n"
                "s_and_b64 vcc, vcc, s[12:13]\n"
                "v_cndmask_b32_e64 %[rc], 15, %[k2], s[14:15]\n"
                "v_cndmask_b32 %[rd], 15, %[k3], vcc\n"
                "v_min_i32 %[rc], %[rc], %[rd]\n"
                "v_min3_i32 %[best], %[ra], %[rb], %[rc]\n"
                "v_cmp_gt_i32 vcc, 10, %[best]\n"
                "v_lshrrev_b32 %[row], 1, %[best]\n"
                "v_lshlrev_b32 %[inc], 4, %[best]\n"
                "v_lshlrev_b32_e64 %[inc], %[inc], 1\n"
                "s_and_b64 vcc, exec, vcc\n"
                "v_lshl_add_u32 %[row], %[row], 8, %[v13]\n"
                "v_cndmask_b32 %[inc], 0, %[inc], vcc\n"
                "s_add_i32 s22, s22, 1\n"
                "v_add_u32 %[v30], %[v21], %[v30]\n"
                "s_cmp_lg_u32 s22, 77\n"
                "v_lshl_add_u32 %[v27], %[v21], 3, %[v27]\n"
                : [bits] "+v"(bits), [run] "+v"(run), [r16] "=&v"(r16), [d] "=&v"(d), [lo] "=&v"(lo), [hi] "=&v"(hi),
                  [cellf] "=&v"(cellf), [cell] "=&v"(cell), [idx] "=&v"(idx), [ra] "=&v"(ra), [rb] "=&v"(rb), [rc] "=&v"(rc),
                  [rd] "=&v"(rd), [best] "=&v"(best), [inc] "=&v"(inc), [row] "=&v"(row), [v30] "+v"(v30), [v27] "+v"(v27)
                : [m0] "v"(m0), [m1] "v"(m1), [A] "v"(A), [B] "v"(B), [f7] "v"(f7), [f19] "v"(f19), [f1] "v"(f1), [u18] "v"(u18),
                  [e0] "v"(e0), [e1] "v"(e1), [e2] "v"(e2), [e3] "v"(e3), [k0] "v"(k0), [k1] "v"(k1), [k2] "v"(k2), [k3] "v"(k3),
                  [v13] "v"(v13), [v21] "v"(v21)
                : "memory", "scc", "vcc", "s12", "s13", "s14", "s15", "s16", "s17", "s18", "s19", "s20", "s21", "s22");
            acc += inc + row + idx;
            e0 += 1.f; e1 += 1.f; e2 += 1.f; e3 += 1.f;     /* (4 simple vector adds + 1 for acc: counted in per_slot) */
        }
    }
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
    if ((threadIdx.x & 63) == 0) {
        const size_t wv = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        out[wv * 3] = t1 - t0;
        out[wv * 3 + 1] = rt0;
        out[wv * 3 + 2] = __builtin_amdgcn_s_memrealtime();
    }
    if (acc == 12345u && run == 3.f) out[0] = 0;
}

struct Entry {
    const char *name;
    const char *salu;
    const void *fn;
    int kind;            /* 0 u32, 1 f32, 2 u64, 3 f64 */
    double per_slot;     /* instructions per "slot" of the block (pairs: 2, scalar x4: 4) */
};
#define E3(NAME, KIND, PER)                                                               \
    {#NAME, "0", (const void *)k_##NAME##_S0, KIND, PER}, {#NAME, "0.56", (const void *)k_##NAME##_S9, KIND, PER}, \
        {#NAME, "1.0", (const void *)k_##NAME##_S16, KIND, PER},

static const Entry kEntries[] = {
    E3(add_u32, 0, 1) E3(lshl_b32, 0, 1) E3(and_or_b32, 0, 1) E3(bfe_u32, 0, 1) E3(min3_i32, 0, 1) E3(min_u32, 0, 1)
    E3(add_f32, 1, 1) E3(fma_f32, 1, 1) E3(cmp_f32, 1, 1) E3(cndmask, 0, 1) E3(cmp_cnd_f32_pair, 1, 2) E3(cmp_u32, 0, 1) E3(o_sub_u32, 0, 1) E3(o_and_b32, 0, 1) E3(o_or_b32, 0, 1) E3(o_xor_b32, 0, 1) E3(o_max_u32, 0, 1) E3(o_max_f32, 1, 1) E3(o_min_f32, 1, 1) E3(o_mul_f32, 1, 1) E3(o_sub_f32, 1, 1) E3(o_mul_u32_u24, 0, 1) E3(o_lshrrev_b32, 0, 1) E3(o_add_u32_e64, 0, 1) E3(o_fmac_f32, 1, 1) E3(o_max_f64, 3, 1) E3(o_add_f16, 0, 1) E3(o_mov_b32, 0, 1) E3(o_lshl_add_u32, 0, 1) E3(o_add3_u32, 0, 1) E3(o_lshl_or_b32, 0, 1) E3(o_add_co_u32, 0, 1) E3(o_cvt_f32_u32, 0, 1) E3(o_cmp_gt_f32_e64, 1, 1) E3(o_mov_b64, 2, 1) E3(o_cvt_f64_f32_only, 3, 1) E3(o_cvt_f32_f64_only, 3, 1) E3(o_add_f32_mov, 1, 2) E3(o_add_u32_add_f32, 0, 2) E3(x_ssgpr_cnd, 0, 1) E3(x_cmps_sand_cnd, 1, 2) E3(x_cmp_sandvcc_cnd, 1, 2) E3(x_cmps_sand_2add_cnd, 1, 4) E3(x_cmp_cnd_cmp_cnd, 1, 4) E3(x_saveexec_add_restore, 0, 2) E3(x_readlane_use, 0, 2) E3(x_sadd_use, 0, 1) E3(x_cmps_cnd, 1, 2) E3(x_cmp_cnd_cnd, 1, 3) E3(x_cmp_add_cnd, 1, 3) E3(x_svcc_cnd, 0, 1) E3(x_cmps_cnd_cnd, 1, 3) E3(x_addco_addc, 0, 2) E3(x_cmp_add_cnde64vcc, 1, 3) E3(cnd_sgpr, 0, 1) E3(cmp_cnd_cnd_triple, 1, 3) E3(add_lshl_pair, 0, 2)
    E3(cmp_addc_pair, 1, 2) E3(cvt_u32_f32, 1, 1) E3(mul_lo_u32, 0, 1) E3(mul_hi_u32, 0, 1) E3(mad_u32_u24, 0, 1)
    E3(readlane, 0, 1) E3(readfirstlane, 0, 1) E3(dpp_mov, 0, 1) E3(dpp_add, 0, 1) E3(mbcnt, 0, 1) E3(bcnt, 0, 1) E3(ffbl, 0, 1)
    E3(add_f64, 3, 1) E3(mul_f64, 3, 1) E3(fma_f64, 3, 1) E3(cmp_f64, 3, 1) E3(floor_f64, 3, 1) E3(lshl_b64, 2, 1)
    E3(lshr_b64, 2, 1) E3(mad_u64_u32, 2, 1) E3(pk_add_f32, 2, 1)
    E3(bk_pk_sub_clamp, 2, 1) E3(bk_sub_f32_e64_clamp, 1, 1) E3(bk_form_c, 2, 2) E3(bk_form_d, 1, 2) E3(bk_form_int, 0, 3)
    E3(ds_read_b32, 0, 1) E3(ds_read_b64, 2, 1) E3(ds_add_u32, 0, 1) E3(ds_add_rtn_u32, 0, 1) E3(ds_write_b8, 0, 1)
    E3(ds_write_b32, 0, 1) E3(ds_bpermute, 0, 1) E3(ds_swizzle, 0, 1) E3(s_add_x4, 0, 4) E3(s_mix_x4, 0, 4)
    {"cvt_f64_f32+cvt_f32_f64", "0", (const void *)k_cvt_f64_f32_S0, 1, 1},
    {"mix_walk_step", "0.19", (const void *)k_mix_walk_step_S0, 1, 166.0 / 64.0},   /* 166 vector instructions per loop iteration in the .s */
};

int main(int argc, char **argv) {
    const int iters = argc > 1 ? std::atoi(argv[1]) : 1500;
    const char *only = argc > 2 ? argv[2] : nullptr;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    unsigned long long *d_out = nullptr;
    const int max_waves = cus * 8 * 4;
    CHECK(hipMalloc(&d_out, (size_t)max_waves * 24));
    std::vector<unsigned long long> h((size_t)max_waves * 3);
    std::printf("# %s, %d CUs, clock %d kHz; iters %d x 64 slots per wave\n", prop.gcnArchName, cus, prop.clockRate, iters);
    std::printf("class,salu_per_valu,waves_per_simd,cycles_per_inst_simd,fastest_wave_cycles_per_inst,slowest_wave_cycles_per_inst,clock_ghz,start_skew_us,kernel_us\n");
    /* w waves per SIMD = 4w waves per CU: one workgroup of 4w waves per CU up to w = 4 (96 KB of LDS each: a
     * second one cannot join it), two of 2w waves beyond (56 KB each: a third cannot); grid = CUs x that, so
     * every block is resident at once and every SIMD holds exactly w waves (a workgroup's waves go round the
     * four SIMDs).  */
    const int ws[] = {1, 2, 3, 4, 5, 6, 8};
    for (const Entry &e : kEntries) {
        if (only && !std::strstr(e.name, only)) continue;
        CHECK(hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        for (int w : ws) {
            const int per_cu = w <= 4 ? 1 : 2;
            if ((4 * w) % per_cu) continue;
            const int waves_blk = 4 * w / per_cu;
            const size_t lds = per_cu == 1 ? 96 * 1024 : 56 * 1024;
            const int blocks = cus * per_cu, nw = blocks * waves_blk;
            CHECK(hipMemset(d_out, 0, (size_t)nw * 24));
            float fseed = 1.0f;
            double dseed = 1.0;
            uint32_t useed = 3u, c0 = (e.kind == 2 || e.kind == 3) ? 8u : 4u;
            uint64_t qseed = 3ull;
            void *args_u[] = {&d_out, (void *)&iters, &useed, &c0}, *args_f[] = {&d_out, (void *)&iters, &fseed, &c0},
                 *args_q[] = {&d_out, (void *)&iters, &qseed, &c0}, *args_d[] = {&d_out, (void *)&iters, &dseed, &c0};
            void **args = e.kind == 0 ? args_u : (e.kind == 1 ? args_f : (e.kind == 2 ? args_q : args_d));
            hipEvent_t a, b;
            CHECK(hipEventCreate(&a));
            CHECK(hipEventCreate(&b));
            /* one untimed launch (code fetch), one measured */
            CHECK(hipLaunchKernel(e.fn, dim3(blocks), dim3(64 * waves_blk), args, lds, nullptr));
            CHECK(hipEventRecord(a));
            CHECK(hipLaunchKernel(e.fn, dim3(blocks), dim3(64 * waves_blk), args, lds, nullptr));
            CHECK(hipEventRecord(b));
            CHECK(hipDeviceSynchronize());
            float ms = 0.f;
            CHECK(hipEventElapsedTime(&ms, a, b));
            CHECK(hipMemcpy(h.data(), d_out, (size_t)nw * 24, hipMemcpyDeviceToHost));
            /* Waves of one SIMD are not served evenly (the oldest ones issue first), so a wave's own duration says
             * little: the SIMD's cost per instruction is the makespan of all its waves over the instructions they
             * issued.  Makespan from s_memrealtime (100 MHz, the same counter everywhere), converted to shader cycles
             * with the clock ratio the waves' own two counters give. */
            std::vector<unsigned long long> v(nw);
            std::vector<double> ratio(nw);
            unsigned long long first_start = ~0ull, last_start = 0, first_end = ~0ull, last_end = 0;
            for (int i = 0; i < nw; i++) {
                const unsigned long long d = h[(size_t)i * 3], r0 = h[(size_t)i * 3 + 1], r1 = h[(size_t)i * 3 + 2];
                v[i] = d;
                ratio[i] = (double)d / (double)(r1 > r0 ? r1 - r0 : 1);
                first_start = std::min(first_start, r0);
                last_start = std::max(last_start, r0);
                first_end = std::min(first_end, r1);
                last_end = std::max(last_end, r1);
            }
            std::sort(v.begin(), v.end());
            std::sort(ratio.begin(), ratio.end());
            const double cyc_per_tick = ratio[nw / 2];                       /* shader cycles per 10 ns */
            const double per = (double)iters * 64.0 * e.per_slot;
            const double makespan = (double)(last_end - first_start) * cyc_per_tick;
            const double fastest = (double)v[0] / per, slowest = (double)v[nw - 1] / per;
            std::printf("%s,%s,%d,%.3f,%.3f,%.3f,%.3f,%.1f,%.1f\n", e.name, e.salu, w, makespan / (per * w), fastest, slowest,
                        cyc_per_tick / 10.0, (double)(last_start - first_start) * 0.01, ms * 1e3);
            std::fflush(stdout);
            CHECK(hipEventDestroy(a));
            CHECK(hipEventDestroy(b));
        }
    }
    return 0;
}
