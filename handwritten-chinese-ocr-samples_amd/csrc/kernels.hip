// gfx950 (MI355X / CDNA4) kernels for the hctr CNN+CTC inference path.
//
// Reference semantics (file:line relative to the reference root) are cited per kernel; the
// tiling, layouts and fusion are this engine's own. Wavefront = 64 lanes throughout.
#include "kernels.h"

#include <algorithm>
#include <climits>
#include <cstdlib>

namespace hctr {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef void __attribute__((address_space(3))) * lptr_t;

// One 1-KiB LDS-DMA piece (global_load_lds_dwordx4: lane i -> LDS lds_dst + 16*i) issued from inline
// asm. hipcc's waitcnt pass drains lgkmcnt(0) at every wait while it can see an LDS-DMA in flight
// (measured: perfect counted waits once the DMA is hidden), so kernels that software-pipeline their
// ds_reads issue the DMA this way and retire it themselves with `s_waitcnt vmcnt(0)` before the
// barrier. M0 carries the LDS byte address and is restored (cdna guide section 5.7).
__device__ __forceinline__ void glds16_asm(const char* gsrc, char* lds_dst) {
    const uint32_t lds = (uint32_t)(uintptr_t)((lptr_t)lds_dst);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds)
                 : "memory");
}

// lane permutation inside a row of 16 lanes on the VALU data path (v_mov_b32_dpp)
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// np.argmax order (utils/ctc_codec.py:75): a NaN counts as the maximum, the FIRST maximum wins
__device__ __forceinline__ bool np_gt(float a, float b) { return a > b || (a != a && b == b); }
__device__ __forceinline__ bool np_eq(float a, float b) { return a == b || (a != a && b != b); }

// Same with a wave-uniform 64-bit base in SGPRs and a 32-bit per-lane byte offset (no 64-bit VALU address).
__device__ __forceinline__ void glds16_asm_s(const char* sbase, uint32_t voff, char* lds_dst) {
    const uint32_t lds = (uint32_t)(uintptr_t)((lptr_t)lds_dst);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds)
                 : "memory");
}

// Four pieces of one wave in ONE asm statement: same per-lane offset, four wave-uniform bases, four LDS addresses; M0 is
// saved and restored once instead of four times (six scalar moves fewer per K step).
__device__ __forceinline__ void glds16x4_asm_s(const char* s0, const char* s1, const char* s2, const char* s3, uint32_t voff,
                                               char* d0, char* d1, char* d2, char* d3) {
    const uint32_t l0 = (uint32_t)(uintptr_t)((lptr_t)d0), l1 = (uint32_t)(uintptr_t)((lptr_t)d1);
    const uint32_t l2 = (uint32_t)(uintptr_t)((lptr_t)d2), l3 = (uint32_t)(uintptr_t)((lptr_t)d3);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
                 "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4\n\t"
                 "s_mov_b32 m0, %9\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(s0), "s"(s1), "s"(s2), "s"(s3), "s"(l0), "s"(l1), "s"(l2), "s"(l3)
                 : "memory");
}

// Four pieces with ONE base, four per-lane offsets and LDS addresses LSTRIDE apart (halo rows): M0 is stepped inside the
// statement, so it takes two scalar inputs instead of five
template <int LSTRIDE>
__device__ __forceinline__ void glds16x4v_asm_s(const char* sbase, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, char* d0) {
    const uint32_t l0 = (uint32_t)(uintptr_t)((lptr_t)d0);
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
                 "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
                 "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
                 "s_add_u32 m0, m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase), "s"(l0), "i"(LSTRIDE)
                 : "memory", "scc");
}

// -------------------------------------------------------------------------------------------
// Shared epilogue of the MFMA conv kernels: + folded-BN bias, optional SE partial sums, ReLU,
// (2,1) max-pool, zeroing of columns >= W, fp16 NHWC store (or fp32 rows in linear mode).
// lane (q, c): for cout block cb (64 couts) the lane owns couts (jj>>1)*32 + q*8 + (jj&1)*4 + i (jj = j & 3),
// i.e. two runs of 8 consecutive couts, of pixel column c and pixel repeat n.
// -------------------------------------------------------------------------------------------
// cout offset of accumulator tile j inside a wave's cout range (see conv_epilogue)
__device__ __forceinline__ constexpr int acc_cout_offset(int j) { return (j >> 2) * 64 + ((j >> 1) & 1) * 32 + (j & 1) * 4; }

// SE scales below this are treated as this value on both sides of the downsample fusion (the accumulators hold
// residual / max(s, floor) and are multiplied by max(s, floor)): keeps the quotient finite for a saturated sigmoid
constexpr float kSeScaleFloor = 1e-12f;

template <int WN, int WM, int JT, bool LINEAR, bool SPLIT, bool PRIVATE_RED = false, bool BIAS_DONE = false,
          bool RESID_IN_ACC = false>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[JT][4], char* smem, int tid, int lane,
                                              int wn, int wm, int n0, int mt, int img, int th, int tw, int hbase,
                                              int w0, unsigned long long* st = nullptr) {
    // diagnostic instance only: st = this workgroup's stamp slots 8.. (after bias, residual, rounding, SE sums)
    auto estamp = [&](int i) {
        if (st != nullptr) {
            __builtin_amdgcn_sched_barrier(0);
            if (tid == 0) st[i] = __builtin_amdgcn_s_memrealtime();
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    constexpr int WC = JT * 16;
    constexpr int BN = WN * WC, BM = WM * 64;
    const int q = lane >> 4;
    const int c = lane & 15;
    const int cw0 = n0 + wn * WC + q * 8;       // + co(j) + i
    // cout offset of accumulator tile j (cb = j>>2 the 64-cout block, jj = j&3): a lane owns two runs of 8
    // consecutive couts per block, q*8.. (jj 0,1) and 32+q*8.. (jj 2,3), so the four lanes of a pixel write
    // 64 contiguous bytes per store instruction (half a cache line without holes).
    auto co = [](int j) { return acc_cout_offset(j); };

    if (!BIAS_DONE) {                   // (the halo4 kernel starts its accumulators at the bias instead)
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const f32x4 b4 = *(const f32x4*)(a.bias + cw0 + co(j));
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][n][i] += b4[i];
        }
    }

    estamp(8);
    if (LINEAR && a.emit_cnt != nullptr) {
        // fused beam front end, PASS 2 (see ConvArgs): list every (class, logit >= vmin[row]) and sum the row's
        // float64 exp terms expf(v - gmax) per class part - the terms row_topk_kernel sums over a stored row.
        static_assert(!LINEAR || WN == kLinearWN, "partials per n-tile");
        const int64_t part = (int64_t)((n0 / BN) * WN + wn) * a.M;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int64_t m = (int64_t)mt * BM + wm * 64 + n * 16 + c;
            const bool mv = m < a.M;
            const float vmin = mv ? a.row_thr[2 * m] : INFINITY;
            const float gmax = mv ? a.row_thr[2 * m + 1] : 0.f;
            double es = 0.0;
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int cls = cw0 + co(j) + i;
                    const float v = acc[j][n][i];
                    if (cls < a.Cout) {
                        es += (double)expf(v - gmax);
                        if (v >= vmin) {
                            const int pos = atomicAdd(a.emit_cnt + m, 1);
                            if (pos < a.emit_cap) {
                                int32_t* e = a.emit_list + ((int64_t)m * a.emit_cap + pos) * 2;
                                e[0] = cls;
                                e[1] = __builtin_bit_cast(int32_t, v);
                            }
                        }
                    }
                }
            es += __shfl_xor(es, 16);
            es += __shfl_xor(es, 32);
            if (q == 0 && mv) a.esum[part + m] = es;
        }
        return;
    }
    if (LINEAR && a.amax_idx != nullptr) {
        // fused greedy argmax: classes rise with (j, i) for a lane and with q, wn, nt beyond it, so a strict
        // '>' keeps the first maximum inside a lane and the (value, class) merge keeps it across lanes.
        // Guarded precision (a.amax_val2 set): the part's runner-up value and largest |logit| ride along.
        static_assert(!LINEAR || WN == kLinearWN, "partials per n-tile");
        const int64_t part = (int64_t)((n0 / BN) * WN + wn) * a.M;
        const bool guard = a.amax_val2 != nullptr;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            float bv = -INFINITY, sv = -INFINITY, av = 0.f;
            int bi = 0x7fffffff;
            if (!guard) {
#pragma unroll
                for (int j = 0; j < JT; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int cls = cw0 + co(j) + i;
                        const float v = acc[j][n][i];
                        if (cls < a.Cout && np_gt(v, bv)) { bv = v; bi = cls; }
                    }
            } else {
#pragma unroll
                for (int j = 0; j < JT; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int cls = cw0 + co(j) + i;
                        const float v = acc[j][n][i];
                        if (cls < a.Cout) {
                            av = fmaxf(av, fabsf(v));
                            if (np_gt(v, bv)) { sv = bv; bv = v; bi = cls; }
                            else if (np_gt(v, sv)) sv = v;
                        }
                    }
            }
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const float ov = __shfl_xor(bv, off);
                const int oi = __shfl_xor(bi, off);
                const bool wins = np_gt(ov, bv) || (np_eq(ov, bv) && oi < bi);
                if (guard) {                       // runner-up of the union: the loser's best or the winner's second
                    const float osv = __shfl_xor(sv, off);
                    const float lose = wins ? bv : ov, keep2 = wins ? osv : sv;
                    sv = np_gt(lose, keep2) ? lose : keep2;
                    av = fmaxf(av, __shfl_xor(av, off));
                }
                if (wins) { bv = ov; bi = oi; }
            }
            const int64_t m = (int64_t)mt * BM + wm * 64 + n * 16 + c;
            if (q == 0 && m < a.M) {
                a.amax_val[part + m] = bv;
                a.amax_idx[part + m] = bi;
                if (guard) {
                    a.amax_val2[part + m] = sv;
                    a.amax_abs[part + m] = av;
                }
            }
            if (a.psum != nullptr) {
                // beam front end, PASS 1: sum of expf(v - part max) per (part, row), and the logit of class 0
                float ps = 0.f;
#pragma unroll
                for (int j = 0; j < JT; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (cw0 + co(j) + i < a.Cout) ps += expf(acc[j][n][i] - bv);
                ps += __shfl_xor(ps, 16);
                ps += __shfl_xor(ps, 32);
                if (q == 0 && m < a.M) {
                    a.psum[part + m] = ps;
                    if (cw0 == 0) a.blank_logit[m] = acc[0][n][0];          // cw0 == 0: n0 == 0, wn == 0 (and q == 0)
                }
            }
        }
        return;
    }
    if (LINEAR) {
        float* out = (float*)a.y;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int64_t m = (int64_t)mt * BM + wm * 64 + n * 16 + c;
            if (m < a.M) {
#pragma unroll
                for (int j = 0; j < JT; ++j)
                    *(f32x4*)(out + m * a.ldo + cw0 + co(j)) = acc[j][n];
            }
        }
        return;
    }

    const int w = w0 + c;
    const bool wvalid = w < a.W;
    half_t* out = (half_t*)a.y;
    const int64_t pix0 = a.out_off + img * a.out_sb + (int64_t)w * a.out_sw + cw0;

    // fused squeeze-excite + residual (BasicBlock :54-58): acc = acc * scale[img][cout] + residual
    if (SPLIT && !RESID_IN_ACC && a.se_scale != nullptr) {
        // f16x3: the residual is hi + lo (planes Cout apart); loaded per (cb, n), accuracy mode only
        const float* sc = a.se_scale + (int64_t)img * a.Cout + cw0;
        if (w < a.out_wlimit) {
#pragma unroll
            for (int cb = 0; cb < JT / 4; ++cb)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const half_t* r = a.resid + pix0 + (int64_t)(hbase + n) * a.out_sh + cb * 64;
                    const f16x8 h0 = *(const f16x8*)r, h1 = *(const f16x8*)(r + 32);
                    const f16x8 l0 = *(const f16x8*)(r + a.Cout), l1 = *(const f16x8*)(r + a.Cout + 32);
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const float rv = e < 8 ? (float)h0[e] + (float)l0[e] : (float)h1[e - 8] + (float)l1[e - 8];
                        const float sv = sc[cb * 64 + (e >> 3) * 32 + (e & 7)];
                        acc[cb * 4 + (e >> 2)][n][e & 3] = fmaf(acc[cb * 4 + (e >> 2)][n][e & 3], sv, rv);
                    }
                }
        }
    } else if (RESID_IN_ACC) {
        // fused downsample (halo4 DSFUSE instance): the residual already sits in the accumulators as r / s
        // (compile-time branch: as a third runtime branch it made hipcc spill in every instance of this epilogue)
        const float* sc = a.se_scale + (int64_t)img * a.Cout + cw0;
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const f32x4 s4 = *(const f32x4*)(sc + co(j));
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][n][i] *= fmaxf(s4[i], kSeScaleFloor);
        }
    } else if (a.se_scale != nullptr) {
        const float* sc = a.se_scale + (int64_t)img * a.Cout + cw0;
        if (w < a.out_wlimit) {
            // all residual loads first (one latency exposure), 2 x 8 couts = 2 x 16 B per (cb, n)
            f16x8 rlo[JT / 4][4], rhi[JT / 4][4];
#pragma unroll
            for (int cb = 0; cb < JT / 4; ++cb)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const half_t* r = a.resid + pix0 + (int64_t)(hbase + n) * a.out_sh + cb * 64;
                    rlo[cb][n] = *(const f16x8*)r;
                    rhi[cb][n] = *(const f16x8*)(r + 32);
                }
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                const f32x4 s4 = *(const f32x4*)(sc + co(j));
#pragma unroll
                for (int n = 0; n < 4; ++n)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = (j & 3) * 4 + i;
                        const float r = e < 8 ? (float)rlo[j >> 2][n][e] : (float)rhi[j >> 2][n][e - 8];
                        acc[j][n][i] = fmaf(acc[j][n][i], s4[i], r);
                    }
            }
        }
    }

    estamp(9);
    if (!SPLIT) {
        // One rounding to fp16 (v_cvt_pk_f16_f32, RNE), then ReLU and the column mask on PACKED halves:
        // rounding is monotonic and keeps the sign, so relu(round(v)) == round(relu(v)). P holds exactly the
        // stored values; about 2 VALU ops per value instead of 7.
        const _Float16 lo1 = a.relu ? (_Float16)0.f : (_Float16)(-INFINITY);
        const f16x2 lo2 = {lo1, lo1};
        const uint32_t keep = wvalid ? 0xffffffffu : 0u;
        uint32_t P[JT][4][2];
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                f32x4 v = acc[j][n];
                if (a.pool) {                                    // (2,1) max-pool -> even n; odd n unused
                    const f32x4 u = acc[j][n | 1];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = fmaxf(acc[j][n & ~1][i], u[i]);
                }
                f16x2 h0 = __builtin_convertvector((f32x2){v[0], v[1]}, f16x2);
                f16x2 h1 = __builtin_convertvector((f32x2){v[2], v[3]}, f16x2);
                h0 = __builtin_elementwise_max(h0, lo2);
                h1 = __builtin_elementwise_max(h1, lo2);
                P[j][n][0] = __builtin_bit_cast(uint32_t, h0) & keep;
                P[j][n][1] = __builtin_bit_cast(uint32_t, h1) & keep;
            }
        estamp(10);
        if (a.se_part != nullptr) {
            // per-(image, channel) sums of the stored values over this block's pixels, fixed reduction
            // order (deterministic: lane tree -> LDS -> one partial row per block; no float atomics).
            if (!PRIVATE_RED) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a trailing LDS-DMA (if any) has landed
                __syncthreads();                   // main-loop LDS no longer needed
            }
            float* red = (float*)smem;             // [WM][BN]
            // Sum over the wave's 64 pixels per cout: first the lane's four rows, then a REDUCE-SCATTER butterfly over
            // the 16 pixel columns of a lane row (DPP quad_perm xor 1, xor 2, row_half_mirror, row_mirror). At every
            // level a lane keeps half of its values and hands the other half to its partner, so the 4 levels cost
            // 16 + 8 + 4 + 2 exchanges instead of 4 x 32, and every lane ends with JT/4 finished sums (one store each,
            // no masked writes). The additions are exactly the full butterfly's (pair sums, quad sums, half-row sums, row
            // sums; an fp add commutes), so the results are bit-identical to summing every value in every lane.
            // Which half a lane keeps must agree between mirror partners: bits e0 = b0^b2, e1 = b1^b2, e2 = b2^b3, e3 = b3
            // of the column c = b3 b2 b1 b0 (c^1 flips only e0, c^2 only e1, c^7 only e2, c^15 only e3).
            constexpr int NV = JT * 4;
            float vals[NV];
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float t[4];
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        t[n] = (float)__builtin_bit_cast(f16x2, P[j][n][i >> 1])[i & 1];
                    vals[j * 4 + i] = (t[0] + t[1]) + (t[2] + t[3]);
                }
            const bool e0 = ((c ^ (c >> 2)) & 1) != 0, e1 = (((c >> 1) ^ (c >> 2)) & 1) != 0;
            const bool e2 = (((c >> 2) ^ (c >> 3)) & 1) != 0, e3 = ((c >> 3) & 1) != 0;
            float r1[NV / 2], r2[NV / 4], r3[NV / 8], r4[NV / 16];
#pragma unroll
            for (int u = 0; u < NV / 2; ++u)
                r1[u] = (e0 ? vals[2 * u + 1] : vals[2 * u]) + dpp_f32<0xB1>(e0 ? vals[2 * u] : vals[2 * u + 1]);
#pragma unroll
            for (int u = 0; u < NV / 4; ++u)
                r2[u] = (e1 ? r1[2 * u + 1] : r1[2 * u]) + dpp_f32<0x4E>(e1 ? r1[2 * u] : r1[2 * u + 1]);
#pragma unroll
            for (int u = 0; u < NV / 8; ++u)
                r3[u] = (e2 ? r2[2 * u + 1] : r2[2 * u]) + dpp_f32<0x141>(e2 ? r2[2 * u] : r2[2 * u + 1]);
#pragma unroll
            for (int u = 0; u < NV / 16; ++u)
                r4[u] = (e3 ? r3[2 * u + 1] : r3[2 * u]) + dpp_f32<0x140>(e3 ? r3[2 * u] : r3[2 * u + 1]);
            const int vlow = (e3 ? 8 : 0) + (e2 ? 4 : 0) + (e1 ? 2 : 0) + (e0 ? 1 : 0);
#pragma unroll
            for (int u = 0; u < NV / 16; ++u) {
                const int v = 16 * u + vlow, j = v >> 2, i = v & 3;      // this lane's finished sum: value j*4 + i
                red[wm * BN + wn * WC + q * 8 + ((j >> 2) * 64 + ((j >> 1) & 1) * 32 + (j & 1) * 4) + i] = r4[u];
            }
            __syncthreads();
            if (tid < BN) {
                float sum = 0.f;
#pragma unroll
                for (int m = 0; m < WM; ++m) sum += red[m * BN + tid];
                const int64_t tile = (int64_t)img * (a.tilesH * a.tilesW) + th * a.tilesW + tw;
                if (n0 + tid < a.Cout) a.se_part[tile * a.Cout + n0 + tid] = sum;
            }
        }
        estamp(11);
        if (a.dbg & 256) {           // dbg 256: timing experiment without the output stores
            uint32_t t = 0;
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int n = 0; n < 4; ++n) t += P[j][n][0] ^ P[j][n][1];
            if (t == 0x12345678u) out[0] = (half_t)1.f;
        } else if (w < a.out_wlimit) {
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if (a.pool && (n & 1)) continue;
                const int ho = a.pool ? ((hbase + n) >> 1) : (hbase + n);
                half_t* o = out + pix0 + (int64_t)ho * a.out_sh;
#pragma unroll
                for (int cb = 0; cb < JT / 4; ++cb) {
                    const int j0 = cb * 4;
                    *(u32x4*)(o + cb * 64) = (u32x4){P[j0][n][0], P[j0][n][1], P[j0 + 1][n][0], P[j0 + 1][n][1]};
                    *(u32x4*)(o + cb * 64 + 32) =
                        (u32x4){P[j0 + 2][n][0], P[j0 + 2][n][1], P[j0 + 3][n][0], P[j0 + 3][n][1]};
                }
            }
        }
        return;
    }
    // f16x3 (SPLIT) tail. ReLU, column mask, fp16 rounding (in place: acc holds exactly what the planes add up to)
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v = acc[j][n][i];
                if (a.pool && (n & 1) == 0) v = fmaxf(v, acc[j][n + 1][i]);   // (2,1) max-pool -> even n
                if (a.relu) v = fmaxf(v, 0.f);
                if (!wvalid) v = 0.f;
                if (SPLIT) {                        // stored as hi + lo: keep what the two planes add up to
                    const half_t hi = (half_t)v;
                    v = a.drop_lo ? (float)hi : (float)hi + (float)(half_t)(v - (float)hi);      // (drop_lo: lo plane = 0 below)
                } else {
                    v = (float)(half_t)v;
                }
                acc[j][n][i] = v;
            }

    estamp(10);
    if (a.se_part != nullptr) {
        // per-(image, channel) sums of the stored values over this block's pixels, fixed reduction
        // order (deterministic: lane tree -> LDS -> one partial row per block; no float atomics).
        if (!PRIVATE_RED) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // a trailing LDS-DMA (if any) has landed
            __syncthreads();                   // main-loop LDS no longer needed
        }
        float* red = (float*)smem;             // [WM][BN]
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float s = (acc[j][0][i] + acc[j][1][i]) + (acc[j][2][i] + acc[j][3][i]);
                // butterfly over the 16 pixel columns of a lane row on the VALU (DPP), not through ds_bpermute:
                // pairs (c, c^1), (c, c^2), then the mirrored lane of the other quad / other half, which holds
                // the same partial sum the xor-4 / xor-8 partner would - bitwise the xor butterfly's result
                s += dpp_f32<0xB1>(s);            // quad_perm [1,0,3,2]
                s += dpp_f32<0x4E>(s);            // quad_perm [2,3,0,1]
                s += dpp_f32<0x141>(s);           // row_half_mirror
                s += dpp_f32<0x140>(s);           // row_mirror
                if (c == 0) red[wm * BN + wn * WC + q * 8 + co(j) + i] = s;
            }
        __syncthreads();
        if (tid < BN) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < WM; ++m) s += red[m * BN + tid];
            const int64_t tile = (int64_t)img * (a.tilesH * a.tilesW) + th * a.tilesW + tw;
            if (n0 + tid < a.Cout) a.se_part[tile * a.Cout + n0 + tid] = s;
        }
    }

    estamp(11);
    if (a.dbg & 256) {           // dbg 256: timing experiment without the output stores
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < JT; ++j)
#pragma unroll
            for (int n = 0; n < 4; ++n) t += acc[j][n][0] + acc[j][n][1] + acc[j][n][2] + acc[j][n][3];
        if (t == 123.456f) out[0] = (half_t)t;
    } else if (w < a.out_wlimit) {
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (a.pool && (n & 1)) continue;
            const int ho = a.pool ? ((hbase + n) >> 1) : (hbase + n);
            half_t* o = out + pix0 + (int64_t)ho * a.out_sh;
#pragma unroll
            for (int cb = 0; cb < JT / 4; ++cb) {
                f16x8 lo, hi;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const half_t hv = (half_t)acc[cb * 4 + (e >> 2)][n][e & 3];
                    if (e < 8) lo[e] = hv; else hi[e - 8] = hv;
                }
                *(f16x8*)(o + cb * 64) = lo;
                *(f16x8*)(o + cb * 64 + 32) = hi;
                if (SPLIT) {                        // planes: [hi | lo | hi]
                    f16x8 l0, l1;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const float v = acc[cb * 4 + (e >> 2)][n][e & 3];
                        const half_t lv = (half_t)(v - (float)(half_t)v);
                        if (e < 8) l0[e] = lv; else l1[e - 8] = lv;
                    }
                    *(f16x8*)(o + a.Cout + cb * 64) = l0;
                    *(f16x8*)(o + a.Cout + cb * 64 + 32) = l1;
                    *(f16x8*)(o + 2 * a.Cout + cb * 64) = lo;
                    *(f16x8*)(o + 2 * a.Cout + cb * 64 + 32) = hi;
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------------------
// conv_mfma: 3x3 (pad 1) / 1x1 convolution + folded BatchNorm (+ReLU, +(2,1) max-pool,
// +squeeze-excite partial sums) as an implicit GEMM on v_mfma_f32_16x16x32_f16.
//
// Reference ops fused here: nn.Conv2d(k,1,pad) -> BatchNorm2d(eval) -> ReLU -> max_pool2d((2,1))
// (models/handwritten_ctr_model.py:116-150, 47-53) and the spatial sum that SELayer's
// AdaptiveAvgPool2d needs (:27); in linear mode: self.linear (:175).
//
// GEMM view: D[cout][pixel] = sum_{tap,cin} Wt[tap][cout][cin] * X[pixel + tap][cin]
//   MFMA A operand = weights (rows = couts), B operand = pixels (cols), so every lane ends up with
//   two runs of 8 consecutive couts of one pixel; the 4 lanes of a pixel store 64 contiguous bytes.
// Block = WN x WM waves; each wave owns JT*16 couts x 64 pixels (JT x 4 MFMA tiles): 64 couts
//   (64 fp32 acc regs) for the 64x256 and 128x128 block tiles, 128 couts for the 256x256 tile.
//   conv mode: a wave's 64 pixels are a 4-row x 16-column patch; MFMA column c = image column,
//   pixel repeat n = image row, so the (2,1) max-pool pairs repeats (0,1),(2,3) inside a lane.
// K loop: taps x (Cin/64) steps; both operand tiles ([rows][64 cin] fp16 = 128-byte rows) are
//   staged with global_load_lds_dwordx4 into a double-buffered LDS image. The zero padding of the
//   convolution is stored in memory (1-pixel zero border), so a tap is only an address offset.
// LDS image: linear per wave-instruction (8 rows x 128 B), 16-byte chunk index XOR (row & 7)
//   applied on the global SOURCE address and again on the ds_read_b128 address (conflict-free for
//   the 16x16x32 operand pattern; cdna guide rule 21).
// -------------------------------------------------------------------------------------------
template <int WN, int WM, int JT, int TAPS, bool LINEAR, bool PIPE, bool SPLIT>
__global__ __launch_bounds__(WN* WM * 64) void conv_mfma_kernel(const ConvArgs a) {
    constexpr int NT = WN * WM * 64;
    constexpr int WC = JT * 16;          // couts per wave (64 or 128)
    constexpr int BN = WN * WC, BM = WM * 64;
    constexpr int NIW = BN * 8 / NT;     // 16-byte chunks of the weight tile per thread
    constexpr int NIX = BM * 8 / NT;     // ... of the pixel tile
    constexpr int TILE_BYTES = (BN + BM) * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv / WM, wm = wv % WM;

    // ---- block -> (m_tile, n_tile), XCD-aware: each XCD walks a contiguous run of the
    //      (m-major, n-minor) order so the n-tiles of one pixel tile share that XCD's L2.
    const int total = a.mtiles * a.ntiles;
    int lin;
    {
        const int id = blockIdx.x, xcd = id & 7, s = id >> 3;
        const int q = total >> 3, r = total & 7;
        lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + s;
    }
    const int nt = lin % a.ntiles;
    const int mt = lin / a.ntiles;
    const int n0 = nt * BN;

    int img = 0, th = 0, tw = 0;
    if (!LINEAR) {
        tw = mt % a.tilesW;
        const int t2 = mt / a.tilesW;
        th = t2 % a.tilesH;
        img = t2 / a.tilesH;
    }
    const int cin = a.Cin;

    // ---- per-thread staging sources: uniform base (SGPRs) + 32-bit per-lane byte offset ----
    const char* xbase;
    if (LINEAR) xbase = (const char*)(a.x + (int64_t)mt * BM * cin);
    else xbase = (const char*)(a.x + img * a.in_sb);
    const char* wbase = (const char*)(a.w + (int64_t)n0 * cin);
    uint32_t xoff[NIX], woff[NIW];
#pragma unroll
    for (int i = 0; i < NIX; ++i) {
        const int g = (wv * NIX + i) * 64 + lane;
        const int row = g >> 3, cp = (g & 7) ^ (row & 7);
        if (LINEAR) {
            int64_t rem = a.M - (int64_t)mt * BM;            // rows left in this tile (>= 1)
            const int r = (int64_t)row < rem ? row : (int)rem - 1;
            xoff[i] = (uint32_t)r * (uint32_t)cin * 2u + cp * 16;
        } else {
            const int h = th * (4 * WM) + (row >> 6) * 4 + ((row >> 4) & 3);
            const int w = tw * kTileW + (row & 15);
            xoff[i] = ((uint32_t)(h + 1) * (uint32_t)a.in_sh + (uint32_t)(w + 1) * (uint32_t)cin) * 2u + cp * 16;
        }
    }
#pragma unroll
    for (int i = 0; i < NIW; ++i) {
        const int g = (wv * NIW + i) * 64 + lane;
        const int row = g >> 3, cp = (g & 7) ^ (row & 7);
        woff[i] = (uint32_t)row * (uint32_t)cin * 2u + cp * 16;
    }

    const int kc_steps = cin / kBK;
    const int nk = TAPS * kc_steps;

    // uniform source offsets of K step k. Order: 64-channel chunk outermost, the 9 taps innermost, so
    // a block re-reads the same 18x18-pixel x 128-byte halo (41 KB) nine times in a row out of L1/L2.
    // (Tap-major order swept all Cin per tap: reuse distance 256 KB x 32 blocks per XCD >> 4 MB L2,
    // measured 17.4 GB FETCH_SIZE per 512->512@16 launch against 2.4 GB of input.)
    auto step_offsets = [&](int k, int64_t& wo, int64_t& xo) {
        int tap = 0, kc = k;
        if (TAPS > 1) { kc = k / TAPS; tap = k - kc * TAPS; }
        xo = (int64_t)kc * (kBK * 2);
        if (TAPS > 1) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            xo += ((int64_t)dy * a.in_sh + (int64_t)dx * cin) * 2;
        }
        wo = ((int64_t)tap * a.CoutPad * cin + (int64_t)kc * kBK) * 2;
    };
    // one 1-KiB LDS-DMA piece (idx < NIW: weight tile, else pixel tile) into buffer buf, issued from inline asm like the
    // halo kernels' (see glds16_asm; measured 3.63 -> 3.53 ms per head-GEMM launch against the builtin)
    auto stage_piece = [&](const char* wsrc, const char* xsrc, int buf, int idx) {
        if (idx < NIW) {
            char* wdst = smem + buf * TILE_BYTES + (wv * NIW) * 1024;
            glds16_asm_s(wsrc, woff[idx], wdst + idx * 1024);
        } else {
            char* xdst = smem + buf * TILE_BYTES + BN * 128 + (wv * NIX) * 1024;
            glds16_asm_s(xsrc, xoff[idx - NIW], xdst + (idx - NIW) * 1024);
        }
    };
    auto stage = [&](int k, int buf) {
        int64_t wo, xo;
        step_offsets(k, wo, xo);
#pragma unroll
        for (int i = 0; i < NIW + NIX; ++i) stage_piece(wbase + wo, xbase + xo, buf, i);
    };

    f32x4 acc[JT][4];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[j][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // per-lane fragment offsets inside a tile: row (lane&15), logical chunk ks*4 + (lane>>4)
    const int q = lane >> 4;
    const int frow = lane & 15;
    const int foff0 = frow * 128 + (((0 + q) ^ (lane & 7)) << 4);
    const int foff1 = frow * 128 + (((4 + q) ^ (lane & 7)) << 4);

    stage(0, 0);
    if (!PIPE) {
        for (int k = 0; k < nk; ++k) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const char* wt = smem + (k & 1) * TILE_BYTES + (wn * WC) * 128;
            const char* xt = smem + (k & 1) * TILE_BYTES + BN * 128 + (wm * 64) * 128;
            if (JT == 8) {
                // 8-accumulator-tile waves (256x256 tile: the head GEMM) run the halo kernels' rolling fragment pipeline:
                // A pairs read two MFMA groups ahead, second-half B fragments during group 1, the next step's DMA burst
                // after the first reads (measured 3.53 -> 3.39 ms per head launch against the half-step form below)
                f16x8 ar[3][2], bq[2][4];
                auto read_a = [&](int g, f16x8 (&dst)[2]) {
                    const char* base = wt + ((g >> 2) ? foff1 : foff0);
                    dst[0] = *(const f16x8*)(base + (2 * (g & 3)) * 2048);
                    dst[1] = *(const f16x8*)(base + (2 * (g & 3) + 1) * 2048);
                };
                auto read_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
                    for (int n = 0; n < 4; ++n) dst[n] = *(const f16x8*)(xt + n * 2048 + (ks ? foff1 : foff0));
                };
                __builtin_amdgcn_sched_barrier(0);
                read_b(0, bq[0]);
                read_a(0, ar[0]);
                __builtin_amdgcn_sched_barrier(0);
                read_a(1, ar[1]);
                __builtin_amdgcn_sched_barrier(0);
                if (k + 1 < nk) stage(k + 1, (k + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    if (g + 2 < 8) read_a(g + 2, ar[(g + 2) % 3]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (g == 1) { read_b(1, bq[1]); __builtin_amdgcn_sched_barrier(0); }
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int n = 0; n < 4; ++n)
                            acc[2 * (g & 3) + jj][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ar[g % 3][jj], bq[g >> 2][n],
                                                                                             acc[2 * (g & 3) + jj][n], 0, 0, 0);
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                continue;
            }
            if (k + 1 < nk) stage(k + 1, (k + 1) & 1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int fo = ks ? foff1 : foff0;
                f16x8 af[JT], bf[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) bf[n] = *(const f16x8*)(xt + n * 2048 + fo);
#pragma unroll
                for (int j = 0; j < JT; ++j) af[j] = *(const f16x8*)(wt + j * 2048 + fo);
                __builtin_amdgcn_s_setprio(1);     // keeps the MFMA cluster together (measured +4 %)
#pragma unroll
                for (int j = 0; j < JT; ++j)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[j], bf[n], acc[j][n], 0, 0, 0);
                __builtin_amdgcn_s_setprio(0);
            }
        }
    } else {
        // Finely interleaved K step: 2*JT groups of {prefetch the next A fragment, one LDS-DMA piece of
        // the next K step every other group, 4 MFMAs}. The two waves that share a SIMD then mix memory
        // issue and matrix work instead of bursting both at the barrier. Measured on MI355X (round 1,
        // config 2): 8.25 ms vs 7.75-8.05 ms per dominant launch for the burst form, so it is OFF by
        // default (HCTR_PIPE=1 enables it for A/B runs).
        constexpr int NG = 2 * JT;
        constexpr int NP = NIW + NIX;
        for (int k = 0; k < nk; ++k) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            // next step's DMA is unconditional (branch-free loop): on the last step it re-stages that
            // step into the idle buffer, which nobody reads (drained before the epilogue reuses LDS).
            const int kn = k + 1 < nk ? k + 1 : k;
            int64_t wo_n, xo_n;
            step_offsets(kn, wo_n, xo_n);
            const char* wsrc_n = wbase + wo_n;
            const char* xsrc_n = xbase + xo_n;
            const int buf_n = (k + 1) & 1;
            const char* wt = smem + (k & 1) * TILE_BYTES + (wn * WC) * 128;
            const char* xt = smem + (k & 1) * TILE_BYTES + BN * 128 + (wm * 64) * 128;
            f16x8 bfr[2][4], afr[2];
#pragma unroll
            for (int n = 0; n < 4; ++n) bfr[0][n] = *(const f16x8*)(xt + n * 2048 + foff0);
            afr[0] = *(const f16x8*)(wt + foff0);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int ks = g / JT, j = g % JT;
                if (g + 1 < NG) {
                    const int ks1 = (g + 1) / JT, j1 = (g + 1) % JT;
                    afr[(g + 1) & 1] = *(const f16x8*)(wt + j1 * 2048 + (ks1 ? foff1 : foff0));
                }
                if (g == JT / 2) {
#pragma unroll
                    for (int n = 0; n < 4; ++n) bfr[1][n] = *(const f16x8*)(xt + n * 2048 + foff1);
                }
                if ((g * NP) / NG != ((g + 1) * NP) / NG)      // NP pieces spread over NG groups
                    stage_piece(wsrc_n, xsrc_n, buf_n, (g * NP) / NG);
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[g & 1], bfr[ks][n], acc[j][n], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    conv_epilogue<WN, WM, JT, LINEAR, SPLIT>(a, acc, smem, tid, lane, wn, wm, n0, mt, img, th, tw,
                                             th * (4 * WM) + wm * 4, tw * kTileW);
}

// HCTR_DBG (timing experiments, results INVALID) applies to every conv launch - unless HCTR_DBG_LAYER names ONE layer, in
// which case the engine sets ConvArgs::dbg for that layer only (the others then run on real data at the real clock)
static int env_dbg() {
    if (getenv("HCTR_DBG_LAYER")) return 0;
    const char* e = getenv("HCTR_DBG");
    return e ? atoi(e) : 0;
}

// hipFuncSetAttribute is per device: remember which devices already raised a kernel's LDS limit
// (a process may own contexts on several GPUs).
static hipError_t raise_lds_limit(const void* fn, int bytes, bool (&done)[64]) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (done[dev]) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done[dev] = true;
    return e;
}

// -------------------------------------------------------------------------------------------
// conv3x3_halo: the 3x3 layers on the 256-cout x (16x16-pixel) tile with the pixel operand staged
// ONCE per 64-channel chunk. The generic kernel re-stages a shifted 16x16 window for each of the
// 9 taps (8 LDS-DMA pieces per wave per K step); on MI355X the burst of DMA issue after every
// barrier is what idles the matrix pipe (SQ counters: MFMA busy 56 %, no LDS conflicts, fabric
// traffic irrelevant). Here a block keeps an 18x18-pixel halo x 64 channels (rows of 128 B, row
// stride 20 pixels so the swizzle key stays cheap) in LDS and reads the tap-shifted B fragments from
// it, so only the 32 KB weight tile streams per K step: 4 + 6/9 pieces per wave per step instead of 8.
// LDS: 2 x 32 KB weights (double-buffered per K step) + 2 x 45 KB halo (double-buffered per chunk).
// -------------------------------------------------------------------------------------------
constexpr int kHaloCols = 20;                            // row stride in pixels (18 used)
constexpr int kHaloRows = 18;
constexpr int kHaloBytes = kHaloRows * kHaloCols * 128;  // 46080
constexpr int kHaloPieces = kHaloRows * kHaloCols / 8;   // 45 one-KiB DMA pieces
constexpr int kHaloLds = 2 * 32768 + 2 * kHaloBytes;     // 157696

template <bool SPLIT>
__global__ __launch_bounds__(512) void conv3x3_halo_kernel(const ConvArgs a) {
    constexpr int WN = 2, WM = 4, JT = 8, BN = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv / WM, wm = wv % WM;

    const int total = a.mtiles * a.ntiles;
    int lin;
    {
        const int id = blockIdx.x, xcd = id & 7, s = id >> 3;
        const int q = total >> 3, r = total & 7;
        lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + s;
    }
    const int nt = lin % a.ntiles;
    const int mt = lin / a.ntiles;
    const int n0 = nt * BN;
    const int tw = mt % a.tilesW;
    const int t2 = mt / a.tilesW;
    const int th = t2 % a.tilesH;
    const int img = t2 / a.tilesH;
    const int cin = a.Cin;
    const int nkc = cin / kBK;

    // ---- DMA sources ------------------------------------------------------------------------
    // halo origin = padded pixel (th*16, tw*16) = output pixel (th*16 - 1, tw*16 - 1)
    const char* xbase = (const char*)(a.x + img * a.in_sb + (int64_t)(th * 16) * a.in_sh + (int64_t)(tw * 16) * cin);
    const char* wbase = (const char*)(a.w + (int64_t)n0 * cin);
    // Asymmetric staging: only waves 0..3 issue LDS-DMA (8 weight pieces per K step + 2 halo pieces on
    // the first six steps of a chunk, each); their SIMD partners 4..7 go straight to their fragment
    // reads and MFMAs after the barrier, so the matrix pipe runs the partner's work while the loader
    // wave pays the DMA issue cost, then the loader's own.
    const bool loader = wv < 4;
    uint32_t woff[8], hoff[12];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int g = ((wv & 3) * 8 + i) * 64 + lane;
        const int row = g >> 3, cp = (g & 7) ^ (row & 7);
        woff[i] = (uint32_t)row * (uint32_t)cin * 2u + cp * 16;
    }
#pragma unroll
    for (int r = 0; r < 12; ++r) {                          // piece ((r>>1)*4 + wv)*2 + (r&1), step r>>1
        const int piece = ((r >> 1) * 4 + (wv & 3)) * 2 + (r & 1);
        const int g = piece * 64 + lane;
        const int row = g >> 3, cp = (g & 7) ^ (row & 7);
        int hy = row / kHaloCols, hx = row - hy * kHaloCols;
        if (hx > 17) hx = 17;                               // pad columns: any valid address
        if (hy > 17) hy = 17;                               // pieces >= 45 are never issued
        hoff[r] = ((uint32_t)hy * (uint32_t)a.in_sh + (uint32_t)hx * (uint32_t)cin) * 2u + cp * 16;
    }
    const int q = lane >> 4, c = lane & 15;
    const int aoff0 = c * 128 + (((0 + q) ^ (lane & 7)) << 4);
    const int aoff1 = c * 128 + (((4 + q) ^ (lane & 7)) << 4);

    auto stage_weights = [&](int kc, int tap, int buf) {
        const char* src = wbase + ((int64_t)tap * a.CoutPad * cin + (int64_t)kc * kBK) * 2;
        char* dst = smem + buf * 32768 + ((wv & 3) * 8) * 1024;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            glds16_asm(src + woff[i], dst + i * 1024);
    };
    auto stage_halo_piece = [&](int kc, int buf, int piece, uint32_t off) {
        if (piece < kHaloPieces) {                          // wave-uniform
            const char* src = xbase + (int64_t)kc * (kBK * 2);
            char* dst = smem + 65536 + buf * kHaloBytes + piece * 1024;
            glds16_asm(src + off, dst);
        }
    };

    f32x4 acc[JT][4];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[j][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

    if (loader) {
#pragma unroll
        for (int r = 0; r < 12; ++r) stage_halo_piece(0, 0, ((r >> 1) * 4 + wv) * 2 + (r & 1), hoff[r]);
        stage_weights(0, 0, 0);
    }

    for (int kc = 0; kc < nkc; ++kc) {
        const bool next_chunk = kc + 1 < nkc;
        const int hbuf = 65536 + (kc & 1) * kHaloBytes + (wm * 4) * (kHaloCols * 128);
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int k = kc * 9 + tap;
            // Retire the previous step's DMA. Steps 0..4 of a chunk issue (after the 8 weight pieces) two
            // pieces of the NEXT chunk's halo from every loader wave; they are cold (HBM) and not needed
            // for several steps, so they may stay in flight across this barrier: vmcnt(2) retires
            // everything older (vmcnt counts in issue order). All other steps drain completely.
            if (tap >= 1 && tap <= 5 && next_chunk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // B fragments: halo pixel row index hr = (wm*4 + n + 1 + dy)*20 + (c + 1 + dx); swizzle key
            // hr & 7 = ((c+1+dx) & 7) ^ 4*((n+1+dy) & 1)  (20 = 4 mod 8, +4 mod 8 = ^4). With the chunk
            // index ks*4 + q, the four (ks, n parity) cases need only two per-lane offsets, v0 and v0^64.
            const int tdy = tap / 3, dx = tap - tdy * 3 - 1;        // tdy = dy + 1
            const int u = c + 1 + dx;
            const int v0 = u * 128 + (((q ^ (u & 7) ^ ((tdy & 1) << 2)) & 7) << 4);
            const char* hb = smem + hbuf + tdy * (kHaloCols * 128);
            const char* be = hb + v0;           // ks=0 & n even, ks=1 & n odd
            const char* bo = hb + (v0 ^ 64);    // ks=0 & n odd,  ks=1 & n even
            const char* wt = smem + (k & 1) * 32768 + (wn * 128) * 128;
            // Rolling fragment pipeline: 8 groups of 8 MFMAs (2 A fragments x 4 B fragments). A pairs
            // are read two groups (16 MFMAs = 256 cycles) ahead into a 3-slot ring, the next ks's B
            // fragments during groups 1-2, so only the first 8 reads after the barrier are exposed.
            f16x8 ar[3][2], bq[2][4];
            auto read_a = [&](int g, f16x8 (&dst)[2]) {
                const int ks = g >> 2, jp = g & 3;
                const char* base = wt + (ks ? aoff1 : aoff0);
                dst[0] = *(const f16x8*)(base + (2 * jp) * 2048);
                dst[1] = *(const f16x8*)(base + (2 * jp + 1) * 2048);
            };
            auto read_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    dst[n] = *(const f16x8*)((((n & 1) ^ ks) ? bo : be) + n * (kHaloCols * 128));
            };
            __builtin_amdgcn_sched_barrier(0);
            read_b(0, bq[0]);
            read_a(0, ar[0]);
            __builtin_amdgcn_sched_barrier(0);
            read_a(1, ar[1]);
            __builtin_amdgcn_sched_barrier(0);
            // The DMA of the next step is issued AFTER the first fragment reads so its issue cost overlaps
            // their LDS latency (the asm DMA is invisible to the compiler's waitcnt bookkeeping).
            if (loader) {
                // next K step's weights (clamped on the very last step: re-stages into the idle buffer)
                int kc1 = kc, tap1 = tap + 1;
                if (tap1 == 9) { tap1 = 0; kc1 = next_chunk ? kc + 1 : kc; }
                if (a.dbg == 1) { kc1 = 0; tap1 = 0; }
                if (a.dbg != 2) stage_weights(kc1, tap1, (k + 1) & 1);
                // next chunk's halo: two pieces per loader wave on steps 0..5 (branch-free offset select)
                if (next_chunk && tap < 6 && a.dbg != 2) {
                    uint32_t h0 = hoff[0], h1 = hoff[1];
                    h0 = tap == 1 ? hoff[2] : h0;  h1 = tap == 1 ? hoff[3] : h1;
                    h0 = tap == 2 ? hoff[4] : h0;  h1 = tap == 2 ? hoff[5] : h1;
                    h0 = tap == 3 ? hoff[6] : h0;  h1 = tap == 3 ? hoff[7] : h1;
                    h0 = tap == 4 ? hoff[8] : h0;  h1 = tap == 4 ? hoff[9] : h1;
                    h0 = tap == 5 ? hoff[10] : h0; h1 = tap == 5 ? hoff[11] : h1;
                    const int p0 = (tap * 4 + wv) * 2;
                    const int kcs = a.dbg == 1 ? 0 : kc + 1;
                    stage_halo_piece(kcs, (kc + 1) & 1, p0, h0);
                    stage_halo_piece(kcs, (kc + 1) & 1, p0 + 1, h1);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const int ks = g >> 2, jp = g & 3;
                if (g + 2 < 8) read_a(g + 2, ar[(g + 2) % 3]);
                __builtin_amdgcn_sched_barrier(0);
                if (g == 1) { read_b(1, bq[1]); __builtin_amdgcn_sched_barrier(0); }
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[2 * jp + jj][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ar[g % 3][jj], bq[ks][n],
                                                                                    acc[2 * jp + jj][n], 0, 0, 0);
                __builtin_amdgcn_s_setprio(0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the last (redundant) DMA has landed
    // (f16x3: the K loop above only sees Cin' = 3 * Cin; the epilogue has to write all three planes of the output)
    conv_epilogue<WN, WM, JT, false, SPLIT>(a, acc, smem, tid, lane, wn, wm, n0, mt, img, th, tw, th * 16 + wm * 4,
                                            tw * 16);
}

// -------------------------------------------------------------------------------------------
// conv3x3_halo4: the same halo-reuse scheme as conv3x3_halo_kernel, but as a 4-wave workgroup
// (128 couts x 16x16 pixels, each wave 128 couts x 64 pixels) with 2 x 16 KB weight buffers and ONE
// 45 KB halo buffer = 77 KB of LDS, so TWO workgroups share a CU. The two waves on a SIMD then
// belong to different workgroups with independent barriers and drift out of phase, which hides
// the per-step barrier / DMA-latency bubble that the 8-wave lockstep structure exposes (SQ counters,
// DESIGN.md). The halo of the next chunk can only be fetched after the last tap of the current one
// (single buffer); the partner workgroup covers that stall.
// -------------------------------------------------------------------------------------------
// LDS layout of conv3x3_halo4_kernel and conv3x3_halo4h_kernel (byte offsets into the dynamic LDS)
namespace halo4_lds {
constexpr int kWeightBuf = 16384;                          // one K step's weight tile; buffer b at kWeights + b * kWeightBuf
constexpr int kWeights = 0;
constexpr int kHalo = kWeights + 2 * kWeightBuf;           // 32768: the halo image (halo4h: its two 32-channel halves)
constexpr int kScratch = kHalo + kHaloBytes;               // 78848: epilogue scratch, [WM = 4][BN = 128] floats of SE sums
constexpr int kScratchBytes = 4 * 128 * 4;
// Halo-offset table of the prefetching instances (kPrefetch in conv3x3_halo4_kernel): 4 waves x 12 pieces x 8 rows x 4 B.
// It ALIASES the epilogue scratch on purpose: the table is read for the last time inside the tile's last K step and the
// scratch is first written after it, so a workgroup that runs ONE tile never has both live. A persistent workgroup's
// epilogue would overwrite the table of its next tile, hence !(kPrefetch && PERSIST) in the kernel.
constexpr int kHaloTable = kScratch;
constexpr int kHaloTableBytes = 4 * 12 * 8 * 4;
constexpr int kNextTile = kScratch + kScratchBytes;        // 80896: two words, the persistent instances' drawn tile index
constexpr int kTotal = kNextTile + 16;                     // 80912
static_assert(kHaloTableBytes <= kScratchBytes, "the halo-offset table fits inside the epilogue scratch it aliases");
static_assert(kNextTile >= kScratch + kScratchBytes, "the next-tile words lie behind the epilogue scratch");
static_assert(kTotal <= 80 * 1024, "two workgroups per CU on 160 KB of LDS");
}  // namespace halo4_lds

// GEOM 0: 16 rows x 16 columns (halo 18 x 18, row stride 20); GEOM 1: 8 rows x 32 columns for the
// H = 8 stage (halo 10 x 34, row stride 36). Both strides are 4 (mod 8) and both halos are 360 rows.
// STAMP: diagnostic instance (hctr_debug_stamps). Thread 0 of every workgroup writes wall-clock stamps
// (s_memrealtime, 100 MHz) of its phases plus its hardware placement to a buffer no other code reads:
//   [0] entry  [1] prologue DMA issued  [2] first operands landed (extra wait + barrier, stamp build only)
//   [3] K loop done  [4] epilogue done (stores issued)  [5] stores drained  [6] HW_ID  [7] XCC_ID
//   [8..11] inside the epilogue: bias added, residual applied, values rounded, SE sums written
// DSFUSE: a block's 1x1 downsample branch (models/handwritten_ctr_model.py:101-108, used at :49-50,57) runs as a
// pre-phase of conv2's K loop instead of as its own launch: acc = Wd * x over the block input's channels (centre
// tap of x's halo), then acc <- (acc + bd) / s + b2, then the 3x3 taps of conv2 accumulate on top and the epilogue
// multiplies by s: s * (W2*t + b2) + (Wd*x + bd). The residual is neither written nor read back (4.2 GB per launch).
// The K loop has its nine taps unrolled: tap / row / parity arithmetic and the step's branches fold into constants, the
// four weight pieces of a wave share ONE per-lane offset (the piece stride moves into the scalar base) and one M0 save /
// restore (measured -2.0 % per step against the rolled loop of rounds 1-3, bit-identical).
// RESPRE: conv2 of an identity block (BasicBlock :54-58, out = relu(o * s + x)). The SE scale s is known before conv2 runs
// (se_premean), so the residual x is fetched in the PROLOGUE - its HBM round trip overlaps the first operands' DMA wait -
// and the accumulators start at x / max(s, floor) + bias; the epilogue multiplies by max(s, floor), exactly what the
// fused downsample does with its 1x1 branch. The epilogue's residual phase (16 loads per lane issued behind the partner
// workgroup's DMA stream: 4.5 of its 7.6 us, profiles/r03_lean_workgroup_phases_*) disappears - and reappears in the
// prologue: measured slower as a whole (see launch_conv_halo4_t), kept as an opt-in experiment.
template <int GEOM, bool SPLIT, bool PERSIST, bool STAMP = false, bool DSFUSE = false, bool RESPRE = false>
__global__ __launch_bounds__(256, 2) void conv3x3_halo4_kernel(const ConvArgs a) {
    static_assert(!DSFUSE || !PERSIST, "downsample fusion: non-persistent instances only");
    static_assert(!RESPRE || (!DSFUSE && !PERSIST && !SPLIT), "residual-in-prologue: plain f16 instances only");
    constexpr int WN = 1, WM = 4, JT = 8, BN = 128;
    constexpr int TR = GEOM ? 8 : 16, TC = GEOM ? 32 : 16;       // tile rows / columns
    constexpr int S = TC + 4;                                      // halo row stride in pixels
    static_assert((TR + 2) * S * 128 == kHaloBytes, "halo footprint");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    auto stamp = [&](int i) {
        if (STAMP && tid == 0) a.stamps[(size_t)blockIdx.x * 16 + i] = __builtin_amdgcn_s_memrealtime();
    };
    stamp(0);
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv;
    const int cin = a.Cin;
    const int nkc = (a.dbg & 64) ? 0 : cin / kBK;       // dbg 64: timing experiment without the K loop
    const int nk = 9 * nkc;
    // The plain instances (f16 and f16x3, with or without the fused downsample) prefetch: a K step reads the NEXT tap's
    // first pixel fragments behind its own MFMA group kBpreAt (see mma_step), and the next chunk's halo reload is issued
    // inside tap 8, behind group kEarlyAt, from a table of piece offsets in LDS (halo4_lds::kHaloTable). Three instance
    // kinds cannot: STAMP and RESPRE have no registers left for the fragments that live across the step boundary (they
    // would spill), and a persistent workgroup's epilogue overwrites the table, which aliases its scratch, after every tile.
    constexpr bool kPrefetch = !PERSIST && !STAMP && !RESPRE;
    static_assert(!(kPrefetch && PERSIST), "the halo-offset table aliases the epilogue scratch: one tile per workgroup");
    constexpr int kRing = 3;        // A-fragment ring slots (prefetch distance kRing - 1 groups); 4 measured within +-0.3 %
    constexpr int kBhalfAt = 1;     // MFMA group before which the second half of the B fragments is read; 0 / 2 within +-0.3 %
    constexpr int kBpreAt = 4;      // group behind which the next tap's fragments are read (bq[0] is dead after group 3); 6: +4.4 %
    constexpr int kEarlyAt = 1;     // group of tap 8 behind which the halo reload is issued; 2 and 3 measured no better

    // ---- tiles of this workgroup. Every XCD owns a contiguous run of the (pixel-tile major, cout-tile
    //      minor) order. Non-persistent: one tile per workgroup. Persistent: the workgroups of an XCD
    //      stride through its run, and a workgroup prefetches its NEXT tile's first halo and weights
    //      while the current tile's epilogue runs (the cold per-tile prologue is ~10-30 % of a launch).
    // every kernel argument the prologue needs is requested here, in ONE batch of scalar loads and one wait (the compiler
    // otherwise fetches them in three dependent rounds, each a scalar-cache round trip on the critical path to the first DMA)
    {
        const int k0 = a.mtiles, k1 = a.ntiles, k2 = a.tilesW, k3 = a.tilesH, k4 = a.Cin, k5 = a.in_sh, k6 = a.nt_shift,
                  k7 = a.th_shift, k8 = a.CoutPad;
        const uint64_t k9 = a.tw_magic;
        const int64_t k10 = a.in_sb;
        const half_t *k11 = a.x, *k12 = a.w;
        const float* k13 = a.bias;
        asm volatile("" ::"s"(k0), "s"(k1), "s"(k2), "s"(k3), "s"(k4), "s"(k5), "s"(k6), "s"(k7), "s"(k8), "s"(k9), "s"(k10),
                     "s"(k11), "s"(k12), "s"(k13));
    }
    const int total = a.mtiles * a.ntiles;
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    const int tq = total >> 3, tr = total & 7;
    const int xbase_lin = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
    const int xcnt = tq + (xcd < tr ? 1 : 0);
    const int nloc = PERSIST ? (int)(gridDim.x >> 3) : 1;
    struct Tile { int n0, mt, img, th, tw; const char* xb; const char* wb; };
    auto tile_at = [&](int idx) {
        Tile t;
        const int lin = xbase_lin + idx;
        int nt, t2, th, img;
        if (a.nt_shift >= 0) { nt = lin & (a.ntiles - 1); t.mt = lin >> a.nt_shift; }
        else { nt = lin % a.ntiles; t.mt = lin / a.ntiles; }
        t.n0 = nt * BN;
        t2 = (int)(((uint64_t)(uint32_t)t.mt * a.tw_magic) >> 40);          // = mt / tilesW (launch_conv checks the range)
        const int tw = t.mt - t2 * a.tilesW;
        if (a.th_shift >= 0) { th = t2 & (a.tilesH - 1); img = t2 >> a.th_shift; }
        else { th = t2 % a.tilesH; img = t2 / a.tilesH; }
        t.img = img; t.th = th; t.tw = tw;
        t.xb = (const char*)(a.x + img * a.in_sb + (int64_t)(th * TR) * a.in_sh + (int64_t)(tw * TC) * cin);
        t.wb = (const char*)(a.w + (int64_t)t.n0 * cin);
        return t;
    };
    int tidx = local;
    if (PERSIST && tidx >= xcnt) return;            // (persistent grids may exceed a short XCD run; a plain grid is exact)
    // Persistent variant, DYNAMIC tile queue (a.tile_counter set): the first two tiles of a workgroup are the static
    // ones (local, local + nloc); every later tile index is drawn from the XCD's atomic counter one tile ahead, so the
    // draw's latency hides behind a whole K loop and the hardware dispatcher's balancing is kept.
    const bool dynamic = PERSIST && a.tile_counter != nullptr;
    int tnext = local + nloc;
    volatile int* lds_next = (volatile int*)(smem + halo4_lds::kNextTile);

    const int wrow = GEOM ? (wm >> 1) * 4 : wm * 4;               // this wave's 4 x 16 patch inside the tile
    const int wcol = GEOM ? (wm & 1) * 16 : 0;
    uint32_t woff[4], hoff[12];
    const int q = lane >> 4, c = lane & 15;
    const int aoff0 = c * 128 + (((0 + q) ^ (lane & 7)) << 4);
    const int aoff1 = c * 128 + (((4 + q) ^ (lane & 7)) << 4);

    auto weight_buf = [&](int k) { return smem + halo4_lds::kWeights + (k & 1) * halo4_lds::kWeightBuf; };      // of K step k
    auto stage_w = [&](const char* wb, int rowcin, const uint32_t (&wo)[4], int kc, int tap, int buf) {
        const char* src = wb + ((int64_t)tap * a.CoutPad * rowcin + (int64_t)kc * kBK) * 2;
        char* dst = weight_buf(buf) + (wv * 4) * 1024;
        const int64_t ps = (int64_t)rowcin * 16;            // piece i = 8 cout rows further on: same lane offset, scalar stride
        glds16x4_asm_s(src, src + ps, src + 2 * ps, src + 3 * ps, wo[0], dst, dst + 1024, dst + 2048, dst + 3072);
    };
    auto stage_weights = [&](const char* wb, int kc, int tap, int buf) { stage_w(wb, cin, woff, kc, tap, buf); };
    auto stage_halo = [&](const char* xb, int kc) {
        const char* src = xb + (int64_t)kc * (kBK * 2);
#pragma unroll
        for (int r = 0; r < 12; ++r)
            if (wv + 4 * r < kHaloPieces) glds16_asm_s(src, hoff[r], smem + halo4_lds::kHalo + (wv + 4 * r) * 1024);
    };
    // per-lane DMA offsets of a source tensor with `rowcin` channels and `in_sh` elements per image row
    // (recomputed where needed - from an opaque lane id, so they are not kept alive across the epilogue)
    auto lane_offsets = [&](int rowcin, int in_sh, uint32_t (&wo)[4], bool with_halo) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int g = (wv * 4 + i) * 64 + ln;
            const int row = g >> 3, cp = (g & 7) ^ (row & 7);
            wo[i] = (uint32_t)row * (uint32_t)rowcin * 2u + cp * 16;
        }
        if (!with_halo) return;
#pragma unroll
        for (int r = 0; r < 12; ++r) {                          // piece wv + 4r
            const int g = (wv + 4 * r) * 64 + ln;
            const int row = g >> 3, cp = (g & 7) ^ (row & 7);
            int hy = row / S, hx = row - hy * S;
            if (hx > TC + 1) hx = TC + 1;                       // pad columns: any valid address
            if (hy > TR + 1) hy = TR + 1;                       // pieces >= 45 are never issued
            hoff[r] = ((uint32_t)hy * (uint32_t)in_sh + (uint32_t)hx * (uint32_t)rowcin) * 2u + cp * 16;
        }
    };
    // kPrefetch: the twelve piece offsets are not kept in registers through the K loop; their lane-row part
    // (hy * in_sh + hx * cin, the same for the eight lanes of an LDS row) goes into the table at halo4_lds::kHaloTable;
    // the lane's own 16-byte chunk term is added back when a piece is issued. Called right after the lane_offsets() of the
    // tensor the K loop reads.
    auto write_halo_table = [&]() {
        uint32_t* htab = (uint32_t*)(smem + halo4_lds::kHaloTable);
        if ((lane & 7) == 0) {
            const uint32_t cp0 = (uint32_t)((lane >> 3) & 7) << 4;           // chunk term of lane & 7 == 0
#pragma unroll
            for (int r = 0; r < 12; ++r) htab[(wv * 12 + r) * 8 + (lane >> 3)] = hoff[r] - cp0;
        }
    };
    const int hbuf = halo4_lds::kHalo + wrow * (S * 128);
    // fragment addresses of a tap inside the halo image: all 18 (tap, even / odd) addresses are six per-lane values
    // (dx = -1, 0, 1; swizzle parity) plus constants - spelled out so that the unrolled loop keeps six address
    // registers, not one or two per tap
    int bx[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int u = wcol + c + d;
        const int v0 = u * 128 + (((q ^ (u & 7)) & 7) << 4);
        bx[d][0] = hbuf + v0;
        bx[d][1] = hbuf + (v0 ^ 64);
    }
    auto b_ptrs = [&](int tap, const char*& be, const char*& bo) {
        const int tdy = tap / 3, d = tap - tdy * 3;
        be = smem + bx[d][tdy & 1] + tdy * (S * 128);
        bo = smem + bx[d][(tdy & 1) ^ 1] + tdy * (S * 128);
    };

    Tile cur = tile_at(tidx);
    int kbase = 0;                                  // weight-buffer parity continues across tiles / phases
    bool first = true;

    int tile_no = 0;
    for (;;) {
        const bool has_next = PERSIST && (tnext < xcnt);
        const char* nxb = cur.xb;
        const char* nwb = cur.wb;
        if (has_next) {
            const Tile t = tile_at(tnext);
            nxb = t.xb;
            nwb = t.wb;
        }
        int drawn = 0;
        if (dynamic && tid == 0)                        // index of the tile after next (used one tile from now)
            drawn = 2 * nloc + __hip_atomic_fetch_add(a.tile_counter + xcd, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f32x4 acc[JT][4];
        // One K step: 64 MFMAs of this wave on the weight tile at `wt` and the pixel fragments at be / bo.
        // Rolling fragment pipeline: 8 groups of 8 MFMAs (2 A fragments x 4 B fragments); A pairs are read two
        // groups ahead into a 3-slot ring, the second half's B fragments during group 1; `stage_next` issues the
        // next step's weight DMA after the first reads so its issue cost overlaps their LDS latency.
        // kPrefetch: the pixel fragments of the NEXT tap's first half are read behind this step's group kBpreAt into
        // bq[0] (dead after group 3) - the halo does not change inside a chunk - so only weight fragments are read between
        // the barrier and the first MFMA. `have_b0`: bq[0] was filled that way by the previous step; `nbe`: != nullptr ->
        // prefetch from (nbe, nbo).
        f16x8 bq[2][4];
        auto mma_step = [&](const char* wt, const char* be, const char* bo, auto&& stage_next, auto&& after_group,
                            bool have_b0 = false, const char* nbe = nullptr, const char* nbo = nullptr,
                            int bhalf_at = kBhalfAt) {
            f16x8 ar[kRing][2];
            auto read_a = [&](int g, f16x8 (&dst)[2]) {
                const int ks = g >> 2, jp = g & 3;
                const char* base = wt + (ks ? aoff1 : aoff0);
                dst[0] = *(const f16x8*)(base + (2 * jp) * 2048);
                dst[1] = *(const f16x8*)(base + (2 * jp + 1) * 2048);
            };
            auto read_b = [&](int ks, f16x8 (&dst)[4]) {
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    dst[n] = *(const f16x8*)((((n & 1) ^ ks) ? bo : be) + n * (S * 128));
            };
            __builtin_amdgcn_sched_barrier(0);
            if (!have_b0) read_b(0, bq[0]);
            read_a(0, ar[0]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 1; g < kRing - 1; ++g) read_a(g, ar[g]);
            __builtin_amdgcn_sched_barrier(0);
            stage_next();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const int ks = g >> 2, jp = g & 3;
                if (g + kRing - 1 < 8) read_a(g + kRing - 1, ar[(g + kRing - 1) % kRing]);
                __builtin_amdgcn_sched_barrier(0);
                if (g == bhalf_at) { read_b(1, bq[1]); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[2 * jp + jj][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                            ar[g % kRing][jj], bq[ks][n], acc[2 * jp + jj][n], 0, 0, 0);
                if (g == kBpreAt && nbe != nullptr) {
#pragma unroll
                    for (int n = 0; n < 4; ++n) bq[0][n] = *(const f16x8*)(((n & 1) ? nbo : nbe) + n * (S * 128));
                }
                after_group(g);
                __builtin_amdgcn_sched_barrier(0);
            }
        };

        if (DSFUSE) {
            // ---- pre-phase: acc = Wd * x (1x1: the centre tap of x's halo), ds_cin / 64 steps ----
            const int dcin = a.ds_cin, nds = dcin / kBK;
            const int tw0 = cur.tw, th0 = cur.th, img0 = cur.img;
            const char* dxb = (const char*)(a.ds_x + img0 * a.ds_in_sb + (int64_t)(th0 * TR) * a.ds_in_sh +
                                            (int64_t)(tw0 * TC) * dcin);
            const char* dwb = (const char*)(a.ds_w + (int64_t)cur.n0 * dcin);
            uint32_t woff_x[4];
            lane_offsets(dcin, a.ds_in_sh, woff_x, true);
            lane_offsets(cin, a.in_sh, woff, false);
            stage_halo(dxb, 0);
            stage_w(dwb, dcin, woff_x, 0, 0, 0);
            __builtin_amdgcn_s_setprio(1);                    // (as the main K loop below)
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[j][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
            __builtin_amdgcn_s_waitcnt(0xc07f);
#pragma unroll 1
            for (int kc = 0; kc < nds; ++kc) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                const char *be, *bo;
                b_ptrs(4, be, bo);
                mma_step(weight_buf(kc), be, bo, [&] {
                    if (kc + 1 < nds) stage_w(dwb, dcin, woff_x, kc + 1, 0, (kc + 1) & 1);
                    else stage_w(cur.wb, cin, woff, 0, 0, (kc + 1) & 1);            // conv2's first step
                }, [&](int) {});
                __builtin_amdgcn_s_barrier();                 // every wave has consumed this chunk's fragments
                asm volatile("" ::: "memory");
                if (kc + 1 < nds) {
                    stage_halo(dxb, kc + 1);
                } else {
                    lane_offsets(cin, a.in_sh, woff, true);   // from here on the halo holds conv2's input t
                    stage_halo(cur.xb, 0);
                    if (kPrefetch) write_halo_table();
                }
            }
            kbase = nds;
            // residual term and conv2's bias: acc <- (Wd*x + bd) / s + b2   (the epilogue multiplies by s)
            const float* sc = a.se_scale + (int64_t)img0 * a.Cout + cur.n0 + q * 8;
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                const int o = acc_cout_offset(j);
                const f32x4 bd = *(const f32x4*)(a.ds_bias + cur.n0 + q * 8 + o);
                const f32x4 b2 = *(const f32x4*)(a.bias + cur.n0 + q * 8 + o);
                const f32x4 s4 = *(const f32x4*)(sc + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float inv = __builtin_amdgcn_rcpf(fmaxf(s4[i], kSeScaleFloor));
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[j][n][i] = fmaf(acc[j][n][i] + bd[i], inv, b2[i]);
                }
            }
        } else {
            if (PERSIST || first) lane_offsets(cin, a.in_sh, woff, true);
            if (first) {
                stage_halo(cur.xb, 0);
                stage_weights(cur.wb, 0, 0, 0);
                if (kPrefetch) write_halo_table();
                first = false;
                if (STAMP) {
                    stamp(1);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    stamp(2);
                }
            }
            if (RESPRE) {
                // accumulators start at residual / max(s, floor) + bias (element order as in conv_epilogue's residual branch)
                const int w = cur.tw * TC + wcol + c;
                const bool wok = w < a.out_wlimit;
                const half_t* rb = a.resid + a.out_off + cur.img * a.out_sb + (int64_t)w * a.out_sw + cur.n0 + q * 8 +
                                   (int64_t)(cur.th * TR + wrow) * a.out_sh;
                const float* sc = a.se_scale + (int64_t)cur.img * a.Cout + cur.n0 + q * 8;
                f16x8 rlo[JT / 4][4], rhi[JT / 4][4];
#pragma unroll
                for (int cb = 0; cb < JT / 4; ++cb)
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const half_t* r = rb + (int64_t)n * a.out_sh + cb * 64;
                        rlo[cb][n] = wok ? *(const f16x8*)r : (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
                        rhi[cb][n] = wok ? *(const f16x8*)(r + 32) : (f16x8){0, 0, 0, 0, 0, 0, 0, 0};
                    }
#pragma unroll
                for (int j = 0; j < JT; ++j) {
                    const f32x4 b4 = *(const f32x4*)(a.bias + cur.n0 + q * 8 + acc_cout_offset(j));
                    const f32x4 s4 = *(const f32x4*)(sc + acc_cout_offset(j));
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float inv = __builtin_amdgcn_rcpf(fmaxf(s4[i], kSeScaleFloor));
                        const int e = (j & 3) * 4 + i;
#pragma unroll
                        for (int n = 0; n < 4; ++n) {
                            const float r = e < 8 ? (float)rlo[j >> 2][n][e] : (float)rhi[j >> 2][n][e - 8];
                            acc[j][n][i] = fmaf(r, inv, b4[i]);
                        }
                    }
                }
            } else {
                // accumulators start at the folded-BN bias (its load hides behind the first operands' DMA)
#pragma unroll
                for (int j = 0; j < JT; ++j) {
                    const f32x4 b4 = *(const f32x4*)(a.bias + cur.n0 + q * 8 + acc_cout_offset(j));
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[j][n] = b4;
                }
            }
        }

        // Retire every scalar (kernarg) load before the loop. A load still pending at the loop header keeps
        // hipcc's counter model "dirty" on every iteration (scalar loads return out of order), and it then
        // drains lgkmcnt(0) at the first MFMA group of each K step instead of the counted wait.
        __builtin_amdgcn_s_waitcnt(0xc07f);                 // lgkmcnt(0), vmcnt/expcnt untouched
        // The whole K loop runs at priority 1 (no flips around the MFMA groups): its LDS reads, DMA issue and barrier beat
        // the partner workgroup's prologue and epilogue VALU work, which stays at 0 (measured -1.5 to -1.9 % per step against flips)
        __builtin_amdgcn_s_setprio(1);
        for (int kc = 0; kc < nkc; ++kc) {
            const bool next_chunk = kc + 1 < nkc;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int k = kc * 9 + tap;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (!(a.dbg & 1024)) __builtin_amdgcn_s_barrier();       // dbg 1024: timing experiment without the per-step barrier
                asm volatile("" ::: "memory");
                const char *be, *bo;
                b_ptrs(tap, be, bo);
                const bool more = k + 1 < nk;
                const bool wrap = tap == 8;
                const int tap1 = more ? (wrap ? 0 : tap + 1) : 0;
                const int kc1 = more ? (wrap ? kc + 1 : kc) : 0;
                const char* wsrc = more ? cur.wb : nwb;
                const char *nbe = nullptr, *nbo = nullptr;
                if (kPrefetch && tap < 8) b_ptrs(tap + 1, nbe, nbo);
                mma_step(weight_buf(kbase + k), be, bo, [&] {
                    // the next K step's weights into the other buffer; on a tile's last step that is the
                    // next tile's first step (persistent variant only).
                    // nothing to stage on the very last step: no DMA is then in flight when the epilogue
                    // starts, so the workgroup can retire without waiting for its output stores
                    if ((more || has_next) && !(a.dbg & 512))    // dbg 512: no weight DMA
                        stage_weights(wsrc, kc1, tap1, (kbase + k + 1) & 1);
                }, [&](int g) {
                    if (kPrefetch && tap == 8 && g == kEarlyAt && next_chunk) {
                        // the last tap reads its second-half pixel fragments at group 0 (bhalf_at below), so after group
                        // kEarlyAt every fragment of the chunk is in registers: one extra barrier, and the next chunk's halo
                        // streams in during the remaining MFMA groups instead of after them
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        __builtin_amdgcn_s_barrier();
                        asm volatile("" ::: "memory");
                        // pieces wv + 4r: r <= 10 exist for every wave (45 pieces), r = 11 for wave 0 only
                        static_assert(kHaloPieces == 45, "halo piece count");
                        const char* hsrc = (next_chunk ? cur.xb + (int64_t)(kc + 1) * (kBK * 2) : nxb);
                        char* d = smem + halo4_lds::kHalo + wv * 1024;
                        int ln = lane;
                        asm volatile("" : "+v"(ln));                       // (nothing of this is hoisted out of the loop)
                        const uint32_t* hrow = (const uint32_t*)(smem + halo4_lds::kHaloTable) + wv * 96 + (ln >> 3);
                        const uint32_t cpl = (uint32_t)((ln ^ (ln >> 3)) & 7) << 4;
                        uint32_t ho[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) ho[r] = hrow[r * 8] + cpl;
                        glds16x4v_asm_s<4096>(hsrc, ho[0], ho[1], ho[2], ho[3], d);
#pragma unroll
                        for (int r = 0; r < 4; ++r) ho[r] = hrow[(4 + r) * 8] + cpl;
                        glds16x4v_asm_s<4096>(hsrc, ho[0], ho[1], ho[2], ho[3], d + 4 * 4096);
#pragma unroll
                        for (int r = 0; r < 4; ++r) ho[r] = hrow[(8 + r) * 8] + cpl;
#pragma unroll
                        for (int r = 8; r < 11; ++r) glds16_asm_s(hsrc, ho[r - 8], d + r * 4096);
                        if (wv == 0) glds16_asm_s(hsrc, ho[3], d + 11 * 4096);
                    }
                }, kPrefetch && tap > 0, nbe, nbo, (kPrefetch && tap == 8) ? 0 : kBhalfAt);
            }
            if (!kPrefetch && (next_chunk || has_next) && !(a.dbg & 32)) {     // dbg 32: timing experiment without the reload
                // single halo buffer: every wave has consumed its last B fragments of this chunk (they fed
                // the MFMAs above), so after this barrier the buffer may be overwritten - with the next
                // chunk, or with the next tile's first chunk (whose latency then hides behind the epilogue).
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                if (next_chunk) stage_halo(cur.xb, kc + 1);
                else stage_halo(nxb, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        // the epilogue's scratch (SE partial sums) lives after the DMA buffers, so DMA may stay in flight
        stamp(3);
        if (a.dbg & 128) {       // dbg 128: timing experiment without the epilogue (keeps the MFMAs alive)
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < JT; ++j)
#pragma unroll
                for (int n = 0; n < 4; ++n) t += acc[j][n][0] + acc[j][n][1] + acc[j][n][2] + acc[j][n][3];
            if (t == 123.456f) ((half_t*)a.y)[0] = (half_t)t;
        } else
        {
            const int tw = cur.tw, th = cur.th, img = cur.img;
            conv_epilogue<WN, WM, JT, false, SPLIT, true, true, DSFUSE || RESPRE>(
                a, acc, smem + halo4_lds::kScratch, tid, lane, 0, wm, cur.n0, cur.mt, img, th, tw, th * TR + wrow,
                tw * TC + wcol, STAMP ? a.stamps + (size_t)blockIdx.x * 16 : nullptr);
        }
        if (!has_next) break;
        kbase += nk;
        tidx = tnext;
        if (dynamic) {                                  // broadcast the drawn index (word alternates per tile: no WAR)
            if (tid == 0) lds_next[tile_no & 1] = drawn;
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_s_barrier();
            tnext = __builtin_amdgcn_readfirstlane(lds_next[tile_no & 1]);
        } else {
            tnext = tidx + nloc;
        }
        ++tile_no;
        cur = tile_at(tidx);
    }
    if (a.dbg & 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (K loop skipped: the prologue DMA is still in flight)
    if (STAMP) {
        stamp(4);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(5);
        if (tid == 0) {
            a.stamps[(size_t)blockIdx.x * 16 + 6] = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
            a.stamps[(size_t)blockIdx.x * 16 + 7] = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
        }
    }
}

// -------------------------------------------------------------------------------------------
// conv3x3_halo4h: the halo4 kernel with the halo held as TWO 32-channel halves (64-byte LDS rows) so that it is
// effectively double-buffered without more LDS. halo4 keeps one 64-channel halo and must stop at every chunk boundary:
// barrier, 12 DMA pieces per wave, wait for them (5.5 % of its K loop, profiles/r03_overhead_experiments.txt). Here a
// chunk's 18 (tap, half) units run as half A's nine taps, then half B's; two units (64 MFMAs per wave) per step:
//   step 0..3: (A0,A1) (A2,A3) (A4,A5) (A6,A7)   step 4: (A8,B0)   step 5..8: (B1,B2) (B3,B4) (B5,B6) (B7,B8)
// Half A is last read in step 4, half B in step 8, so the NEXT chunk's half A streams in during steps 5-7 and a chunk's
// own half B during its steps 0-2 (two pieces per wave and step, issued behind the step's weight pieces, so the next
// step's counted wait leaves them in flight): no extra barrier, no stall, the same number of DMA pieces.
// LDS rows are 64 B (32 channels): a 16x16x32 operand fragment is 16 rows x 64 B = 1 KiB; the 16-byte slot of chunk q in
// row r is q ^ 2*((r >> 2) & 1), conflict-free for ds_read_b128 at every row alignment (checked exhaustively against the
// instruction's 4 x 16 lane groups). Weight step buffer = 2 units x [128 couts][32 cin] = 16 KB, double-buffered.
// f16 only, non-persistent, no fused downsample (those launches stay on halo4).
// -------------------------------------------------------------------------------------------
template <int GEOM>
__global__ __launch_bounds__(256, 2) void conv3x3_halo4h_kernel(const ConvArgs a) {
    constexpr int WN = 1, WM = 4, JT = 8, BN = 128;
    constexpr int TR = GEOM ? 8 : 16, TC = GEOM ? 32 : 16;
    constexpr int S = TC + 4;
    constexpr int kHalf = (TR + 2) * S * 64;                  // bytes of one 32-channel halo half (23040)
    constexpr int kHalfPieces = (kHalf + 1023) / 1024;        // 23 one-KiB pieces, the last one half full
    static_assert(2 * kHalf == kHaloBytes && kHalfPieces == 23, "halo footprint");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv;
    const int cin = a.Cin;
    const int nkc = cin / kBK;
    {
        const int k0 = a.mtiles, k1 = a.ntiles, k2 = a.tilesW, k3 = a.tilesH, k4 = a.Cin, k5 = a.in_sh, k6 = a.nt_shift,
                  k7 = a.th_shift, k8 = a.CoutPad;
        const uint64_t k9 = a.tw_magic;
        const int64_t k10 = a.in_sb;
        const half_t *k11 = a.x, *k12 = a.w;
        const float* k13 = a.bias;
        asm volatile("" ::"s"(k0), "s"(k1), "s"(k2), "s"(k3), "s"(k4), "s"(k5), "s"(k6), "s"(k7), "s"(k8), "s"(k9), "s"(k10),
                     "s"(k11), "s"(k12), "s"(k13));
    }
    const int total = a.mtiles * a.ntiles;
    const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
    const int tq = total >> 3, tr = total & 7;
    const int lin = (xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq) + local;
    int nt, mt, t2, th, img;
    if (a.nt_shift >= 0) { nt = lin & (a.ntiles - 1); mt = lin >> a.nt_shift; }
    else { nt = lin % a.ntiles; mt = lin / a.ntiles; }
    const int n0 = nt * BN;
    t2 = (int)(((uint64_t)(uint32_t)mt * a.tw_magic) >> 40);
    const int tw = mt - t2 * a.tilesW;
    if (a.th_shift >= 0) { th = t2 & (a.tilesH - 1); img = t2 >> a.th_shift; }
    else { th = t2 % a.tilesH; img = t2 / a.tilesH; }
    const char* xb = (const char*)(a.x + img * a.in_sb + (int64_t)(th * TR) * a.in_sh + (int64_t)(tw * TC) * cin);
    const char* wb = (const char*)(a.w + (int64_t)n0 * cin);

    const int wrow = GEOM ? (wm >> 1) * 4 : wm * 4;
    const int wcol = GEOM ? (wm & 1) * 16 : 0;
    const int q = lane >> 4, c = lane & 15;
    // ---- per-lane DMA offsets: a piece is 16 LDS rows x 64 B; lane l fills slot l & 3 of row l >> 2 ----
    // Weights: piece i of a wave is 16 cout rows further on (the swizzle key (row >> 2) & 1 does not change), so ONE lane
    // offset serves all four and the piece stride goes into the scalar base. Halo: a piece's pixel -> (hy, hx) needs a
    // division, six of them held in registers spill (the K loop is fully unrolled, 128 accumulators + 56 fragment
    // registers live) and a spill reload drains vmcnt; they are recomputed at the issue point instead (a dozen VALU
    // instructions per piece in the shadow of the MFMAs) from an opaque copy of the lane id so the compiler cannot
    // hoist them back out of the loop.
    uint32_t woff0;
    {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int prow = ln >> 2, slot = ln & 3;
        const int row = ((wv * 4) & 7) * 16 + prow;             // cout row inside the unit's [128][32] tile
        woff0 = (uint32_t)row * (uint32_t)cin * 2u + (uint32_t)((slot ^ (((row >> 2) & 1) << 1)) << 4);
    }
    const int wpiece = 16 * cin * 2;                            // bytes between a wave's weight pieces
    // weights of step s of chunk kc (units 2s, 2s+1) into buffer buf: waves 0,1 stage the first unit, 2,3 the second
    auto stage_w = [&](int kc, int s, int buf) {
        const int u = 2 * s + (wv >> 1);
        const int tap = u < 9 ? u : u - 9, half = u < 9 ? 0 : 1;
        const char* src = wb + ((int64_t)tap * a.CoutPad * cin + (int64_t)kc * kBK + half * 32) * 2;
        char* dst = smem + halo4_lds::kWeights + buf * halo4_lds::kWeightBuf + (wv * 4) * 1024;
#pragma unroll
        for (int i = 0; i < 4; ++i) glds16_asm_s(src + i * wpiece, woff0, dst + i * 1024);
    };
    // pieces r0, r0+1 (of this wave's six; piece wv + 4r, the 24th slot repeats piece 22) of half `half` of chunk kc
    auto stage_h2 = [&](int kc, int half, int r0) {
        const char* src = xb + ((int64_t)kc * kBK + half * 32) * 2;
        char* dst = smem + halo4_lds::kHalo + half * kHalf;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int prow = ln >> 2, slot = ln & 3;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int r = r0 + rr;
            int hp = wv + 4 * r;
            if (hp > kHalfPieces - 1) hp = kHalfPieces - 1;
            const int hr = hp * 16 + prow;                      // halo pixel index hy * S + hx
            int hy = (int)(((uint32_t)hr * (65536u / S + 1u)) >> 16), hx = hr - hy * S;      // hr < 512: exact
            if (hx > TC + 1) hx = TC + 1;                       // pad columns: any valid address
            if (hy > TR + 1) hy = TR + 1;                       // rows past the halo (second half of the last piece): masked
            const uint32_t off = ((uint32_t)hy * (uint32_t)a.in_sh + (uint32_t)hx * (uint32_t)cin) * 2u +
                                 (uint32_t)((slot ^ (((hr >> 2) & 1) << 1)) << 4);
            if (hp == kHalfPieces - 1) {                        // the last piece covers only 8 rows: upper lanes stay out
                if (lane < 32) glds16_asm_s(src, off, dst + hp * 1024);
            } else {
                glds16_asm_s(src, off, dst + hp * 1024);
            }
        }
    };
    const int aoff = c * 64 + ((q ^ (((c >> 2) & 1) << 1)) << 4);

    // prologue: half A of chunk 0 (all six pieces of every wave) and the weights of step 0
    stage_h2(0, 0, 0);
    stage_h2(0, 0, 2);
    stage_h2(0, 0, 4);
    stage_w(0, 0, 0);
    f32x4 acc[JT][4];
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        const f32x4 b4 = *(const f32x4*)(a.bias + n0 + q * 8 + acc_cout_offset(j));
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[j][n] = b4;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_s_setprio(1);
    int gstep = 0;
    bool halo_prev = false;
    for (int kc = 0; kc < nkc; ++kc) {
        const bool next_chunk = kc + 1 < nkc;
#pragma unroll
        for (int s = 0; s < 9; ++s, ++gstep) {               // fully unrolled: taps, halves and piece indices are constants
            if (halo_prev) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");      // the two halo pieces of the last step may fly on
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // fragment addresses of the step's two units
            const char* wt = smem + halo4_lds::kWeights + (gstep & 1) * halo4_lds::kWeightBuf + aoff;
            const char *be[2], *bo[2];
#pragma unroll
            for (int uu = 0; uu < 2; ++uu) {
                const int u = 2 * s + uu;
                const int tap = u < 9 ? u : u - 9, half = u < 9 ? 0 : 1;
                const int tdy = tap / 3, dx = tap - tdy * 3 - 1;
                const int hr0 = (wrow + tdy) * S + wcol + c + 1 + dx;           // halo pixel of pixel-repeat n = 0
                const char* hb = smem + halo4_lds::kHalo + half * kHalf + hr0 * 64;
                const int slot = q ^ (((hr0 >> 2) & 1) << 1);
                be[uu] = hb + (slot << 4);                                      // even n (S / 4 is odd: the key flips with n)
                bo[uu] = hb + ((slot ^ 2) << 4);
            }
            const bool more = !(s == 8 && !next_chunk);
            const bool halo_now = (s < 3) || (next_chunk && s >= 5 && s < 8);
            f16x8 ar[3][2], bq[2][4];
            auto read_a = [&](int g, f16x8 (&dst)[2]) {
                const char* base = wt + (g >> 2) * 8192 + (2 * (g & 3)) * 1024;
                dst[0] = *(const f16x8*)base;
                dst[1] = *(const f16x8*)(base + 1024);
            };
            auto read_b = [&](int uu, f16x8 (&dst)[4]) {
#pragma unroll
                for (int n = 0; n < 4; ++n) dst[n] = *(const f16x8*)(((n & 1) ? bo[uu] : be[uu]) + n * (S * 64));
            };
            __builtin_amdgcn_sched_barrier(0);
            read_b(0, bq[0]);
            read_a(0, ar[0]);
            __builtin_amdgcn_sched_barrier(0);
            read_a(1, ar[1]);
            __builtin_amdgcn_sched_barrier(0);
            if (more) {
                const int s1 = s == 8 ? 0 : s + 1, kc1 = s == 8 ? kc + 1 : kc;
                stage_w(kc1, s1, (gstep + 1) & 1);
            }
            if (halo_now) {
                if (s < 3) stage_h2(kc, 1, 2 * s);                   // this chunk's half B (first read in step 4)
                else stage_h2(kc + 1, 0, 2 * (s - 5));               // the next chunk's half A (half A was last read in step 4)
            }
            halo_prev = halo_now;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if (g + 2 < 8) read_a(g + 2, ar[(g + 2) % 3]);
                __builtin_amdgcn_sched_barrier(0);
                if (g == 1) { read_b(1, bq[1]); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[2 * (g & 3) + jj][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ar[g % 3][jj], bq[g >> 2][n],
                                                                                         acc[2 * (g & 3) + jj][n], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __builtin_amdgcn_s_setprio(0);
    conv_epilogue<WN, WM, JT, false, false, true, true, false>(a, acc, smem + halo4_lds::kScratch, tid, lane, 0, wm, n0, mt, img, th, tw,
                                                               th * TR + wrow, tw * TC + wcol);
}

// One launch of a halo4 / halo4h instance: LDS limit raised once per device (one done[] table per instance: the static
// lives in the template), HCTR_DBG applied unless `with_env_dbg` is false.
template <auto KERNEL>
static hipError_t launch_halo4_instance(const ConvArgs& a0, int grid, hipStream_t s, bool with_env_dbg = true) {
    static bool done[64] = {};
    hipError_t e0 = raise_lds_limit((const void*)KERNEL, halo4_lds::kTotal, done);
    if (e0 != hipSuccess) return e0;
    static const int dbg = env_dbg();
    ConvArgs a = a0;
    if (with_env_dbg) a.dbg |= dbg;
    hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), halo4_lds::kTotal, s, a);
    return hipGetLastError();
}

template <int GEOM, bool SPLIT, bool PERSIST>
static hipError_t launch_conv_halo4_tp(const ConvArgs& a, hipStream_t s) {
    int grid = a.mtiles * a.ntiles;
    if (PERSIST) {
        static int cus[64] = {};
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev >= 0 && dev < 64 && cus[dev] == 0) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus[dev] = prop.multiProcessorCount;
            if (cus[dev] <= 0) cus[dev] = 256;
        }
        const int resident = 2 * ((dev >= 0 && dev < 64) ? cus[dev] : 256);     // two workgroups per CU
        if (grid > resident) grid = resident;
        grid = (grid + 7) / 8 * 8;                         // whole XCD rounds (extra workgroups exit at once)
    }
    return launch_halo4_instance<conv3x3_halo4_kernel<GEOM, SPLIT, PERSIST>>(a, grid, s);
}
template <int GEOM, bool SPLIT>
static hipError_t launch_conv_halo4_t(const ConvArgs& a, hipStream_t s) {
    const int grid = a.mtiles * a.ntiles;
    if (a.ds_x != nullptr) {
        if (GEOM != 0) return hipErrorInvalidValue;               // (the engine only fuses on the 16x16 geometry)
        return launch_halo4_instance<conv3x3_halo4_kernel<0, SPLIT, false, false, true>>(a, grid, s);
    }
    if (a.stamps != nullptr && !SPLIT)       // (the diagnostic instance times the real kernel: no HCTR_DBG)
        return launch_halo4_instance<conv3x3_halo4_kernel<GEOM, false, false, true>>(a, grid, s, false);
    // persistent tiles with a STATIC stride measured 6-8 % slower on every layer (r01); HCTR_PERSIST=2 draws tiles
    // from an atomic queue instead (a.tile_counter, zeroed by the engine once per forward)
    static const int persist = [] { const char* e = getenv("HCTR_PERSIST"); return e ? atoi(e) : 0; }();
    if constexpr (!SPLIT) {
        // conv2 of an identity block with the residual fetched in the prologue (RESPRE instance): A/B switch HCTR_RESPRE=1,
        // OFF by default - measured 126.7 vs 125.4 ms per step (three interleaved rounds): the fetch costs the same ~4 us
        // in the prologue as in the epilogue, and the instance has no room for the next-tap fragment prefetch
        static const int respre = [] { const char* e = getenv("HCTR_RESPRE"); return e ? atoi(e) : 0; }();
        if (respre && persist == 0 && a.resid != nullptr && a.se_scale != nullptr)
            return launch_halo4_instance<conv3x3_halo4_kernel<GEOM, false, false, false, false, true>>(a, grid, s);
    }
    if (persist == 0 || (persist == 2 && a.tile_counter == nullptr)) return launch_conv_halo4_tp<GEOM, SPLIT, false>(a, s);
    ConvArgs b = a;
    if (persist != 2) b.tile_counter = nullptr;
    return launch_conv_halo4_tp<GEOM, SPLIT, true>(b, s);
}
template <int GEOM>
static hipError_t launch_conv_halo4(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;                 // division-free tile decomposition for the kernel's prologue
    auto shift_of = [](int v) { int sft = 0; while ((1 << sft) < v) ++sft; return (1 << sft) == v ? sft : -1; };
    a.nt_shift = shift_of(a.ntiles);
    a.th_shift = shift_of(a.tilesH);
    if (a.tilesW < 1 || (uint64_t)a.mtiles * (uint64_t)a.tilesW >= ((uint64_t)1 << 40)) return hipErrorInvalidValue;
    a.tw_magic = (((uint64_t)1 << 40) + (uint64_t)a.tilesW - 1) / (uint64_t)a.tilesW;
    // HCTR_HALFHALO=1: the half-buffered halo variant for the plain f16 launches (A/B)
    static const bool halfhalo = [] { const char* e = getenv("HCTR_HALFHALO"); return e ? atoi(e) != 0 : false; }();
    static const int persist = [] { const char* e = getenv("HCTR_PERSIST"); return e ? atoi(e) : 0; }();
    if (halfhalo && !a.split && a.ds_x == nullptr && a.stamps == nullptr && persist == 0 && a.Cin % kBK == 0)
        return launch_halo4_instance<conv3x3_halo4h_kernel<GEOM>>(a, a.mtiles * a.ntiles, s);
    return a.split ? launch_conv_halo4_t<GEOM, true>(a, s) : launch_conv_halo4_t<GEOM, false>(a, s);
}

template <bool SPLIT>
static hipError_t launch_conv_halo_t(const ConvArgs& a, hipStream_t s) {
    static bool done[64] = {};
    hipError_t e0 = raise_lds_limit((const void*)conv3x3_halo_kernel<SPLIT>, kHaloLds, done);
    if (e0 != hipSuccess) return e0;
    static const int dbg = env_dbg();
    ConvArgs b = a;
    b.dbg |= dbg;
    hipLaunchKernelGGL(conv3x3_halo_kernel<SPLIT>, dim3(a.mtiles * a.ntiles), dim3(512), kHaloLds, s, b);
    return hipGetLastError();
}
static hipError_t launch_conv_halo(const ConvArgs& a, hipStream_t s) {
    return a.split ? launch_conv_halo_t<true>(a, s) : launch_conv_halo_t<false>(a, s);
}

size_t conv_lds_bytes(ConvTile tile) {
    switch (tile) {
        case TILE_64x256: return 2 * (64 + 256) * 128;
        case TILE_256x256: return 2 * (256 + 256) * 128;
        default: return 2 * (128 + 128) * 128;
    }
}

template <int WN, int WM, int JT, int TAPS, bool LINEAR, bool PIPE, bool SPLIT>
static hipError_t launch_conv_ts(const ConvArgs& a, size_t lds, hipStream_t s) {
    auto kern = conv_mfma_kernel<WN, WM, JT, TAPS, LINEAR, PIPE, SPLIT>;
    static bool done[64] = {};
    hipError_t e0 = raise_lds_limit((const void*)kern, (int)lds, done);
    if (e0 != hipSuccess) return e0;
    const int grid = a.mtiles * a.ntiles;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WN * WM * 64), lds, s, a);
    return hipGetLastError();
}
template <int WN, int WM, int JT, int TAPS, bool LINEAR, bool PIPE>
static hipError_t launch_conv_t(const ConvArgs& a, size_t lds, hipStream_t s) {
    // the split (f16x3) epilogue only exists for the fp16-output configurations the engine uses in that mode
    if constexpr (!LINEAR && !PIPE) {
        if (a.split) return launch_conv_ts<WN, WM, JT, TAPS, LINEAR, PIPE, true>(a, lds, s);
    }
    return launch_conv_ts<WN, WM, JT, TAPS, LINEAR, PIPE, false>(a, lds, s);
}

hipError_t launch_conv(const ConvArgs& a, ConvTile tile, int taps, bool linear_f32, hipStream_t s) {
    const size_t lds = conv_lds_bytes(tile);
    // HCTR_HALO (read by the engine too): 0 = generic kernels, 1 = 8-wave halo kernel on 256x256 tiles,
    // 2 (default) = TILE_HALO4 chosen by the engine wherever a 3x3 layer allows it
    static const int halo = [] { const char* e = getenv("HCTR_HALO"); return e ? atoi(e) : 2; }();
    static const bool pipe = [] { const char* e = getenv("HCTR_PIPE"); return e ? atoi(e) != 0 : false; }();
    if (linear_f32) {
        if (tile == TILE_256x256)
            return pipe ? launch_conv_t<2, 4, 8, 1, true, true>(a, lds, s) : launch_conv_t<2, 4, 8, 1, true, false>(a, lds, s);
        return launch_conv_t<2, 2, 4, 1, true, false>(a, lds, s);
    }
    switch (tile) {
        case TILE_HALO4:
            return taps == 9 ? launch_conv_halo4<0>(a, s) : hipErrorInvalidValue;
        case TILE_HALO4_8x32:
            return taps == 9 ? launch_conv_halo4<1>(a, s) : hipErrorInvalidValue;
        case TILE_64x256:
            return taps == 9 ? launch_conv_t<1, 4, 4, 9, false, false>(a, lds, s)
                             : launch_conv_t<1, 4, 4, 1, false, false>(a, lds, s);
        case TILE_256x256:
            if (taps == 9 && halo) return launch_conv_halo(a, s);
            if (taps == 9)
                return pipe ? launch_conv_t<2, 4, 8, 9, false, true>(a, lds, s)
                            : launch_conv_t<2, 4, 8, 9, false, false>(a, lds, s);
            return launch_conv_t<2, 4, 8, 1, false, false>(a, lds, s);
        default:
            return taps == 9 ? launch_conv_t<2, 2, 4, 9, false, false>(a, lds, s)
                             : launch_conv_t<2, 2, 4, 1, false, false>(a, lds, s);
    }
}

// -------------------------------------------------------------------------------------------
// stem: NormalizePAD + conv0_1 (1 -> 64, 3x3, pad 1) + folded bn0_1 + ReLU, fp32 math, fp16 out.
// utils/dataset.py:83-93 (x/255, (x-0.5)/0.5, replicate the last valid column to the batch width)
// and models/handwritten_ctr_model.py:116-118. Memory-bound: 1 B in, 128 B out per pixel.
// One thread = one pixel x 8 output channels (one 16-byte store).
// -------------------------------------------------------------------------------------------
constexpr int kStemRows = 16;       // rows per thread (sliding 3x3 window in registers)

__global__ __launch_bounds__(256) void stem_kernel(const void* __restrict__ img, int img_f32,
                                                   const int32_t* __restrict__ widths,
                                                   const float* __restrict__ w9,
                                                   const float* __restrict__ bias,
                                                   half_t* __restrict__ y, int B, int W, int Wa, int split) {
    // thread = (8-channel group, image column); it walks kStemRows rows keeping the 3x3 window and its
    // 72 weights in registers: 3 new pixels and one 16-byte store per output pixel.
    const int cg = threadIdx.x & 7;
    const int w = blockIdx.x * 32 + (threadIdx.x >> 3);
    const int h0 = blockIdx.y * kStemRows;
    const int b = blockIdx.z;
    if (w >= W) return;
    float wt[8][9], bs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        bs[e] = bias[cg * 8 + e];
#pragma unroll
        for (int t = 0; t < 9; ++t) wt[e][t] = w9[(cg * 8 + e) * 9 + t];
    }
    const int wlim = widths ? widths[b] : W;
    auto pixel = [&](int hh, int ww) -> float {
        if (hh < 0 || hh >= 128 || ww < 0 || ww >= W) return 0.f;       // conv zero padding (normalised space)
        const int wsrc = ww < wlim ? ww : wlim - 1;                       // NormalizePAD replicate pad
        const int64_t off = ((int64_t)b * 128 + hh) * W + wsrc;
        if (img_f32) return ((const float*)img)[off];
        float x = (float)((const uint8_t*)img)[off] / 255.0f;
        return (x - 0.5f) / 0.5f;
    };
    float win[3][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) win[r + 1][d] = pixel(h0 - 1 + r, w - 1 + d);
    const int cs = split ? 192 : 64;                 // channels per pixel ([hi | lo | hi] planes when split)
    for (int r = 0; r < kStemRows; ++r) {
        const int h = h0 + r;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            win[0][d] = win[1][d];
            win[1][d] = win[2][d];
            win[2][d] = pixel(h + 1, w - 1 + d);
        }
        f16x8 o, ol;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float sv = bs[e];
#pragma unroll
            for (int t = 0; t < 9; ++t) sv = fmaf(wt[e][t], win[t / 3][t % 3], sv);
            sv = fmaxf(sv, 0.f);
            o[e] = (half_t)sv;
            ol[e] = split == 2 ? (half_t)0.f : (half_t)(sv - (float)o[e]);
        }
        half_t* dst = y + (((int64_t)b * 130 + h + 1) * Wa + (w + 1)) * cs + cg * 8;
        *(f16x8*)dst = o;
        if (split) {
            *(f16x8*)(dst + 64) = ol;
            *(f16x8*)(dst + 128) = o;
        }
    }
}

// border rows / columns of a padded NHWC activation (one block per (row, image); 16-byte stores)
__global__ __launch_bounds__(256) void zero_borders_kernel(half_t* __restrict__ p, int H, int W, int Wa, int C) {
    const int row = blockIdx.x, b = blockIdx.y;
    u32x4* r = (u32x4*)(p + ((int64_t)b * (H + 2) + row) * (int64_t)Wa * C);
    const int vpp = C >> 3;                                 // 16-byte vectors per pixel
    const u32x4 z = {0u, 0u, 0u, 0u};
    if (row == 0 || row == H + 1) {
        for (int i = threadIdx.x; i < Wa * vpp; i += 256) r[i] = z;
        return;
    }
    for (int i = threadIdx.x; i < vpp; i += 256) r[i] = z;                               // column 0
    const int first = (W + 1) * vpp, n = (Wa - W - 1) * vpp;                              // columns W+1 .. Wa-1
    for (int i = threadIdx.x; i < n; i += 256) r[first + i] = z;
}

hipError_t launch_zero_borders(half_t* p, int B, int H, int W, int Wa, int C, hipStream_t s) {
    if (B == 0) return hipSuccess;
    if (C % 8 != 0 || Wa < W + 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zero_borders_kernel, dim3(H + 2, B), dim3(256), 0, s, p, H, W, Wa, C);
    return hipGetLastError();
}

hipError_t launch_stem(const void* img, int img_f32, const int32_t* widths_dev, const float* w9,
                       const float* bias, half_t* y, int B, int W, int Wa, int split, hipStream_t s) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(stem_kernel, dim3((W + 31) / 32, 128 / kStemRows, B), dim3(256), 0, s, img, img_f32, widths_dev,
                       w9, bias, y, B, W, Wa, split);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// stem_conv0_2: the two stem convolutions in one kernel (models/handwritten_ctr_model.py:116-123 with NormalizePAD,
// utils/dataset.py:83-93, in front). conv0_1 (1 -> 64 channels) is HBM-bound when it runs alone: 128 B in, 16 kB out
// per pixel column, which conv0_2 reads straight back. Here a workgroup computes conv0_1 + bn0_1 + ReLU for the
// 18 x 18-pixel halo of its 16 x 16 output tile from a 20 x 20 patch of the image (fp32 FMAs in the order of
// stem_kernel: the halo holds bit for bit what that kernel stores) and writes it into the swizzled LDS halo image of
// the halo kernels; conv0_2 + bn0_2 + ReLU + (2,1) max-pool then run as 9 taps of MFMAs from it. Weights of conv0_2
// (9 taps x 64 couts x 64 cin) stream in 2-tap pieces of 16 KB through two buffers.
// 4 waves, each 64 couts x (4 rows x 16 columns); LDS 2 x 16 KB + 45 KB + 1.6 KB patch: two workgroups per CU, so
// one's conv0_1 arithmetic (VALU) overlaps the other's MFMAs.
// -------------------------------------------------------------------------------------------
constexpr int kS2Halo = 32768;                       // LDS offsets
constexpr int kS2Patch = 32768 + kHaloBytes;
constexpr int kS2Lds = kS2Patch + 20 * 20 * 4;       // 80448

__global__ __launch_bounds__(256, 2) void stem_conv0_2_kernel(const ConvArgs a) {
    constexpr int JT = 4, S = kHaloCols;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total = a.mtiles;
    int lin;
    {
        const int id = blockIdx.x, xcd = id & 7, sl = id >> 3;
        const int qd = total >> 3, r = total & 7;
        lin = (xcd < r ? xcd * (qd + 1) : r * (qd + 1) + (xcd - r) * qd) + sl;
    }
    const int tw = lin % a.tilesW;
    const int t2 = lin / a.tilesW;
    const int th = t2 % a.tilesH;
    const int img = t2 / a.tilesH;
    const int W = a.W;

    // ---- conv0_2 weights of K step st (taps 2st, 2st+1; the last step has one tap): 16 one-KiB pieces, 4 per wave ----
    auto stage_w = [&](int st, int buf) {
        const char* src = (const char*)a.w + (size_t)st * (2 * 64 * 64 * 2);
        char* dst = smem + buf * 16384 + (wv * 4) * 1024;
        const int npieces = st == 4 ? 8 : 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = wv * 4 + i;
            if (piece < npieces) {                                  // wave-uniform
                const int g = piece * 64 + lane;
                const int row = g >> 3, cp = (g & 7) ^ (row & 7);
                glds16_asm(src + (uint32_t)row * 128u + cp * 16, dst + i * 1024);
            }
        }
    };
    stage_w(0, 0);
    stage_w(1, 1);                                   // both buffers are free here: two steps' weights fly during the conv0_1 phase

    // ---- 20 x 20 patch of the normalised image (zero outside the image: conv0_1's padding; columns >= the line's
    //      width replicate its last column: NormalizePAD) ----
    float* patch = (float*)(smem + kS2Patch);
    {
        const int wlim = a.img_widths ? a.img_widths[img] : W;
        for (int e = tid; e < 400; e += 256) {
            const int py = e / 20, px = e - py * 20;
            const int hh = th * 16 - 2 + py, ww = tw * 16 - 2 + px;
            float v = 0.f;
            if (hh >= 0 && hh < 128 && ww >= 0 && ww < W) {
                const int wsrc = ww < wlim ? ww : wlim - 1;
                const int64_t off = ((int64_t)img * 128 + hh) * W + wsrc;
                if (a.img_f32) {
                    v = ((const float*)a.img)[off];
                } else {
                    const float x = (float)((const uint8_t*)a.img)[off] / 255.0f;
                    v = (x - 0.5f) / 0.5f;
                }
            }
            patch[e] = v;
        }
    }
    // conv0_1 weights of this thread's 8-channel group
    const int cg = tid & 7;
    float wt[8][9], bs[8];
    {
        const f32x4* wp = (const f32x4*)(a.stem_w + cg * 72);
        const f32x4* bp = (const f32x4*)(a.stem_b + cg * 8);
#pragma unroll
        for (int v = 0; v < 18; ++v) {
            const f32x4 w4 = wp[v];
#pragma unroll
            for (int i = 0; i < 4; ++i) wt[(v * 4 + i) / 9][(v * 4 + i) % 9] = w4[i];
        }
        const f32x4 b0 = bp[0], b1 = bp[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) { bs[i] = b0[i]; bs[4 + i] = b1[i]; }
    }
    __syncthreads();
    // ---- conv0_1 + bn0_1 + ReLU into the halo: unit = (halo pixel, 8 channels) -> one 16-byte LDS store ----
    for (int u = tid >> 3; u < kHaloRows * 18; u += 32) {
        const int hy = u / 18, hx = u - hy * 18;
        const int r = th * 16 - 1 + hy, col = tw * 16 - 1 + hx;       // image position of this conv0_1 output
        f16x8 o;
        if (r >= 0 && r < 128 && col >= 0 && col < W) {
            float win[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) win[t] = patch[(hy + t / 3) * 20 + hx + t % 3];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float sv = bs[e];
#pragma unroll
                for (int t = 0; t < 9; ++t) sv = fmaf(wt[e][t], win[t], sv);
                o[e] = (half_t)fmaxf(sv, 0.f);
            }
        } else {                                                       // conv0_2's zero padding / columns >= W
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)0.f;
        }
        const int hr = hy * S + hx;
        *(f16x8*)(smem + kS2Halo + hr * 128 + ((cg ^ (hr & 7)) << 4)) = o;
    }

    // ---- conv0_2: 9 taps x 2 k-slices; a wave owns 64 couts x (rows wv*4.. +3) x 16 columns ----
    const int q = lane >> 4, c = lane & 15;
    const int aoff0 = c * 128 + (((0 + q) ^ (lane & 7)) << 4);
    const int aoff1 = c * 128 + (((4 + q) ^ (lane & 7)) << 4);
    const int wrow = wv * 4;
    f32x4 acc[JT][4];
#pragma unroll
    for (int j = 0; j < JT; ++j)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[j][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int st = 0; st < 5; ++st) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's weight pieces of step st have landed
        __syncthreads();                                               // ... everyone's, and (st == 0) the halo is written
        if (st >= 1 && st + 1 < 5) stage_w(st + 1, (st + 1) & 1);      // (step 1's weights were issued up front)
        const int ntap = st == 4 ? 1 : 2;
        for (int tt = 0; tt < ntap; ++tt) {
            const int tap = st * 2 + tt;
            const int tdy = tap / 3, dx = tap - tdy * 3 - 1;
            const int u = c + 1 + dx;
            const int v0 = u * 128 + (((q ^ (u & 7) ^ ((tdy & 1) << 2)) & 7) << 4);
            const char* hb = smem + kS2Halo + (wrow + tdy) * (S * 128);
            const char* be = hb + v0;
            const char* bo = hb + (v0 ^ 64);
            const char* wtile = smem + (st & 1) * 16384 + tt * 8192;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f16x8 af[JT], bf[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) bf[n] = *(const f16x8*)((((n & 1) ^ ks) ? bo : be) + n * (S * 128));
#pragma unroll
                for (int j = 0; j < JT; ++j) af[j] = *(const f16x8*)(wtile + j * 2048 + (ks ? aoff1 : aoff0));
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int j = 0; j < JT; ++j)
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[j], bf[n], acc[j][n], 0, 0, 0);
                __builtin_amdgcn_s_setprio(0);
            }
        }
    }
    conv_epilogue<1, 4, JT, false, false>(a, acc, smem, tid, lane, 0, wv, 0, lin, img, th, tw, th * 16 + wrow, tw * 16);
}

hipError_t launch_stem_conv0_2(const ConvArgs& a, hipStream_t s) {
    if (a.mtiles == 0) return hipSuccess;
    static bool done[64] = {};
    hipError_t e0 = raise_lds_limit((const void*)stem_conv0_2_kernel, kS2Lds, done);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(stem_conv0_2_kernel, dim3(a.mtiles), dim3(256), kS2Lds, s, a);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// Squeeze-excite mean WITHOUT materialising conv2's output first.
// SELayer needs mean_{h,w}(bn2(conv2(t))) (models/handwritten_ctr_model.py:27,51-53). The convolution is
// linear, so with S_tap[ci] = sum over output positions of t[h+dy][w+dx][ci] (zero outside the image)
//     mean[c] = bias[c] + (1/HW) * sum_tap sum_ci W[tap][c][ci] * S_tap[ci],
// and S_tap follows from nine statistics of t per (image, channel): the total T, the sums of row 0,
// row H-1, column 0, column W-1 and the four corner values:
//     S(dy,dx) = T - [dy=+1] R0 - [dy=-1] RL - [dx=+1] C0 - [dx=-1] CL + corner(dy,dx)   (if dy,dx != 0)
// T comes from conv1's epilogue (per-tile sums of the stored fp16 values), the rest from se_border
// below and four direct reads. The scale is then known BEFORE conv2 runs, so conv2's epilogue applies
// relu(acc * scale + residual) itself and the separate read-o/read-r/write pass disappears.
// -------------------------------------------------------------------------------------------
constexpr int kBorderSeg = 8;       // each border line is summed by 8 blocks (partials reduced in se_premean)

__global__ __launch_bounds__(256) void se_border_kernel(const half_t* __restrict__ t, int H, int W, int Wa, int C,
                                                        int split, const float* __restrict__ tsum_part, int tiles,
                                                        float* __restrict__ out) {
    __shared__ float red[256 * 8];
    const int b = blockIdx.x, job = blockIdx.y;        // 0: row 0, 1: row H-1, 2: col 0, 3: col W-1, 4: whole-image total
    const int seg = blockIdx.z;
    if (job == 4) {
        // T = sum over the image of t, from conv1's per-tile sums [b][tile][C]: this block adds the tiles of its
        // segment in order (se_premean adds the 8 segment sums in order: fixed association, bit-reproducible)
        const int per = (tiles + kBorderSeg - 1) / kBorderSeg;
        const int t0 = seg * per, t1 = t0 + per < tiles ? t0 + per : tiles;
        for (int ci = threadIdx.x; ci < C; ci += 256) {
            const float* p = tsum_part + (int64_t)b * tiles * C + ci;
            float s0 = 0.f, s1 = 0.f;
            int i = t0;
            for (; i + 1 < t1; i += 2) { s0 += p[(int64_t)i * C]; s1 += p[(int64_t)(i + 1) * C]; }
            if (i < t1) s0 += p[(int64_t)i * C];
            out[(((int64_t)b * 5 + 4) * kBorderSeg + seg) * C + ci] = s0 + s1;
        }
        return;
    }
    const int cv = C >> 3;                             // 16-byte vectors per pixel
    const int v = threadIdx.x % cv, lanes = 256 / cv, p0 = threadIdx.x / cv;
    const int cs = split ? 3 * C : C;                  // channels per pixel in memory
    const half_t* img = t + (int64_t)b * (H + 2) * Wa * cs;
    const int count = job < 2 ? W : H;
    const int per = (count + kBorderSeg - 1) / kBorderSeg;
    const int pbeg = seg * per, pend = pbeg + per < count ? pbeg + per : count;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (threadIdx.x < lanes * cv) {
        auto addr = [&](int p) {
            const int h = job == 0 ? 0 : (job == 1 ? H - 1 : p);
            const int w = job == 2 ? 0 : (job == 3 ? W - 1 : p);
            return img + ((int64_t)(h + 1) * Wa + (w + 1)) * cs + v * 8;
        };
        // four pixels' loads in flight at a time (the kernel is a chain of L2 round trips otherwise); the additions
        // keep their order, so the sums are bit-identical to the one-at-a-time loop
        int p = pbeg + p0;
        for (; p + 3 * lanes < pend; p += 4 * lanes) {
            f16x8 x[4], xl[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const half_t* px = addr(p + u * lanes);
                x[u] = *(const f16x8*)px;
                if (split) xl[u] = *(const f16x8*)(px + C);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)x[u][e];
                if (split) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += (float)xl[u][e];
                }
            }
        }
        for (; p < pend; p += lanes) {
            const half_t* px = addr(p);
            const f16x8 x = *(const f16x8*)px;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)x[e];
            if (split) {
                const f16x8 xl = *(const f16x8*)(px + C);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)xl[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < cv) {                            // fixed-order reduction over the position lanes
        float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int l = 0; l < lanes; ++l)
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += red[(l * cv + threadIdx.x) * 8 + e];
#pragma unroll
        for (int e = 0; e < 8; ++e)
            out[(((int64_t)b * 5 + job) * kBorderSeg + seg) * C + threadIdx.x * 8 + e] = s[e];
    }
}

hipError_t launch_se_border(const half_t* t, int B, int H, int W, int Wa, int C, int split, const float* tsum_part,
                            int tiles, float* out, hipStream_t s) {
    hipLaunchKernelGGL(se_border_kernel, dim3(B, 5, kBorderSeg), dim3(256), 0, s, t, H, W, Wa, C, split, tsum_part, tiles, out);
    return hipGetLastError();
}

// one block per (image, 64 output channels); 4 k-slices x 64 couts per block. The block that finishes an image LAST
// (agent-scope counter per image) also runs the SELayer FCs on the completed means (models/handwritten_ctr_model.py:
// 19-29) and writes the channel scales: one launch instead of two, and no second pass over the per-tile sums.
__global__ __launch_bounds__(256) void se_premean_kernel(const float* __restrict__ border,
                                                         const half_t* __restrict__ t,
                                                         const half_t* __restrict__ w,
                                                         const float* __restrict__ bias, int H, int W, int Wa,
                                                         int C, int CoutPad, int split,
                                                         float* __restrict__ mean, const float* __restrict__ w1,
                                                         const float* __restrict__ w2, float* __restrict__ scale,
                                                         int32_t* __restrict__ counter) {
    __shared__ float S[9 * 512];
    __shared__ float part[256];
    __shared__ int last_flag;
    const int b = blockIdx.x, cg = blockIdx.y;
    const int cs = split ? 3 * C : C;                  // channels per pixel / weight row length
    const half_t* img = t + (int64_t)b * (H + 2) * Wa * cs;
    for (int ci = threadIdx.x; ci < C; ci += 256) {
        float bsum[5];
#pragma unroll
        for (int jb = 0; jb < 5; ++jb) {               // fixed-order sum of the segment partials
            const float* bd = border + (((int64_t)b * 5 + jb) * kBorderSeg) * C + ci;
            float sv = 0.f;
#pragma unroll
            for (int sg = 0; sg < kBorderSeg; ++sg) sv += bd[(int64_t)sg * C];
            bsum[jb] = sv;
        }
        const float R0 = bsum[0], RL = bsum[1], C0 = bsum[2], CL = bsum[3], T = bsum[4];
        auto px = [&](int hp, int wp) {
            const half_t* q = img + ((int64_t)hp * Wa + wp) * cs + ci;
            return split ? (float)q[0] + (float)q[C] : (float)q[0];
        };
        const float t00 = px(1, 1), t0L = px(1, W), tL0 = px(H, 1), tLL = px(H, W);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;
            float sv = T;
            if (dy == 1) sv -= R0;
            if (dy == -1) sv -= RL;
            if (dx == 1) sv -= C0;
            if (dx == -1) sv -= CL;
            if (dy == 1 && dx == 1) sv += t00;
            if (dy == 1 && dx == -1) sv += t0L;
            if (dy == -1 && dx == 1) sv += tL0;
            if (dy == -1 && dx == -1) sv += tLL;
            S[tap * C + ci] = sv;
        }
    }
    __syncthreads();
    // cout c = cg*64 + cl is stored row blk*64 + s with perm64(s) = cl (engine.cpp perm64)
    const int cl = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int jj = (cl >> 5) * 2 + ((cl >> 2) & 1), qq = (cl >> 3) & 3, ii = cl & 3;
    const int srow = jj * 16 + qq * 4 + ii;
    float acc = 0.f;
    const int kper = 9 * C / 4;                        // this slice's share of the 9*C reduction
    // eight 16-byte weight loads in flight per round (one dependent L2 round trip per 8 values otherwise); the FMAs
    // keep their order, so the mean is bit-identical to the one-vector-at-a-time loop
    int kk0 = slice * kper;
    const int kend = (slice + 1) * kper;
    for (; kk0 + 64 <= kend; kk0 += 64) {
        f16x8 wv8[8], wl8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int kk = kk0 + u * 8;
            const int tap = kk / C, ci = kk - tap * C;
            const half_t* wr = w + ((int64_t)tap * CoutPad + cg * 64 + srow) * cs + ci;
            wv8[u] = *(const f16x8*)wr;
            if (split) wl8[u] = *(const f16x8*)(wr + 2 * C);       // weight rows are [w_hi | w_hi | w_lo]
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int kk = kk0 + u * 8;
            const int tap = kk / C, ci = kk - tap * C;
            if (split) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf((float)wv8[u][e] + (float)wl8[u][e], S[tap * C + ci + e], acc);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = fmaf((float)wv8[u][e], S[tap * C + ci + e], acc);
            }
        }
    }
    for (int kk = kk0; kk < kend; kk += 8) {           // tail (C = 128: 288 = 4 x 64 + 32 values per slice)
        const int tap = kk / C, ci = kk - tap * C;
        const half_t* wr = w + ((int64_t)tap * CoutPad + cg * 64 + srow) * cs + ci;
        const f16x8 wv = *(const f16x8*)wr;
        if (split) {
            const f16x8 wl = *(const f16x8*)(wr + 2 * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf((float)wv[e] + (float)wl[e], S[tap * C + ci + e], acc);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf((float)wv[e], S[tap * C + ci + e], acc);
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 64) {
        const float tot = (part[threadIdx.x] + part[64 + threadIdx.x]) + (part[128 + threadIdx.x] + part[192 + threadIdx.x]);
        const int c = cg * 64 + threadIdx.x;
        mean[(int64_t)b * C + c] = bias[c] + tot / ((float)H * (float)W);
    }
    // ---- hand-off: the means of this block are published (every storing wave drains, barrier, agent-scope release),
    //      then the image's counter is bumped; the block that draws the last ticket acquires and runs the FCs ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int ticket = __hip_atomic_fetch_add(counter + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = ticket == (int)gridDim.y - 1;
        if (last) {
            __hip_atomic_store(counter + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next launch
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        last_flag = last;
    }
    __syncthreads();
    if (!last_flag) return;
    float* mean_s = S;                                 // (S is free again)
    float* hid = S + 512;
    for (int c = threadIdx.x; c < C; c += 256)
        mean_s[c] = __hip_atomic_load(mean + (int64_t)b * C + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int R = C / 16;
    {
        const int r = threadIdx.x >> 3, l = threadIdx.x & 7;     // hidden: R <= 32 outputs, 8 lanes each
        float sv = 0.f;
        if (r < R)
            for (int c = l; c < C; c += 8) sv = fmaf(w1[r * C + c], mean_s[c], sv);
        sv += __shfl_xor(sv, 1);
        sv += __shfl_xor(sv, 2);
        sv += __shfl_xor(sv, 4);
        if (r < R && l == 0) hid[r] = fmaxf(sv, 0.f);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float sv = 0.f;
        for (int r = 0; r < R; ++r) sv = fmaf(w2[c * R + r], hid[r], sv);
        scale[(int64_t)b * C + c] = 1.f / (1.f + expf(-sv));
    }
}

hipError_t launch_se_premean(const float* border, const half_t* t, const half_t* w, const float* bias, int B, int H,
                             int W, int Wa, int C, int CoutPad, int split, float* mean, const float* w1,
                             const float* w2, float* scale, int32_t* counter, hipStream_t s) {
    if (C > 512 || C % 64 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(se_premean_kernel, dim3(B, C / 64), dim3(256), 0, s, border, t, w, bias, H, W, Wa, C, CoutPad,
                       split, mean, w1, w2, scale, counter);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// se_fc: SELayer's FC(c -> c/16) ReLU FC(c/16 -> c) sigmoid on the pooled means
// (models/handwritten_ctr_model.py:19-29). One block per image; partial sums are reduced in a
// fixed order so the result is bit-reproducible.
// -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_fc_kernel(const float* __restrict__ part, int tiles,
                                                    const float* __restrict__ w1,
                                                    const float* __restrict__ w2,
                                                    float* __restrict__ scale, int C, float inv_hw) {
    __shared__ float mean[512];
    __shared__ float hid[32];
    const int b = blockIdx.x;
    const int R = C / 16;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float* p = part + (int64_t)b * tiles * C + c;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int t = 0;
        for (; t + 3 < tiles; t += 4) {
            s0 += p[(int64_t)t * C];
            s1 += p[(int64_t)(t + 1) * C];
            s2 += p[(int64_t)(t + 2) * C];
            s3 += p[(int64_t)(t + 3) * C];
        }
        for (; t < tiles; ++t) s0 += p[(int64_t)t * C];
        mean[c] = ((s0 + s1) + (s2 + s3)) * inv_hw;
    }
    __syncthreads();
    // hidden: R <= 32 outputs, 8 lanes each
    {
        const int r = threadIdx.x >> 3, l = threadIdx.x & 7;
        float s = 0.f;
        if (r < R)
            for (int c = l; c < C; c += 8) s = fmaf(w1[r * C + c], mean[c], s);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (r < R && l == 0) hid[r] = fmaxf(s, 0.f);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int r = 0; r < R; ++r) s = fmaf(w2[c * R + r], hid[r], s);
        scale[(int64_t)b * C + c] = 1.f / (1.f + expf(-s));
    }
}

hipError_t launch_se_fc(const float* se_part, int tiles_per_img, const float* w1, const float* w2,
                        float* scale, int B, int C, float inv_hw, hipStream_t s) {
    hipLaunchKernelGGL(se_fc_kernel, dim3(B), dim3(256), 0, s, se_part, tiles_per_img, w1, w2, scale, C, inv_hw);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// se_apply: out = relu(o * scale[b][c] + residual), in place on o
// (models/handwritten_ctr_model.py:30 and :57-58). Runs over the whole padded buffer: border
// elements are 0 in both operands and stay 0. HBM-bound, 16-byte vectors.
// -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_apply_kernel(half_t* __restrict__ o, const half_t* __restrict__ r,
                                                       const float* __restrict__ scale,
                                                       int64_t img_vecs, int64_t total_vecs, int C) {
    const int cv = C >> 3;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < total_vecs; v += (int64_t)gridDim.x * 256) {
        const int b = (int)(v / img_vecs);
        const int c0 = (int)(v % cv) << 3;
        const f16x8 ov = *(const f16x8*)(o + v * 8);
        const f16x8 rv = *(const f16x8*)(r + v * 8);
        const f32x4 s0 = *(const f32x4*)(scale + (int64_t)b * C + c0);
        const f32x4 s1 = *(const f32x4*)(scale + (int64_t)b * C + c0 + 4);
        f16x8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float sc = e < 4 ? s0[e] : s1[e - 4];
            y[e] = (half_t)fmaxf(fmaf((float)ov[e], sc, (float)rv[e]), 0.f);
        }
        *(f16x8*)(o + v * 8) = y;
    }
}

hipError_t launch_se_apply(half_t* o, const half_t* r, const float* scale, int64_t img_elems,
                           int B, int C, hipStream_t s) {
    const int64_t img_vecs = img_elems / 8, total = img_vecs * B;
    int64_t grid = (total + 255) / 256;
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(se_apply_kernel, dim3((unsigned)grid), dim3(256), 0, s, o, r, scale, img_vecs, total, C);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// argmax_rows: np.argmax(preds, 2) (utils/ctc_codec.py:75): first maximum wins.
// One wave per row; lanes read 16-byte vectors; tie-break on the lower index.
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ void argmax_merge_np(float& v, int& i, float ov, int oi) {
    if (np_gt(ov, v) || (np_eq(ov, v) && oi < i)) { v = ov; i = oi; }
}

__device__ __forceinline__ void argmax_merge(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ __launch_bounds__(256) void argmax_rows_kernel(const float* __restrict__ x, int64_t ld, int64_t M,
                                                          int C, int32_t* __restrict__ idx, int tB, int tW) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* p = x + row * ld;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    const int c4 = C & ~3;
    for (int c = lane * 4; c < c4; c += 256) {
        const f32x4 v = *(const f32x4*)(p + c);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (np_gt(v[e], bv)) { bv = v[e]; bi = c + e; }
    }
    for (int c = c4 + lane; c < C; c += 64) {
        const float v = p[c];
        if (np_gt(v, bv)) { bv = v; bi = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        argmax_merge_np(bv, bi, ov, oi);
    }
    if (lane == 0) {
        // tB > 0: input rows are r = t*tB + b (WBC order), output is [b][t]
        const int64_t o = tB > 0 ? (row % tB) * tW + row / tB : row;
        idx[o] = (bi == 0x7fffffff) ? 0 : bi;
    }
}

// second stage of the fused head argmax: thread per row over the P = ntiles * WN partials (class ranges rise with p).
// Guarded precision: with the runner-up / |logit| partials it also forms the row's top-1/top-2 margin over ALL classes
// (the runner-up of the row is the second largest of the union of every part's best two) and its largest |logit|.
__global__ __launch_bounds__(256) void argmax_partials_kernel(const float* __restrict__ val, const int32_t* __restrict__ cls,
                                                              int P, int64_t M, int32_t* __restrict__ idx,
                                                              const float* __restrict__ val2, const float* __restrict__ absp,
                                                              float* __restrict__ margin, float* __restrict__ rowabs) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float bv = -INFINITY, sv = -INFINITY, av = 0.f;
    int bi = 0x7fffffff;
    for (int p = 0; p < P; ++p) {
        const float v = val[(int64_t)p * M + m];
        const int i = cls[(int64_t)p * M + m];
        const bool wins = np_gt(v, bv) || (np_eq(v, bv) && i < bi);
        if (val2 != nullptr) {
            const float v2 = val2[(int64_t)p * M + m];
            const float lose = wins ? bv : v, keep2 = wins ? v2 : sv;
            sv = np_gt(lose, keep2) ? lose : keep2;
            av = fmaxf(av, absp[(int64_t)p * M + m]);
        }
        if (wins) { bv = v; bi = i; }
    }
    if (idx != nullptr) idx[m] = (bi == 0x7fffffff) ? 0 : bi;
    if (val2 != nullptr) {
        margin[m] = bv - sv;
        rowabs[m] = av;
    }
}

hipError_t launch_argmax_partials(const float* val, const int32_t* cls, int P, int64_t M, int32_t* idx, hipStream_t s,
                                  const float* val2, const float* absp, float* margin, float* rowabs) {
    if (M <= 0) return hipSuccess;
    if (val2 != nullptr && (absp == nullptr || margin == nullptr || rowabs == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(argmax_partials_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, val, cls, P, M, idx, val2,
                       absp, margin, rowabs);
    return hipGetLastError();
}

// Guarded precision on stored logits (hctr_forward_logits): one wave per row, top-1/top-2 margin (exact ties give 0,
// a NaN gives NaN) and largest |logit|. Same figures as the fused partials produce.
__global__ __launch_bounds__(256) void row_guard_kernel(const float* __restrict__ x, int64_t ld, int64_t M, int C,
                                                        float* __restrict__ margin, float* __restrict__ rowabs) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* p = x + row * ld;
    float bv = -INFINITY, sv = -INFINITY, av = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float v = p[c];
        av = fmaxf(av, fabsf(v));
        if (np_gt(v, bv)) { sv = bv; bv = v; }
        else if (np_gt(v, sv)) sv = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off), osv = __shfl_xor(sv, off);
        const bool wins = np_gt(ov, bv);
        const float lose = wins ? bv : ov, keep2 = wins ? osv : sv;
        sv = np_gt(lose, keep2) ? lose : keep2;
        if (wins) bv = ov;
        av = fmaxf(av, __shfl_xor(av, off));
    }
    if (lane == 0) {
        margin[row] = bv - sv;
        rowabs[row] = av;
    }
}

hipError_t launch_row_guard(const float* logits, int64_t ld, int64_t M, int C, float* margin, float* rowabs, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(row_guard_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, logits, ld, M, C, margin, rowabs);
    return hipGetLastError();
}

// one block per line: the smallest top-2 margin over the line's columns (pad columns included: the reference decodes
// them too, utils/ctc_codec.py:75 over test.py:170-186's padded batch) and the line's largest |logit|
__global__ __launch_bounds__(256) void line_guard_kernel(const float* __restrict__ margin, const float* __restrict__ rowabs,
                                                         int W, float* __restrict__ out) {
    __shared__ float smin[4], smax[4];
    __shared__ int sbad[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float mn = INFINITY, mx = 0.f;
    int bad = 0;
    for (int t = threadIdx.x; t < W; t += 256) {
        const float mg = margin[(int64_t)b * W + t];
        bad |= (mg != mg) ? 1 : 0;
        mn = fminf(mn, mg);
        mx = fmaxf(mx, rowabs[(int64_t)b * W + t]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
        bad |= __shfl_xor(bad, off);
    }
    if (lane == 0) { smin[wv] = mn; smax[wv] = mx; sbad[wv] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        mn = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        mx = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
        bad = sbad[0] | sbad[1] | sbad[2] | sbad[3];
        out[2 * b] = bad ? NAN : mn;
        out[2 * b + 1] = mx;
    }
}

hipError_t launch_line_guard(const float* margin, const float* rowabs, int B, int W, float* out, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(line_guard_kernel, dim3(B), dim3(256), 0, s, margin, rowabs, W, out);
    return hipGetLastError();
}

hipError_t launch_argmax_rows(const float* logits, int64_t ld, int64_t M, int C, int32_t* idx, int tB, int tW,
                              hipStream_t s) {
    const int64_t grid = (M + 3) / 4;
    hipLaunchKernelGGL(argmax_rows_kernel, dim3((unsigned)grid), dim3(256), 0, s, logits, ld, M, C, idx, tB, tW);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// ctc_collapse: greedy CTC collapse (utils/ctc_codec.py:89-93): keep column t iff
// idx[t] != 0 (blank) && idx[t] != C-1 (unknown) && !(t > 0 && idx[t-1] == idx[t]) - the
// previous column is compared RAW. One wave per line; ballot + popcount compaction keeps order.
// -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ctc_collapse_kernel(const int32_t* __restrict__ idx, int W, int C,
                                                          int32_t* __restrict__ labels,
                                                          int32_t* __restrict__ lengths) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t* p = idx + (int64_t)b * W;
    int32_t* o = labels + (int64_t)b * W;
    int base = 0;
    for (int t0 = 0; t0 < W; t0 += 64) {
        const int t = t0 + lane;
        int cur = 0, prev = -1;
        if (t < W) {
            cur = p[t];
            if (t > 0) prev = p[t - 1];
        }
        const bool keep = (t < W) && cur != 0 && cur != C - 1 && cur != prev;
        const unsigned long long m = __ballot(keep);
        if (keep) o[base + __popcll(m & ((1ull << lane) - 1ull))] = cur;
        base += __popcll(m);
    }
    // the callers copy the whole [B][W] array out: the places beyond the text are zeros, not what the buffer held
    for (int t = base + lane; t < W; t += 64) o[t] = 0;
    if (lane == 0) lengths[b] = base;
}

hipError_t launch_ctc_collapse(const int32_t* idx, int B, int W, int C, int32_t* labels, int32_t* lengths,
                               hipStream_t s) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(64), 0, s, idx, W, C, labels, lengths);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// layout helpers for the API-parity paths (the fused fast path never materialises WBC logits)
// -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rows_to_wbc_kernel(const float* __restrict__ rows, int64_t ld, int B,
                                                          int W, int C, float* __restrict__ out, int Bfull,
                                                          int b0) {
    const int64_t r = blockIdx.x;                  // sub-batch row index t*B + b
    const int t = (int)(r / B), b = (int)(r % B);
    const float* src = rows + ((int64_t)b * W + t) * ld;
    float* dst = out + ((int64_t)t * Bfull + b0 + b) * C;
    for (int c = threadIdx.x; c < C; c += 256) dst[c] = src[c];
}

__global__ __launch_bounds__(256) void wbc_to_rows_kernel(const float* __restrict__ wbc, int B, int W, int C,
                                                          float* __restrict__ rows, int64_t ld) {
    const int64_t r = blockIdx.x;                  // input row index t*B + b
    const int t = (int)(r / B), b = (int)(r % B);
    const float* src = wbc + r * C;
    float* dst = rows + ((int64_t)b * W + t) * ld;
    for (int c = threadIdx.x; c < C; c += 256) dst[c] = src[c];
}

hipError_t launch_logits_to_wbc(const float* logits, int64_t ld, int B, int W, int C, float* out, int Bfull,
                                int b0, hipStream_t s) {
    if ((int64_t)B * W == 0) return hipSuccess;
    hipLaunchKernelGGL(rows_to_wbc_kernel, dim3((unsigned)((int64_t)B * W)), dim3(256), 0, s, logits, ld, B, W, C, out,
                       Bfull, b0);
    return hipGetLastError();
}

hipError_t launch_wbc_to_rows(const float* wbc, int B, int W, int C, float* rows, int64_t ld, hipStream_t s) {
    if ((int64_t)B * W == 0) return hipSuccess;
    hipLaunchKernelGGL(wbc_to_rows_kernel, dim3((unsigned)((int64_t)B * W)), dim3(256), 0, s, wbc, B, W, C, rows, ld);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// row_topk: scipy.special.log_softmax (utils/ctc_codec.py:65) + the top-`search_depth`
// candidates by descending log-prob (:127,186) + the count of candidates above ln(0.001) (:128,144).
// One 256-thread block per (b, t) row; the row is held in LDS; k selection passes.
// log-softmax is evaluated as the reference does in float32: tmp = x - max; tmp - log(sum(exp(tmp)));
// the sum is accumulated in float64 (order-independent to fp32 precision).
// Ties between equal log-probs: the lower class index comes first (the reference's order for
// ties is numpy's unstable argsort, i.e. unspecified).
// -------------------------------------------------------------------------------------------
constexpr int kMaxRowLds = 12288;   // floats (48 KiB): supports C <= 12288

__device__ __forceinline__ double block_sum_d(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void row_topk_kernel(const float* __restrict__ x, int64_t ld, int B, int W,
                                                       int C, int k, double thresh,
                                                       int32_t* __restrict__ topk_idx,
                                                       float* __restrict__ topk_logp,
                                                       float* __restrict__ blank_logp,
                                                       float* __restrict__ stats,
                                                       int32_t* __restrict__ cand_count) {
    __shared__ float row[kMaxRowLds];
    __shared__ float rv[4];
    __shared__ int ri[4];
    __shared__ double rd[4];
    const int64_t r = blockIdx.x;                  // t*B + b
    const int t = (int)(r / B), b = (int)(r % B);
    const float* p = x + ((int64_t)b * W + t) * ld;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    float mx = -INFINITY;
    for (int c = tid; c < C; c += 256) {
        const float v = p[c];
        row[c] = v;
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) rv[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
    double s = 0.0;
    for (int c = tid; c < C; c += 256) s += (double)expf(row[c] - mx);
    s = block_sum_d(s, rd);
    const float logs = logf((float)s);
    // in-place: row[c] = log-prob (float32, as the reference computes it)
    int cnt = 0;
    for (int c = tid; c < C; c += 256) {
        const float lp = (row[c] - mx) - logs;
        row[c] = lp;
        cnt += ((double)lp > thresh) ? 1 : 0;
    }
    if (cand_count) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
        __syncthreads();
        if (lane == 0) ri[wv] = cnt;
        __syncthreads();
        if (tid == 0) cand_count[r] = ri[0] + ri[1] + ri[2] + ri[3];
    }
    __syncthreads();
    if (tid == 0) {
        blank_logp[r] = row[0];
        if (stats) { stats[2 * r] = mx; stats[2 * r + 1] = logs; }
    }
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < k; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = tid; c < C; c += 256) {
            const float v = row[c];
            const bool after = (v < pv) || (v == pv && c > pi);
            if (after && (v > bv || (v == bv && c < bi))) { bv = v; bi = c; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            argmax_merge(bv, bi, ov, oi);
        }
        __syncthreads();
        if (lane == 0) { rv[wv] = bv; ri[wv] = bi; }
        __syncthreads();
        bv = rv[0]; bi = ri[0];
#pragma unroll
        for (int q = 1; q < 4; ++q) argmax_merge(bv, bi, rv[q], ri[q]);
        pv = bv; pi = bi;
        if (tid == 0) {
            topk_idx[r * k + j] = (bi == 0x7fffffff) ? 0 : bi;
            topk_logp[r * k + j] = bv;
        }
    }
}

hipError_t launch_row_topk(const float* logits, int64_t ld, int B, int W, int C, int k, double thresh,
                           int32_t* topk_idx, float* topk_logp, float* blank_logp, float* stats,
                           int32_t* cand_count, hipStream_t s) {
    if ((int64_t)B * W == 0) return hipSuccess;
    if (C > kMaxRowLds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(row_topk_kernel, dim3((unsigned)((int64_t)B * W)), dim3(256), 0, s, logits, ld, B, W, C, k,
                       thresh, topk_idx, topk_logp, blank_logp, stats, cand_count);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void row_candidates_kernel(const float* __restrict__ x, int64_t ld, int B, int W,
                                                            int C, double thresh, const float* __restrict__ stats,
                                                            const int64_t* __restrict__ cand_off, int pad,
                                                            int32_t* __restrict__ cand_idx,
                                                            float* __restrict__ cand_logp) {
    // ascending class order, like np.where (utils/ctc_codec.py:144). stats[2r], stats[2r+1] are the
    // row max and log-sum from row_topk, so the float32 log-prob is recomputed bit-identically.
    // cand_off == null: the padded layout, row r at r * pad, candidates beyond the first pad dropped.
    const int64_t r = blockIdx.x;
    const int t = (int)(r / B), b = (int)(r % B);
    const float* p = x + ((int64_t)b * W + t) * ld;
    const float mx = stats[2 * r], logs = stats[2 * r + 1];
    const int lane = threadIdx.x;
    const int64_t row0 = cand_off ? cand_off[r] : r * pad;
    int64_t base = row0;
    for (int c0 = 0; c0 < C; c0 += 64) {
        const int c = c0 + lane;
        float lp = 0.f;
        bool keep = false;
        if (c < C) {
            lp = (p[c] - mx) - logs;
            keep = (double)lp > thresh;
        }
        const unsigned long long m = __ballot(keep);
        const int64_t o = base + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && (cand_off || o - row0 < pad)) {
            cand_idx[o] = c;
            cand_logp[o] = lp;
        }
        base += __popcll(m);
    }
}

// log_softmax_rows: scipy.special.log_softmax(preds, axis=2) (utils/ctc_codec.py:65) for the whole
// tensor, float32 in / float32 out, same arithmetic as row_topk. Rows are independent (any layout).
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* __restrict__ x, int C,
                                                               float* __restrict__ y) {
    __shared__ float rv[4];
    __shared__ double rd[4];
    const int64_t r = blockIdx.x;
    const float* p = x + r * C;
    float* o = y + r * C;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float mx = -INFINITY;
    for (int c = tid; c < C; c += 256) mx = fmaxf(mx, p[c]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) rv[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
    double s = 0.0;
    for (int c = tid; c < C; c += 256) s += (double)expf(p[c] - mx);
    s = block_sum_d(s, rd);
    const float logs = logf((float)s);
    for (int c = tid; c < C; c += 256) o[c] = (p[c] - mx) - logs;
}

hipError_t launch_log_softmax_rows(const float* x, int64_t rows, int C, float* y, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(log_softmax_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, x, C, y);
    return hipGetLastError();
}

hipError_t launch_row_candidates(const float* logits, int64_t ld, int B, int W, int C, double thresh,
                                 const float* stats, const int64_t* cand_off, int pad, int32_t* cand_idx,
                                 float* cand_logp, hipStream_t s) {
    if ((int64_t)B * W == 0) return hipSuccess;
    if (!cand_off && pad < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(row_candidates_kernel, dim3((unsigned)((int64_t)B * W)), dim3(64), 0, s, logits, ld, B, W, C,
                       thresh, stats, cand_off, pad, cand_idx, cand_logp);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// Fused beam front end (see ConvArgs in kernels.h): the two small kernels between / after the two head passes.
// Same arithmetic as row_topk_kernel on a stored row: float32 log-prob = (v - max) - logf((float)sum) with the sum
// of expf(v - max) accumulated in float64; top-k by (log-prob desc, class asc); candidates are (double)lp > thresh.
// -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_thresholds_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                              int P, int64_t M, int k, double cand_thresh,
                                                              int want_candidates, float* __restrict__ row_thr,
                                                              int32_t* __restrict__ emit_cnt) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    // k largest part maxima (multiset), kept sorted descending in registers / scratch (k <= kBeamMaxK)
    float top[kBeamMaxK];
#pragma unroll
    for (int i = 0; i < kBeamMaxK; ++i) top[i] = -INFINITY;
    float gmax = -INFINITY;
    for (int p = 0; p < P; ++p) {
        float v = pmax[(int64_t)p * M + m];
        gmax = fmaxf(gmax, v);
#pragma unroll
        for (int i = 0; i < kBeamMaxK; ++i) {              // insertion: v sinks to its place, the smallest drops out
            if (i < k) {
                const float t = top[i];
                const bool sw = v > t;
                top[i] = sw ? v : t;
                v = sw ? t : v;
            }
        }
    }
    float tau = INFINITY;
#pragma unroll
    for (int i = 0; i < kBeamMaxK; ++i)
        if (i == k - 1) tau = top[i];
    // every top-k logit of the row is >= the k-th largest part maximum; a hair below it, so that a class whose
    // log-prob ROUNDS to the k-th one's (and would win the tie on its lower index) is listed as well
    float vmin = tau - 1e-5f * fmaxf(1.f, fabsf(tau));
    if (want_candidates) {
        // value bound of the candidate lists: log-prob > cand_thresh <=> v > max + log(sum) + thresh; the sum
        // estimated from the per-part sums (relative error ~1e-6) and the bound lowered by 1e-3 so that the exact
        // test in beam_select_kernel sees a superset
        double sum = 0.0;
        for (int p = 0; p < P; ++p)
            sum += (double)psum[(int64_t)p * M + m] * exp((double)pmax[(int64_t)p * M + m] - (double)gmax);
        const float vb = (float)((double)gmax + log(sum) + cand_thresh - 1e-3);
        vmin = fminf(vmin, vb);
    }
    row_thr[2 * m] = vmin;
    row_thr[2 * m + 1] = gmax;
    emit_cnt[m] = 0;
}

hipError_t launch_beam_thresholds(const float* pmax, const float* psum, int P, int64_t M, int k, double cand_thresh,
                                  int want_candidates, float* row_thr, int32_t* emit_cnt, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    if (k < 1 || k > kBeamMaxK || k > P) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_thresholds_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, pmax, psum, P, M, k,
                       cand_thresh, want_candidates, row_thr, emit_cnt);
    return hipGetLastError();
}

// one wave per row m = b*W + t; outputs at r = t*B + b
__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ row_thr, const int32_t* __restrict__ emit_cnt,
                                                          const int32_t* __restrict__ emit_list, int cap,
                                                          const double* __restrict__ esum, int P,
                                                          const float* __restrict__ blank_logit, int B, int W, int k,
                                                          double cand_thresh, int32_t* __restrict__ topk_idx,
                                                          float* __restrict__ topk_logp, float* __restrict__ blank_logp,
                                                          float* __restrict__ stats, int32_t* __restrict__ cand_count,
                                                          int32_t* __restrict__ overflow) {
    const int lane = threadIdx.x & 63;
    const int64_t M = (int64_t)B * W;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int b = (int)(m / W), t = (int)(m % W);
    const int64_t r = (int64_t)t * B + b;
    const int cnt = emit_cnt[m];
    if (cnt > cap && lane == 0) atomicExch(overflow, 1);
    const int n = cnt < cap ? cnt : cap;
    const float gmax = row_thr[2 * m + 1];
    double sum = 0.0;                                       // fixed order over the parts
    for (int p = 0; p < P; ++p) sum += esum[(int64_t)p * M + m];
    const float logs = logf((float)sum);
    const int32_t* e = emit_list + (int64_t)m * cap * 2;
    int c_above = 0;
    for (int i = lane; i < n; i += 64) {
        const float lp = (__builtin_bit_cast(float, e[2 * i + 1]) - gmax) - logs;
        c_above += ((double)lp > cand_thresh) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c_above += __shfl_xor(c_above, off);
    if (lane == 0) {
        blank_logp[r] = (blank_logit[m] - gmax) - logs;
        if (stats) { stats[2 * r] = gmax; stats[2 * r + 1] = logs; }
        if (cand_count) cand_count[r] = c_above;
    }
    // k selection rounds over the listed classes, (log-prob desc, class asc) like row_topk_kernel
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < k; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = lane; i < n; i += 64) {
            const int cls = e[2 * i];
            const float lp = (__builtin_bit_cast(float, e[2 * i + 1]) - gmax) - logs;
            const bool after = (lp < pv) || (lp == pv && cls > pi);
            if (after && (lp > bv || (lp == bv && cls < bi))) { bv = lp; bi = cls; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            argmax_merge(bv, bi, ov, oi);
        }
        pv = bv; pi = bi;
        if (lane == 0) {
            topk_idx[r * k + j] = (bi == 0x7fffffff) ? 0 : bi;
            topk_logp[r * k + j] = bv;
        }
    }
}

hipError_t launch_beam_select(const float* row_thr, const int32_t* emit_cnt, const int32_t* emit_list, int cap,
                              const double* esum, int P, const float* blank_logit, int B, int W, int k,
                              double cand_thresh, int32_t* topk_idx, float* topk_logp, float* blank_logp,
                              float* stats, int32_t* cand_count, int32_t* overflow, hipStream_t s) {
    const int64_t M = (int64_t)B * W;
    if (M <= 0) return hipSuccess;
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, row_thr, emit_cnt, emit_list, cap,
                       esum, P, blank_logit, B, W, k, cand_thresh, topk_idx, topk_logp, blank_logp, stats, cand_count,
                       overflow);
    return hipGetLastError();
}

// one wave per row: the listed classes whose log-prob exceeds the threshold, in ascending class order (np.where,
// utils/ctc_codec.py:144), written to the row's CSR slot - or, with cand_off == null, to r * pad, the first pad of them
__global__ __launch_bounds__(256) void beam_candidates_kernel(const int32_t* __restrict__ emit_cnt,
                                                              const int32_t* __restrict__ emit_list, int cap,
                                                              const float* __restrict__ stats, int B, int W,
                                                              double cand_thresh, const int64_t* __restrict__ cand_off,
                                                              int pad, int32_t* __restrict__ cand_idx,
                                                              float* __restrict__ cand_logp) {
    const int lane = threadIdx.x & 63;
    const int64_t M = (int64_t)B * W;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int b = (int)(m / W), t = (int)(m % W);
    const int64_t r = (int64_t)t * B + b;
    const int cnt = emit_cnt[m];
    const int n = cnt < cap ? cnt : cap;
    const float gmax = stats[2 * r], logs = stats[2 * r + 1];
    const int32_t* e = emit_list + (int64_t)m * cap * 2;
    const int64_t base = cand_off ? cand_off[r] : r * pad;
    for (int i = lane; i < n; i += 64) {
        const int cls = e[2 * i];
        const float lp = (__builtin_bit_cast(float, e[2 * i + 1]) - gmax) - logs;
        if (!((double)lp > cand_thresh)) continue;
        int rank = 0;                                       // candidates with a smaller class come first
        for (int u = 0; u < n; ++u) {
            const float lu = (__builtin_bit_cast(float, e[2 * u + 1]) - gmax) - logs;
            rank += ((double)lu > cand_thresh && e[2 * u] < cls) ? 1 : 0;
        }
        if (!cand_off && rank >= pad) continue;
        cand_idx[base + rank] = cls;
        cand_logp[base + rank] = lp;
    }
}

hipError_t launch_beam_candidates(const int32_t* emit_cnt, const int32_t* emit_list, int cap, const float* stats,
                                  int B, int W, double cand_thresh, const int64_t* cand_off, int pad, int32_t* cand_idx,
                                  float* cand_logp, hipStream_t s) {
    const int64_t M = (int64_t)B * W;
    if (M <= 0) return hipSuccess;
    if (!cand_off && pad < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_candidates_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, emit_cnt, emit_list, cap, stats,
                       B, W, cand_thresh, cand_off, pad, cand_idx, cand_logp);
    return hipGetLastError();
}


// -------------------------------------------------------------------------------------------
// CTC loss: torch.nn.CTCLoss over preds.log_softmax(2) (main.py:205,379-409); its gradient follows further down.
// Emissions: for row (line b, step t) the log-probs of the line's distinct classes D_b (slot 0 = blank) at
// emis[(b*W + t) * D + j]; the alpha recursion reads nothing else. See CtcLines in kernels.h.
// -------------------------------------------------------------------------------------------

// Log-sum-exp of the row p[0..C) by a 256-thread block (float32 max, float64 exp-sum and log), every thread's result.
// One pass over the row: eight loads in flight per thread, a running (max, exp-sum) rescaled when the max grows.
// A NaN anywhere in the row makes the result NaN: the exp-sum carries it, and `bad` where no sum was formed yet.
// see(v, c) is handed every element a thread loads, in ascending c (greedy_rowstat_kernel's top-2; the loss passes
// nothing, and its code is what it was).
template <class See>
__device__ __forceinline__ double ctc_row_lse(const float* __restrict__ p, int C, See see) {
    __shared__ float rv[4];
    __shared__ double rd[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float tm = -INFINITY;
    double ts = 0.0;
    bool bad = false;                              // a NaN met while the running max was still -inf
    for (int c0 = tid; c0 < C; c0 += 8 * 256) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = c0 + k * 256 < C ? p[c0 + k * 256] : -INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c0 + k * 256 < C) see(v[k], c0 + k * 256);
        float cm = v[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) cm = fmaxf(cm, v[k]);
        if (cm > tm) {
            ts *= (double)expf(tm - cm);
            tm = cm;
        }
        if (tm != -INFINITY) {
#pragma unroll
            for (int k = 0; k < 8; ++k) ts += (double)expf(v[k] - tm);
        } else {                                   // fmaxf drops a NaN: one among nothing but -inf must still count
#pragma unroll
            for (int k = 0; k < 8; ++k) bad |= v[k] != v[k];
        }
    }
    float mx = tm;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) rv[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
    const double s = block_sum_d(bad ? (double)NAN : tm == -INFINITY ? 0.0 : ts * (double)expf(tm - mx), rd);
    return (double)mx + log(s);                    // NaN for a row with a NaN or +inf; a row of nothing but -inf: -inf
}

// One 256-thread block per (t, line): log-sum-exp of the row in one pass over it, then the slots of D_b as
// float32(z - lse). Rows t >= T_b are not read. KEEP (the gradient's pass) also keeps the row's log-sum-exp,
// lse_out[b*W + t]; the arithmetic is the same, so emis is bit-identical either way.
template <bool KEEP>
__device__ __forceinline__ void ctc_lse_row(const float* __restrict__ x, int64_t ld, int64_t sb, int64_t st, int C,
                                            const CtcLines& m, int b0, int W, float* __restrict__ emis,
                                            double* __restrict__ lse_out) {
    const int64_t r = blockIdx.x;                  // b*W + t
    const int b = (int)(r / W), t = (int)(r % W), gb = b0 + b;
    if (t >= m.T[gb]) return;                      // (block-uniform)
    const float* p = x + ((int64_t)b * sb + (int64_t)t * st) * ld;
    const int tid = threadIdx.x;
    const double lse = ctc_row_lse(p, C, [](float, int) {});
    const int nd = m.nd[gb];
    const int32_t* cls = m.cls + (int64_t)gb * m.D;
    float* e = emis + ((int64_t)b * W + t) * m.D;
    for (int j = tid; j < nd; j += 256) e[j] = (float)((double)p[cls[j]] - lse);
    if (KEEP && tid == 0) lse_out[r] = lse;
}

__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ x, int64_t ld, int64_t sb, int64_t st,
                                                      int C, const CtcLines m, int b0, int W,
                                                      float* __restrict__ emis) {
    ctc_lse_row<false>(x, ld, sb, st, C, m, b0, W, emis, nullptr);
}

__global__ __launch_bounds__(256) void ctc_rowlse_kernel(const float* __restrict__ x, int64_t ld, int64_t sb, int64_t st,
                                                         int C, const CtcLines m, int b0, int W,
                                                         float* __restrict__ emis, double* __restrict__ lse_out) {
    ctc_lse_row<true>(x, ld, sb, st, C, m, b0, W, emis, lse_out);
}

__device__ __forceinline__ float ctc_logadd(float a, float b) {
    const float mx = fmaxf(a, b);
    if (mx == -INFINITY) return -INFINITY;
    return mx + log1pf(expf(-fabsf(a - b)));
}

// max + log(1 + exp(mid - max) + exp(min - max)): torch's CPU kernel's three-way log-add with the max term's
// exp(0) = 1 folded; -inf when all three are
__device__ __forceinline__ float ctc_logsum3(float la1, float la2, float la3) {
    const float mx = fmaxf(la1, fmaxf(la2, la3));
    const float mn = fminf(la1, fminf(la2, la3));
    const float md = __builtin_amdgcn_fmed3f(la1, la2, la3);
    const float v = mx + __logf(1.f + __expf(md - mx) + __expf(mn - mx));
    return mx == -INFINITY ? -INFINITY : v;
}

// ---- what the three recursions (alpha, beta, Viterbi) share. One workgroup of NW wave64s per line walks the extended
// target (blank, l1, blank, ..., lL, blank), S = 2L + 1 states; thread i holds the NS contiguous states
// [i*NS, i*NS + NS). FWD: time runs up and a state is fed from the two states below it; !FWD is the mirror image. ----

// the emission slot of each of the lane's states (0 for a blank and for a state beyond S) and whether the two-state
// transition exists: into s from s-2 where l_s != l_{s-2} (FWD), out of s into s+2 where l_{s+2} != l_s (!FWD)
template <int NS, bool FWD>
__device__ __forceinline__ void ctc_lane_setup(const int32_t* __restrict__ ts, int S, int (&slot)[NS], bool (&skip)[NS]) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = (int)threadIdx.x * NS + i;
        const bool lab = (s & 1) && s < S;
        slot[i] = lab ? ts[s >> 1] : 0;
        skip[i] = FWD ? lab && s >= 3 && ts[s >> 1] != ts[(s >> 1) - 1]
                      : lab && s + 2 < S && ts[(s >> 1) + 1] != ts[s >> 1];
    }
}

// The hand-over across a wave boundary of the forward recursion: xb[step parity][wave] = the wave's two states next to
// the boundary, nearest first, written by its last lane once a step is done - one barrier per step when NW > 1, none
// for a one-wave line. (ctc_beta_kernel keeps the mirror image, written by lane 0, as a local lambda.)
template <int NS, int NW>
__device__ __forceinline__ void ctc_publish(float (&xb)[2][NW][2], int parity, const float (&a)[NS]) {
    static_assert(NW == 1 || NS >= 2, "a wave boundary hands over two states from one lane");
    if (NW > 1) {
        if ((threadIdx.x & 63) == 63) {
            xb[parity][threadIdx.x >> 6][0] = a[NS - 1];
            xb[parity][threadIdx.x >> 6][1] = a[NS >= 2 ? NS - 2 : 0];
        }
        __syncthreads();
    }
}

// n1, n2 = the states one and two beyond the lane's own, of the step published under `parity`: from the neighbour lane
// over __shfl_up (FWD) / __shfl_down, across a wave boundary from xb, -inf beyond the line's first / last state
template <int NS, int NW, bool FWD>
__device__ __forceinline__ void ctc_neighbours(const float (&xb)[2][NW][2], int parity, const float (&a)[NS], float& n1,
                                               float& n2) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float e1 = a[FWD ? NS - 1 : 0], e2 = a[NS >= 2 ? (FWD ? NS - 2 : 1) : 0];
    n1 = FWD ? __shfl_up(e1, 1) : __shfl_down(e1, 1);
    n2 = NS >= 2 ? (FWD ? __shfl_up(e2, 1) : __shfl_down(e2, 1)) : (FWD ? __shfl_up(e1, 2) : __shfl_down(e1, 2));
    if (lane == (FWD ? 0 : 63)) {
        const bool has = FWD ? wv > 0 : wv < NW - 1;
        const int from = has ? (FWD ? wv - 1 : wv + 1) : 0;
        n1 = has ? xb[parity][from][0] : -INFINITY;
        n2 = has ? xb[parity][from][1] : -INFINITY;
    }
    if (NS == 1 && lane == (FWD ? 1 : 62)) n2 = -INFINITY;      // (NS == 1 only with NW == 1)
}

// one row of a prefetch ring: the lane's NS entries of row r. The rings hold the rows of the next PF steps, in flight
// while a step is computed, statically indexed by unrolling the step loop PF times.
template <int NS>
__device__ __forceinline__ void ctc_ring_load(const float* r, const int (&idx)[NS], float (&e)[NS]) {
#pragma unroll
    for (int i = 0; i < NS; ++i) e[i] = r[idx[i]];
}

// The forward recursion of one line over its emissions, in float32. `step` is the policy:
//   start(gb, S, a)               once, with the states of step 0
//   combine(la1, la2, la3, i, code) -> the value of the lane's state i from its three predecessors (s, s-1, s-2; -inf
//                                 where the skip does not exist), before the emission is added; code is the step's scratch
//   row(t, a, code)               after step t >= 1
//   finish(gb, L, S, last, prev)  thread 0, with the final values of states S-1 and S-2;  none(gb) for a line marked T = 0
template <int PF, int NW, class Step>
__device__ __forceinline__ void ctc_forward_line(const float* __restrict__ emis, const CtcLines& m, int b0, int W,
                                                 Step step) {
    constexpr int NS = Step::NS;
    __shared__ float xb[2][NW][2];
    __shared__ float fin[2];
    const int b = blockIdx.x, gb = b0 + b, tid = threadIdx.x;
    const int T = m.T[gb], L = m.L[gb], S = 2 * L + 1;
    if (T == 0) {                                  // no alignment (host-side feasibility test); block-uniform
        if (tid == 0) step.none(gb);
        return;
    }
    int slot[NS];
    bool skip[NS];
    ctc_lane_setup<NS, true>(m.slot + m.off[gb], S, slot, skip);
    const int D = m.D;
    const float* base = emis + (int64_t)b * W * D;
    float a[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = tid * NS + i;
        a[i] = (s == 0 || (s == 1 && S > 1)) ? base[slot[i]] : -INFINITY;
    }
    step.start(gb, S, a);
    ctc_publish<NS, NW>(xb, 0, a);
    float e[PF][NS];
#pragma unroll
    for (int k = 0; k < PF; ++k) ctc_ring_load(base + (int64_t)min(1 + k, T - 1) * D, slot, e[k]);
    for (int t0 = 1; t0 < T; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            if (t < T) {                           // (block-uniform)
                float p1, p2;
                ctc_neighbours<NS, NW, true>(xb, (t - 1) & 1, a, p1, p2);
                unsigned code = 0;
#pragma unroll
                for (int i = NS - 1; i >= 0; --i) {      // descending: a[i-1], a[i-2] still hold step t-1
                    const float la2 = i >= 1 ? a[i >= 1 ? i - 1 : 0] : p1;
                    const float la3 = skip[i] ? (i >= 2 ? a[i >= 2 ? i - 2 : 0] : (i == 1 ? p1 : p2)) : -INFINITY;
                    a[i] = step.combine(a[i], la2, la3, i, code) + e[k][i];
                }
                step.row(t, a, code);
                ctc_publish<NS, NW>(xb, t & 1, a);
            }
            ctc_ring_load(base + (int64_t)min(t + PF, T - 1) * D, slot, e[k]);   // refill the slot just used
        }
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = tid * NS + i;
        if (s == S - 1) fin[0] = a[i];
        if (s == S - 2) fin[1] = a[i];
    }
    __syncthreads();
    if (tid == 0) step.finish(gb, L, S, fin[0], fin[1]);
}

// The log-sum policy: alpha is float32, the step is ctc_logsum3.
// nll[gb] = -logaddexp(alpha_T[S-1], alpha_T[S-2]) (-alpha_T[0] for L = 0), +inf for a line marked T = 0.
// STORE (the gradient's pass) also writes every row of alpha, ast[aoff[gb] + t*S + s] for s < S; the recursion's
// arithmetic is the same, so nll is bit-identical either way.
template <int NS_, bool STORE>
struct CtcSum {
    static constexpr int NS = NS_;
    float* __restrict__ nll;
    const int64_t* __restrict__ aoff;              // (STORE only)
    float* __restrict__ ast;
    float* arow;
    int S;
    __device__ __forceinline__ void start(int gb, int S_, const float (&a)[NS]) {
        if (STORE) {
            S = S_;
            arow = ast + aoff[gb] + (int)threadIdx.x * NS;
            row(0, a, 0);
        }
    }
    __device__ __forceinline__ float combine(float la1, float la2, float la3, int, unsigned&) const {
        return ctc_logsum3(la1, la2, la3);
    }
    __device__ __forceinline__ void row(int, const float (&a)[NS], unsigned) {
        if (STORE) {
#pragma unroll
            for (int i = 0; i < NS; ++i)
                if ((int)threadIdx.x * NS + i < S) arow[i] = a[i];
            arow += S;
        }
    }
    __device__ __forceinline__ void none(int gb) const { nll[gb] = INFINITY; }
    __device__ __forceinline__ void finish(int gb, int L, int, float last, float prev) const {
        nll[gb] = L == 0 ? -last : -ctc_logadd(last, prev);
    }
};

template <int NS, int PF, int NW>
__global__ __launch_bounds__(64 * NW) void ctc_alpha_kernel(const float* __restrict__ emis, const CtcLines m, int b0,
                                                             int W, float* __restrict__ nll) {
    ctc_forward_line<PF, NW>(emis, m, b0, W, CtcSum<NS, false>{nll, nullptr, nullptr, nullptr, 0});
}

template <int NS, int PF, int NW>
__global__ __launch_bounds__(64 * NW) void ctc_alpha_store_kernel(const float* __restrict__ emis, const CtcLines m, int b0,
                                                                   int W, float* __restrict__ nll,
                                                                   const int64_t* __restrict__ aoff,
                                                                   float* __restrict__ ast) {
    ctc_forward_line<PF, NW>(emis, m, b0, W, CtcSum<NS, true>{nll, aoff, ast, nullptr, 0});
}

hipError_t launch_ctc_lse(const float* x, int64_t ld, int64_t sb, int64_t st, int C, const CtcLines& m, int b0, int nb,
                          int W, float* emis, double* lse, hipStream_t s) {
    if (nb <= 0 || W <= 0) return hipSuccess;
    const dim3 grid((unsigned)((int64_t)nb * W));
    if (lse)
        hipLaunchKernelGGL(ctc_rowlse_kernel, grid, dim3(256), 0, s, x, ld, sb, st, C, m, b0, W, emis, lse);
    else
        hipLaunchKernelGGL(ctc_lse_kernel, grid, dim3(256), 0, s, x, ld, sb, st, C, m, b0, W, emis);
    return hipGetLastError();
}

// The instances (NS states per lane, PF emission rows in flight, NW wave64s per line) of the alpha, beta and Viterbi
// kernels; a batch launches the first whose 64 * NS * NW states hold its largest extended target 2L + 1. A long target
// spreads over more waves (one barrier per step) rather than more states per lane: the recursion is latency-bound, and
// a batch of lines occupies few of the 1024 SIMDs.
#define HCTR_CTC_LADDER(X) X(1, 4, 1) X(2, 4, 1) X(2, 4, 2) X(2, 4, 4) X(2, 4, 8) X(2, 4, 16) X(4, 2, 16)

template <int NS_, int PF_, int NW_>
struct CtcRung {
    static constexpr int NS = NS_, PF = PF_, NW = NW_;
};
// visit(CtcRung<NS, PF, NW>) of the rung that max_states launches; false beyond the ladder
template <class F>
bool ctc_rung(int max_states, F visit) {
#define CTC_RUNG(NS, PF, NW)           \
    if (max_states <= 64 * NS * NW) {  \
        visit(CtcRung<NS, PF, NW>{});  \
        return true;                   \
    }
    HCTR_CTC_LADDER(CTC_RUNG)
#undef CTC_RUNG
    return false;
}
template <class F>
hipError_t ctc_launch_rung(int max_states, F launch) {
    return ctc_rung(max_states, launch) ? hipGetLastError() : hipErrorInvalidValue;
}
int ctc_viterbi_lane_states(int max_states) {
    int ns = 0;
    ctc_rung(max_states, [&](auto r) { ns = decltype(r)::NS; });
    return ns;
}
#define CTC_RUNG_STATES(NS, PF, NW) , 64 * NS * NW
const int kCtcMaxStates = std::max({0 HCTR_CTC_LADDER(CTC_RUNG_STATES)});
#undef CTC_RUNG_STATES

hipError_t launch_ctc_alpha(const float* emis, const CtcLines& m, int b0, int nb, int W, int max_states, float* nll,
                            const int64_t* aoff, float* ast, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    return ctc_launch_rung(max_states, [&](auto r) {
        using R = decltype(r);
        if (ast)
            hipLaunchKernelGGL((ctc_alpha_store_kernel<R::NS, R::PF, R::NW>), dim3((unsigned)nb), dim3(64 * R::NW), 0, s,
                               emis, m, b0, W, nll, aoff, ast);
        else
            hipLaunchKernelGGL((ctc_alpha_kernel<R::NS, R::PF, R::NW>), dim3((unsigned)nb), dim3(64 * R::NW), 0, s, emis, m,
                               b0, W, nll);
    });
}

// -------------------------------------------------------------------------------------------
// CTC loss gradient with respect to caller logits: w_b * (softmax(z_t) - gamma_t), gamma the posterior occupancy.
// ctc_rowlse_kernel keeps each row's log-sum-exp, ctc_alpha_store_kernel keeps every alpha row; ctc_beta_kernel runs
// the backward recursion and overwrites the alpha rows with the states' log-occupancies; ctc_grad_rows_kernel writes
// the gradient rows.
// -------------------------------------------------------------------------------------------

// The mirror image of ctc_forward_line over the shared pieces (FWD = false): t runs down from T-1 and the two states
// above a lane's own come from the right. a[] holds beta_{t+1} (torch's convention: the emission at t+1 included);
// step t forms
// bp(s) = logsumexp(beta_{t+1}(s), beta_{t+1}(s+1), beta_{t+1}(s+2) if l_{s+2} != l_s), overwrites the stored
// alpha_t(s) with y_t(s) = alpha_t(s) + nll + bp(s) (the log of the state's share of the posterior: alpha_t * beta_t
// has the emission twice, alpha_t * bp once), and continues with beta_t = bp + lp_t. The virtual row beta_T = (0 at
// state S-1, -inf elsewhere) makes step T-1 like every other. A second ring holds the alpha rows of the next PF steps.
// Lines without an alignment (T = 0) and lines whose loss is +inf are left alone: the row kernel writes their zeros.
template <int NS, int PF, int NW>
__global__ __launch_bounds__(64 * NW) void ctc_beta_kernel(const float* __restrict__ emis, const CtcLines m, int W,
                                                            const float* __restrict__ nll,
                                                            const int64_t* __restrict__ aoff, float* __restrict__ ast) {
    static_assert(NW == 1 || NS >= 2, "a wave boundary hands over two states from one lane");
    __shared__ float xb[2][NW][2];                 // [step parity][wave] = {state wave_begin, state wave_begin+1}
    const int gb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = m.T[gb], L = m.L[gb], S = 2 * L + 1;
    if (T == 0) return;                            // (block-uniform)
    const float nl = nll[gb];
    if (nl == INFINITY) return;                    // (block-uniform)
    int slot[NS];
    bool skip[NS];
    ctc_lane_setup<NS, false>(m.slot + m.off[gb], S, slot, skip);
    const int D = m.D;
    const float* base = emis + (int64_t)gb * W * D;
    float* abase = ast + aoff[gb];
    int sc[NS];                                    // the lane's states, clamped into the row for the loads
    float a[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = tid * NS + i;
        sc[i] = min(s, S - 1);
        a[i] = s == S - 1 ? 0.f : -INFINITY;
    }
    auto publish = [&](int parity) {             // ctc_publish's mirror, kept local: through the shared helper the
                                                   // kernel took 4 more VGPRs and 3 % more time at 64 x 2000
        if (NW > 1) {
            if (lane == 0) {
                xb[parity][wv][0] = a[0];
                xb[parity][wv][1] = a[NS >= 2 ? 1 : 0];
            }
            __syncthreads();
        }
    };
    publish(0);
    float e[PF][NS], al[PF][NS];
    auto ring_load = [&](int k, int row) {         // the emission ring and the alpha ring, a state's two loads together
        const float* r = base + (int64_t)row * D;
        const float* ar = abase + (int64_t)row * S;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            e[k][i] = r[slot[i]];
            al[k][i] = ar[sc[i]];
        }
    };
#pragma unroll
    for (int k = 0; k < PF; ++k) ring_load(k, max(T - 1 - k, 0));
    int par = 0;
    for (int t0 = T - 1; t0 >= 0; t0 -= PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 - k;
            if (t >= 0) {                          // (block-uniform)
                float q1, q2;
                ctc_neighbours<NS, NW, false>(xb, par, a, q1, q2);
                float* yr = abase + (int64_t)t * S + tid * NS;
#pragma unroll
                for (int i = 0; i < NS; ++i) {         // ascending: a[i+1], a[i+2] still hold step t+1
                    const float la2 = i + 1 < NS ? a[i + 1 < NS ? i + 1 : 0] : q1;
                    const float la3 = skip[i] ? (i + 2 < NS ? a[i + 2 < NS ? i + 2 : 0] : (i + 2 == NS ? q1 : q2))
                                              : -INFINITY;
                    const float bp = ctc_logsum3(a[i], la2, la3);
                    if (tid * NS + i < S) yr[i] = (al[k][i] + nl) + bp;
                    a[i] = bp + e[k][i];
                }
                par ^= 1;
                publish(par);
            }
            ring_load(k, max(t - PF, 0));          // refill the slots just used
        }
    }
}

// One 256-thread block per (line, step), like ctc_lse: the row of y (S log-occupancies) gives the states' shares
// q_s = exp(y_s); they are normalised by their own sum over the row (exp(-nll) * exp(nll) = 1 in exact arithmetic; the
// division takes out the rounding drift that alpha_t and beta_t have in common, so gamma sums to 1 to float32 rounding
// at every step), the even states are the blank's share, and the share of class slot j is summed over the target
// positions pos[soff[j] .. soff[j+1]) that carry it, in a fixed order (no atomics: the result does not depend on
// scheduling). The logits row is read once, eight loads in flight: grad = w * exp(z - lse) for all C classes, then the
// line's <= D classes again as w * (exp(z - lse) - gamma). Rows t >= T and the rows of lines whose loss is +inf are
// zeros.
__global__ __launch_bounds__(256) void ctc_grad_rows_kernel(const float* __restrict__ x, int C, int B, int W,
                                                            const CtcLines m, const double* __restrict__ lse,
                                                            const float* __restrict__ nll, const float* __restrict__ wt,
                                                            const int64_t* __restrict__ aoff,
                                                            const float* __restrict__ ast,
                                                            const int32_t* __restrict__ soff,
                                                            const int32_t* __restrict__ pos, float* __restrict__ grad) {
    __shared__ double rd[4];
    const int64_t r = blockIdx.x;                  // b*W + t
    const int b = (int)(r / W), t = (int)(r % W), tid = threadIdx.x;
    const float* p = x + ((int64_t)t * B + b) * C;
    float* o = grad + ((int64_t)t * B + b) * C;
    const int T = m.T[b];
    if (t >= T || nll[b] == INFINITY) {            // (block-uniform)
        for (int c = tid; c < C; c += 256) o[c] = 0.f;
        return;
    }
    const int S = 2 * m.L[b] + 1;
    const float* y = ast + aoff[b] + (int64_t)t * S;
    double qe = 0.0, qo = 0.0;
    for (int s = 2 * tid; s < S; s += 512) {
        qe += (double)expf(y[s]);
        if (s + 1 < S) qo += (double)expf(y[s + 1]);
    }
    const double blank = block_sum_d(qe, rd);
    const double Z = blank + block_sum_d(qo, rd);
    const double l = lse[r];
    const float w = wt[b];
    for (int c0 = tid; c0 < C; c0 += 8 * 256) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = c0 + k * 256 < C ? p[c0 + k * 256] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (c0 + k * 256 < C) o[c0 + k * 256] = w * expf((float)((double)v[k] - l));
    }
    __syncthreads();                               // the line's classes are written a second time, by other threads
    const int nd = m.nd[b];
    const int32_t* cls = m.cls + (int64_t)b * m.D;
    const int32_t* so = soff + (int64_t)b * (m.D + 1);
    const int32_t* ps = pos + m.off[b];
    for (int j = tid; j < nd; j += 256) {
        double g = blank;
        if (j > 0) {
            g = 0.0;
            for (int k = so[j]; k < so[j + 1]; ++k) g += (double)expf(y[2 * ps[k] + 1]);
        }
        const int c = cls[j];
        o[c] = w * (expf((float)((double)p[c] - l)) - (float)(g / Z));
    }
}

hipError_t launch_ctc_beta(const float* emis, const CtcLines& m, int B, int W, int max_states, const float* nll,
                           const int64_t* aoff, float* ast, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    return ctc_launch_rung(max_states, [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL((ctc_beta_kernel<R::NS, R::PF, R::NW>), dim3((unsigned)B), dim3(64 * R::NW), 0, s, emis, m, W, nll,
                           aoff, ast);
    });
}

hipError_t launch_ctc_grad_rows(const float* x, int C, int B, int W, const CtcLines& m, const double* lse,
                                const float* nll, const float* wt, const int64_t* aoff, const float* ast,
                                const int32_t* soff, const int32_t* pos, float* grad, hipStream_t s) {
    if (B <= 0 || W <= 0) return hipSuccess;
    hipLaunchKernelGGL(ctc_grad_rows_kernel, dim3((unsigned)((int64_t)B * W)), dim3(256), 0, s, x, C, B, W, m, lse, nll, wt,
                       aoff, ast, soff, pos, grad);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// CTC forced alignment (hctr_ctc_align*): the best path of a known transcription over the emissions of ctc_lse_kernel.
// ctc_viterbi_kernel is ctc_forward_line under the max-plus policy with 2-bit backpointers, ctc_backtrace_kernel walks
// them back and writes the path, the character spans and their log-probabilities.
// -------------------------------------------------------------------------------------------

// The max-plus policy: v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), [l_s != l_{s-2}] v_{t-1}(s-2)) + lp_t(s) in float32. Ties
// are part of the contract: a predecessor replaces the running best only when strictly greater, in the order s, s-1,
// s-2. The choice (0, 1 or 2 states down) of the lane's NS states is packed into one byte, state i at bits 2i, and
// stored at bp[boff[gb] + t * ceil(S / NS) + lane index] for t >= 1: consecutive lanes, consecutive bytes. score[gb] is
// the better of v_{T-1}(S-1) and v_{T-1}(S-2) (S-1 on a tie; state 0 for L = 0) and endst[gb] that state; a line marked
// T = 0 gets -inf and -1, and so does a line whose best score is -inf (masked logits leave it no path). A NaN score
// (a non-finite logits row) stays NaN with the end state S-2 or S-1: comparisons with NaN are false.
template <int NS_>
struct CtcMax {
    static constexpr int NS = NS_;
    static_assert(NS <= 4, "one byte holds the backpointers of a lane");
    const int64_t* __restrict__ boff;
    uint8_t* __restrict__ bp;
    float* __restrict__ score;
    int32_t* __restrict__ endst;
    uint8_t* brow;
    int stride;                                    // bytes per step: the lanes that hold a state
    __device__ __forceinline__ void start(int gb, int S, const float (&)[NS]) {
        stride = (S + NS - 1) / NS;
        brow = bp + boff[gb] + (int)threadIdx.x;
    }
    __device__ __forceinline__ float combine(float best, float la2, float la3, int i, unsigned& code) const {
        unsigned from = 0;
        if (la2 > best) { best = la2; from = 1; }
        if (la3 > best) { best = la3; from = 2; }
        code |= from << (2 * i);
        return best;
    }
    __device__ __forceinline__ void row(int t, const float (&)[NS], unsigned code) const {
        if ((int)threadIdx.x < stride) brow[(int64_t)t * stride] = (uint8_t)code;
    }
    __device__ __forceinline__ void none(int gb) const {
        score[gb] = -INFINITY;
        endst[gb] = -1;
    }
    __device__ __forceinline__ void finish(int gb, int L, int S, float last, float prev) const {
        const bool end = L == 0 || last >= prev;
        const float best = end ? last : prev;
        score[gb] = best;
        endst[gb] = best == -INFINITY ? -1 : (end ? S - 1 : S - 2);    // every path masked out: no alignment
    }
};

template <int NS, int PF, int NW>
__global__ __launch_bounds__(64 * NW) void ctc_viterbi_kernel(const float* __restrict__ emis, const CtcLines m, int b0,
                                                               int W, const int64_t* __restrict__ boff,
                                                               uint8_t* __restrict__ bp, float* __restrict__ score,
                                                               int32_t* __restrict__ endst) {
    ctc_forward_line<PF, NW>(emis, m, b0, W, CtcMax<NS>{boff, bp, score, endst, nullptr, 0});
}

// One 256-thread workgroup per line. The walk t = T-1 .. 1 is serial and every step's read depends on the one before,
// so the backpointers are staged kBtSteps steps at a time in LDS: the state falls by at most two per step, so step r of
// a chunk that starts in state s can only need the bytes of the states [s - 2r, s] of its row. All threads load the
// window (independent byte loads, all in flight together), then every thread walks the chunk on LDS broadcasts with
// the same scalar state; thread 0 stores the state of every step and, where the state changes, the span ends. After
// the walk the steps are mapped to classes and the spans' log-probabilities summed (ascending t, float32) in parallel.
// sh = log2 of the recursion instance's states per lane. Lines without an alignment (T = 0 or endst < 0): path and spans -1,
// logp -inf.
constexpr int kBtSteps = 32;
__global__ __launch_bounds__(256) void ctc_backtrace_kernel(const float* __restrict__ emis, const CtcLines m, int b0, int W,
                                                            int sh, const int64_t* __restrict__ boff,
                                                            const uint8_t* __restrict__ bp,
                                                            const int32_t* __restrict__ endst, int32_t* __restrict__ path,
                                                            int32_t* __restrict__ sstart, int32_t* __restrict__ send,
                                                            float* __restrict__ slogp) {
    constexpr int WB = 2 * kBtSteps + 2;           // window bytes per step at one state per byte (sh = 0)
    __shared__ uint8_t win[kBtSteps][WB];
    const int b = blockIdx.x, gb = b0 + b, tid = threadIdx.x;
    const int T = m.T[gb], L = m.L[gb], S = 2 * L + 1;
    const int32_t* ts = m.slot + m.off[gb];
    int32_t* P = path + (int64_t)gb * W;
    int32_t* st = sstart + m.off[gb];
    int32_t* en = send + m.off[gb];
    float* lg = slogp + m.off[gb];
    for (int j = tid; j < L; j += 256) {
        st[j] = -1;
        en[j] = -1;
        lg[j] = -INFINITY;
    }
    if (T == 0 || endst[gb] < 0) {                 // (block-uniform) infeasible by length, or every path is -inf
        for (int t = tid; t < W; t += 256) P[t] = -1;
        return;
    }
    __syncthreads();                               // thread 0 overwrites the spans below
    const int stride = (S + (1 << sh) - 1) >> sh, smask = (1 << sh) - 1;
    const uint8_t* rows = bp + boff[gb];
    int s = min(max(endst[gb], 0), S - 1);
    int above = -1;                                // state of step t + 1
    for (int t0 = T - 1; t0 >= 1; t0 -= kBtSteps) {
        const int n = min(kBtSteps, t0);           // steps t0, t0-1, ..., t0-n+1 read rows of the same numbers
        const int hi = s >> sh, lo = max(s - 2 * (n - 1), 0) >> sh, wb = hi - lo + 1;      // wb <= WB
        for (int idx = tid; idx < n * wb; idx += 256) {
            const int r = idx / wb, col = lo + idx % wb;
            if (col >= (max(s - 2 * r, 0) >> sh)) win[r][col - lo] = rows[(int64_t)(t0 - r) * stride + col];
        }
        __syncthreads();
        for (int r = 0; r < n; ++r) {
            const int t = t0 - r;
            const int from = (win[r][(s >> sh) - lo] >> (2 * (s & smask))) & 3;
            if (tid == 0) {
                P[t] = s;
                if (s & 1) {
                    if (s != above) en[s >> 1] = t + 1;
                    if (from) st[s >> 1] = t;
                }
            }
            above = s;
            s = __builtin_amdgcn_readfirstlane(max(s - from, 0));
        }
        __syncthreads();                           // the window is loaded again
    }
    if (tid == 0) {                                // step 0 has no predecessor
        P[0] = s;
        if (s & 1) {
            if (s != above) en[s >> 1] = 1;
            st[s >> 1] = 0;
        }
    }
    __syncthreads();
    const int32_t* cls = m.cls + (int64_t)gb * m.D;
    for (int t = tid; t < W; t += 256) {
        const int v = t < T ? P[t] : -1;
        P[t] = v < 0 ? -1 : ((v & 1) ? cls[ts[v >> 1]] : 0);
    }
    const int D = m.D;
    const float* base = emis + (int64_t)b * W * D;
    for (int j = tid; j < L; j += 256) {
        const int t1 = st[j], t2 = en[j];
        if (t1 < 0 || t2 <= t1) continue;
        const float* q = base + ts[j];
        float acc = q[(int64_t)t1 * D];
        for (int t = t1 + 1; t < t2; ++t) acc += q[(int64_t)t * D];
        lg[j] = acc;
    }
}

hipError_t launch_ctc_viterbi(const float* emis, const CtcLines& m, int b0, int nb, int W, int max_states,
                              const int64_t* boff, uint8_t* bp, float* score, int32_t* endst, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    return ctc_launch_rung(max_states, [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL((ctc_viterbi_kernel<R::NS, R::PF, R::NW>), dim3((unsigned)nb), dim3(64 * R::NW), 0, s, emis, m, b0,
                           W, boff, bp, score, endst);
    });
}

hipError_t launch_ctc_backtrace(const float* emis, const CtcLines& m, int b0, int nb, int W, int max_states,
                                const int64_t* boff, const uint8_t* bp, const int32_t* endst, int32_t* path,
                                int32_t* span_start, int32_t* span_end, float* span_logp, hipStream_t s) {
    if (nb <= 0 || max_states > kCtcMaxStates) return nb <= 0 ? hipSuccess : hipErrorInvalidValue;
    const int ns = ctc_viterbi_lane_states(max_states), sh = ns == 1 ? 0 : ns == 2 ? 1 : 2;
    hipLaunchKernelGGL(ctc_backtrace_kernel, dim3((unsigned)nb), dim3(256), 0, s, emis, m, b0, W, sh, boff, bp, endst, path,
                       span_start, span_end, span_logp);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// Greedy recognition (hctr_recognize*): the greedy path is itself a CTC path, so its spans need no recursion.
// greedy_rowstat_kernel reads every row once for argmax, runner-up and log-sum-exp; greedy_spans_kernel collapses a
// line and sums each character's run; ctc_emis_gather_kernel forms the emissions of the decoded text from the kept
// log-sum-exp, for the loss's own ctc_alpha ladder.
// -------------------------------------------------------------------------------------------
constexpr int kNoIdx = 0x7fffffff;

// np.argmax's order between two (value, class) pairs of distinct classes: NaN counts as the maximum, the lower class
// wins a tie. The empty pair (-inf, kNoIdx) loses to every real one.
__device__ __forceinline__ bool np_beats(float a, int ai, float b, int bi) {
    return np_gt(a, b) || (np_eq(a, b) && ai < bi);
}

// the best two of the union of two best-two pairs over disjoint classes
__device__ __forceinline__ void top2_merge(float& bv, int& bi, float& sv, int& si, float obv, int obi, float osv, int osi) {
    const bool wins = np_beats(obv, obi, bv, bi);
    const float lv = wins ? bv : obv, kv = wins ? osv : sv;      // the losing best against the winner's own runner-up
    const int li = wins ? bi : obi, ki = wins ? osi : si;
    const bool l2 = np_beats(lv, li, kv, ki);
    sv = l2 ? lv : kv;
    si = l2 ? li : ki;
    if (wins) { bv = obv; bi = obi; }
}

// One 256-thread block per row r = b*W + t of the pass (logits at x + (b*sb + t*st) * ld): ctc_row_lse's pass over the
// row, which also carries each thread's best two elements. A thread sees its classes in ascending order, so strict
// comparisons keep the first index; elements equal to -inf never enter, and the row's last thread settles the rows
// that have fewer than two others.
__global__ __launch_bounds__(256) void greedy_rowstat_kernel(const float* __restrict__ x, int64_t ld, int64_t sb, int64_t st,
                                                             int C, int W, int32_t* __restrict__ k1,
                                                             int32_t* __restrict__ k2, float* __restrict__ lp1,
                                                             float* __restrict__ lp2, double* __restrict__ lse_out) {
    __shared__ float wbv[4], wsv[4];
    __shared__ int wbi[4], wsi[4];
    const int64_t r = blockIdx.x;
    const int b = (int)(r / W), t = (int)(r % W);
    const float* p = x + ((int64_t)b * sb + (int64_t)t * st) * ld;
    float bv = -INFINITY, sv = -INFINITY;
    int bi = kNoIdx, si = kNoIdx;
    const double lse = ctc_row_lse(p, C, [&](float v, int c) {
        if (!(v <= sv)) {                          // above the runner-up, or a NaN on either side
            const bool nb = np_gt(v, bv), ns = !nb && np_gt(v, sv);     // (selects: the four stay in registers)
            sv = nb ? bv : ns ? v : sv;
            si = nb ? bi : ns ? c : si;
            bv = nb ? v : bv;
            bi = nb ? c : bi;
        }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        top2_merge(bv, bi, sv, si, __shfl_xor(bv, off), __shfl_xor(bi, off), __shfl_xor(sv, off), __shfl_xor(si, off));
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { wbv[tid >> 6] = bv; wbi[tid >> 6] = bi; wsv[tid >> 6] = sv; wsi[tid >> 6] = si; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) top2_merge(bv, bi, sv, si, wbv[w], wbi[w], wsv[w], wsi[w]);
        // what never entered is -inf: the first such class is the answer where fewer than two others exist
        if (bi == kNoIdx) bi = 0;
        if (si == kNoIdx) si = bi == 0 ? 1 : 0;
        k1[r] = bi;
        k2[r] = si;
        lp1[r] = (float)((double)bv - lse);
        lp2[r] = (float)((double)sv - lse);
        lse_out[r] = lse;
    }
}

// One 256-thread block per line over the row figures [b][t]. Wave 0 marks the kept columns (ctc_collapse_kernel's rule
// and compaction; the previous column is compared raw, so a run may straddle a 64-column chunk) and writes each
// character's label and first column; then a thread per character walks its run: the ascending-t float32 sum of lp1,
// the run's end and its peak column (largest lp1, first on ties), whose runner-up it reports. path_logp: per-thread
// strided sums, an xor tree per wave, the four waves in order.
__global__ __launch_bounds__(256) void greedy_spans_kernel(const int32_t* __restrict__ k1, const int32_t* __restrict__ k2,
                                                           const float* __restrict__ lp1, const float* __restrict__ lp2,
                                                           int W, int C, int32_t* labels, int32_t* lengths,
                                                           int32_t* span_start, int32_t* __restrict__ span_end,
                                                           float* __restrict__ char_logp, int32_t* __restrict__ alt_label,
                                                           float* __restrict__ alt_logp, float* __restrict__ path_logp) {
    __shared__ int s_n;
    __shared__ float s_part[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int64_t o = (int64_t)b * W;
    const int32_t* p = k1 + o;
    if (tid < 64) {
        int base = 0;
        for (int t0 = 0; t0 < W; t0 += 64) {
            const int t = t0 + lane;
            int cur = 0, prev = -1;
            if (t < W) {
                cur = p[t];
                if (t > 0) prev = p[t - 1];
            }
            const bool keep = (t < W) && cur != 0 && cur != C - 1 && cur != prev;
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const int j = base + __popcll(m & ((1ull << lane) - 1ull));
                labels[o + j] = cur;
                span_start[o + j] = t;
            }
            base += __popcll(m);
        }
        if (lane == 0) { lengths[b] = base; s_n = base; }
    }
    float ps = 0.f;
    for (int t = tid; t < W; t += 256) ps += lp1[o + t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ps += __shfl_xor(ps, off);
    if (lane == 0) s_part[tid >> 6] = ps;
    __syncthreads();
    if (tid == 0) path_logp[b] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    const int n = s_n;
    for (int j = tid; j < n; j += 256) {
        const int label = labels[o + j], s = span_start[o + j];
        float sum = 0.f, pv = lp1[o + s];
        int pt = s, t = s;
        for (; t < W && p[t] == label; ++t) {
            const float v = lp1[o + t];
            sum += v;
            if (v > pv) { pv = v; pt = t; }
        }
        span_end[o + j] = t;
        char_logp[o + j] = sum;
        alt_label[o + j] = k2[o + pt];
        alt_logp[o + j] = sum != sum ? sum : lp2[o + pt];      // a NaN row in the span: NaN, whichever column peaked
    }
    for (int j = n + tid; j < W; j += 256) {                   // past the text: zeros, so whole arrays compare equal
        labels[o + j] = 0; span_start[o + j] = 0; span_end[o + j] = 0; alt_label[o + j] = 0;
        char_logp[o + j] = 0.f; alt_logp[o + j] = 0.f;
    }
}

// emissions of the decoded text from the kept log-sum-exp: thread per (row r = b*W + t, slot j), D values read per row
__global__ __launch_bounds__(256) void ctc_emis_gather_kernel(const float* __restrict__ x, int64_t ld, int64_t sb, int64_t st,
                                                              const CtcLines m, int b0, int64_t rows, int W,
                                                              const double* __restrict__ lse, float* __restrict__ emis) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = i / m.D;
    const int j = (int)(i % m.D);
    if (r >= rows) return;
    const int b = (int)(r / W), t = (int)(r % W), gb = b0 + b;
    if (t >= m.T[gb] || j >= m.nd[gb]) return;
    const float* p = x + ((int64_t)b * sb + (int64_t)t * st) * ld;
    emis[r * m.D + j] = (float)((double)p[m.cls[(int64_t)gb * m.D + j]] - lse[r]);
}

hipError_t launch_greedy_rowstat(const float* x, int64_t ld, int64_t sb, int64_t st, int C, int nb, int W, int32_t* k1,
                                 int32_t* k2, float* lp1, float* lp2, double* lse, hipStream_t s) {
    const int64_t rows = (int64_t)nb * W;
    if (rows <= 0) return hipSuccess;
    if (rows > INT32_MAX || C < 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(greedy_rowstat_kernel, dim3((unsigned)rows), dim3(256), 0, s, x, ld, sb, st, C, W, k1, k2, lp1, lp2,
                       lse);
    return hipGetLastError();
}

hipError_t launch_greedy_spans(const int32_t* k1, const int32_t* k2, const float* lp1, const float* lp2, int nb, int W,
                               int C, int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end,
                               float* char_logp, int32_t* alt_label, float* alt_logp, float* path_logp, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    hipLaunchKernelGGL(greedy_spans_kernel, dim3((unsigned)nb), dim3(256), 0, s, k1, k2, lp1, lp2, W, C, labels, lengths,
                       span_start, span_end, char_logp, alt_label, alt_logp, path_logp);
    return hipGetLastError();
}

hipError_t launch_ctc_emis_gather(const float* x, int64_t ld, int64_t sb, int64_t st, const CtcLines& m, int b0, int nb,
                                  int W, const double* lse, float* emis, hipStream_t s) {
    const int64_t rows = (int64_t)nb * W, grid = (rows * m.D + 255) / 256;
    if (rows <= 0) return hipSuccess;
    if (grid > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctc_emis_gather_kernel, dim3((unsigned)grid), dim3(256), 0, s, x, ld, sb, st, m, b0, rows, W, lse,
                       emis);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// Edit distance (hctr_edit_distance, hctr_evaluate*): the Levenshtein recursion of a hypothesis h_1..h_H against a
// reference r_1..r_L, D[i][j] = min(D[i-1][j-1] + (r_i != h_j), D[i-1][j] + 1, D[i][j-1] + 1), all int32 and exact.
// edit_distance_kernel sweeps it lane-skewed and, with STORE, keeps 2-bit backpointers; edit_backtrace_kernel walks
// them back from (L, H) and writes the counts and the two maps.
// -------------------------------------------------------------------------------------------

// The instances (NS reference rows per lane, NW wave64s per line); a batch launches the first whose 64 * NS * NW rows
// hold its longest reference. As in HCTR_CTC_LADDER a long reference spreads over more waves before it takes more rows
// per lane; the last rung takes four rows, because every lane in use is one more step of the skewed sweep.
#define HCTR_EDIT_LADDER(X) X(1, 1) X(2, 1) X(2, 2) X(2, 4) X(2, 8) X(4, 8)
constexpr int kEditPF = 4;                         // hypothesis symbols in flight per lane

// The sweep: thread k owns the rows k*NS + 1 .. k*NS + NS and keeps their D[row][j-1] in registers. At step d it works
// on column j = d - k + 1 (when 1 <= j <= H). D[k*NS][j], the row above its first, is what thread k-1 finished at step
// d-1: it arrives over __shfl_up, across a wave boundary through xb[step parity][wave] with one barrier per step (none
// for a one-wave line); the value that arrived a step earlier is D[k*NS][j-1]. Thread 0 takes j and j-1. A thread
// outside its columns keeps its registers, so after the H + lanes - 1 steps every row holds D[row][H]. Rows beyond L
// compute figures nobody reads: a row depends on the rows above it only.
// STORE: the backpointer of a cell by the contract's tie order (0 diagonal, 1 deletion, 2 insertion), the NS cells of
// a thread in one byte (row i at bits 2i), at bp[boff[b] + d * lanes + k], lanes = ceil(L / NS): the bytes one step
// stores are consecutive, although its threads work on different columns.
template <int NS, int NW, bool STORE>
__global__ __launch_bounds__(64 * NW) void edit_distance_kernel(const EditLines m, int b0,
                                                                 const int32_t* __restrict__ line_of,
                                                                 const int32_t* __restrict__ hyp,
                                                                 const int32_t* __restrict__ hlen, int stride,
                                                                 const int64_t* __restrict__ boff,
                                                                 uint8_t* __restrict__ bp, int32_t* __restrict__ edits) {
    static_assert(NS <= 4, "one byte holds the backpointers of a lane");
    __shared__ int xb[2][NW];
    // ob = the line's place in edits; its reference is line ob's, or with m.wrap line (ob mod wrap)'s (the LM sweep)
    const int b = blockIdx.x, ob = line_of ? line_of[b] : b0 + b, gb = m.wrap > 0 ? ob % m.wrap : ob, tid = threadIdx.x;
    const int L = m.L[gb], H = hlen[b];
    const int32_t* __restrict__ r = m.ref + m.off[gb];
    const int32_t* __restrict__ h = hyp + (int64_t)b * stride;
    const int lanes = (L + NS - 1) / NS;
    int left[NS], rs[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int row = tid * NS + i + 1;
        left[i] = row;                             // D[row][0]
        rs[i] = row <= L ? r[row - 1] : 0;
    }
    int diag0 = tid * NS;                          // D[k*NS][j-1] of the thread's next column
    const int nsteps = (L > 0 && H > 0) ? H + lanes - 1 : 0;     // (block-uniform)
    uint8_t* brow = nullptr;
    if (STORE) brow = bp + boff[b] + tid;
    if (NW > 1) {
        if ((tid & 63) == 63) xb[1][tid >> 6] = left[NS - 1];      // "step -1"; never read by a thread in its columns
        __syncthreads();
    }
    int e[kEditPF];
#pragma unroll
    for (int k = 0; k < kEditPF; ++k) e[k] = nsteps ? h[min(max(k - tid, 0), H - 1)] : 0;
    for (int d0 = 0; d0 < nsteps; d0 += kEditPF) {
#pragma unroll
        for (int k = 0; k < kEditPF; ++k) {
            const int d = d0 + k;
            if (d < nsteps) {                      // (block-uniform)
                const int j = d - tid + 1;
                int top = __shfl_up(left[NS - 1], 1);
                if (NW > 1 && (tid & 63) == 0 && tid > 0) top = xb[(d - 1) & 1][(tid >> 6) - 1];
                if (tid == 0) top = j;
                if (j >= 1 && j <= H) {
                    const int hs = e[k];
                    int up = top, dg = diag0;
                    unsigned code = 0;
#pragma unroll
                    for (int i = 0; i < NS; ++i) {
                        const int sub = dg + (rs[i] != hs ? 1 : 0), del = up + 1, ins = left[i] + 1;
                        const int v = min(sub, min(del, ins));
                        if (STORE) code |= (v == sub ? 0u : v == del ? 1u : 2u) << (2 * i);
                        dg = left[i];
                        left[i] = v;
                        up = v;
                    }
                    diag0 = top;
                    if (STORE && tid < lanes) brow[(int64_t)d * lanes] = (uint8_t)code;
                }
                if (NW > 1) {
                    if ((tid & 63) == 63) xb[d & 1][tid >> 6] = left[NS - 1];
                    __syncthreads();
                }
            }
            if (nsteps) e[k] = h[min(max(d + kEditPF - tid, 0), H - 1)];      // refill the slot just used
        }
    }
    if (L == 0) {
        if (tid == 0) edits[ob] = H;
    } else if (tid == (L - 1) / NS) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i == (L - 1) % NS) edits[ob] = left[i];
    }
}

// One 256-thread workgroup per line, as ctc_backtrace_kernel: the walk from (L, H) is serial, so the backpointers are
// staged in LDS a (kEditWin + 1)^2 window of cells at a time - a step lowers i, j or both by one, so the walk stays in
// the window [i0 - kEditWin, i0] x [j0 - kEditWin, j0] for more than kEditWin steps. All threads load the window
// (independent byte loads), then every thread walks it on LDS broadcasts with the same scalar state and thread 0
// stores the maps. On the border j = 0 what is left of the reference is deleted, on i = 0 what is left of the
// hypothesis inserted. Deletions and insertions are counted in the walk; the substitutions afterwards in parallel from
// hyp_map (int32 sums, so the order does not matter), and hits = L - S - D. hyp_map past H is zeroed.
// sh = log2 of the sweep instance's rows per lane.
constexpr int kEditWin = 32;
__global__ __launch_bounds__(256) void edit_backtrace_kernel(const EditLines m, int b0, const int32_t* __restrict__ line_of,
                                                             const int32_t* __restrict__ hyp,
                                                             const int32_t* __restrict__ hlen, int stride, int sh,
                                                             const int64_t* __restrict__ boff,
                                                             const uint8_t* __restrict__ bp, int32_t* __restrict__ counts,
                                                             int32_t* ref_map, int32_t* hyp_map) {
    constexpr int WC = kEditWin + 1;
    __shared__ uint8_t win[WC][WC + 3];            // [column][lane byte]; at most WC lanes at one row per lane
    __shared__ int s_sub[4];
    const int b = blockIdx.x, gb = line_of ? line_of[b] : b0 + b, tid = threadIdx.x;
    const int L = m.L[gb], H = hlen[b];
    const int32_t* __restrict__ r = m.ref + m.off[gb];
    const int32_t* __restrict__ h = hyp + (int64_t)b * stride;
    int32_t* rm = ref_map + m.off[gb];
    int32_t* hm = hyp_map + (int64_t)gb * stride;
    const int lanes = (L + (1 << sh) - 1) >> sh, smask = (1 << sh) - 1;
    const uint8_t* rows = bp + boff[b];
    int i = L, j = H, ndel = 0, nins = 0;
    while (i > 0 && j > 0) {                       // (block-uniform)
        const int ilo = max(i - kEditWin, 1), jlo = max(j - kEditWin, 1);
        const int klo = (ilo - 1) >> sh, kn = ((i - 1) >> sh) - klo + 1, jn = j - jlo + 1;
        for (int idx = tid; idx < jn * kn; idx += 256) {
            const int jj = jlo + idx / kn, k = klo + idx % kn;
            win[jj - jlo][k - klo] = rows[(int64_t)(jj - 1 + k) * lanes + k];
        }
        __syncthreads();
        while (i >= ilo && j >= jlo) {
            const int k = (i - 1) >> sh;
            const int from = (win[j - jlo][k - klo] >> (2 * ((i - 1) & smask))) & 3;
            if (tid == 0) {
                if (from != 2) rm[i - 1] = from == 0 ? j - 1 : -1;
                if (from != 1) hm[j - 1] = from == 0 ? i - 1 : -1;
            }
            ndel += from == 1;
            nins += from == 2;
            i = __builtin_amdgcn_readfirstlane(i - (from != 2));
            j = __builtin_amdgcn_readfirstlane(j - (from != 1));
        }
        __syncthreads();                           // the window is loaded again
    }
    ndel += i;
    nins += j;
    for (int t = tid; t < i; t += 256) rm[t] = -1;
    for (int t = tid; t < j; t += 256) hm[t] = -1;
    for (int t = H + tid; t < stride; t += 256) hm[t] = 0;
    __syncthreads();                               // thread 0's hyp_map, read below
    int nsub = 0;
    for (int t = tid; t < H; t += 256) {
        const int at = hm[t];
        if (at >= 0 && r[at] != h[t]) ++nsub;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nsub += __shfl_xor(nsub, off);
    if ((tid & 63) == 0) s_sub[tid >> 6] = nsub;
    __syncthreads();
    if (tid == 0) {
        nsub = s_sub[0] + s_sub[1] + s_sub[2] + s_sub[3];
        int32_t* c = counts + (int64_t)gb * 4;
        c[0] = L - nsub - ndel;
        c[1] = nsub;
        c[2] = ndel;
        c[3] = nins;
    }
}

template <int NS_, int NW_>
struct EditRung {
    static constexpr int NS = NS_, NW = NW_;
};
// visit(EditRung<NS, NW>) of the rung that a longest reference of max_len launches; false beyond the ladder
template <class F>
bool edit_rung(int max_len, F visit) {
#define EDIT_RUNG(NS, NW)              \
    if (max_len <= 64 * NS * NW) {     \
        visit(EditRung<NS, NW>{});     \
        return true;                   \
    }
    HCTR_EDIT_LADDER(EDIT_RUNG)
#undef EDIT_RUNG
    return false;
}
int edit_lane_rows(int max_len) {
    int ns = 0;
    edit_rung(max_len, [&](auto r) { ns = decltype(r)::NS; });
    return ns;
}
#define EDIT_RUNG_ROWS(NS, NW) , 64 * NS * NW
const int kEditMaxRows = std::max({0 HCTR_EDIT_LADDER(EDIT_RUNG_ROWS)});
#undef EDIT_RUNG_ROWS

hipError_t launch_edit_distance(const EditLines& m, int b0, const int32_t* line_of, int nb, const int32_t* hyp,
                                const int32_t* hlen, int stride, int max_len, const int64_t* boff, uint8_t* bp,
                                int32_t* edits, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    const bool ok = edit_rung(max_len, [&](auto r) {
        using R = decltype(r);
        if (bp)
            hipLaunchKernelGGL((edit_distance_kernel<R::NS, R::NW, true>), dim3((unsigned)nb), dim3(64 * R::NW), 0, s, m, b0,
                               line_of, hyp, hlen, stride, boff, bp, edits);
        else
            hipLaunchKernelGGL((edit_distance_kernel<R::NS, R::NW, false>), dim3((unsigned)nb), dim3(64 * R::NW), 0, s, m,
                               b0, line_of, hyp, hlen, stride, nullptr, nullptr, edits);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_edit_backtrace(const EditLines& m, int b0, const int32_t* line_of, int nb, const int32_t* hyp,
                                 const int32_t* hlen, int stride, int max_len, const int64_t* boff, const uint8_t* bp,
                                 int32_t* counts, int32_t* ref_map, int32_t* hyp_map, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    const int ns = edit_lane_rows(max_len);
    if (!ns) return hipErrorInvalidValue;
    hipLaunchKernelGGL(edit_backtrace_kernel, dim3((unsigned)nb), dim3(256), 0, s, m, b0, line_of, hyp, hlen, stride,
                       ns == 1 ? 0 : ns == 2 ? 1 : 2, boff, bp, counts, ref_map, hyp_map);
    return hipGetLastError();
}


// -------------------------------------------------------------------------------------------
// Prefix beam search without a language model (hctr_nbest*): the search of utils/ctc_codec.py:212-285 with a zero LM,
// as csrc/beam_search.cpp's beam_step restates it, on the front end's per-row lists (k classes, descending float32
// log-probs) where they lie on the device. One workgroup per line, sequential over the line's steps; all state in LDS.
//
// A step turns the ordered list of n <= beam hypotheses (pb, pnb, length, last label, fingerprint) into at most
// n * (k + 1) entries, one SLOT each: slot i < n is hypothesis i's own prefix, slot n + i * k + j its extension by the
// row's class j (the own entries, which carry the two-term merges, share one round of the threads). An extension can only coincide with a prefix already in the list (two extensions of different
// prefixes of equal length differ in their parents), so entries are merged by looking the extension up among the n
// hypotheses: the extension's slot goes unused and the prefix's own slot takes its mass and the smaller first-touch key.
// Hence pb' has at most one contribution and pnb' at most two, and logaddexp of two terms is symmetric: no atomics and
// no ordering question. The first-touch key of a slot is (i * k + j) * 2 + {0 own, 1 extension} of the first pair that
// touched it (the own entry of hypothesis i is first touched by the row's first usable class j0). Keys are unique, so
// (total descending, key ascending) is a total order - Python's stable sort over dict insertion order - and a slot's
// place in the next list is the number of slots that beat it (rank by counting, all-pairs on LDS broadcasts). Totals
// are compared as order-preserving integers, NaN last, so the ranks are a permutation whatever the inputs hold.
//
// Identity: a hypothesis carries (length, 64-bit fingerprint of its labels, fingerprint of its parent prefix); the
// fingerprint of prefix + c is beam_mix(fingerprint(prefix), c), a bijection of its first argument. Hypothesis m IS the
// extension of hypothesis p by c iff len_m = len_p + 1, last_m = c and parent_m = fingerprint_p; a false match needs
// two different label strings of equal length in one list with equal fingerprints (DESIGN.md 4f has the bound).
//
// History: per step and kept place one {parent place, appended label or -1}, hist[(b*W + t) * beam + place];
// prefix_backtrace_kernel walks it, one lane per returned hypothesis. Two barriers per step (entries -> ranks -> next
// list); the next row's k classes are loaded before the step's arithmetic and stored to LDS behind it.
// Float64 throughout; logaddexp is numpy's formula (npy_logaddexp), as in beam_search.cpp.
// -------------------------------------------------------------------------------------------

// The instances (beam, k, wave64s per line); a call launches the first that holds its beam and k. The arithmetic does
// not depend on the rung: it sizes the LDS arrays and the threads over which the slots are spread.
#define HCTR_BEAM_LADDER(X) X(10, 10, 1) X(16, 16, 4) X(32, 32, 4)

// numpy's formula - x + log1p(exp(y - x)) for x > y, y + log1p(exp(x - y)) otherwise - without its branches, which
// lanes of one wave would take both ways: the larger argument plus log1p(exp(-|x - y|)), the same operands bit for bit
__device__ __forceinline__ double beam_logaddexp(double x, double y) {
    if (x == y) return x + 0.693147180559945309417232121458176568;      // (also -inf, -inf: no inf - inf)
    return fmax(x, y) + log1p(exp(-fabs(x - y)));  // NaN in, NaN out (fmax drops one NaN, exp(NaN) brings it back)
}

// total() of the reference with a zero LM: log-prob + len * len_bonus, the product rounded on its own as Python does
__device__ __forceinline__ double beam_total(double logp, int len, double len_bonus) {
#pragma clang fp contract(off)
    const double pt = (double)len * len_bonus;
    return logp + pt;
}

// order-preserving integer image of a total: larger double <-> larger integer, -0 = +0, NaN below -inf; never 0
__device__ __forceinline__ unsigned long long beam_ord(double t) {
    if (t != t) return 1ull;
    if (t == 0.0) t = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(t);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ unsigned long long beam_mix(unsigned long long h, int c) {
    unsigned long long z = h + (unsigned long long)(unsigned)(c + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// total() with the n-gram model: pt = s * lm_panelty + len * len_bonus, each product rounded on its own, then log-prob + pt
__device__ __forceinline__ double beam_total_lm(double logp, double s, int len, double lm_panelty, double len_bonus) {
#pragma clang fp contract(off)
    const double pt = s * lm_panelty + (double)len * len_bonus;
    return logp + pt;
}

// what the ranking reads of a slot, one 16-byte LDS load: the total's integer image and the first-touch key
struct alignas(16) BeamSortKey {
    unsigned long long ord;
    unsigned key, pad;
};

// LM = true is the search of hctr_nbest_lm* (DESIGN.md 4g): the same steps, slots, merges, keys and ranks; besides, a
// hypothesis carries the n-gram score of its prefix (float64, summed left to right) and its last word ids in the fixed
// form of lm_word_logp, an extension adds one term to its parent's, and every valid entry is ranked by its log-prob +
// (score of prefix + the step's suffix) * lm_panelty + len * len_bonus. Tl holds the end steps of the pre-pass, 0 for a
// line without a greedy text, which returns nothing. With LM = false none of it is compiled.
// GRID (with LM) is the search of hctr_lm_sweep* (DESIGN.md 4i): workgroup ob = g * nb + b searches line b under the
// weights lm.grid[g] = {lm_panelty, len_bonus}. The lists, word ids, suffixes and end steps are line b's, shared by the
// pairs; history and outputs are grid line ob's. Nothing else differs, so pair g computes what the single-pair
// instance computes with its two weights.
template <int BEAM, int K, int NW, bool LM, bool GRID = false>
__global__ __launch_bounds__(64 * NW) void prefix_beam_kernel(const int32_t* __restrict__ idx, const float* __restrict__ lp,
                                                              int nb, int W, int k, int unk, int beam, int nbest,
                                                              double len_bonus, const int32_t* __restrict__ Tl,
                                                              int2* __restrict__ hist, int32_t* __restrict__ o_len,
                                                              double* __restrict__ o_logp, double* __restrict__ o_score,
                                                              int32_t* __restrict__ o_cnt, const BeamLm lm) {
    constexpr int NT = 64 * NW, SLOTS = BEAM * (K + 1);
    constexpr int LB = LM ? BEAM : 1, LS = LM ? SLOTS : 1, LK = LM ? K : 1, NCX = kLmMaxOrder - 1;
    __shared__ double h_lm[2][LB], e_lm[LS];       // n-gram score of a hypothesis' / an entry's prefix
    __shared__ int h_cx[2][LB][NCX], r_w[2][LK];   // its context; the word ids of the row's classes
    constexpr double NINF = -__builtin_huge_val();
    // the list, double-buffered: place r of step t's list is written while step t's slots still read the old one
    __shared__ double h_pb[2][BEAM], h_pnb[2][BEAM], h_tot[2][BEAM];
    __shared__ unsigned long long h_hash[2][BEAM], h_par[2][BEAM];
    __shared__ int h_len[2][BEAM], h_last[2][BEAM];
    __shared__ BeamSortKey e_sort[SLOTS];          // ord 0 = the slot holds no entry
    __shared__ double e_pb[SLOTS], e_pnb[SLOTS], e_tot[SLOTS];
    __shared__ int r_cls[2][K];
    __shared__ double r_lp[2][K];
    __shared__ int r_meta[2][2];                   // {the row's first usable class j0, the place of the blank}, -1 = none
    __shared__ int s_n[2], s_valid[NW];
    static_assert(LM || !GRID, "the grid is a grid of LM weights");
    const int ob = blockIdx.x, b = GRID ? ob % nb : ob, tid = threadIdx.x, k1 = k + 1;
    const int T = Tl[b];
    int2* __restrict__ hb = hist + (int64_t)ob * W * beam;
    double lm_w = lm.lm_panelty, len_w = len_bonus;
    if constexpr (GRID) {
        const double2 w = lm.grid[ob / nb];
        lm_w = w.x; len_w = w.y;
    }

    // a row's classes into LDS (wave 0; every lane of it takes part in the ballots)
    auto put_row = [&](int buf, bool have, int c, float l, int w) {
        const unsigned long long usable = __ballot(have && (unsigned)c < (unsigned)unk);
        const unsigned long long blank = __ballot(have && c == 0);
        if (have) { r_cls[buf][tid] = c; r_lp[buf][tid] = (double)l; }
        if constexpr (LM) {
            if (have) r_w[buf][tid] = w;
        }
        if (tid == 0) {
            r_meta[buf][0] = usable ? __ffsll((long long)usable) - 1 : -1;
            r_meta[buf][1] = blank ? __ffsll((long long)blank) - 1 : -1;
        }
    };
    if (tid < 64) {
        const bool have = T > 0 && tid < k;
        const int64_t a = (int64_t)b * k + tid;
        int w = -1;
        if constexpr (LM) w = have ? lm.wid[a] : -1;
        put_row(0, have, have ? idx[a] : 0, have ? lp[a] : 0.f, w);
    }
    if (tid == 0) {                                // [((), 0, -inf)]
        h_pb[0][0] = 0.0; h_pnb[0][0] = NINF; h_tot[0][0] = 0.0;
        h_hash[0][0] = 0x243F6A8885A308D3ull; h_par[0][0] = 0ull;
        h_len[0][0] = 0; h_last[0][0] = -1;
        s_n[0] = 1;
        if constexpr (LM) {                        // score 0 in the <s> context
            h_lm[0][0] = 0.0;
            for (int q = 0; q < NCX; ++q) h_cx[0][0][q] = q == NCX - 1 ? lm.bos : -1;
        }
    }
    int4 sfx = make_int4(-2, -2, -2, -2);          // the step's suffix as word ids, -2 = no more
    if constexpr (LM) {
        if (T > 0) sfx = lm.suffix[(int64_t)b * W];
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < T; ++t, cur ^= 1) {
        const int nxt = cur ^ 1, n = s_n[cur];
        if (n == 0) break;                         // (block-uniform) every class of some row was <unknown>: nothing is left
        const bool pre = t + 1 < T && tid < k;
        int pc = 0, pw = -1;
        float pl = 0.f;
        if (pre) {
            const int64_t a = ((int64_t)(t + 1) * nb + b) * k + tid;
            pc = idx[a];
            pl = lp[a];
            if constexpr (LM) pw = lm.wid[a];
        }
        int4 sfx_next = sfx;
        if constexpr (LM) {
            if (t + 1 < T) sfx_next = lm.suffix[(int64_t)b * W + t + 1];
        }
        const int j0 = r_meta[cur][0], jb = r_meta[cur][1], E = n * k1;
        // entries
        int nvalid = 0;                            // valid entries of this wave's slots (wave-uniform)
        for (int e0 = 0; e0 < E; e0 += NT) {       // (block-uniform trips: the ballot below counts whole waves)
            const int e = e0 + tid;
            const bool in = e < E;
            // (a lane past the last slot idles through the cheap side, the extension of hypothesis 0 by class 0)
            const int i = !in ? 0 : e < n ? e : (e - n) / k, jj = !in ? 1 : e < n ? 0 : e - n - i * k + 1;
            const int leni = h_len[cur][i], lasti = h_last[cur][i];
            bool valid;
            unsigned key;
            double pb = NINF, pnb = NINF, tot;
            if (jj == 0) {                         // the prefix's own entry
                valid = j0 >= 0;
                key = (unsigned)(i * k + max(j0, 0)) * 2u;
                if (jb >= 0) pb = h_tot[cur][i] + r_lp[cur][jb];
                int jt = -1;
#pragma unroll 4
                for (int j = 0; j < k; ++j)        // (independent LDS loads: unrolled, they overlap)
                    if (r_cls[cur][j] == lasti) jt = j;
                if (jt >= 0 && lasti > 0 && lasti < unk) {
                    const double l = r_lp[cur][jt];
                    const unsigned long long want = h_par[cur][i];
                    int p = -1;                    // the hypothesis whose extension by the last label this prefix is
#pragma unroll 4
                    for (int q = 0; q < n; ++q)
                        if (h_len[cur][q] == leni - 1 && h_hash[cur][q] == want) p = q;
                    double ext = NINF;
                    if (p >= 0) {
                        ext = (h_last[cur][p] != lasti ? h_tot[cur][p] : h_pb[cur][p]) + l;
                        key = min(key, (unsigned)(p * k + jt) * 2u + 1u);
                    }
                    pnb = beam_logaddexp(h_pnb[cur][i] + l, ext);
                }
                tot = beam_logaddexp(pb, pnb);
            } else {                               // the extension by class j
                const int j = jj - 1, c = r_cls[cur][j];
                valid = c > 0 && c < unk;
                key = (unsigned)(i * k + j) * 2u + 1u;
                if (valid) {
                    const unsigned long long mine = h_hash[cur][i];
#pragma unroll 4
                    for (int m = 0; m < n; ++m)    // already in the list: its own slot takes this mass
                        if (h_len[cur][m] == leni + 1 && h_last[cur][m] == c && h_par[cur][m] == mine) valid = false;
                }
                pnb = (c != lasti ? h_tot[cur][i] : h_pb[cur][i]) + r_lp[cur][j];
                tot = pnb;                         // logaddexp(-inf, x) = x
            }
            valid = valid && in;
            nvalid += __popcll(__ballot(valid));
            double total = 0.0;
            if constexpr (LM) {
                if (valid) {
                    int cx[NCX];
#pragma unroll
                    for (int q = 0; q < NCX; ++q) cx[q] = h_cx[cur][i][q];
                    double sc = h_lm[cur][i];
                    if (jj) {
                        const int w = r_w[cur][jj - 1];
                        sc += lm_word_logp(lm.table, cx, w);
                        lm_roll(cx, w);
                    }
                    e_lm[e] = sc;
                    int4 rest = sfx;
#pragma unroll 1
                    for (int q = 0; q < 4 && rest.x != -2; ++q) {
                        sc += lm_word_logp(lm.table, cx, rest.x);
                        lm_roll(cx, rest.x);
                        rest = make_int4(rest.y, rest.z, rest.w, -2);
                    }
                    total = beam_total_lm(tot, sc, leni + (jj ? 1 : 0), lm_w, len_w);
                }
            } else {
                total = beam_total(tot, leni + (jj ? 1 : 0), len_bonus);
            }
            if (in) {
                e_sort[e] = BeamSortKey{valid ? beam_ord(total) : 0ull, key, 0u};
                e_pb[e] = pb; e_pnb[e] = pnb; e_tot[e] = tot;
            }
        }
        if ((tid & 63) == 0) s_valid[tid >> 6] = nvalid;
        __syncthreads();
        // ranks; the first `beam` become the next list
        for (int e = tid; e < E; e += NT) {
            const unsigned long long ord = e_sort[e].ord;
            const unsigned key = e_sort[e].key;
            int rank = 0;
#pragma unroll 8
            for (int f = 0; f < E; ++f) {          // (broadcast loads, eight in flight)
                const BeamSortKey o = e_sort[f];
                rank += (o.ord > ord) || (o.ord == ord && o.key < key);
            }
            if (e == 0) {
                int cnt = 0;
                for (int w = 0; w < NW; ++w) cnt += s_valid[w];
                s_n[nxt] = min(cnt, beam);
            }
            if (ord != 0ull && rank < beam) {
                const int i = e < n ? e : (e - n) / k, jj = e < n ? 0 : e - n - i * k + 1;
                const int c = jj ? r_cls[cur][jj - 1] : -1;
                const unsigned long long hi = h_hash[cur][i];
                h_pb[nxt][rank] = e_pb[e]; h_pnb[nxt][rank] = e_pnb[e]; h_tot[nxt][rank] = e_tot[e];
                h_len[nxt][rank] = h_len[cur][i] + (jj ? 1 : 0);
                h_last[nxt][rank] = jj ? c : h_last[cur][i];
                h_hash[nxt][rank] = jj ? beam_mix(hi, c) : hi;
                h_par[nxt][rank] = jj ? hi : h_par[cur][i];
                if constexpr (LM) {
                    h_lm[nxt][rank] = e_lm[e];
                    const int w = jj ? r_w[cur][jj - 1] : -1;
#pragma unroll
                    for (int q = 0; q < NCX; ++q)
                        h_cx[nxt][rank][q] = !jj ? h_cx[cur][i][q] : q + 1 < NCX ? h_cx[cur][i][q + 1] : w;
                }
                hb[(int64_t)t * beam + rank] = make_int2(i, c);
            }
        }
        if (tid < 64) put_row(nxt, pre, pc, pl, pw);
        sfx = sfx_next;
        __syncthreads();
    }
    const int n = LM && T == 0 ? 0 : s_n[cur];
    if (tid < nbest) {
        const bool have = tid < n;
        const int len = have ? h_len[cur][tid] : 0;
        const double logp = have ? h_tot[cur][tid] : NINF;
        const int64_t o = (int64_t)ob * nbest + tid;
        o_len[o] = len;
        o_logp[o] = logp;
        if constexpr (LM) {
            const double sc = have ? h_lm[cur][tid] : NINF;
            o_score[o] = have ? beam_total_lm(logp, sc, len, lm_w, len_w) : NINF;
            lm.o_lm[o] = sc;
        } else {
            o_score[o] = have ? beam_total(logp, len, len_bonus) : NINF;
        }
    }
    if (tid == 0) o_cnt[ob] = min(n, nbest);
}

// labels of the returned hypotheses, one lane each: from the last step back, place to parent place, the appended labels
// filling the text from its end. The labels array is zero on entry. Places and positions are clamped, so a history
// left unspecified by a NaN row is walked without leaving the line's arrays. With wrap > 0 the steps of line b are
// Tl[b mod wrap]: the grid lines of hctr_lm_sweep*, which share the end steps of their lines.
__global__ __launch_bounds__(64) void prefix_backtrace_kernel(const int2* __restrict__ hist, const int32_t* __restrict__ Tl,
                                                              int wrap, int W, int beam, int nbest,
                                                              const int32_t* __restrict__ o_len,
                                                              const int32_t* __restrict__ o_cnt,
                                                              int32_t* __restrict__ labels) {
    const int b = blockIdx.x, s = threadIdx.x;
    if (s >= min(o_cnt[b], nbest)) return;
    const int2* __restrict__ hb = hist + (int64_t)b * W * beam;
    int32_t* __restrict__ out = labels + ((int64_t)b * nbest + s) * W;
    int pos = min(max(o_len[(int64_t)b * nbest + s], 0), W), place = s;
    for (int t = min(Tl[wrap > 0 ? b % wrap : b], W) - 1; t >= 0 && pos > 0; --t) {
        const int2 h = hb[(int64_t)t * beam + place];
        if (h.y >= 0) out[--pos] = h.y;
        place = (int)min((unsigned)h.x, (unsigned)(beam - 1));
    }
}

// Pre-pass of the LM-scored search, one workgroup per line over its first L = Tl[b] columns: the LM word id of every
// class of the line's lists (wid, laid out as idx); the greedy line of utils/ctc_codec.py:188-195 - the top-1 class of
// column t is kept when it is not blank, not <unknown> and not the top-1 class of column t - 1 - and from it, per step
// t, the first <= 4 kept entries with a stamp > t as word ids (suffix[b * W + t], -2 = no more) and the end step
// min(last stamp + 4, L), 0 when nothing was kept. The suffixes come from one backward walk (thread 0, a window of four)
// through 256-column chunks staged in LDS; everything else is spread over the threads.
__global__ __launch_bounds__(256) void beam_lm_prepass_kernel(const int32_t* __restrict__ idx, int nb, int W, int k, int C,
                                                              const int32_t* __restrict__ Tl,
                                                              const int32_t* __restrict__ words, int32_t* __restrict__ wid,
                                                              int4* __restrict__ suffix, int32_t* __restrict__ end) {
    __shared__ int s_w[256];                       // word id of the chunk's kept entries, -2 = column not kept
    __shared__ int4 s_suf[256];
    const int b = blockIdx.x, tid = threadIdx.x, unk = C - 1;
    const int L = min(max(Tl[b], 0), W);
    for (int e = tid; wid && e < L * k; e += 256) {
        const int t = e / k, j = e - t * k;
        const int64_t a = ((int64_t)t * nb + b) * k + j;
        const int c = idx[a];
        wid[a] = (unsigned)c < (unsigned)C ? words[c] : -1;
    }
    int4 win = make_int4(-2, -2, -2, -2);
    int last = -1;
    for (int base = L > 0 ? ((L - 1) / 256) * 256 : -1; base >= 0; base -= 256) {
        const int t = base + tid;
        int w = -2;
        if (t < L) {
            const int c = idx[((int64_t)t * nb + b) * k];
            const int prev = t > 0 ? idx[((int64_t)(t - 1) * nb + b) * k] : -1;
            if (c != 0 && c != unk && c != prev) w = words && (unsigned)c < (unsigned)C ? words[c] : -1;
        }
        s_w[tid] = w;
        __syncthreads();
        if (tid == 0) {
            for (int u = 255; u >= 0; --u) {
                s_suf[u] = win;
                const int wu = s_w[u];
                if (wu != -2) {
                    if (last < 0) last = base + u;
                    win = make_int4(wu, win.x, win.y, win.z);
                }
            }
        }
        __syncthreads();
        if (t < L) suffix[(int64_t)b * W + t] = s_suf[tid];
    }
    if (tid == 0) end[b] = last < 0 ? 0 : min(last + 4, L);
}

template <int BEAM_, int K_, int NW_>
struct BeamRung {
    static constexpr int BEAM = BEAM_, K = K_, NW = NW_;
};
#define BEAM_RUNG_MAX(BEAM, K, NW) , BEAM
constexpr int kBeamLadderMax = std::max({0 HCTR_BEAM_LADDER(BEAM_RUNG_MAX)});
#undef BEAM_RUNG_MAX
static_assert(kBeamLadderMax == kBeamMaxK, "the last rung holds the documented limits of hctr_nbest*");

hipError_t launch_prefix_beam(const int32_t* idx, const float* lp, int nb, int W, int k, int C, int beam, int nbest,
                              double len_bonus, const int32_t* T, int2* hist, int32_t* len, double* logp, double* score,
                              int32_t* cnt, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    if (k < 1 || beam < 1 || nbest < 1 || nbest > beam || C < 2 || W < 1) return hipErrorInvalidValue;
#define BEAM_RUNG(BEAM, K, NW)                                                                                       \
    if (beam <= BEAM && k <= K) {                                                                                    \
        hipLaunchKernelGGL((prefix_beam_kernel<BEAM, K, NW, false>), dim3((unsigned)nb), dim3(64 * NW), 0, s, idx, lp, nb, \
                           W, k, C - 1, beam, nbest, len_bonus, T, hist, len, logp, score, cnt, BeamLm{});          \
        return hipGetLastError();                                                                                    \
    }
    HCTR_BEAM_LADDER(BEAM_RUNG)
#undef BEAM_RUNG
    return hipErrorInvalidValue;
}

hipError_t launch_beam_lm_prepass(const int32_t* idx, int nb, int W, int k, int C, const int32_t* T, const int32_t* words,
                                  int32_t* wid, int4* suffix, int32_t* end, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    if (k < 1 || C < 2 || W < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_lm_prepass_kernel, dim3((unsigned)nb), dim3(256), 0, s, idx, nb, W, k, C, T, words, wid, suffix,
                       end);
    return hipGetLastError();
}

hipError_t launch_prefix_beam_lm(const int32_t* idx, const float* lp, int nb, int W, int k, int C, int beam, int nbest,
                                 double len_bonus, const int32_t* end, const BeamLm& lm, int2* hist, int32_t* len,
                                 double* logp, double* score, int32_t* cnt, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    if (k < 1 || beam < 1 || nbest < 1 || nbest > beam || C < 2 || W < 1) return hipErrorInvalidValue;
    if (!lm.table.slots || lm.table.order < 1 || lm.table.order > kLmMaxOrder || !lm.wid || !lm.suffix || !lm.o_lm)
        return hipErrorInvalidValue;
#define BEAM_RUNG(BEAM, K, NW)                                                                                       \
    if (beam <= BEAM && k <= K) {                                                                                    \
        hipLaunchKernelGGL((prefix_beam_kernel<BEAM, K, NW, true>), dim3((unsigned)nb), dim3(64 * NW), 0, s, idx, lp, nb,  \
                           W, k, C - 1, beam, nbest, len_bonus, end, hist, len, logp, score, cnt, lm);               \
        return hipGetLastError();                                                                                    \
    }
    HCTR_BEAM_LADDER(BEAM_RUNG)
#undef BEAM_RUNG
    return hipErrorInvalidValue;
}

hipError_t launch_prefix_beam_lm_grid(const int32_t* idx, const float* lp, int nb, int W, int k, int C, int beam, int G,
                                      const int32_t* end, const BeamLm& lm, int2* hist, int32_t* len, double* logp,
                                      double* score, int32_t* cnt, hipStream_t s) {
    if (nb <= 0 || G <= 0) return hipSuccess;
    if (k < 1 || beam < 1 || C < 2 || W < 1 || (int64_t)G * nb > INT32_MAX) return hipErrorInvalidValue;
    if (!lm.table.slots || lm.table.order < 1 || lm.table.order > kLmMaxOrder || !lm.wid || !lm.suffix || !lm.o_lm ||
        !lm.grid)
        return hipErrorInvalidValue;
#define BEAM_RUNG(BEAM, K, NW)                                                                                       \
    if (beam <= BEAM && k <= K) {                                                                                    \
        hipLaunchKernelGGL((prefix_beam_kernel<BEAM, K, NW, true, true>), dim3((unsigned)(G * nb)), dim3(64 * NW), 0, s, \
                           idx, lp, nb, W, k, C - 1, beam, 1, 0.0, end, hist, len, logp, score, cnt, lm);            \
        return hipGetLastError();                                                                                    \
    }
    HCTR_BEAM_LADDER(BEAM_RUNG)
#undef BEAM_RUNG
    return hipErrorInvalidValue;
}

hipError_t launch_prefix_backtrace(const int2* hist, const int32_t* T, int nb, int W, int beam, int nbest,
                                   const int32_t* len, const int32_t* cnt, int32_t* labels, hipStream_t s, int wrap) {
    if (nb <= 0) return hipSuccess;
    if (beam < 1 || nbest < 1 || nbest > 64 || wrap < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prefix_backtrace_kernel, dim3((unsigned)nb), dim3(64), 0, s, hist, T, wrap, W, beam, nbest, len, cnt,
                       labels);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// The skip search (hctr_nbest_skip*): __cbs_skip__ of utils/ctc_codec.py:124-181 on the front end's
// thresholded candidate lists in the padded layout - row r = t*nb + b holds cnt[r] classes in ascending order at
// ci / cl[r * kBeamMaxK ..], its blank log-prob at bl[r]. A sibling of prefix_beam_kernel: the same list, slots, merges,
// keys, ranks and history; one workgroup per line over the end[b] steps of the pre-pass.
//
// A step whose row has ONE candidate updates every hypothesis in place. A run of such steps is wave 0's alone, one lane
// per hypothesis with its state in registers: lane j of the wave fetches step t + j's (count, class, log-prob, blank
// log-prob, word id), a ballot finds where the run ends, and the steps are taken from the lanes by broadcast - one
// round of memory latency per 64 steps, no LDS traffic and no barrier inside the run; the other waves wait at the one
// barrier behind it. A step costs at most one logaddexp and, when it appends, one lm_word_logp. Its history record is
// {same place, appended label or -1}, so prefix_backtrace_kernel walks it like any other.
//
// A step with m != 1 candidates is prefix_beam_kernel's step with k := m (the candidates in class order, so are the
// first-touch keys), behind one more phase of wave 0: the row goes to LDS and, when an in-place step has appended a
// label since the last ranked step, the list is FOLDED - hypotheses of equal (length, fingerprint) become the first of
// them with pb = logaddexp over their pb in list order and pnb likewise, the rest close up (an in-place step never
// merges, so "a" with pb finite and "aa" become "aa", "aa"; the reference's dict sums them in this step, since equal
// texts see the same candidates and spread the same terms). h_src keeps each survivor's place before the fold for the
// step's history record. After the fold the texts are distinct and the one-lookup merges hold again.
//
// A line with a row of more than kBeamMaxK candidates inside its end step is not searched (status 3); m = 0 empties
// the list (status 2); the result is the first nbest of the final list as it stands - after a trailing run of in-place
// steps unsorted and possibly with a text twice. LM = false is the zero LM: no table, no word ids, lm_score 0.
// -------------------------------------------------------------------------------------------
template <int BEAM, int NW, bool LM>
__global__ __launch_bounds__(64 * NW) void prefix_beam_skip_kernel(
    const int32_t* __restrict__ cnt, const int32_t* __restrict__ ci, const float* __restrict__ cl,
    const float* __restrict__ bl, int nb, int W, int unk, int beam, int nbest, double len_bonus,
    const int32_t* __restrict__ Tl, const int32_t* __restrict__ words, int2* __restrict__ hist,
    int32_t* __restrict__ o_len, double* __restrict__ o_logp, double* __restrict__ o_score, int32_t* __restrict__ o_cnt,
    int32_t* __restrict__ o_status, int32_t* __restrict__ o_ranked, const BeamLm lm) {
    constexpr int K = kBeamMaxK, NT = 64 * NW, SLOTS = BEAM * (K + 1);
    constexpr int LB = LM ? BEAM : 1, LS = LM ? SLOTS : 1, LK = LM ? K : 1, NCX = kLmMaxOrder - 1;
    constexpr double NINF = -__builtin_huge_val();
    __shared__ double h_lm[2][LB], e_lm[LS];
    __shared__ int h_cx[2][LB][NCX], r_w[LK];
    __shared__ double h_pb[2][BEAM], h_pnb[2][BEAM], h_tot[2][BEAM];
    __shared__ unsigned long long h_hash[2][BEAM], h_par[2][BEAM];
    __shared__ int h_len[2][BEAM], h_last[2][BEAM], h_src[BEAM];
    __shared__ BeamSortKey e_sort[SLOTS];          // ord 0 = the slot holds no entry
    __shared__ double e_pb[SLOTS], e_pnb[SLOTS], e_tot[SLOTS];
    __shared__ int r_cls[K];
    __shared__ double r_lp[K];
    __shared__ int r_meta[2];                      // {the row's first usable class j0, the place of the blank}, -1 = none
    __shared__ int s_n[2], s_valid[NW], s_scan[NW][2], s_run[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = min(max(Tl[b], 0), W);
    int2* __restrict__ hb = hist + (int64_t)b * W * beam;

    // the line's rows once: how many of its steps are ranked ones, and whether one of them is beyond the cap
    int ranked = 0, big = 0;
    for (int t = tid; t < T; t += NT) {
        const int m = cnt[(int64_t)t * nb + b];
        ranked += m != 1;
        big |= m > K;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ranked += __shfl_xor(ranked, off);
        big |= __shfl_xor(big, off);
    }
    if ((tid & 63) == 0) { s_scan[tid >> 6][0] = ranked; s_scan[tid >> 6][1] = big; }
    if (tid == 0) {                                // [((), 0, -inf)]
        h_pb[0][0] = 0.0; h_pnb[0][0] = NINF; h_tot[0][0] = 0.0;
        h_hash[0][0] = 0x243F6A8885A308D3ull; h_par[0][0] = 0ull;
        h_len[0][0] = 0; h_last[0][0] = -1;
        s_n[0] = 1;
        if constexpr (LM) {                        // score 0 in the <s> context
            h_lm[0][0] = 0.0;
            for (int q = 0; q < NCX; ++q) h_cx[0][0][q] = q == NCX - 1 ? lm.bos : -1;
        }
    }
    __syncthreads();
    ranked = 0; big = 0;
    for (int w = 0; w < NW; ++w) { ranked += s_scan[w][0]; big |= s_scan[w][1]; }
    int status = T == 0 ? 1 : big ? 3 : 0;
    const int Te = status ? 0 : T;                 // (block-uniform)

    int cur = 0, t = 0;
    bool dirty = false;                            // an in-place step has appended a label since the last ranked step
    while (t < Te) {
        const int nxt = cur ^ 1;
        int n = s_n[cur];
        if (n == 0) break;                         // (block-uniform) a row without a usable candidate: nothing is left
        const int m = cnt[(int64_t)t * nb + b];
        if (m == 1) {
            // ---- a run of in-place steps: wave 0, hypothesis tid in registers ----
            if (tid < 64) {
                const bool live = tid < n;
                const int hi = live ? tid : 0;     // (a lane past the list idles through hypothesis 0's arithmetic)
                double pb = h_pb[cur][hi], pnb = h_pnb[cur][hi], tot = h_tot[cur][hi];
                unsigned long long hash = h_hash[cur][hi], par = h_par[cur][hi];
                int len = h_len[cur][hi], last = h_last[cur][hi];
                double sc = 0.0;
                int cx[NCX];
                if constexpr (LM) {
                    sc = h_lm[cur][hi];
#pragma unroll
                    for (int q = 0; q < NCX; ++q) cx[q] = h_cx[cur][hi][q];
                }
                bool app = false;
                int t2 = t;
                for (bool more = true; more;) {
                    const int tj = t2 + tid;
                    const bool in = tj < Te;
                    const int64_t r = (int64_t)(in ? tj : t2) * nb + b;
                    const int mj = in ? cnt[r] : 0;
                    const int cj = ci[r * K];
                    const float lj = cl[r * K], l0j = bl[r];
                    int wj = -1;
                    if constexpr (LM) wj = mj == 1 && (unsigned)cj <= (unsigned)unk ? words[cj] : -1;
                    const unsigned long long stop = __ballot(mj != 1);
                    const int run = stop ? __ffsll((long long)stop) - 1 : 64;
                    for (int j = 0; j < run; ++j) {
                        const int c = __shfl(cj, j);
                        const double l = (double)__shfl(lj, j), l0 = (double)__shfl(l0j, j);
                        const int w = __shfl(wj, j);
                        int label = -1;
                        if (c == 0) {
                            pb = tot + l;
                            tot = beam_logaddexp(pb, pnb);
                        } else if (c > 0 && c < unk) {
                            const bool rep = c == last;
                            if (rep && pb == NINF) {       // the repeat read as the same character: pb first, from the old pnb
                                pb = tot + l0;
                                pnb = pnb + l;
                                tot = beam_logaddexp(pb, pnb);
                            } else {
                                pnb = (rep ? pb : tot) + l;
                                pb = NINF;
                                tot = pnb;
                                label = c;
                                par = hash;
                                hash = beam_mix(hash, c);
                                ++len;
                                last = c;
                                if constexpr (LM) {
                                    sc += lm_word_logp(lm.table, cx, w);
                                    lm_roll(cx, w);
                                }
                            }
                        }
                        app = app || label >= 0;
                        if (live) hb[(int64_t)(t2 + j) * beam + tid] = make_int2(tid, label);
                    }
                    t2 += run;
                    more = run == 64 && t2 < Te;
                }
                if (live) {
                    h_pb[cur][tid] = pb; h_pnb[cur][tid] = pnb; h_tot[cur][tid] = tot;
                    h_hash[cur][tid] = hash; h_par[cur][tid] = par;
                    h_len[cur][tid] = len; h_last[cur][tid] = last;
                    if constexpr (LM) {
                        h_lm[cur][tid] = sc;
#pragma unroll
                        for (int q = 0; q < NCX; ++q) h_cx[cur][tid][q] = cx[q];
                    }
                }
                const bool any = __any(app && live);
                if (tid == 0) { s_run[0] = t2; s_run[1] = any; }
            }
            __syncthreads();
            t = s_run[0];
            dirty = dirty || s_run[1] != 0;
            continue;
        }
        // ---- a ranked step. Phase 0 (wave 0): the row into LDS; the fold ----
        const bool fold = dirty;
        if (tid < 64) {
            const bool have = tid < m;
            const int64_t a = ((int64_t)t * nb + b) * K + tid;
            const int c = have ? ci[a] : 0;
            const unsigned long long usable = __ballot(have && (unsigned)c < (unsigned)unk);
            const unsigned long long blank = __ballot(have && c == 0);
            if (have) { r_cls[tid] = c; r_lp[tid] = (double)cl[a]; }
            if constexpr (LM) {
                if (have) r_w[tid] = (unsigned)c <= (unsigned)unk ? words[c] : -1;
            }
            if (tid == 0) {
                r_meta[0] = usable ? __ffsll((long long)usable) - 1 : -1;
                r_meta[1] = blank ? __ffsll((long long)blank) - 1 : -1;
            }
            if (fold) {
                const bool live = tid < n;
                const int i = live ? tid : 0;
                const int leni = h_len[cur][i];
                const unsigned long long hashi = h_hash[cur][i];
                double pb = h_pb[cur][i], pnb = h_pnb[cur][i];
                int first = i;
                for (int q = 0; q < n; ++q) {
                    if (q == i || h_len[cur][q] != leni || h_hash[cur][q] != hashi) continue;
                    if (q < first) first = q;
                    if (q > i) { pb = beam_logaddexp(pb, h_pb[cur][q]); pnb = beam_logaddexp(pnb, h_pnb[cur][q]); }
                }
                const bool keep = live && first == i;
                const unsigned long long km = __ballot(keep);
                if (keep) {
                    const int pos = __popcll(km & ((1ull << tid) - 1ull));
                    h_pb[nxt][pos] = pb; h_pnb[nxt][pos] = pnb; h_tot[nxt][pos] = beam_logaddexp(pb, pnb);
                    h_hash[nxt][pos] = hashi; h_par[nxt][pos] = h_par[cur][i];
                    h_len[nxt][pos] = leni; h_last[nxt][pos] = h_last[cur][i];
                    h_src[pos] = i;
                    if constexpr (LM) {
                        h_lm[nxt][pos] = h_lm[cur][i];
#pragma unroll
                        for (int q = 0; q < NCX; ++q) h_cx[nxt][pos][q] = h_cx[cur][i][q];
                    }
                }
                if (tid == 0) s_n[nxt] = __popcll(km);
            }
        }
        __syncthreads();
        if (fold) {
            cur ^= 1;
            n = s_n[cur];
        }
        const int out = cur ^ 1, k = m, k1 = m + 1;
        int4 sfx = make_int4(-2, -2, -2, -2);      // the step's suffix as word ids, -2 = no more
        if constexpr (LM) sfx = lm.suffix[(int64_t)b * W + t];
        const int j0 = r_meta[0], jb = r_meta[1], E = n * k1;
        // entries (prefix_beam_kernel's, with k = m)
        int nvalid = 0;                            // valid entries of this wave's slots (wave-uniform)
        for (int e0 = 0; e0 < E; e0 += NT) {       // (block-uniform trips: the ballot below counts whole waves)
            const int e = e0 + tid;
            const bool in = e < E;
            const int i = !in ? 0 : e < n ? e : (e - n) / k, jj = !in ? (k ? 1 : 0) : e < n ? 0 : e - n - i * k + 1;
            const int leni = h_len[cur][i], lasti = h_last[cur][i];
            bool valid;
            unsigned key;
            double pb = NINF, pnb = NINF, tot;
            if (jj == 0) {                         // the prefix's own entry
                valid = j0 >= 0;
                key = (unsigned)(i * k + max(j0, 0)) * 2u;
                if (jb >= 0) pb = h_tot[cur][i] + r_lp[jb];
                int jt = -1;
#pragma unroll 4
                for (int j = 0; j < k; ++j)
                    if (r_cls[j] == lasti) jt = j;
                if (jt >= 0 && lasti > 0 && lasti < unk) {
                    const double l = r_lp[jt];
                    const unsigned long long want = h_par[cur][i];
                    int p = -1;                    // the hypothesis whose extension by the last label this prefix is
#pragma unroll 4
                    for (int q = 0; q < n; ++q)
                        if (h_len[cur][q] == leni - 1 && h_hash[cur][q] == want) p = q;
                    double ext = NINF;
                    if (p >= 0) {
                        ext = (h_last[cur][p] != lasti ? h_tot[cur][p] : h_pb[cur][p]) + l;
                        key = min(key, (unsigned)(p * k + jt) * 2u + 1u);
                    }
                    pnb = beam_logaddexp(h_pnb[cur][i] + l, ext);
                }
                tot = beam_logaddexp(pb, pnb);
            } else {                               // the extension by class j
                const int j = jj - 1, c = r_cls[j];
                valid = c > 0 && c < unk;
                key = (unsigned)(i * k + j) * 2u + 1u;
                if (valid) {
                    const unsigned long long mine = h_hash[cur][i];
#pragma unroll 4
                    for (int q = 0; q < n; ++q)    // already in the list: its own slot takes this mass
                        if (h_len[cur][q] == leni + 1 && h_last[cur][q] == c && h_par[cur][q] == mine) valid = false;
                }
                pnb = (c != lasti ? h_tot[cur][i] : h_pb[cur][i]) + r_lp[j];
                tot = pnb;                         // logaddexp(-inf, x) = x
            }
            valid = valid && in;
            nvalid += __popcll(__ballot(valid));
            double total = 0.0;
            if constexpr (LM) {
                if (valid) {
                    int cx[NCX];
#pragma unroll
                    for (int q = 0; q < NCX; ++q) cx[q] = h_cx[cur][i][q];
                    double sc = h_lm[cur][i];
                    if (jj) {
                        const int w = r_w[jj - 1];
                        sc += lm_word_logp(lm.table, cx, w);
                        lm_roll(cx, w);
                    }
                    e_lm[e] = sc;
                    int4 rest = sfx;
#pragma unroll 1
                    for (int q = 0; q < 4 && rest.x != -2; ++q) {
                        sc += lm_word_logp(lm.table, cx, rest.x);
                        lm_roll(cx, rest.x);
                        rest = make_int4(rest.y, rest.z, rest.w, -2);
                    }
                    total = beam_total_lm(tot, sc, leni + (jj ? 1 : 0), lm.lm_panelty, len_bonus);
                }
            } else {
                total = beam_total(tot, leni + (jj ? 1 : 0), len_bonus);
            }
            if (in) {
                e_sort[e] = BeamSortKey{valid ? beam_ord(total) : 0ull, key, 0u};
                e_pb[e] = pb; e_pnb[e] = pnb; e_tot[e] = tot;
            }
        }
        if ((tid & 63) == 0) s_valid[tid >> 6] = nvalid;
        __syncthreads();
        // ranks; the first `beam` become the next list
        for (int e = tid; e < E; e += NT) {
            const unsigned long long ord = e_sort[e].ord;
            const unsigned key = e_sort[e].key;
            int rank = 0;
#pragma unroll 8
            for (int f = 0; f < E; ++f) {          // (broadcast loads, eight in flight)
                const BeamSortKey o = e_sort[f];
                rank += (o.ord > ord) || (o.ord == ord && o.key < key);
            }
            if (e == 0) {
                int c2 = 0;
                for (int w = 0; w < NW; ++w) c2 += s_valid[w];
                s_n[out] = min(c2, beam);
            }
            if (ord != 0ull && rank < beam) {
                const int i = e < n ? e : (e - n) / k, jj = e < n ? 0 : e - n - i * k + 1;
                const int c = jj ? r_cls[jj - 1] : -1;
                const unsigned long long hi = h_hash[cur][i];
                h_pb[out][rank] = e_pb[e]; h_pnb[out][rank] = e_pnb[e]; h_tot[out][rank] = e_tot[e];
                h_len[out][rank] = h_len[cur][i] + (jj ? 1 : 0);
                h_last[out][rank] = jj ? c : h_last[cur][i];
                h_hash[out][rank] = jj ? beam_mix(hi, c) : hi;
                h_par[out][rank] = jj ? hi : h_par[cur][i];
                if constexpr (LM) {
                    h_lm[out][rank] = e_lm[e];
                    const int w = jj ? r_w[jj - 1] : -1;
#pragma unroll
                    for (int q = 0; q < NCX; ++q)
                        h_cx[out][rank][q] = !jj ? h_cx[cur][i][q] : q + 1 < NCX ? h_cx[cur][i][q + 1] : w;
                }
                hb[(int64_t)t * beam + rank] = make_int2(fold ? h_src[i] : i, c);
            }
        }
        __syncthreads();
        cur = out;
        dirty = false;
        ++t;
    }
    const int n = status ? 0 : s_n[cur];
    if (!status && n == 0) status = 2;
    if (tid < nbest) {
        const bool have = tid < n;
        const int len = have ? h_len[cur][tid] : 0;
        const double logp = have ? h_tot[cur][tid] : NINF;
        const int64_t o = (int64_t)b * nbest + tid;
        o_len[o] = len;
        o_logp[o] = logp;
        if constexpr (LM) {
            const double sc = have ? h_lm[cur][tid] : NINF;
            o_score[o] = have ? beam_total_lm(logp, sc, len, lm.lm_panelty, len_bonus) : NINF;
            lm.o_lm[o] = sc;
        } else {
            o_score[o] = have ? beam_total(logp, len, len_bonus) : NINF;
            lm.o_lm[o] = have ? 0.0 : NINF;
        }
    }
    if (tid == 0) {
        o_cnt[b] = min(n, nbest);
        o_status[b] = status;
        o_ranked[b] = ranked;
    }
}

// the instances (beam, wave64s per line), every one with kBeamMaxK candidates per ranked step: 330, 528 and 1056 slots
#define HCTR_SKIP_LADDER(X) X(10, 1) X(16, 4) X(32, 4)

hipError_t launch_prefix_beam_skip(const int32_t* cnt, const int32_t* ci, const float* cl, const float* bl, int nb, int W,
                                   int C, int beam, int nbest, double len_bonus, const int32_t* end, const int32_t* words,
                                   const BeamLm& lm, int2* hist, int32_t* len, double* logp, double* score,
                                   int32_t* o_cnt, int32_t* status, int32_t* ranked, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    if (beam < 1 || nbest < 1 || nbest > beam || C < 2 || W < 1 || !lm.o_lm) return hipErrorInvalidValue;
    const bool use_lm = lm.table.slots != nullptr;
    if (use_lm && (lm.table.order < 1 || lm.table.order > kLmMaxOrder || !lm.suffix || !words)) return hipErrorInvalidValue;
#define SKIP_RUNG(BEAM, NW)                                                                                             \
    if (beam <= BEAM) {                                                                                                 \
        if (use_lm)                                                                                                     \
            hipLaunchKernelGGL((prefix_beam_skip_kernel<BEAM, NW, true>), dim3((unsigned)nb), dim3(64 * NW), 0, s, cnt, ci, \
                               cl, bl, nb, W, C - 1, beam, nbest, len_bonus, end, words, hist, len, logp, score, o_cnt,  \
                               status, ranked, lm);                                                                     \
        else                                                                                                            \
            hipLaunchKernelGGL((prefix_beam_skip_kernel<BEAM, NW, false>), dim3((unsigned)nb), dim3(64 * NW), 0, s, cnt, \
                               ci, cl, bl, nb, W, C - 1, beam, nbest, len_bonus, end, words, hist, len, logp, score,     \
                               o_cnt, status, ranked, lm);                                                              \
        return hipGetLastError();                                                                                       \
    }
    HCTR_SKIP_LADDER(SKIP_RUNG)
#undef SKIP_RUNG
    return hipErrorInvalidValue;
}

// -------------------------------------------------------------------------------------------
// Keyword spotting (hctr_spot*): for a (line, query) pair the probability that the line's text contains the query (the
// forward recursion over the query's KMP automaton lifted to CTC, 2L states) and the best tight segment that reads the
// query (max-plus over its 2L - 1 extended states, each carrying its start column). See SpotArgs in kernels.h and
// DESIGN.md 4j. One wave64 per pair, one lane per state; the four waves of a workgroup take four queries of one line and
// walk its columns in step (they share T), so plain barriers order each wave's LDS rows.
// The containment masses are float64 and linear: the transition matrix is stochastic, the total mass stays 1 and the
// accepting mass only grows, so nothing needs rescaling while log P stays above float64's floor (about -700).
// Every sum has a fixed order that depends on the query alone (its local slots, its edge list), never on where the
// chunk put its classes: a pair's result is the same bits in any chunk and any launch.
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ double spot_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);      // a + b == b + a: every lane ends with the same bits
    return v;
}

// the better of two (score, start) candidates: the strictly greater score, the larger start on equal scores
__device__ __forceinline__ void spot_take(float& m, int& ms, float c, int cs) {
    if (c > m || (c == m && cs > ms)) {
        m = c;
        ms = cs;
    }
}

constexpr int kSpotPF = 4, kSpotWaves = 4;

__global__ __launch_bounds__(64 * kSpotWaves) void spot_kernel(const SpotArgs a) {
    __shared__ double s_st[kSpotWaves][64];              // the states' masses of the previous column
    __shared__ double s_p[kSpotWaves][kSpotSlots + 1];   // the column's probabilities by local slot, rest and 1
    __shared__ float s_lp[kSpotWaves][kSpotSlots + 1];   // and their logs (slots 0..nq)
    __shared__ uint16_t s_edge[kSpotWaves][kSpotMaxEdges];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, gb = a.b0 + b;
    const int T = a.T[gb], D = a.D;
    const int own = (int)blockIdx.x * kSpotWaves + wv;
    const bool valid = own < a.npairs;
    const int pi = valid ? own : (int)blockIdx.x * kSpotWaves;      // a wave without a pair shadows the block's first: it
    const int k = __builtin_amdgcn_readfirstlane(a.pair_q[pi]);     // keeps the barriers' count and writes nothing
    const int32_t* au = a.blob + a.qoff[k];
    const int L = __builtin_amdgcn_readfirstlane(au[0]), nq = __builtin_amdgcn_readfirstlane(au[1]);
    const int maxdeg = __builtin_amdgcn_readfirstlane(au[2]);
    const int ne = min(__builtin_amdgcn_readfirstlane(au[3]), kSpotMaxEdges);
    const int S = 2 * L, SS = 2 * L - 1;
    const int32_t *qslot = au + 4, *ptr = qslot + L, *mlo = ptr + S + 1, *mhi = mlo + S, *ed = mhi + S;
    for (int e = lane; e < ne; e += 64) s_edge[wv][e] = (uint16_t)ed[e];
    const int e0 = lane < S ? ptr[lane] : 0, e1 = lane < S ? ptr[lane + 1] : 0;
    const uint64_t mask = lane < S ? ((uint64_t)(uint32_t)mlo[lane] | ((uint64_t)(uint32_t)mhi[lane] << 32)) : 0;
    const int gs = lane <= nq ? a.gslot[(int64_t)pi * kSpotSlots + lane] : 0;      // the lane's emission column
    // the segment's extended states q_1, blank, q_2, ..., q_L: lane s, characters on the even ones
    const bool seg_on = lane < SS, is_chr = seg_on && !(lane & 1);
    const int myslot = is_chr ? qslot[lane >> 1] : 0;
    const bool skip = is_chr && lane >= 2 && qslot[lane >> 1] != qslot[(lane >> 1) - 1];
    double st = lane == 0 ? 1.0 : 0.0;
    float sc = -INFINITY, best = -INFINITY;
    int sst = -1, bs = -1, be = -1;
    if (lane == nq + 2) s_p[wv][lane] = 1.0;
    const float* base = a.emis + (int64_t)b * a.W * D;
    float e[kSpotPF];
#pragma unroll
    for (int i = 0; i < kSpotPF; ++i) e[i] = T > 0 ? base[(int64_t)min(i, T - 1) * D + gs] : 0.f;
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += kSpotPF) {
#pragma unroll
        for (int i = 0; i < kSpotPF; ++i) {
            const int t = t0 + i;
            if (t < T) {                                   // (block-uniform)
                const float le = e[i];
                const double p = lane <= nq ? exp((double)le) : 0.0;
                const double seen = spot_wave_sum(p);      // p(0) + the query's classes, in local slot order
                if (lane <= nq) {
                    s_p[wv][lane] = p;
                    s_lp[wv][lane] = le;
                }
                if (lane == 0) s_p[wv][nq + 1] = fmax(0.0, 1.0 - seen);
                s_st[wv][lane] = st;
                __syncthreads();
                // Z: what every state sends back to it; the others: their in-edges, in the host's order
                double fall = 0.0;
                for (int j = 0; j <= nq + 1; ++j)
                    if ((mask >> j) & 1) fall += s_p[wv][j];
                const double z = spot_wave_sum(st * fall);
                double acc = 0.0;
                for (int j = 0; j < maxdeg; ++j) {
                    if (e0 + j < e1) {
                        const unsigned w = s_edge[wv][e0 + j];
                        acc += s_st[wv][w & 63] * s_p[wv][w >> 8];
                    }
                }
                st = lane == 0 ? z : acc;
                // the segment: a fresh start (score 0, start t) is offered to the first state at every column
                const float lp = s_lp[wv][myslot];
                float c1 = __shfl_up(sc, 1), c2 = __shfl_up(sc, 2);
                int s1 = __shfl_up(sst, 1), s2 = __shfl_up(sst, 2);
                if (lane == 0) {
                    c1 = 0.f;
                    s1 = t;
                }
                if (!skip) {
                    c2 = -INFINITY;
                    s2 = -1;
                }
                float m = sc;
                int ms = sst;
                spot_take(m, ms, c1, s1);
                spot_take(m, ms, c2, s2);
                sc = seg_on ? m + lp : -INFINITY;
                sst = sc == -INFINITY ? -1 : ms;           // a state nothing has reached has no start
                if (lane == SS - 1 && sc > best) {         // strictly greater: the earliest end wins
                    best = sc;
                    bs = sst;
                    be = t + 1;
                }
                __syncthreads();                           // the rows are rewritten by the next column
                e[i] = base[(int64_t)min(t + kSpotPF, T - 1) * D + gs];      // refill the slot just used
            }
        }
    }
    if (!valid) return;
    const int64_t o = (int64_t)gb * a.Q + k;
    if (lane == S - 1 && a.contain) a.contain[o] = (float)log(st);      // log 0 = -inf: T = 0, or no path holds the query
    if (lane == SS - 1) {
        if (a.seg) a.seg[o] = best;
        if (a.seg_start) a.seg_start[o] = bs;
        if (a.seg_end) a.seg_end[o] = be;
    }
}

hipError_t launch_spot(const SpotArgs& a, hipStream_t s) {
    if (a.nb <= 0 || a.npairs <= 0) return hipSuccess;
    if (a.D < 1 || a.W < 1 || a.Q < 1) return hipErrorInvalidValue;
    for (int l0 = 0; l0 < a.nb; l0 += 65535) {             // (grid.y's limit)
        SpotArgs c = a;
        c.b0 = a.b0 + l0;
        c.nb = std::min(65535, a.nb - l0);
        c.emis = a.emis + (int64_t)l0 * a.W * a.D;
        const dim3 grid((unsigned)((a.npairs + kSpotWaves - 1) / kSpotWaves), (unsigned)c.nb);
        hipLaunchKernelGGL(spot_kernel, grid, dim3(64 * kSpotWaves), 0, s, c);
    }
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// Lexicon recognition (hctr_lexicon*): the exact log p(entry | line) of every entry of a closed list at once, by one CTC
// forward pass over the trie of the lexicon. The forward variable of an extended-target state depends only on the
// labels up to it, so entries that share a prefix share that part of the recursion. Every trie node v has two states,
// n_v (the last column emitted c_v) and b_v (the last column was a blank after the prefix):
//   a'(n_v) = logsum3(a(n_v), a(b_p), [p != root and c_p != c_v] a(n_p)) + lp_t(c_v)
//   a'(b_v) = logsum3(a(b_v), a(n_v), -inf) + lp_t(0)
// which is the loss's recursion with the loss's ctc_logsum3 in the loss's argument order: a score has the bits of -nll
// of ctc_alpha_kernel with the entry as the line's target. Within a step a node needs its own and its parent's previous
// states only, so the step is parallel across the unit's nodes (the loss's recursion leaves the chip almost empty).
// One workgroup per (line, unit of the partition, lex_flat.h); a thread keeps its NPT nodes' states in registers and
// publishes them in LDS for its children, double-buffered: one barrier per step, 16 bytes of LDS per node. The emissions
// of the next PF steps are in flight while a step is computed, as in ctc_forward_line. After step T - 1 every owned
// node writes logadd(b_v, n_v) once per entry that ends on it: no atomics, and copies of ancestors write nothing.
// -------------------------------------------------------------------------------------------
constexpr int kLexPF = 4, kLexThreads = 1024;

template <int NPT>
__global__ __launch_bounds__(kLexThreads) void lexicon_trie_kernel(const LexArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* st = (float2*)smem;                           // [2][nn]: (n_v, b_v) of the previous and the current step
    const int u = a.u0 + (int)blockIdx.x, b = blockIdx.y, gb = a.b0 + b;
    const int T = max(a.T[gb], 1), D = a.D, tid = threadIdx.x, nt = blockDim.x;      // (the host admits T >= 1 only)
    const int n0 = a.uoff[u], nn = min(a.uoff[u + 1] - n0, a.max_unit), c0 = a.coff[u];
    const float* base = a.emis + (int64_t)b * a.W * D;
    int par[NPT], slot[NPT];
    bool skip[NPT], live[NPT];
    float an[NPT], ab[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int v = tid + i * nt;
        live[i] = v < nn;
        const int w = live[i] ? a.node[n0 + v] : 0;
        par[i] = min(w & kLexParMask, nn - 1);
        skip[i] = (w & kLexSkip) != 0;
        slot[i] = live[i] ? a.umap[c0 + a.kidx[n0 + v]] : 0;
        an[i] = (w & kLexFirst) ? base[slot[i]] : -INFINITY;
        ab[i] = v == 0 ? base[0] : -INFINITY;
        if (live[i]) st[v] = make_float2(an[i], ab[i]);
    }
    float e[kLexPF][NPT], eb[kLexPF];
#pragma unroll
    for (int k = 0; k < kLexPF; ++k) {
        const float* r = base + (int64_t)min(1 + k, T - 1) * D;
        ctc_ring_load(r, slot, e[k]);
        eb[k] = r[0];
    }
    __syncthreads();
    for (int t0 = 1; t0 < T; t0 += kLexPF) {
#pragma unroll
        for (int k = 0; k < kLexPF; ++k) {
            const int t = t0 + k;
            if (t < T) {                                   // (block-uniform)
                const float2* prev = st + ((t - 1) & 1) * nn;
                float2* cur = st + (t & 1) * nn;
#pragma unroll
                for (int i = 0; i < NPT; ++i) {
                    if (live[i]) {
                        const int v = tid + i * nt;
                        const float2 p = prev[par[i]];
                        const float n1 = ctc_logsum3(an[i], p.y, skip[i] ? p.x : -INFINITY) + e[k][i];
                        const float b1 = ctc_logsum3(ab[i], an[i], -INFINITY) + eb[k];
                        an[i] = v == 0 ? -INFINITY : n1;   // the root has the blank state only
                        ab[i] = b1;
                        cur[v] = make_float2(an[i], ab[i]);
                    }
                }
                __syncthreads();
            }
            const float* r = base + (int64_t)min(t + kLexPF, T - 1) * D;      // refill the slot just used
            ctc_ring_load(r, slot, e[k]);
            eb[k] = r[0];
        }
    }
    float* out = a.score + (int64_t)gb * a.N;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        if (live[i]) {
            const int v = n0 + tid + i * nt;
            const int e0 = a.eptr[v], e1 = a.eptr[v + 1];
            if (e0 < e1) {
                const float sc = ctc_logadd(ab[i], an[i]);
                for (int j = e0; j < e1; ++j) out[a.elist[j]] = sc;
            }
        }
    }
}

template <int NPT>
static hipError_t launch_lexicon_trie_t(const LexArgs& a, int threads, hipStream_t s) {
    static bool raised[64] = {};
    const int lds = 2 * a.max_unit * (int)sizeof(float2);
    hipError_t e = raise_lds_limit((const void*)lexicon_trie_kernel<NPT>, 2 * kLexMaxUnit * (int)sizeof(float2), raised);
    if (e != hipSuccess) return e;
    for (int l0 = 0; l0 < a.nb; l0 += 65535) {            // (grid.y's limit)
        LexArgs c = a;
        c.b0 = a.b0 + l0;
        c.nb = std::min(65535, a.nb - l0);
        c.emis = a.emis + (int64_t)l0 * a.W * a.D;
        hipLaunchKernelGGL(lexicon_trie_kernel<NPT>, dim3((unsigned)a.nu, (unsigned)c.nb), dim3(threads), lds, s, c);
    }
    return hipGetLastError();
}

hipError_t launch_lexicon_trie(const LexArgs& a, hipStream_t s) {
    if (a.nb <= 0 || a.nu <= 0) return hipSuccess;
    if (a.D < 1 || a.W < 1 || a.N < 1 || a.max_unit < 2 || a.max_unit > kLexMaxUnit) return hipErrorInvalidValue;
    if (a.max_unit <= kLexThreads) return launch_lexicon_trie_t<1>(a, (a.max_unit + 63) / 64 * 64, s);
    if (a.max_unit <= 2 * kLexThreads) return launch_lexicon_trie_t<2>(a, kLexThreads, s);
    return launch_lexicon_trie_t<4>(a, kLexThreads, s);
}

__global__ __launch_bounds__(256) void lexicon_classes_kernel(const int32_t* __restrict__ list, int D, int B,
                                                              int32_t* __restrict__ cls, int32_t* __restrict__ nd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)B * D) cls[i] = list[i % D];
    if (i < B) nd[i] = D;
}

hipError_t launch_lexicon_classes(const int32_t* list, int D, int B, int32_t* cls, int32_t* nd, hipStream_t s) {
    if (B <= 0 || D <= 0) return hipSuccess;
    const int64_t n = (int64_t)B * D;
    hipLaunchKernelGGL(lexicon_classes_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, list, D, B, cls, nd);
    return hipGetLastError();
}

// One workgroup per line. rank[e] = (double)score[e] + (double)prior[e]. log_total = max + log(sum of exp(rank - max)):
// thread i of 256 adds its entries i, i + 256, .. in ascending order, the 256 partial sums are combined by block_sum_d
// (a butterfly within each wave, then (w0 + w1) + (w2 + w3)): the order is a function of N alone. The n best are taken
// one per round: every thread offers the best of its entries that come after the previous winner in the order (rank
// descending, index ascending), and the block takes the best offer. No atomics.
__global__ __launch_bounds__(256) void lexicon_rank_kernel(const float* __restrict__ score, const float* __restrict__ prior,
                                                           int N, int n, int32_t* __restrict__ top_entry,
                                                           float* __restrict__ top_logp, double* __restrict__ top_rank,
                                                           double* __restrict__ log_total, int32_t* __restrict__ count) {
    __shared__ double rd[4];
    __shared__ double wr[4];
    __shared__ int wi[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* sc = score + (int64_t)b * N;
    auto rank = [&](int e) { return (double)sc[e] + (prior ? (double)prior[e] : 0.0); };
    auto better = [](double r, int i, double r2, int i2) { return r > r2 || (r == r2 && i < i2); };
    // every thread ends with the block's best (rank, index) offer
    auto block_best = [&](double r, int i) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double r2 = __shfl_xor(r, off);
            const int i2 = __shfl_xor(i, off);
            if (better(r2, i2, r, i)) {
                r = r2;
                i = i2;
            }
        }
        __syncthreads();
        if (lane == 0) {
            wr[wv] = r;
            wi[wv] = i;
        }
        __syncthreads();
        r = wr[0];
        i = wi[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (better(wr[w], wi[w], r, i)) {
                r = wr[w];
                i = wi[w];
            }
        return make_double2(r, (double)i);
    };
    double mx = -INFINITY;
    for (int e = tid; e < N; e += 256) mx = fmax(mx, rank(e));
    mx = block_best(mx, INT_MAX).x;
    double sum = 0.0;
    if (mx != -INFINITY)
        for (int e = tid; e < N; e += 256) sum += exp(rank(e) - mx);
    sum = block_sum_d(sum, rd);
    if (tid == 0) log_total[b] = mx == -INFINITY ? -INFINITY : mx + log(sum);
    double pr = INFINITY;
    int pi = -1, got = 0;
    for (int k = 0; k < n; ++k) {
        double br = -INFINITY;
        int bi = INT_MAX;
        for (int e = tid; e < N; e += 256) {
            const double r = rank(e);
            if (r != -INFINITY && (r < pr || (r == pr && e > pi)) && better(r, e, br, bi)) {
                br = r;
                bi = e;
            }
        }
        const double2 w = block_best(br, bi);
        pr = w.x;
        pi = (int)w.y;
        const bool have = pi != INT_MAX;
        if (tid == 0) {
            top_entry[(int64_t)b * n + k] = have ? pi : -1;
            top_logp[(int64_t)b * n + k] = have ? sc[pi] : -INFINITY;
            top_rank[(int64_t)b * n + k] = have ? pr : -INFINITY;
        }
        if (!have) {                                       // (block-uniform) nothing is left: the later places are empty too
            pr = -INFINITY;
            pi = INT_MAX;
        } else {
            ++got;
        }
    }
    if (tid == 0) count[b] = got;
}

hipError_t launch_lexicon_rank(const float* score, const float* prior, int B, int N, int n, int32_t* top_entry,
                               float* top_logp, double* top_rank, double* log_total, int32_t* count, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (N < 1 || n < 1 || n > kLexMaxTop) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lexicon_rank_kernel, dim3((unsigned)B), dim3(256), 0, s, score, prior, N, n, top_entry, top_logp,
                       top_rank, log_total, count);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// Pattern-constrained recognition (hctr_pattern*): the probability that a line's text matches a pattern, and the best
// reading that does, by the CTC forward (sum) and Viterbi (max) recursions over the CTC lift of a deterministic finite
// automaton (pat_flat.h). The automaton is deterministic, so every CTC path has one state sequence and both are exact.
//   a_t(s) = logsum over the in-edges of a_{t-1}(src) + lp_t(label(s))
//   v_t(s) = max    over the in-edges of v_{t-1}(src) + lp_t(label(s)), backpointer = the first maximal source
// The n-ary log-sum: m = the float32 maximum of the sources; sum = the float64 sum, in edge order, of
// (double)__expf(a(src) - m); the result is m + __logf((float)sum) in float32, -inf when m is. A state fed by one live
// source keeps its value exactly (sum = 1).
// One workgroup per line; thread i owns the states i, i + nt, .. (NPT of them). The step's states are published in LDS,
// double-buffered - float2 (a, v) with VIT, float a without: one barrier per step. A state walks its in-edges twice over
// the previous buffer (max and max-plus, then the sum). The emissions of the next PF steps are in flight while a step is
// computed, as in ctc_forward_line. ELDS stages the edge list in LDS behind the states; otherwise it is read through L2.
// With VIT every step writes one uint16 backpointer per state, coalesced; a state at -inf (and every state at t = 0)
// stores its own index, so every stored backpointer is a valid state whatever the logits hold. No atomics; the final
// reductions over the accepting states are thread 0's, in ascending state order.
// -------------------------------------------------------------------------------------------
constexpr int kPatThreads = 1024, kPatLds = 160 * 1024;

template <bool VIT>
struct PatState {
    using type = float;
    static __device__ __forceinline__ float make(float a, float) { return a; }
};
template <>
struct PatState<true> {
    using type = float2;
    static __device__ __forceinline__ float2 make(float a, float v) { return make_float2(a, v); }
};
__device__ __forceinline__ float pat_a(float x) { return x; }
__device__ __forceinline__ float pat_a(float2 x) { return x.x; }
__device__ __forceinline__ float pat_v(float) { return -INFINITY; }
__device__ __forceinline__ float pat_v(float2 x) { return x.y; }
__device__ __forceinline__ float pat_add(float x, float w) { return x + w; }
__device__ __forceinline__ float2 pat_add(float2 x, float w) { return make_float2(x.x + w, x.y + w); }
__device__ __forceinline__ float pat_lse(float m, double sum) { return m == -INFINITY ? -INFINITY : m + __logf((float)sum); }

// WGT (kind 2, PatWeights): every in-edge adds its float32 weight to its source's value before the max and the sum, the
// start list and the accepting list add theirs, and logp is not clamped (it is no probability). WLDS (with ELDS) stages
// the edge weights in LDS between the states and the edge list. Without WGT, w is not read and the code is kind 0's.
template <int NPT, bool VIT, bool ELDS, bool WGT, bool WLDS>
__device__ __forceinline__ void pattern_body(const PatArgs& a, const PatWeights& w) {
    using PS = PatState<VIT>;
    using St = typename PS::type;
    constexpr int PF = NPT >= 8 ? 1 : NPT >= 4 ? 2 : 4;      // ring depth: NPT * PF emissions in flight per thread
    constexpr int UNR = WGT && !VIT && NPT >= 8 ? 1 : 2;     // edge loops: unrolled by 2 that instance spills (20 bytes)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    St* st = (St*)smem;                                   // [2][S]: the previous and the current step
    const int S = a.S, D = a.D, b = blockIdx.x, gb = a.b0 + b, tid = threadIdx.x, nt = blockDim.x;
    const int T = min(max(a.T[gb], 1), a.W);              // (the host admits 1 <= T <= W only)
    const uint16_t* es = a.in_src;
    const float* ew = w.in_w;
    if (ELDS) {
        uint16_t* l = (uint16_t*)(smem + 2 * (size_t)S * sizeof(St) + (WGT && WLDS ? 4 * (size_t)a.E : 0));
        for (int j = tid; j < a.E; j += nt) l[j] = a.in_src[j];
        es = l;
    }
    if (WGT && WLDS) {
        float* l = (float*)(smem + 2 * (size_t)S * sizeof(St));
        for (int j = tid; j < a.E; j += nt) l[j] = w.in_w[j];
        ew = l;
    }
    const float* base = a.emis + (int64_t)b * a.W * D;
    uint16_t* bpl = VIT ? a.bp + (int64_t)b * a.W * S : nullptr;
    int slot[NPT];
    unsigned edges[NPT];                                  // first edge (18 bits: E <= 2^18) | in-degree << 18 (<= 2^13)
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int s = tid + i * nt;
        const bool live = s < S;
        slot[i] = live ? a.slot[s] : 0;
        edges[i] = live ? (unsigned)a.in_ptr[s] | (unsigned)(a.in_ptr[s + 1] - a.in_ptr[s]) << 18 : 0u;
        if (live) {
            st[s] = PS::make(-INFINITY, -INFINITY);
            if (VIT) bpl[s] = (uint16_t)s;
        }
    }
    __syncthreads();
    for (int j = tid; j < a.num_start; j += nt) {
        const int s = min(max(a.start[j], 0), S - 1);
        const float lp = WGT ? base[a.slot[s]] + w.start_w[j] : base[a.slot[s]];
        st[s] = PS::make(lp, lp);
    }
    float e[PF][NPT];
#pragma unroll
    for (int k = 0; k < PF; ++k) ctc_ring_load(base + (int64_t)min(1 + k, T - 1) * D, slot, e[k]);
    __syncthreads();
    for (int t0 = 1; t0 < T; t0 += PF) {
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int t = t0 + k;
            if (t < T) {                                   // (block-uniform)
                const St* prev = st + ((t - 1) & 1) * S;
                St* cur = st + (t & 1) * S;
#pragma unroll
                for (int i = 0; i < NPT; ++i) {
                    const int s = tid + i * nt;
                    if (s < S) {
                        const int e0 = (int)(edges[i] & 0x3FFFFu), e1 = e0 + (int)(edges[i] >> 18);
                        float m = -INFINITY, vm = -INFINITY;
                        int arg = s;
#pragma unroll UNR
                        for (int j = e0; j < e1; ++j) {
                            const int src = es[j];
                            const St p = WGT ? pat_add(prev[src], ew[j]) : prev[src];
                            m = fmaxf(m, pat_a(p));
                            if (VIT && pat_v(p) > vm) {
                                vm = pat_v(p);
                                arg = src;
                            }
                        }
                        double sum = 0.0;
                        if (m != -INFINITY) {
#pragma unroll UNR
                            for (int j = e0; j < e1; ++j)
                                sum += (double)__expf((WGT ? pat_a(prev[es[j]]) + ew[j] : pat_a(prev[es[j]])) - m);
                        }
                        cur[s] = PS::make(pat_lse(m, sum) + e[k][i], vm + e[k][i]);
                        if (VIT) bpl[(int64_t)t * S + s] = (uint16_t)arg;
                    }
                }
                __syncthreads();
            }
            ctc_ring_load(base + (int64_t)min(t + PF, T - 1) * D, slot, e[k]);      // refill the slot just used
        }
    }
    if (tid == 0) {
        const St* fin = st + ((T - 1) & 1) * S;
        float m = -INFINITY, vm = -INFINITY;
        int arg = -1;
        for (int j = 0; j < a.num_accept; ++j) {
            const int s = min(max(a.accept[j], 0), S - 1);
            const St p = WGT ? pat_add(fin[s], w.accept_w[j]) : fin[s];
            m = fmaxf(m, pat_a(p));
            if (VIT && pat_v(p) > vm) {
                vm = pat_v(p);
                arg = s;
            }
        }
        double sum = 0.0;
        if (m != -INFINITY)
            for (int j = 0; j < a.num_accept; ++j) {
                const float x = pat_a(fin[min(max(a.accept[j], 0), S - 1)]);
                sum += (double)__expf((WGT ? x + w.accept_w[j] : x) - m);
            }
        const float lp = pat_lse(m, sum);
        a.logp[gb] = !WGT && lp > 0.f ? 0.f : lp;         // a probability near 1 may round above 0; a NaN stays one
        if (VIT) {
            a.best[gb] = vm;
            a.endst[gb] = arg;
        }
    }
}

template <int NPT, bool VIT, bool ELDS>
__global__ __launch_bounds__(kPatThreads) void pattern_kernel(const PatArgs a) {
    pattern_body<NPT, VIT, ELDS, false, false>(a, PatWeights{});
}

template <int NPT, bool VIT, bool ELDS, bool WLDS>
__global__ __launch_bounds__(kPatThreads) void pattern_w_kernel(const PatArgs a, const PatWeights w) {
    pattern_body<NPT, VIT, ELDS, true, WLDS>(a, w);
}

static int pattern_npt(int S) { return S <= kPatThreads ? 1 : S <= 2 * kPatThreads ? 2 : S <= 4 * kPatThreads ? 4 : 8; }

bool pattern_edges_in_lds(int S, int E, bool viterbi) {
    return 2 * (int64_t)S * (viterbi ? 8 : 4) + 2 * (int64_t)E <= kPatLds;
}

template <int NPT, bool VIT, bool ELDS>
static hipError_t launch_pattern_t(const PatArgs& a, hipStream_t s) {
    static bool raised[64] = {};
    const int threads = ((a.S + NPT - 1) / NPT + 63) / 64 * 64;
    const int lds = 2 * a.S * (VIT ? 8 : 4) + (ELDS ? 2 * a.E : 0);
    if (threads > kPatThreads || lds > kPatLds) return hipErrorInvalidValue;
    hipError_t e = raise_lds_limit((const void*)pattern_kernel<NPT, VIT, ELDS>, kPatLds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pattern_kernel<NPT, VIT, ELDS>), dim3((unsigned)a.nb), dim3(threads), lds, s, a);
    return hipGetLastError();
}

template <int NPT>
static hipError_t launch_pattern_n(const PatArgs& a, bool vit, hipStream_t s) {
    const bool elds = pattern_edges_in_lds(a.S, a.E, vit);
    if (vit) return elds ? launch_pattern_t<NPT, true, true>(a, s) : launch_pattern_t<NPT, true, false>(a, s);
    return elds ? launch_pattern_t<NPT, false, true>(a, s) : launch_pattern_t<NPT, false, false>(a, s);
}

hipError_t launch_pattern(const PatArgs& a, bool viterbi, hipStream_t s) {
    if (a.nb <= 0) return hipSuccess;
    if (a.S < 1 || a.S > kPatMaxStates || a.E < a.S || a.E > kPatMaxEdges || a.D < 1 || a.W < 1 || a.num_accept < 1 ||
        a.num_start < 1)
        return hipErrorInvalidValue;
    switch (pattern_npt(a.S)) {
        case 1: return launch_pattern_n<1>(a, viterbi, s);
        case 2: return launch_pattern_n<2>(a, viterbi, s);
        case 4: return launch_pattern_n<4>(a, viterbi, s);
        default: return launch_pattern_n<8>(a, viterbi, s);
    }
}

int pattern_states_per_thread(int S) { return pattern_npt(S); }

bool pattern_weights_in_lds(int S, int E, bool viterbi) {
    return 2 * (int64_t)S * (viterbi ? 8 : 4) + 6 * (int64_t)E <= kPatLds;
}

template <int NPT, bool VIT, bool ELDS, bool WLDS>
static hipError_t launch_pattern_w_t(const PatArgs& a, const PatWeights& w, hipStream_t s) {
    static bool raised[64] = {};
    const int threads = ((a.S + NPT - 1) / NPT + 63) / 64 * 64;
    const int lds = 2 * a.S * (VIT ? 8 : 4) + (ELDS ? 2 * a.E : 0) + (WLDS ? 4 * a.E : 0);
    if (threads > kPatThreads || lds > kPatLds) return hipErrorInvalidValue;
    hipError_t e = raise_lds_limit((const void*)pattern_w_kernel<NPT, VIT, ELDS, WLDS>, kPatLds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pattern_w_kernel<NPT, VIT, ELDS, WLDS>), dim3((unsigned)a.nb), dim3(threads), lds, s, a, w);
    return hipGetLastError();
}

// the weights in LDS (then the edges are too), else the edges alone where they fit, else both through L2
template <int NPT, bool VIT>
static hipError_t launch_pattern_w_n(const PatArgs& a, const PatWeights& w, hipStream_t s) {
    if (pattern_weights_in_lds(a.S, a.E, VIT)) return launch_pattern_w_t<NPT, VIT, true, true>(a, w, s);
    if (pattern_edges_in_lds(a.S, a.E, VIT)) return launch_pattern_w_t<NPT, VIT, true, false>(a, w, s);
    return launch_pattern_w_t<NPT, VIT, false, false>(a, w, s);
}

hipError_t launch_pattern_weighted(const PatArgs& a, const PatWeights& w, bool viterbi, hipStream_t s) {
    if (a.nb <= 0) return hipSuccess;
    if (a.S < 1 || a.S > kPatMaxStates || a.E < a.S || a.E > kPatMaxEdges || a.D < 1 || a.W < 1 || a.num_accept < 1 ||
        a.num_start < 1 || !w.in_w || !w.accept_w || !w.start_w)
        return hipErrorInvalidValue;
    switch (pattern_npt(a.S)) {
        case 1: return viterbi ? launch_pattern_w_n<1, true>(a, w, s) : launch_pattern_w_n<1, false>(a, w, s);
        case 2: return viterbi ? launch_pattern_w_n<2, true>(a, w, s) : launch_pattern_w_n<2, false>(a, w, s);
        case 4: return viterbi ? launch_pattern_w_n<4, true>(a, w, s) : launch_pattern_w_n<4, false>(a, w, s);
        default: return viterbi ? launch_pattern_w_n<8, true>(a, w, s) : launch_pattern_w_n<8, false>(a, w, s);
    }
}

// One workgroup per line. Thread 0 walks the backpointers from the end state down to column 0 and leaves the state of
// every column in `path`; then all threads turn states into classes and fetch each column's emission; then thread 0
// collapses the path into characters with their spans and the float32 sums of their emissions, in ascending t. The walk
// is T dependent loads: serial by nature.
__global__ __launch_bounds__(256) void pattern_trace_kernel(const PatTraceArgs a) {
    const int b = blockIdx.x, gb = a.b0 + b, tid = threadIdx.x, W = a.W, S = a.S;
    const int end = a.endst[gb];
    const int T = end < 0 ? 0 : min(max(a.T[gb], 1), W);
    int32_t* path = a.path + (int64_t)gb * W;
    float* lpv = a.lpv + (int64_t)b * W;
    if (tid == 0) {
        const uint16_t* bp = a.bp + (int64_t)b * W * S;
        int s = min(end, S - 1);
        for (int t = T - 1; t >= 0; --t) {
            path[t] = s;
            s = min((int)bp[(int64_t)t * S + s], S - 1);
        }
    }
    __syncthreads();
    const float* base = a.emis + (int64_t)b * W * a.D;
    for (int t = tid; t < W; t += 256) {
        if (t < T) {
            const int s = path[t];
            path[t] = a.label[s];
            lpv[t] = base[(int64_t)t * a.D + a.slot[s]];
        } else {
            path[t] = -1;
        }
        a.labels[(int64_t)gb * W + t] = 0;
        a.span_start[(int64_t)gb * W + t] = 0;
        a.span_end[(int64_t)gb * W + t] = 0;
        a.char_logp[(int64_t)gb * W + t] = 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0, prev = 0;
        float acc = 0.f;
        const int64_t o = (int64_t)gb * W;
        for (int t = 0; t < T; ++t) {
            const int c = path[t];
            if (c != prev && prev != 0) {                  // the run of `prev` ends before column t
                a.span_end[o + n - 1] = t;
                a.char_logp[o + n - 1] = acc;
            }
            if (c != 0 && c != prev) {
                a.labels[o + n] = c;
                a.span_start[o + n] = t;
                acc = 0.f;
                ++n;
            }
            if (c != 0) acc += lpv[t];
            prev = c;
        }
        if (prev != 0) {
            a.span_end[o + n - 1] = T;
            a.char_logp[o + n - 1] = acc;
        }
        a.lengths[gb] = n;
    }
}

hipError_t launch_pattern_trace(const PatTraceArgs& a, hipStream_t s) {
    if (a.nb <= 0) return hipSuccess;
    if (a.S < 1 || a.S > kPatSetMaxStates || a.D < 1 || a.W < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pattern_trace_kernel, dim3((unsigned)a.nb), dim3(256), 0, s, a);
    return hipGetLastError();
}

// -------------------------------------------------------------------------------------------
// The set form (pat_build_sets): the same two recursions over the same CTC states, in block form. The block of DFA
// state p is beta_p and every eps_(p,.). Every state is fed by whole blocks less at most one state each:
//   beta_q    <- block q
//   eps_(q,c) <- itself, and for every arc (p, A, q) with c in A: block p without eps_(p,c)
// so a step is the totals of every block over the buffer just written, then every state from the totals of its source
// blocks: O(S + in-arcs) a step, whatever the sets hold.
// Totals of block p (one wave per block; blocks w, w + waves, .. are wave w's): lane l takes the members l, l + 64, ..
// in ascending order (member 0 = beta_p, member j = the block's j-th eps state), the 64 lanes combine by the butterfly
// over the lane offsets 32, 16, 8, 4, 2, 1. Two passes: m = the float32 maximum and i* = the lowest state that holds it
// (and, with VIT, the two best v with their states, ties to the lower state); then all = the float64 sum of
// (double)__expf(a - m) over the members and rest = the same sum without i*. The order is a function of the tables only.
// A source term of eps_(q,c) from block p: X = rest if eps_(p,c) is i*, all - (double)__expf(a(eps_(p,c)) - m) if it
// exists otherwise (the maximal term survives: nothing cancels), all if it does not; y = m + __logf((float)X), -inf
// where X is 0 or m is -inf. The state is pattern_kernel's n-ary log-sum over [its own value, y of each in-arc in
// ascending p], plus the emission. beta_q = m + __logf((float)all) of its block, plus the emission.
// Max: the candidate of block p is its best v, or its second best where the best is eps_(p,c) itself; among the own
// value and the candidates the greatest wins, ties to the lowest state - pattern_kernel's first maximal source in
// ascending order, so every Viterbi output has its bits.
// One workgroup per line, two barriers a step. The two step buffers are in LDS behind the totals (SLDS) or in the call's
// scratch, which only this workgroup touches. The emissions of a thread's first four states are in flight over the
// totals. No atomics; thread 0 reduces the final blocks in ascending q.
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ bool pat_better(float xa, int ia, float xb, int ib) { return xa > xb || (xa == xb && ia < ib); }

template <bool VIT, bool SLDS>
__global__ __launch_bounds__(kPatThreads) void pattern_set_kernel(const PatSetArgs a) {
    using PS = PatState<VIT>;
    using St = typename PS::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = a.S, nQ = a.nQ, D = a.D, b = blockIdx.x, gb = a.b0 + b, tid = threadIdx.x, nt = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int T = min(max(a.T[gb], 1), a.W);              // (the host admits 1 <= T <= W only)
    double* t_all = (double*)smem;                        // the totals of the previous step's blocks, [nQ] each
    double* t_rest = t_all + nQ;
    float* t_m = (float*)(t_rest + nQ);
    int* t_i = (int*)(t_m + nQ);
    float* t_v1 = (float*)(t_i + nQ);                     // (VIT only)
    float* t_v2 = t_v1 + nQ;
    int* t_i1 = (int*)(t_v2 + nQ);
    int* t_i2 = t_i1 + nQ;
    St* st = SLDS ? (St*)(smem + (size_t)nQ * (VIT ? 40 : 24)) : (St*)(a.states + (int64_t)b * 4 * S);      // [2][S]
    const float* base = a.emis + (int64_t)b * a.W * D;
    uint16_t* bpl = VIT ? a.bp + (int64_t)b * a.W * S : nullptr;
    const uint2* meta = (const uint2*)a.meta;
    uint2 mt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) mt[i] = tid + i * nt < S ? meta[tid + i * nt] : make_uint2(0u, 0u);
    for (int s = tid; s < S; s += nt) {
        const unsigned x = meta[s].x;
        const float lp = x >> 31 ? base[x & 0xFFFFu] : -INFINITY;
        st[s] = PS::make(lp, lp);
        if (VIT) bpl[s] = (uint16_t)s;
    }
    __syncthreads();
    for (int t = 1; t <= T; ++t) {                        // t = T: the totals of the last step alone
        const St* prev = st + ((t - 1) & 1) * S;
        const float* row = base + (int64_t)min(t, T - 1) * D;
        float e4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) e4[i] = row[mt[i].x & 0xFFFFu];
        for (int p = wave; p < nQ; p += nw) {
            const int e0 = nQ + a.blk_ptr[p], n = 1 + a.blk_ptr[p + 1] - a.blk_ptr[p];
            float m = -INFINITY, v1 = -INFINITY, v2 = -INFINITY;
            int im = 0x7FFFFFFF, i1 = -1, i2 = -1;
            for (int j = lane; j < n; j += 64) {
                const int idx = j ? e0 + j - 1 : p;
                const St x = prev[idx];
                if (pat_a(x) > m) {
                    m = pat_a(x);
                    im = idx;
                }
                if (VIT) {
                    const float xv = pat_v(x);
                    if (xv > v1) {
                        v2 = v1; i2 = i1;
                        v1 = xv; i1 = idx;
                    } else if (xv > v2) {
                        v2 = xv; i2 = idx;
                    }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const float om = __shfl_xor(m, off);
                const int oi = __shfl_xor(im, off);
                if (pat_better(om, oi, m, im)) {
                    m = om;
                    im = oi;
                }
                if (VIT) {
                    const float ov1 = __shfl_xor(v1, off), ov2 = __shfl_xor(v2, off);
                    const int oi1 = __shfl_xor(i1, off), oi2 = __shfl_xor(i2, off);
                    if (pat_better(ov1, oi1, v1, i1)) {
                        const bool k = pat_better(v1, i1, ov2, oi2);
                        v2 = k ? v1 : ov2; i2 = k ? i1 : oi2;
                        v1 = ov1; i1 = oi1;
                    } else {
                        const bool k = pat_better(ov1, oi1, v2, i2);
                        v2 = k ? ov1 : v2; i2 = k ? oi1 : i2;
                    }
                }
            }
            double all = 0.0, rest = 0.0;
            if (m > -INFINITY) {                           // (wave-uniform)
                for (int j = lane; j < n; j += 64) {
                    const int idx = j ? e0 + j - 1 : p;
                    const double ex = (double)__expf(pat_a(prev[idx]) - m);
                    all += ex;
                    if (idx != im) rest += ex;
                }
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    all += __shfl_xor(all, off);
                    rest += __shfl_xor(rest, off);
                }
            } else {
                im = p;
            }
            if (lane == 0) {
                t_all[p] = all; t_rest[p] = rest; t_m[p] = m; t_i[p] = im;
                if (VIT) { t_v1[p] = v1; t_v2[p] = v2; t_i1[p] = i1; t_i2[p] = i2; }
            }
        }
        __syncthreads();
        if (t == T) break;
        St* cur = st + (t & 1) * S;
        // a source term: block p's total without the state ex (0xFFFF: the block holds no such state)
        auto term = [&](unsigned p, unsigned ex) -> float {
            const float mp = t_m[p];
            if (!(mp > -INFINITY)) return -INFINITY;
            const double X = ex == 0xFFFFu        ? t_all[p]
                             : (int)ex == t_i[p] ? t_rest[p]
                                                 : t_all[p] - (double)__expf(pat_a(prev[ex]) - mp);
            return X > 0.0 ? mp + __logf((float)X) : -INFINITY;
        };
        auto update = [&](int s, uint2 ms, float e) {
            float aa, vv = -INFINITY;
            int arg = s;
            if (s < nQ) {
                aa = pat_lse(t_m[s], t_all[s]);
                if (VIT) {
                    vv = t_v1[s];
                    if (vv > -INFINITY) arg = t_i1[s];
                }
            } else {
                const St own = prev[s];
                const unsigned deg = (ms.x >> 16) & 0x7FFFu, first = ms.y;
                float m = fmaxf(-INFINITY, pat_a(own));
                if (VIT && pat_v(own) > vv) vv = pat_v(own);
                for (unsigned k = 0; k < deg; ++k) {
                    const unsigned w = a.in_arc[first + k], p = w & 0xFFFFu, ex = w >> 16;
                    m = fmaxf(m, term(p, ex));
                    if (VIT) {
                        const bool top = t_i1[p] == (int)ex;
                        const float cv = top ? t_v2[p] : t_v1[p];
                        const int ci = top ? t_i2[p] : t_i1[p];
                        if (cv > vv || (cv == vv && cv > -INFINITY && ci < arg)) {
                            vv = cv;
                            arg = ci;
                        }
                    }
                }
                double sum = 0.0;
                if (m != -INFINITY) {
                    sum = (double)__expf(pat_a(own) - m);
                    for (unsigned k = 0; k < deg; ++k) {
                        const unsigned w = a.in_arc[first + k];
                        sum += (double)__expf(term(w & 0xFFFFu, w >> 16) - m);
                    }
                }
                aa = pat_lse(m, sum);
            }
            cur[s] = PS::make(aa + e, vv + e);
            if (VIT) bpl[(int64_t)t * S + s] = (uint16_t)arg;
        };
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (tid + i * nt < S) update(tid + i * nt, mt[i], e4[i]);
        for (int s = tid + 4 * nt; s < S; s += nt) {
            const uint2 ms = meta[s];
            update(s, ms, row[ms.x & 0xFFFFu]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        float m = -INFINITY, vm = -INFINITY;
        int arg = -1;
        for (int j = 0; j < a.num_finals; ++j) {
            const int q = min(max(a.finals[j], 0), nQ - 1);
            m = fmaxf(m, pat_lse(t_m[q], t_all[q]));
            if (VIT) {
                const float cv = t_v1[q];
                const int ci = t_i1[q];
                if (cv > vm || (cv == vm && cv > -INFINITY && ci < arg)) {
                    vm = cv;
                    arg = ci;
                }
            }
        }
        double sum = 0.0;
        if (m != -INFINITY)
            for (int j = 0; j < a.num_finals; ++j) {
                const int q = min(max(a.finals[j], 0), nQ - 1);
                sum += (double)__expf(pat_lse(t_m[q], t_all[q]) - m);
            }
        const float lp = pat_lse(m, sum);
        a.logp[gb] = lp > 0.f ? 0.f : lp;                 // a probability near 1 may round above 0; a NaN stays one
        if (VIT) {
            a.best[gb] = vm;
            a.endst[gb] = arg;
        }
    }
}

static int pattern_set_lds(int S, int nQ, bool viterbi, bool states) {
    const int64_t bytes = (int64_t)nQ * (viterbi ? 40 : 24) + (states ? 2 * (int64_t)S * (viterbi ? 8 : 4) : 0);
    return bytes > kPatLds ? -1 : (int)bytes;
}

bool pattern_set_states_in_lds(int S, int nQ, bool viterbi) { return pattern_set_lds(S, nQ, viterbi, true) >= 0; }

template <bool VIT, bool SLDS>
static hipError_t launch_pattern_set_t(const PatSetArgs& a, hipStream_t s) {
    static bool raised[64] = {};
    const int lds = pattern_set_lds(a.S, a.nQ, VIT, SLDS);
    if (lds < 0 || (!SLDS && !a.states)) return hipErrorInvalidValue;
    // a thread per state up to 1024, and a wave per block up to 16: the results do not depend on it
    const int threads = std::min(kPatThreads, std::max((a.S + 63) / 64, std::min(a.nQ, 16)) * 64);
    hipError_t e = raise_lds_limit((const void*)pattern_set_kernel<VIT, SLDS>, kPatLds, raised);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pattern_set_kernel<VIT, SLDS>), dim3((unsigned)a.nb), dim3(threads), lds, s, a);
    return hipGetLastError();
}

// a.states == nullptr: the step buffers in LDS (the caller has asked pattern_set_states_in_lds)
hipError_t launch_pattern_set(const PatSetArgs& a, bool viterbi, hipStream_t s) {
    if (a.nb <= 0) return hipSuccess;
    if (a.S < 1 || a.S > kPatSetMaxStates || a.nQ < 1 || a.nQ > kPatSetMaxDfaStates || a.nQ > a.S || a.D < 1 ||
        a.D > 0xFFFF || a.W < 1 || a.num_finals < 1)
        return hipErrorInvalidValue;
    if (viterbi) return a.states ? launch_pattern_set_t<true, false>(a, s) : launch_pattern_set_t<true, true>(a, s);
    return a.states ? launch_pattern_set_t<false, false>(a, s) : launch_pattern_set_t<false, true>(a, s);
}

// -------------------------------------------------------------------------------------------
// Word-sequence recognition (hctr_words*): the best segmentation of a line into lexicon entries, by token passing over
// the lexicon's trie with the word ends looped back to the root (include/hctr_hip.h has the definition). Viterbi only:
//   a'(n_u) = max(a(n_u), a(b_0), pick.score) + lp_t(c_u)            u a child of the root
//   a'(n_v) = max(a(n_v), a(b_p), [c_p != c_v] a(n_p)) + lp_t(c_v)   deeper nodes
//   a'(b_v) = max(a(b_v), a(n_v)) + lp_t(0),  a'(b_0) = a(b_0) + lp_t(0)
// in float32, the earlier-listed source winning ties (a later one must be strictly greater, so a NaN state stays NaN and
// wins nothing). A state carries its origin (s << 2 | k): the column of the current word's first label and which exit
// record of column s - 1 it came from (0 = the line's start or b_0). After every column the end nodes' states are
// reduced to two exit records, R1 the best of (a(n_v) + x_v, last = slot_v) and (a(b_v) + x_v, last = 0) by (score
// descending, blank first, node ascending), R2 the best whose `last` differs from R1's: a root's child takes R1 unless
// R1 ended on the child's own label, the CTC rule that equal labels need a blank between them. The pair is a mergeable
// summary - the pair of a union is found among the parts' four records - so the reduction tree does not matter: a
// thread folds its nodes, a wave merges by shuffles, the waves' partials meet in LDS and every thread merges them.
// One workgroup per line, one barrier per column: it publishes the column's states and the waves' partials together.
// Two storage forms with one body (words_step) and the same bits: NPT > 0 keeps the two step buffers in LDS (16 bytes a
// state, 32 a node) with a thread's NPT nodes' tables in registers and their emissions of the next PF columns in flight;
// NPT = 0 keeps them in the call's scratch and a thread walks its nodes tid, tid + 1024, .. per column. No atomics.
// -------------------------------------------------------------------------------------------
constexpr int kWordsThreads = 1024, kWordsPF = 4;
constexpr int32_t kWordsEnd = 1 << 28;                    // in a thread's copy of node[v]: an entry ends on v

struct __attribute__((aligned(16))) WordsSt {
    float n, b;
    uint32_t on, ob;
};
struct WordsPair {                                        // R1 and R2, field by field (they stay in registers)
    float s1;
    int n1, l1;
    uint32_t o1;
    float s2;
    int n2, l2;
    uint32_t o2;
};

__device__ __forceinline__ WordsPair words_none() {
    return WordsPair{-INFINITY, 0x7FFFFFFF, -1, 0u, -INFINITY, 0x7FFFFFFF, -1, 0u};
}

// (score descending, blank first, node ascending)
__device__ __forceinline__ bool words_better(float xs, int xn, int xl, float ys, int yn, int yl) {
    if (xs != ys) return xs > ys;
    const bool xz = xl == 0, yz = yl == 0;
    if (xz != yz) return xz;
    return xn < yn;
}

// a candidate joins the pair; one at -inf or NaN is none
__device__ __forceinline__ void words_put(WordsPair& p, float s, int n, int l, uint32_t o) {
    if (!(s > -INFINITY)) return;
    if (words_better(s, n, l, p.s1, p.n1, p.l1)) {
        if (p.l1 != l) {
            p.s2 = p.s1; p.n2 = p.n1; p.l2 = p.l1; p.o2 = p.o1;
        }
        p.s1 = s; p.n1 = n; p.l1 = l; p.o1 = o;
    } else if (l != p.l1 && words_better(s, n, l, p.s2, p.n2, p.l2)) {
        p.s2 = s; p.n2 = n; p.l2 = l; p.o2 = o;
    }
}

// the states of node v after column t >= 1 from the previous buffer and the records of column t - 1; its exits join fold
__device__ __forceinline__ WordsSt words_step(int v, int word, int slot, float x, int t, float e, float eb,
                                              const WordsSt* prev, int nn, const WordsPair& R, WordsPair& fold) {
    const WordsSt self = prev[v];
    if (v == 0) return WordsSt{-INFINITY, self.b + eb, 0u, 0u};      // the root: b_0 alone
    const WordsSt p = prev[min(word & kLexParMask, nn - 1)];
    float m = self.n;
    uint32_t om = self.on;
    if (word & kLexFirst) {
        if (p.b > m) {
            m = p.b;
            om = (uint32_t)t << 2;
        }
        const bool one = R.l1 != slot;
        const float ps = one ? R.s1 : R.s2;
        if (ps > m) {
            m = ps;
            om = (uint32_t)t << 2 | (one ? 1u : 2u);
        }
    } else {
        if (p.b > m) {
            m = p.b;
            om = p.ob;
        }
        if ((word & kLexSkip) && p.n > m) {
            m = p.n;
            om = p.on;
        }
    }
    float mb = self.b;
    uint32_t ob = self.ob;
    if (self.n > mb) {
        mb = self.n;
        ob = self.on;
    }
    const WordsSt o{m + e, mb + eb, om, ob};
    if (word & kWordsEnd) {
        words_put(fold, o.n + x, v, slot, o.on);
        words_put(fold, o.b + x, v, 0, o.ob);
    }
    return o;
}

// column 0
__device__ __forceinline__ WordsSt words_first(int v, int word, int slot, float x, const float* row, WordsPair& fold) {
    WordsSt o{-INFINITY, -INFINITY, 0u, 0u};
    if (v == 0) o.b = row[0];
    else if (word & kLexFirst) o.n = row[slot];
    if (word & kWordsEnd) words_put(fold, o.n + x, v, slot, 0u);
    return o;
}

// a column's end: the waves' pairs meet in LDS behind the barrier that also publishes the column's states; every thread
// merges the partials and returns the column's records, thread 0 stores them
__device__ __forceinline__ WordsPair words_close(int t, WordsPair fold, WordsRec (*part)[kWordsThreads / 64][2],
                                                 WordsRec* rec) {
    const int tid = threadIdx.x, nw = blockDim.x >> 6;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float s1 = __shfl_xor(fold.s1, m, 64), s2 = __shfl_xor(fold.s2, m, 64);
        const int n1 = __shfl_xor(fold.n1, m, 64), n2 = __shfl_xor(fold.n2, m, 64);
        const int l1 = __shfl_xor(fold.l1, m, 64), l2 = __shfl_xor(fold.l2, m, 64);
        const int o1 = __shfl_xor((int)fold.o1, m, 64), o2 = __shfl_xor((int)fold.o2, m, 64);
        words_put(fold, s1, n1, l1, (uint32_t)o1);
        words_put(fold, s2, n2, l2, (uint32_t)o2);
    }
    if ((tid & 63) == 0) {
        part[t & 1][tid >> 6][0] = WordsRec{fold.s1, fold.n1, fold.l1, fold.o1};
        part[t & 1][tid >> 6][1] = WordsRec{fold.s2, fold.n2, fold.l2, fold.o2};
    }
    __syncthreads();
    WordsPair R = words_none();
    for (int w = 0; w < nw; ++w) {
        const WordsRec p1 = part[t & 1][w][0], p2 = part[t & 1][w][1];
        words_put(R, p1.score, p1.node, p1.last, p1.origin);
        words_put(R, p2.score, p2.node, p2.last, p2.origin);
    }
    if (tid == 0) {
        rec[2 * t] = WordsRec{R.s1, R.n1, R.l1, R.o1};
        rec[2 * t + 1] = WordsRec{R.s2, R.n2, R.l2, R.o2};
    }
    return R;
}

template <int NPT>
__global__ __launch_bounds__(kWordsThreads) void words_trie_kernel(const WordsArgs a) {
    constexpr bool LDS = NPT > 0;
    constexpr int NR = LDS ? NPT : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ WordsRec part[2][kWordsThreads / 64][2];
    const int b = blockIdx.x, gb = a.b0 + b, tid = threadIdx.x, nt = blockDim.x, nn = a.nn, D = a.D;
    const int T = min(max(a.T[gb], 1), a.W);              // (the host admits 1 <= T <= W only)
    WordsSt* st = LDS ? (WordsSt*)smem : (WordsSt*)a.states + (int64_t)b * 2 * nn;
    const float* base = a.emis + (int64_t)b * a.W * D;
    WordsRec* rec = a.rec + (int64_t)b * a.W * 2;
    WordsPair fold = words_none();
    if constexpr (LDS) {
        int word[NR], slot[NR];
        float x[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int v = tid + i * nt;
            const bool live = v < nn;
            word[i] = live ? a.node[v] | (a.entry[v] >= 0 ? kWordsEnd : 0) : 0;
            slot[i] = live ? a.slot[v] : 0;
            x[i] = live ? a.weight[v] : 0.f;
            if (live) st[v] = words_first(v, word[i], slot[i], x[i], base, fold);
        }
        float e[kWordsPF][NR], eb[kWordsPF];
#pragma unroll
        for (int k = 0; k < kWordsPF; ++k) {
            const float* r = base + (int64_t)min(1 + k, T - 1) * D;
            ctc_ring_load(r, slot, e[k]);
            eb[k] = r[0];
        }
        WordsPair R = words_close(0, fold, part, rec);
        for (int t0 = 1; t0 < T; t0 += kWordsPF) {
#pragma unroll
            for (int k = 0; k < kWordsPF; ++k) {
                const int t = t0 + k;
                if (t < T) {                               // (block-uniform)
                    const WordsSt* prev = st + ((t - 1) & 1) * nn;
                    WordsSt* cur = st + (t & 1) * nn;
                    fold = words_none();
#pragma unroll
                    for (int i = 0; i < NR; ++i) {
                        const int v = tid + i * nt;
                        if (v < nn) cur[v] = words_step(v, word[i], slot[i], x[i], t, e[k][i], eb[k], prev, nn, R, fold);
                    }
                    R = words_close(t, fold, part, rec);
                }
                const float* r = base + (int64_t)min(t + kWordsPF, T - 1) * D;      // refill the slot just used
                ctc_ring_load(r, slot, e[k]);
                eb[k] = r[0];
            }
        }
    } else {
        for (int v = tid; v < nn; v += nt)
            st[v] = words_first(v, a.node[v] | (a.entry[v] >= 0 ? kWordsEnd : 0), a.slot[v], a.weight[v], base, fold);
        WordsPair R = words_close(0, fold, part, rec);
        for (int t = 1; t < T; ++t) {
            const WordsSt* prev = st + ((t - 1) & 1) * nn;
            WordsSt* cur = st + (t & 1) * nn;
            const float* r = base + (int64_t)t * D;
            const float eb = r[0];
            fold = words_none();
            for (int v = tid; v < nn; v += nt) {
                const int sl = a.slot[v];
                cur[v] = words_step(v, a.node[v] | (a.entry[v] >= 0 ? kWordsEnd : 0), sl, a.weight[v], t, r[sl], eb, prev, nn,
                                    R, fold);
            }
            R = words_close(t, fold, part, rec);
        }
    }
}

template <int NPT>
static hipError_t launch_words_trie_t(const WordsArgs& a, int threads, hipStream_t s) {
    static bool raised[64] = {};
    const int lds = NPT > 0 ? 2 * a.nn * (int)sizeof(WordsSt) : 0;
    if (NPT > 0) {
        hipError_t e = raise_lds_limit((const void*)words_trie_kernel<NPT>, 2 * kWordsLdsNodes * (int)sizeof(WordsSt), raised);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(words_trie_kernel<NPT>, dim3((unsigned)a.nb), dim3(threads), lds, s, a);
    return hipGetLastError();
}

// a.states == nullptr: the step buffers in LDS (nn <= kWordsLdsNodes)
hipError_t launch_words_trie(const WordsArgs& a, hipStream_t s) {
    if (a.nb <= 0) return hipSuccess;
    if (a.nn < 2 || a.nn > kWordsMaxNodes || a.D < 2 || a.W < 1 || a.W >= (1 << 30) || !a.rec) return hipErrorInvalidValue;
    if (a.states) return launch_words_trie_t<0>(a, kWordsThreads, s);
    if (a.nn > kWordsLdsNodes) return hipErrorInvalidValue;
    if (a.nn <= kWordsThreads) return launch_words_trie_t<1>(a, (a.nn + 63) / 64 * 64, s);
    if (a.nn <= 2 * kWordsThreads) return launch_words_trie_t<2>(a, kWordsThreads, s);
    return launch_words_trie_t<4>(a, kWordsThreads, s);
}

// One workgroup of 64 per line: all lanes clear the line's outputs, then lane 0 walks the records from R1(T - 1) back to
// the line's start twice, once to count the words and the labels, once to fill. A record of column s - 1 is followed
// only when 1 <= s <= the column of the record before it, a node is used only inside [1, nn), and a spelling is at most
// kLexMaxLen parents long: every index is in range whatever the records hold, and the walk ends within T steps.
__global__ __launch_bounds__(64) void words_backtrace_kernel(const WordsTraceArgs a) {
    const int b = blockIdx.x, gb = a.b0 + b, lane = threadIdx.x, W = a.W, nn = a.nn, mw = a.max_words;
    const int T = min(max(a.T[gb], 1), W);
    int32_t* words = a.words + (int64_t)gb * mw;
    int32_t* starts = a.starts + (int64_t)gb * mw;
    int32_t* labels = a.labels + (int64_t)gb * W;
    for (int j = lane; j < mw; j += 64) {
        words[j] = -1;
        starts[j] = -1;
    }
    for (int j = lane; j < W; j += 64) labels[j] = 0;
    __syncthreads();
    if (lane != 0) return;
    const WordsRec* rec = a.rec + (int64_t)b * W * 2;
    const WordsRec end = rec[2 * (T - 1)];
    int cnt = 0, L = 0;
    for (int pass = 0; pass < 2; ++pass) {
        WordsRec r = end;
        int col = T - 1, i = cnt, pos = min(L, W);
        for (int it = 0; it < T; ++it) {
            if (!(r.score > -INFINITY) || r.node < 1 || r.node >= nn) break;
            const int s = (int)(r.origin >> 2), k = (int)(r.origin & 3u);
            int len = 0;
            for (int u = r.node; u > 0 && len < kLexMaxLen; u = min(a.node[u] & kLexParMask, nn - 1)) {
                if (pass) {
                    --pos;
                    if (pos >= 0 && pos < W) labels[pos] = a.cls[a.slot[u]];
                }
                ++len;
            }
            if (pass) {
                --i;
                if (i >= 0 && i < mw) {
                    words[i] = a.entry[r.node];
                    starts[i] = s;
                }
            } else {
                ++cnt;
                L += len;
            }
            if (k < 1 || k > 2 || s < 1 || s > col) break;
            col = s - 1;
            r = rec[2 * col + (k - 1)];
        }
    }
    a.count[gb] = cnt;
    a.lengths[gb] = min(L, W);
    a.score[gb] = cnt > 0 ? end.score : -INFINITY;
}

hipError_t launch_words_backtrace(const WordsTraceArgs& a, hipStream_t s) {
    if (a.nb <= 0) return hipSuccess;
    if (a.nn < 2 || a.nn > kWordsMaxNodes || a.W < 1 || a.max_words < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(words_backtrace_kernel, dim3((unsigned)a.nb), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace hctr
