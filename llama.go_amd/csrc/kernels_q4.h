// csrc/kernels_q4.h — block-int4 weights (dtype 2 = ml.TYPE_Q4_0: named at ml.go:88 and sized at ml.go:123-124, refused by the loader at llama.go:956-959).
//
//     interchange / registration format: blocks of QK = 32 weights { float d; uint8 qs[16] } = 20 bytes,  w = d * (n - 8); element 2j of a block is the
//                                        low nibble of qs[j], element 2j + 1 its high nibble (ggml's Q4_0 of the reference's vintage)
//     quantiser (ours, k_quantize_q8's shape): d = fl32(max|w| / 7), q = clamp(rint(fl32(w / d)), -7, 7), n = q + 8   (d = 0 -> q = 0)
//                                        a block that holds a NaN or an infinity: d = NaN, q = 0.  It never emits n = 0 (q = -8); registered blocks
//                                        that hold it are kept exactly.
// HBM layout: a nibble plane [rows][K / 2] bytes and an fp32 scale plane [rows][K / 32] in the same allocation (Buffer::scales), K % 32 == 0: a lane's
// 8-byte load is 16 consecutive weights.
//
// The equality everything here rests on: a 4-bit quant q in [-8, 7] with block scale d IS a block-int8 weight with the same q and the same d.
// (float)(n - 8) is exact however it is computed, so a kernel that differs from k_gemv_q8s (kernels_q8.h) / k_gemv_q8_rows (kernels_rows.h) only in
// where a slot's 16 quants come from feeds identical operands into identical fp32 operations: k_gemv_q4s / k_gemv_q4_rows give the bits of the int8
// kernels over the expansion (k_expand_q4: same q, same d, no requantising).  The lane -> column map (KI, TPR, TH per shape) is gemv_q8's; the rows in
// flight (U) are not part of the summation order and are chosen for the halved rows.  Prologue and epilogue helpers (wg_row_block, gemv_prefetch_fin,
// wave_sum_lane63, gemv_finish) are the int8 kernels' own.
#pragma once
#include "kernels_q8.h"
#include "kernels_rows.h"

namespace lh {

typedef unsigned int u2 __attribute__((ext_vector_type(2)));

// The 16 nibbles of an 8-byte load as the 16 floats dot16_q8 sees, in its pairing: chunk k of four weights is w0[k] = (e0, e1), w1[k] = (e2, e3).
// Byte b of the load holds elements 2b (low nibble) and 2b + 1 (high nibble).  The low and the high nibbles of a dword are turned into two dwords of
// four SIGNED bytes n - 8 each - mask, then ((n + 0x78) ^ 0x80) per byte, which no carry leaves (k_expand_q4's step) - and every byte is converted
// the way dot16_q8 converts its quants (v_cvt_f32_i32 with a sign-extending byte select): 7 integer instructions and 8 converts per 8 weights.
// (Written as (float)n - 8.0f the compiler moves the subtraction in front of the convert and isolates every nibble on its own: and / shift, add, convert
// = 3 instructions per weight, 2.5 x the vector instructions of k_gemv_q8s per row - measured 17 % slower than int8 on the 7B decode loop.)
__device__ __forceinline__ void unpack16_q4(const u2 q, f2 (&w0)[4], f2 (&w1)[4]) {
#pragma unroll
    for (int dw = 0; dw < 2; ++dw) {
        const int lo = (int)(((q[dw] & 0x0f0f0f0fu) + 0x78787878u) ^ 0x80808080u), hi = (int)((((q[dw] >> 4) & 0x0f0f0f0fu) + 0x78787878u) ^ 0x80808080u);
        w0[2 * dw] = f2{(float)(int)(signed char)(lo), (float)(int)(signed char)(hi)};
        w1[2 * dw] = f2{(float)(int)(signed char)(lo >> 8), (float)(int)(signed char)(hi >> 8)};
        w0[2 * dw + 1] = f2{(float)(int)(signed char)(lo >> 16), (float)(int)(signed char)(hi >> 16)};
        w1[2 * dw + 1] = f2{(float)(lo >> 24), (float)(hi >> 24)};
    }
}

// dot16_q8 (kernels_q8.h) over the unpacked nibbles: the same two packed accumulator pairs in the same order, the same final adds
__device__ __forceinline__ float dot16_q4(const u2 q, const f4 (&x)[4]) {
    f2 w0[4], w1[4];
    unpack16_q4(q, w0, w1);
    f2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a0 = __builtin_elementwise_fma(w0[k], f2{x[k].x, x[k].y}, a0);
        a1 = __builtin_elementwise_fma(w1[k], f2{x[k].z, x[k].w}, a1);
    }
    return (a0.x + a0.y) + (a1.x + a1.y);
}

// ---------------------------------------------------------------------------------------------------
// k_gemv_q4s — k_gemv_q8s with a row of K / 2 bytes: slot j loads the 8 bytes at qb + c * 8 (scalar row base + constant lane offset, non-temporal,
// rows beyond the workgroup's range redirected to the activation vector: 4K bytes cover a nibble row and a scale row) and unpacks them.
// ---------------------------------------------------------------------------------------------------
template <int KI, int U, int TPR, int PRO, int EPI, int MAP, int TH = 1024>
__global__ __launch_bounds__(TH) void k_gemv_q4s(const GemvArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.x, a.hd, a.wg_r);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int G = TH / TPR, NWR = TPR / 64;
    static_assert(TPR % 64 == 0, "a row group must be a whole number of waves");
    double* sred = (double*)smem_raw;            // [16]
    float* red = (float*)(smem_raw + 16 * 8);    // [rows of this workgroup][NWR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tr = tid % TPR, wr = wave % NWR;
    const uint32_t grp = (uint32_t)__builtin_amdgcn_readfirstlane(tid / TPR);   // uniform within a wave
    const uint32_t K = a.K, K16 = K >> 4;
    uint32_t r0, r1;
    wg_row_block(a.M, a.wg_q, a.wg_r, &r0, &r1);
    // matrix bases as scalar integers + distances, virtual bases for MAP_BLOCK (see k_gemv_q8s)
    const uint64_t q0 = (uint64_t)sgpr_ptr(a.w[0]), s0 = (uint64_t)sgpr_ptr(a.ws[0]);
    const uint64_t dq1 = MAP == MAP_SINGLE ? 0 : (uint64_t)sgpr_ptr(a.w[1]) - q0, ds1 = MAP == MAP_SINGLE ? 0 : (uint64_t)sgpr_ptr(a.ws[1]) - s0;
    const uint64_t dq2 = MAP == MAP_BLOCK ? (uint64_t)sgpr_ptr(a.w[2]) - q0 - dq1 : 0, ds2 = MAP == MAP_BLOCK ? (uint64_t)sgpr_ptr(a.ws[2]) - s0 - ds1 : 0;
    const uint64_t xdummy = (uint64_t)sgpr_ptr(a.x);
    const uint32_t rpm = a.rows_per_mat;
    const uint64_t qrow = (uint64_t)(K >> 1), srow = (uint64_t)(K >> 5) * 4u;
    const uint64_t e1q = dq1 - (uint64_t)rpm * qrow, e2q = dq2 - (uint64_t)rpm * qrow, e1s = ds1 - (uint64_t)rpm * srow, e2s = ds2 - (uint64_t)rpm * srow;
    const uint32_t mlo = (r0 >= rpm ? 1u : 0u) + (r0 >= 2u * rpm ? 1u : 0u), mhi = (r1 - 1u >= rpm ? 1u : 0u) + (r1 - 1u >= 2u * rpm ? 1u : 0u);
    const bool one_mat = mhi - mlo <= 1u;
    const uint64_t qv_wg = q0 + (mlo >= 1u ? e1q : 0) + (mlo == 2u ? e2q : 0), sv_wg = s0 + (mlo >= 1u ? e1s : 0) + (mlo == 2u ? e2s : 0);
    const uint32_t bnd = (mlo + 1u) * rpm;
    const uint64_t nq = (mlo == 0u ? e1q : 0) + (mlo == 1u ? e2q : 0), ns = (mlo == 0u ? e1s : 0) + (mlo == 1u ? e2s : 0);
    const uint32_t fin = (EPI == EPI_STORE || EPI == EPI_RESID) ? (uint32_t)tid : 2u * (uint32_t)tid;
    float resid_pre;
    double2 cs_pre;
    uint32_t past_pre;
    gemv_prefetch_fin<EPI>(a, r0, r1, fin, &resid_pre, &cs_pre, &past_pre);
    f4 xr[KI][4];
    bool act[KI];
    uint32_t qoff[KI], soff[KI];
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        const uint32_t c = tr + j * TPR;
        act[j] = c < K16;
        qoff[j] = act[j] ? c * 8u : 0u;
        soff[j] = act[j] ? (c >> 1) * 4u : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) xr[j][k] = act[j] ? ((const f4*)a.x)[c * 4 + k] : f4{0.f, 0.f, 0.f, 0.f};
    }
    f4 gr[PRO == PRO_RMSNORM ? KI : 1][4];
    if (PRO == PRO_RMSNORM) {
#pragma unroll
        for (int j = 0; j < KI; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) gr[j][k] = act[j] ? ((const f4*)a.gamma)[(tr + j * TPR) * 4 + k] : f4{0.f, 0.f, 0.f, 0.f};
    }

    // slot u of this group holds row rb + G*u
    auto fetch = [&](u2 (&wd)[U][KI], float (&sd)[U][KI], uint32_t row_base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = row_base + G * u;
            uint64_t qb = xdummy, sb = xdummy;
            if (MAP == MAP_BLOCK) {
                if (row < r1) {
                    uint64_t bq = qv_wg + (row >= bnd ? nq : 0), bs = sv_wg + (row >= bnd ? ns : 0);
                    if (!one_mat) {
                        bq = q0 + (row >= rpm ? e1q : 0) + (row >= 2u * rpm ? e2q : 0);
                        bs = s0 + (row >= rpm ? e1s : 0) + (row >= 2u * rpm ? e2s : 0);
                    }
                    qb = bq + (uint64_t)row * qrow;
                    sb = bs + (uint64_t)row * srow;
                }
            } else
            if (row < r1) {   // scalar condition: s_cselect on the two addresses, no exec masking
                uint32_t m = 0, r = row;
                if (MAP == MAP_PAIR) { m = row & 1u; r = row >> 1; }
                qb = q0 + (m >= 1u ? dq1 : 0) + (uint64_t)r * qrow;
                sb = s0 + (m >= 1u ? ds1 : 0) + (uint64_t)r * srow;
            }
            typedef const u2 __attribute__((address_space(1))) gu2;
            typedef const float __attribute__((address_space(1))) gf32;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                wd[u][j] = __builtin_nontemporal_load((gu2*)(qb + qoff[j]));
                sd[u][j] = *(gf32*)(sb + soff[j]);
            }
        }
    };
    u2 wA[U][KI], wB[U][KI];
    float scA[U][KI], scB[U][KI];
    fetch(wA, scA, r0 + grp);
    constexpr uint32_t STEP = G * U;

    if (PRO == PRO_RMSNORM) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < KI; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (act[j]) {
                    s += (double)__fmul_rn(xr[j][k].x, xr[j][k].x);
                    s += (double)__fmul_rn(xr[j][k].y, xr[j][k].y);
                    s += (double)__fmul_rn(xr[j][k].z, xr[j][k].z);
                    s += (double)__fmul_rn(xr[j][k].w, xr[j][k].w);
                }
            }
        s = wave_sum_f64(s);
        if (lane == 0) sred[wave] = s;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < NWR; ++k) tot += sred[grp * NWR + k];
        const float scale = (float)(1.0 / sqrt(tot / (double)K + 1e-5));
#pragma unroll
        for (int j = 0; j < KI; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (act[j]) {
                    const f4 g = gr[j][k];
                    xr[j][k].x = __fmul_rn(g.x, __fmul_rn(xr[j][k].x, scale));
                    xr[j][k].y = __fmul_rn(g.y, __fmul_rn(xr[j][k].y, scale));
                    xr[j][k].z = __fmul_rn(g.z, __fmul_rn(xr[j][k].z, scale));
                    xr[j][k].w = __fmul_rn(g.w, __fmul_rn(xr[j][k].w, scale));
                }
            }
    }

    auto consume = [&](const u2 (&wd)[U][KI], const float (&sd)[U][KI], uint32_t rb) {
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KI; ++j) s = fmaf(sd[u][j], dot16_q4(wd[u][j], xr[j]), s);
            acc[u] = s;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = wave_sum_lane63(acc[u]);
        if (lane == 63) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t row = rb + G * u;
                if (row < r1) red[(row - r0) * NWR + wr] = acc[u];
            }
        }
    };
    for (uint32_t rb = r0 + grp; rb < r1; rb += 2 * STEP) {
        fetch(wB, scB, rb + STEP);
        consume(wA, scA, rb);
        fetch(wA, scA, rb + 2 * STEP);
        consume(wB, scB, rb + STEP);   // rows >= r1: loaded from the dummy, results dropped by the row test
    }
    __syncthreads();
    gemv_finish<EPI, NWR>(a, red, r0, r1, fin, resid_pre, cs_pre, past_pre);
}

// ---------------------------------------------------------------------------------------------------
// k_gemv_q4_rows — the same step for k_gemv_q8_rows (kernels_rows.h): NC activation rows, the 16 nibbles of a load unpacked ONCE and multiplied
// into every row's pair of packed accumulators; per activation row the arithmetic and its order are k_gemv_q4s' = k_gemv_q8s'.
// ---------------------------------------------------------------------------------------------------
template <int KI, int U, int TPR, int TH, int NC, int PRO, int EPI, int MAP>
__global__ __launch_bounds__(TH) void k_gemv_q4_rows(const GemvRowsArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.x, a.rows, a.wg_q);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int G = TH / TPR, NWR = TPR / 64;
    static_assert(TPR % 64 == 0, "a row group must be a whole number of waves");
    double* sred = (double*)smem_raw;                        // [NC][16]
    float* red = (float*)(smem_raw + NC * 16 * 8);           // [weight rows of this workgroup][NC][NWR]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tr = tid % TPR, wr = wave % NWR;
    const uint32_t grp = (uint32_t)__builtin_amdgcn_readfirstlane(tid / TPR);   // uniform within a wave
    const uint32_t K = a.K, K16 = K >> 4;
    uint32_t r0, r1;
    wg_row_block(a.M, a.wg_q, a.wg_r, &r0, &r1);
    const uint64_t q0 = (uint64_t)sgpr_ptr(a.w[0]), s0 = (uint64_t)sgpr_ptr(a.ws[0]);
    const uint64_t dq1 = MAP == MAP_SINGLE ? 0 : (uint64_t)sgpr_ptr(a.w[1]) - q0, ds1 = MAP == MAP_SINGLE ? 0 : (uint64_t)sgpr_ptr(a.ws[1]) - s0;
    const uint64_t dq2 = MAP == MAP_BLOCK ? (uint64_t)sgpr_ptr(a.w[2]) - q0 - dq1 : 0, ds2 = MAP == MAP_BLOCK ? (uint64_t)sgpr_ptr(a.ws[2]) - s0 - ds1 : 0;
    const uint64_t xdummy = (uint64_t)sgpr_ptr(a.x);
    const uint32_t rpm = a.rows_per_mat;
    const uint64_t qrow = (uint64_t)(K >> 1), srow = (uint64_t)(K >> 5) * 4u;
    const uint64_t e1q = dq1 - (uint64_t)rpm * qrow, e2q = dq2 - (uint64_t)rpm * qrow, e1s = ds1 - (uint64_t)rpm * srow, e2s = ds2 - (uint64_t)rpm * srow;
    const uint32_t mlo = (r0 >= rpm ? 1u : 0u) + (r0 >= 2u * rpm ? 1u : 0u), mhi = (r1 - 1u >= rpm ? 1u : 0u) + (r1 - 1u >= 2u * rpm ? 1u : 0u);
    const bool one_mat = mhi - mlo <= 1u;
    const uint64_t qv_wg = q0 + (mlo >= 1u ? e1q : 0) + (mlo == 2u ? e2q : 0), sv_wg = s0 + (mlo >= 1u ? e1s : 0) + (mlo == 2u ? e2s : 0);
    const uint32_t bnd = (mlo + 1u) * rpm;
    const uint64_t nq = (mlo == 0u ? e1q : 0) + (mlo == 1u ? e2q : 0), ns = (mlo == 0u ? e1s : 0) + (mlo == 1u ? e2s : 0);
    bool act[KI];
    uint32_t qoff[KI], soff[KI];
    f4 xr[NC][KI][4];
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        const uint32_t ch = (uint32_t)tr + (uint32_t)j * TPR;
        act[j] = ch < K16;
        qoff[j] = act[j] ? ch * 8u : 0u;
        soff[j] = act[j] ? (ch >> 1) * 4u : 0u;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float* xc = a.x + (size_t)((uint32_t)c < a.n ? c : 0) * a.ldx;
#pragma unroll
            for (int k = 0; k < 4; ++k) xr[c][j][k] = act[j] ? ((const f4*)xc)[ch * 4 + k] : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
    auto fetch = [&](u2 (&wd)[U][KI], float (&sd)[U][KI], uint32_t row_base) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = row_base + G * u;
            uint64_t qb = xdummy, sb = xdummy;
            if (MAP == MAP_BLOCK) {
                if (row < r1) {
                    uint64_t bq = qv_wg + (row >= bnd ? nq : 0), bs = sv_wg + (row >= bnd ? ns : 0);
                    if (!one_mat) {
                        bq = q0 + (row >= rpm ? e1q : 0) + (row >= 2u * rpm ? e2q : 0);
                        bs = s0 + (row >= rpm ? e1s : 0) + (row >= 2u * rpm ? e2s : 0);
                    }
                    qb = bq + (uint64_t)row * qrow;
                    sb = bs + (uint64_t)row * srow;
                }
            } else
            if (row < r1) {
                uint32_t m = 0, r = row;
                if (MAP == MAP_PAIR) { m = row & 1u; r = row >> 1; }
                qb = q0 + (m >= 1u ? dq1 : 0) + (uint64_t)r * qrow;
                sb = s0 + (m >= 1u ? ds1 : 0) + (uint64_t)r * srow;
            }
            typedef const u2 __attribute__((address_space(1))) gu2;
            typedef const float __attribute__((address_space(1))) gf32;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                wd[u][j] = __builtin_nontemporal_load((gu2*)(qb + qoff[j]));
                sd[u][j] = *(gf32*)(sb + soff[j]);
            }
        }
    };
    u2 wA[U][KI], wB[U][KI];
    float scA[U][KI], scB[U][KI];
    fetch(wA, scA, r0 + grp);

    if (PRO == PRO_RMSNORM) {
        f4 gr[KI][4];
#pragma unroll
        for (int j = 0; j < KI; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) gr[j][k] = act[j] ? ((const f4*)a.gamma)[((uint32_t)tr + (uint32_t)j * TPR) * 4 + k] : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < KI; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (act[j]) {
                        s += (double)__fmul_rn(xr[c][j][k].x, xr[c][j][k].x);
                        s += (double)__fmul_rn(xr[c][j][k].y, xr[c][j][k].y);
                        s += (double)__fmul_rn(xr[c][j][k].z, xr[c][j][k].z);
                        s += (double)__fmul_rn(xr[c][j][k].w, xr[c][j][k].w);
                    }
                }
            s = wave_sum_f64(s);
            if (lane == 0) sred[c * 16 + wave] = s;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double tot = 0.0;
#pragma unroll
            for (int k = 0; k < NWR; ++k) tot += sred[c * 16 + grp * NWR + k];
            const float scale = (float)(1.0 / sqrt(tot / (double)K + 1e-5));
#pragma unroll
            for (int j = 0; j < KI; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (act[j]) {
                        const f4 g = gr[j][k];
                        xr[c][j][k].x = __fmul_rn(g.x, __fmul_rn(xr[c][j][k].x, scale));
                        xr[c][j][k].y = __fmul_rn(g.y, __fmul_rn(xr[c][j][k].y, scale));
                        xr[c][j][k].z = __fmul_rn(g.z, __fmul_rn(xr[c][j][k].z, scale));
                        xr[c][j][k].w = __fmul_rn(g.w, __fmul_rn(xr[c][j][k].w, scale));
                    }
                }
        }
    }

    auto consume = [&](const u2 (&wd)[U][KI], const float (&sd)[U][KI], uint32_t rb) {
        float acc[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[u][c] = 0.f;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                f2 w0[4], w1v[4];      // the 16 quants of the chunk as floats, unpacked once for all activation rows
                unpack16_q4(wd[u][j], w0, w1v);
#pragma unroll
                for (int c = 0; c < NC; ++c) {   // dot16_q8's two packed chains and their final adds, then the chunk's scale: k_gemv_q8s' order
                    f2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        a0 = __builtin_elementwise_fma(w0[k], f2{xr[c][j][k].x, xr[c][j][k].y}, a0);
                        a1 = __builtin_elementwise_fma(w1v[k], f2{xr[c][j][k].z, xr[c][j][k].w}, a1);
                    }
                    acc[u][c] = fmaf(sd[u][j], (a0.x + a0.y) + (a1.x + a1.y), acc[u][c]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[u][c] = wave_sum_lane63(acc[u][c]);
        if (lane == 63) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t row = rb + G * u;
                if (row < r1) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) red[((size_t)(row - r0) * NC + c) * NWR + wr] = acc[u][c];
                }
            }
        }
    };
    constexpr uint32_t STEP = G * U;
    for (uint32_t rb = r0 + grp; rb < r1; rb += 2 * STEP) {
        fetch(wB, scB, rb + STEP);
        consume(wA, scA, rb);
        fetch(wA, scA, rb + 2 * STEP);
        consume(wB, scB, rb + STEP);   // rows >= r1: loaded from the dummy, results dropped by the row test
    }
    __syncthreads();
    const uint32_t fin = (EPI == EPI_STORE || EPI == EPI_RESID) ? (uint32_t)tid : 2u * (uint32_t)tid;
    if (r0 + fin >= r1) return;
    const uint32_t v = r0 + fin;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if ((uint32_t)c >= a.n) break;
        const float* p0 = red + ((size_t)fin * NC + c) * NWR;
        float s0v = 0.f;
#pragma unroll
        for (int k = 0; k < NWR; ++k) s0v += p0[k];
        if (EPI == EPI_STORE) {
            a.y[(size_t)c * a.ldy + v] = s0v;
        } else if (EPI == EPI_RESID) {
            a.y[(size_t)c * a.ldy + v] = __fadd_rn(s0v, a.resid[(size_t)c * a.ldy + v]);
        } else {
            const float* p1 = p0 + (size_t)NC * NWR;
            float s1v = 0.f;
#pragma unroll
            for (int k = 0; k < NWR; ++k) s1v += p1[k];
            if (EPI == EPI_SILU_MUL) {
                a.y[(size_t)c * a.ldy + (v >> 1)] = __fmul_rn(silu_ref(s0v), s1v);
            } else {
                const uint32_t d = a.d;
                const uint32_t pos = a.rows ? a.rows[c].pos : a.past + (uint32_t)c;
                float* kcb = a.rows ? a.rows[c].kc + a.kv_off : a.k_cache;
                float* vcb = a.rows ? a.rows[c].vc + a.kv_off : a.v_cache;
                if (v < 2 * d) {
                    const uint32_t e = v < d ? v : v - d;
                    const double2 cs = a.rope[(size_t)pos * (a.hd >> 1) + ((e % a.hd) >> 1)];
                    float o0, o1;
                    rope_rotate(s0v, s1v, cs, &o0, &o1);
                    float* dst = v < d ? a.q_out + (size_t)c * d + e : kcb + (size_t)pos * d + e;
                    dst[0] = o0;
                    dst[1] = o1;
                } else {
                    float* dst = vcb + (size_t)pos * d + (v - 2 * d);
                    dst[0] = s0v;
                    dst[1] = s1v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// k_expand_q4 — a nibble plane of n8 8-byte units -> the int8 plane of the same quants (16 bytes per unit); the scales are the model's own and are
// not copied.  Per byte n - 8 is ((n + 0x78) ^ 0x80): no carry leaves a byte (n + 0x78 <= 0x87).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_expand_q4(const u2* __restrict__ src, u4* __restrict__ dst, uint64_t n8) {
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (; i < n8; i += stride) {
        const u2 v = src[i];
        u4 o;
#pragma unroll
        for (int dw = 0; dw < 2; ++dw) {
            const uint32_t lo = ((v[dw] & 0x0f0f0f0fu) + 0x78787878u) ^ 0x80808080u, hi = (((v[dw] >> 4) & 0x0f0f0f0fu) + 0x78787878u) ^ 0x80808080u;
            o[2 * dw] = (lo & 0xffu) | ((hi & 0xffu) << 8) | ((lo & 0xff00u) << 8) | ((hi & 0xff00u) << 16);
            o[2 * dw + 1] = ((lo >> 16) & 0xffu) | (((hi >> 16) & 0xffu) << 8) | ((lo >> 8) & 0xff0000u) | (hi & 0xff000000u);
        }
        dst[i] = o;
    }
}

// Quantiser: one thread per block of 32 weights of an fp32 matrix [rows][K] -> planes (k_quantize_q8's shape; the rule at the top of the file).
__global__ __launch_bounds__(256) void k_quantize_q4(const float* __restrict__ src, unsigned char* __restrict__ q, float* __restrict__ scales, uint64_t nblocks) {
    uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (; b < nblocks; b += stride) {
        f4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ((const f4*)src)[b * 8 + i];
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) m = fmaxf(fmaxf(fmaxf(m, fabsf(v[i].x)), fabsf(v[i].y)), fmaxf(fabsf(v[i].z), fabsf(v[i].w)));
        bool nonfinite = false;   // a NaN or an infinity in the block: scale NaN, quants 0 (d > 0 is false below)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float f[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) nonfinite |= (__builtin_bit_cast(uint32_t, f[k]) & 0x7f800000u) == 0x7f800000u;
        }
        const float d = nonfinite ? __builtin_nanf("") : __fdiv_rn(m, 7.0f);
        unsigned int packed[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // eight weights = four bytes: element 2j in the low nibble of byte j, 2j + 1 in the high one
            const float f[8] = {v[2 * i].x, v[2 * i].y, v[2 * i].z, v[2 * i].w, v[2 * i + 1].x, v[2 * i + 1].y, v[2 * i + 1].z, v[2 * i + 1].w};
            unsigned int p = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float t = d > 0.f ? rintf(__fdiv_rn(f[k], d)) : 0.f;
                t = fminf(fmaxf(t, -7.f), 7.f);
                p |= (unsigned)((int)t + 8) << (4 * k);
            }
            packed[i] = p;
        }
        *(u4*)(q + b * 16) = u4{packed[0], packed[1], packed[2], packed[3]};
        scales[b] = d;
    }
}

// Registration from the 20-byte interchange blocks { float d; uint8 qs[16] } -> planes: every nibble as it is (n = 0 included).
__global__ __launch_bounds__(256) void k_q4_deinterleave(const unsigned int* __restrict__ blocks, unsigned char* __restrict__ q, float* __restrict__ scales, uint64_t nblocks) {
    uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (; b < nblocks; b += stride) {
        const unsigned int* s = blocks + b * 5;
        scales[b] = __builtin_bit_cast(float, s[0]);
        *(u4*)(q + b * 16) = u4{s[1], s[2], s[3], s[4]};
    }
}

}  // namespace lh
