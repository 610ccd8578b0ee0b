// csrc/kernels_q41.h — Q4_1 weights (dtype 3 = ml.TYPE_Q4_1: named at ml.go:89 and sized at ml.go:123-124, refused by the loader at llama.go:956-959).
//
//     interchange / registration format: blocks of QK = 32 weights { float d; float m; uint8 qs[16] } = 24 bytes; element 2j of a block is the low nibble
//                                        of qs[j], element 2j + 1 its high nibble, n in [0, 15] (ggml's Q4_1 of the reference's vintage, dtype 2's order)
//     the value of a weight:             w' = fl32(fma(d, n, m)) - ONE rounding, an fp32 number.  Every kernel here forms it with one FMA, so a Q4_1 model
//                                        and the fp32 model of its w' (k_expand_q41) hold identical values; none exists only inside a kernel.
//     quantiser (ours, k_quantize_q4's shape): m = min w, d = fl32(fl32(max w - m) / 15), n = clamp(rint(fl32(fl32(w - m) / d)), 0, 15)   (d = 0 -> n = 0,
//                                        w' = m); a block that holds a NaN or an infinity, or whose max w - min w overflows: d = m = NaN, n = 0.  Registered blocks are kept
//                                        bit for bit.
// HBM layout: a nibble plane [rows][K / 2] bytes and an fp32 plane of (d, m) pairs [rows][K / 32][2] in the same allocation (Buffer::scales), K % 32 == 0:
// a lane's 8-byte nibble load is 16 consecutive weights, and ONE 8-byte load brings their block's d and m.
//
// Unlike dtype 2 this is no block-int8 weight (w = d n + m has an offset), so nothing here is "the int8 kernel with another load": the kernels own their
// unpack and their arithmetic, and keep only k_gemv_q4s' lane -> column map (KI, TPR, TH per shape), launch forms and double-buffered fetch.  The unpack
// is cheaper than dtype 2's: nibbles are unsigned, so a dword is two masks and a shift (3 integer instructions per 8 weights, no bias step), the bytes
// convert with the unsigned byte-select converts, and w' is a packed FMA with d and m broadcast.  The 16 w' of a slot go through dot16_q8's two packed
// accumulator pairs in its order; the slot sums are then ADDED in j order (no per-slot scale FMA - the scale is inside w').
// Prologue and epilogue helpers (wg_row_block, gemv_prefetch_fin, wave_sum_lane63, gemv_finish) are the int8 kernels' own.
#pragma once
#include "kernels_q4.h"

namespace lh {

// The 16 w' of an 8-byte load, in dot16_q8's pairing: chunk k of four weights is w0[k] = (e0, e1), w1[k] = (e2, e3).  Byte b of the load holds elements
// 2b (low nibble) and 2b + 1 (high nibble).  (The masked dwords pass through an empty asm so that the byte selects below stay byte selects: left to
// itself the compiler folds mask, shift and select into one bit-field extract per weight, the and / shift / convert per weight that cost dtype 2 17 %.)
__device__ __forceinline__ void unpack16_q41(const u2 q, const f2 dm, f2 (&w0)[4], f2 (&w1)[4]) {
    const f2 dd = {dm.x, dm.x}, mm = {dm.y, dm.y};
#pragma unroll
    for (int dw = 0; dw < 2; ++dw) {
        uint32_t lo = q[dw] & 0x0f0f0f0fu, hi = (q[dw] >> 4) & 0x0f0f0f0fu;
        asm("" : "+v"(lo), "+v"(hi));
        w0[2 * dw] = __builtin_elementwise_fma(dd, f2{(float)(lo & 0xffu), (float)(hi & 0xffu)}, mm);
        w1[2 * dw] = __builtin_elementwise_fma(dd, f2{(float)((lo >> 8) & 0xffu), (float)((hi >> 8) & 0xffu)}, mm);
        w0[2 * dw + 1] = __builtin_elementwise_fma(dd, f2{(float)((lo >> 16) & 0xffu), (float)((hi >> 16) & 0xffu)}, mm);
        w1[2 * dw + 1] = __builtin_elementwise_fma(dd, f2{(float)(lo >> 24), (float)(hi >> 24)}, mm);
    }
}

// dot16_q8's two packed chains and final adds over 16 unpacked w'
__device__ __forceinline__ float dot16_w(const f2 (&w0)[4], const f2 (&w1)[4], const f4 (&x)[4]) {
    f2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        a0 = __builtin_elementwise_fma(w0[k], f2{x[k].x, x[k].y}, a0);
        a1 = __builtin_elementwise_fma(w1[k], f2{x[k].z, x[k].w}, a1);
    }
    return (a0.x + a0.y) + (a1.x + a1.y);
}

// Where the rows of a launch start: the nibble and pair planes of up to three matrices as scalar integers + distances, virtual bases for MAP_BLOCK
// (k_gemv_q8s' scheme).  Rows beyond the workgroup's range are redirected to the activation vector: its 4K bytes cover a nibble row (K / 2) and a
// pair row (K / 4).
template <int MAP>
struct Q41Rows {
    uint64_t q0, p0, dq1, dp1, e1q, e2q, e1p, e2p, qv_wg, pv_wg, nq, np, xdummy, qrow, prow;
    uint32_t rpm, bnd, r1;
    bool one_mat;
    __device__ __forceinline__ Q41Rows(const float* const (&w)[3], const float* const (&ws)[3], const float* x, uint32_t K, uint32_t rpm_, uint32_t r0, uint32_t r1_) {
        q0 = (uint64_t)sgpr_ptr(w[0]); p0 = (uint64_t)sgpr_ptr(ws[0]);
        dq1 = MAP == MAP_SINGLE ? 0 : (uint64_t)sgpr_ptr(w[1]) - q0; dp1 = MAP == MAP_SINGLE ? 0 : (uint64_t)sgpr_ptr(ws[1]) - p0;
        const uint64_t dq2 = MAP == MAP_BLOCK ? (uint64_t)sgpr_ptr(w[2]) - q0 - dq1 : 0, dp2 = MAP == MAP_BLOCK ? (uint64_t)sgpr_ptr(ws[2]) - p0 - dp1 : 0;
        xdummy = (uint64_t)sgpr_ptr(x);
        rpm = rpm_; r1 = r1_;
        qrow = (uint64_t)(K >> 1); prow = (uint64_t)(K >> 5) * 8u;
        e1q = dq1 - (uint64_t)rpm * qrow; e2q = dq2 - (uint64_t)rpm * qrow; e1p = dp1 - (uint64_t)rpm * prow; e2p = dp2 - (uint64_t)rpm * prow;
        const uint32_t mlo = (r0 >= rpm ? 1u : 0u) + (r0 >= 2u * rpm ? 1u : 0u), mhi = (r1 - 1u >= rpm ? 1u : 0u) + (r1 - 1u >= 2u * rpm ? 1u : 0u);
        one_mat = mhi - mlo <= 1u;
        qv_wg = q0 + (mlo >= 1u ? e1q : 0) + (mlo == 2u ? e2q : 0); pv_wg = p0 + (mlo >= 1u ? e1p : 0) + (mlo == 2u ? e2p : 0);
        bnd = (mlo + 1u) * rpm;
        nq = (mlo == 0u ? e1q : 0) + (mlo == 1u ? e2q : 0); np = (mlo == 0u ? e1p : 0) + (mlo == 1u ? e2p : 0);
    }
    // the two plane addresses of weight row `row` (scalar conditions: s_cselect on the addresses, no exec masking)
    __device__ __forceinline__ void at(uint32_t row, uint64_t* qb, uint64_t* pb) const {
        *qb = xdummy; *pb = xdummy;
        if (row >= r1) return;
        if (MAP == MAP_BLOCK) {
            uint64_t bq = qv_wg + (row >= bnd ? nq : 0), bp = pv_wg + (row >= bnd ? np : 0);
            if (!one_mat) {
                bq = q0 + (row >= rpm ? e1q : 0) + (row >= 2u * rpm ? e2q : 0);
                bp = p0 + (row >= rpm ? e1p : 0) + (row >= 2u * rpm ? e2p : 0);
            }
            *qb = bq + (uint64_t)row * qrow;
            *pb = bp + (uint64_t)row * prow;
        } else {
            uint32_t m = 0, r = row;
            if (MAP == MAP_PAIR) { m = row & 1u; r = row >> 1; }
            *qb = q0 + (m >= 1u ? dq1 : 0) + (uint64_t)r * qrow;
            *pb = p0 + (m >= 1u ? dp1 : 0) + (uint64_t)r * prow;
        }
    }
};

// U weight rows of a row group into one register set: per slot an 8-byte non-temporal nibble load and the 8-byte (d, m) load of its block
template <int U, int KI, int G, int MAP>
__device__ __forceinline__ void fetch_q41(const Q41Rows<MAP>& R, const uint32_t (&qoff)[KI], const uint32_t (&poff)[KI], u2 (&wd)[U][KI], f2 (&pd)[U][KI], uint32_t row_base) {
    typedef const u2 __attribute__((address_space(1))) gu2;
    typedef const f2 __attribute__((address_space(1))) gf2;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint64_t qb, pb;
        R.at(row_base + G * u, &qb, &pb);
#pragma unroll
        for (int j = 0; j < KI; ++j) {
            wd[u][j] = __builtin_nontemporal_load((gu2*)(qb + qoff[j]));
            pd[u][j] = *(gf2*)(pb + poff[j]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// k_gemv_q41s — the one-row decode stream: k_gemv_q4s' lane map and launch forms (slot j of lane tr holds the 16 weights at column 16 (tr + j TPR)),
// every epilogue and the RMSNorm prologue; per slot the sum of 16 w' x products, the slot sums added in j order, then the wave and workgroup sums.
// ---------------------------------------------------------------------------------------------------
template <int KI, int U, int TPR, int PRO, int EPI, int MAP, int TH = 1024>
__global__ __launch_bounds__(TH) void k_gemv_q41s(const GemvArgs a) {
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
    const Q41Rows<MAP> R(a.w, a.ws, a.x, K, a.rows_per_mat, r0, r1);
    const uint32_t fin = (EPI == EPI_STORE || EPI == EPI_RESID) ? (uint32_t)tid : 2u * (uint32_t)tid;
    float resid_pre;
    double2 cs_pre;
    uint32_t past_pre;
    gemv_prefetch_fin<EPI>(a, r0, r1, fin, &resid_pre, &cs_pre, &past_pre);
    f4 xr[KI][4];
    bool act[KI];
    uint32_t qoff[KI], poff[KI];
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        const uint32_t c = tr + j * TPR;
        act[j] = c < K16;
        qoff[j] = act[j] ? c * 8u : 0u;
        poff[j] = act[j] ? (c >> 1) * 8u : 0u;
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
    u2 wA[U][KI], wB[U][KI];
    f2 pA[U][KI], pB[U][KI];
    fetch_q41<U, KI, G>(R, qoff, poff, wA, pA, r0 + grp);   // slot u of this group holds row rb + G*u
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

    auto consume = [&](const u2 (&wd)[U][KI], const f2 (&pd)[U][KI], uint32_t rb) {
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                f2 w0[4], w1[4];
                unpack16_q41(wd[u][j], pd[u][j], w0, w1);
                s = __fadd_rn(s, dot16_w(w0, w1, xr[j]));
            }
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
        fetch_q41<U, KI, G>(R, qoff, poff, wB, pB, rb + STEP);
        consume(wA, pA, rb);
        fetch_q41<U, KI, G>(R, qoff, poff, wA, pA, rb + 2 * STEP);
        consume(wB, pB, rb + STEP);   // rows >= r1: loaded from the dummy, results dropped by the row test
    }
    __syncthreads();
    gemv_finish<EPI, NWR>(a, red, r0, r1, fin, resid_pre, cs_pre, past_pre);
}

// ---------------------------------------------------------------------------------------------------
// k_gemv_q41_rows — NC activation rows on one weight pass: the 16 nibbles of a load are unpacked and dequantised ONCE, and the 16 w' go into every
// activation row's pair of packed accumulators; per activation row the arithmetic and its order are k_gemv_q41s', so row i of a pass equals the
// one-row step bit for bit (the lossless speculative routes rest on that).
// ---------------------------------------------------------------------------------------------------
template <int KI, int U, int TPR, int TH, int NC, int PRO, int EPI, int MAP>
__global__ __launch_bounds__(TH) void k_gemv_q41_rows(const GemvRowsArgs a) {
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
    const Q41Rows<MAP> R(a.w, a.ws, a.x, K, a.rows_per_mat, r0, r1);
    bool act[KI];
    uint32_t qoff[KI], poff[KI];
    f4 xr[NC][KI][4];
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        const uint32_t ch = (uint32_t)tr + (uint32_t)j * TPR;
        act[j] = ch < K16;
        qoff[j] = act[j] ? ch * 8u : 0u;
        poff[j] = act[j] ? (ch >> 1) * 8u : 0u;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float* xc = a.x + (size_t)((uint32_t)c < a.n ? c : 0) * a.ldx;
#pragma unroll
            for (int k = 0; k < 4; ++k) xr[c][j][k] = act[j] ? ((const f4*)xc)[ch * 4 + k] : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
    u2 wA[U][KI], wB[U][KI];
    f2 pA[U][KI], pB[U][KI];
    fetch_q41<U, KI, G>(R, qoff, poff, wA, pA, r0 + grp);

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

    auto consume = [&](const u2 (&wd)[U][KI], const f2 (&pd)[U][KI], uint32_t rb) {
        float acc[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[u][c] = 0.f;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                f2 w0[4], w1[4];      // the 16 w' of the chunk, formed once for all activation rows
                unpack16_q41(wd[u][j], pd[u][j], w0, w1);
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[u][c] = __fadd_rn(acc[u][c], dot16_w(w0, w1, xr[c][j]));
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
        fetch_q41<U, KI, G>(R, qoff, poff, wB, pB, rb + STEP);
        consume(wA, pA, rb);
        fetch_q41<U, KI, G>(R, qoff, poff, wA, pA, rb + 2 * STEP);
        consume(wB, pB, rb + STEP);   // rows >= r1: loaded from the dummy, results dropped by the row test
    }
    __syncthreads();
    // the epilogues of k_gemv_q4_rows (= k_gemv_q8_rows'), per activation row what gemv_finish does for the one row
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
// k_expand_q41 — a nibble plane of n8 8-byte units and its pair plane -> the fp32 matrix of the w' (64 bytes per unit, four 16-byte stores): the image
// the fp32 schedule runs over, and the matrices of the expanded twin.  Unit i belongs to block i / 2.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_expand_q41(const u2* __restrict__ nib, const f2* __restrict__ pairs, f4* __restrict__ dst, uint64_t n8) {
    uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (; i < n8; i += stride) {
        f2 w0[4], w1[4];
        unpack16_q41(nib[i], pairs[i >> 1], w0, w1);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[i * 4 + k] = f4{w0[k].x, w0[k].y, w1[k].x, w1[k].y};
    }
}

// Quantiser: one thread per block of 32 weights of an fp32 matrix [rows][K] -> planes (k_quantize_q4's shape; the rule at the top of the file).
__global__ __launch_bounds__(256) void k_quantize_q41(const float* __restrict__ src, unsigned char* __restrict__ q, f2* __restrict__ pairs, uint64_t nblocks) {
    uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (; b < nblocks; b += stride) {
        f4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = ((const f4*)src)[b * 8 + i];
        float lo = v[0].x, hi = v[0].x;
        bool nonfinite = false;   // a NaN or an infinity in the block: d = m = NaN, nibbles 0 (d > 0 is false below)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float f[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo = fminf(lo, f[k]);
                hi = fmaxf(hi, f[k]);
                nonfinite |= (__builtin_bit_cast(uint32_t, f[k]) & 0x7f800000u) == 0x7f800000u;
            }
        }
        const float span = __fsub_rn(hi, lo);
        nonfinite |= (__builtin_bit_cast(uint32_t, span) & 0x7f800000u) == 0x7f800000u;   // finite weights whose max - min overflows: no finite d exists
        const float m = nonfinite ? __builtin_nanf("") : lo;
        const float d = nonfinite ? __builtin_nanf("") : __fdiv_rn(span, 15.0f);
        unsigned int packed[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // eight weights = four bytes: element 2j in the low nibble of byte j, 2j + 1 in the high one
            const float f[8] = {v[2 * i].x, v[2 * i].y, v[2 * i].z, v[2 * i].w, v[2 * i + 1].x, v[2 * i + 1].y, v[2 * i + 1].z, v[2 * i + 1].w};
            unsigned int p = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                float t = d > 0.f ? rintf(__fdiv_rn(__fsub_rn(f[k], m), d)) : 0.f;
                t = fminf(fmaxf(t, 0.f), 15.f);
                p |= (unsigned)(int)t << (4 * k);
            }
            packed[i] = p;
        }
        *(u4*)(q + b * 16) = u4{packed[0], packed[1], packed[2], packed[3]};
        pairs[b] = f2{d, m};
    }
}

// Registration from the 24-byte interchange blocks { float d; float m; uint8 qs[16] } -> planes: every bit as it is.
__global__ __launch_bounds__(256) void k_q41_deinterleave(const unsigned int* __restrict__ blocks, unsigned char* __restrict__ q, u2* __restrict__ pairs, uint64_t nblocks) {
    uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (; b < nblocks; b += stride) {
        const unsigned int* s = blocks + b * 6;
        pairs[b] = u2{s[0], s[1]};
        *(u4*)(q + b * 16) = u4{s[2], s[3], s[4], s[5]};
    }
}

}  // namespace lh
