// csrc/kernels_f16.h — f16 weight matrices kept f16 in HBM (dtype 1 = ml.TYPE_F16, ml.go:87): the decode weight stream for one and for 2..8
// activation rows, and the exact conversions between the two widths.
//
// Widening an IEEE half to fp32 is exact (every half, subnormals included, is an fp32 value), so a kernel that loads halves, widens them in
// registers and then does what the fp32 kernel does - the same lane -> column map, the same fmaf chain per lane, the same DPP wave sum, the same
// cross-wave order - produces the bits of the fp32 kernel over the widened matrix.  k_gemv_sa_h / k_gemv_rows_h are k_gemv_sa (kernels_llama.h) /
// k_gemv_rows (kernels_rows.h) with exactly that one change: slot j of thread tid loads the four HALVES at columns 4 (tid + j TH) .. + 3 of the row
// (an 8-byte non-temporal load, scalar row base + constant lane offset, row_bytes = 2 K) where the fp32 kernels load four floats.  Every product
// and sum stays fp32.  The number of rows in flight (U) is not part of the summation order, so the launch sites choose it for the halved rows.
// The prologue / epilogue code (rmsnorm_prologue, gemv_prefetch_fin, gemv_finish, gemv_row_base, wg_row_block) is the fp32 kernels' own.
#pragma once
#include "kernels_llama.h"
#include "kernels_rows.h"

namespace lh {

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ h4 ld_nt_h4(const h4* p) { return __builtin_nontemporal_load(p); }
// exact: v_cvt_f32_f16 with the kernel's default mode (f16 denormals kept)
__device__ __forceinline__ f4 widen4(h4 v) { return __builtin_convertvector(v, f4); }

template <int KI, int U, int TH, int PRO, int EPI, int MAP>
__global__ __launch_bounds__(TH) void k_gemv_sa_h(const GemvArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.x, a.hd, a.wg_r);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NW = TH / 64;
    double* sred = (double*)smem_raw;                // [NW]
    float* red = (float*)(smem_raw + NW * 8);        // [rows of this workgroup][NW] per-wave partial dot products
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t K4 = a.K >> 2;
    uint32_t r0, r1;
    wg_row_block(a.M, a.wg_q, a.wg_r, &r0, &r1);
    const char *w0 = (const char*)a.w[0], *w1 = (const char*)a.w[1], *w2 = (const char*)a.w[2];
    const char* xdummy = (const char*)a.x;           // K floats: a row of K halves is half its extent, every lane offset stays inside it
    const uint32_t rpm = a.rows_per_mat;
    const uint64_t row_bytes = (uint64_t)a.K * 2;

    const uint32_t fin = (EPI == EPI_STORE || EPI == EPI_RESID) ? (uint32_t)tid : 2u * (uint32_t)tid;
    float resid_pre;
    double2 cs_pre;
    uint32_t past_pre;
    gemv_prefetch_fin<EPI>(a, r0, r1, fin, &resid_pre, &cs_pre, &past_pre);
    f4 xr[KI];
    f4 gr[KI];
    bool act[KI];
    uint32_t loff[KI];
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        act[j] = (uint32_t)(tid + j * TH) < K4;
        loff[j] = act[j] ? (uint32_t)(tid + j * TH) * 8u : 0u;
        xr[j] = act[j] ? ((const f4*)a.x)[tid + j * TH] : f4{0.f, 0.f, 0.f, 0.f};
        if (PRO == PRO_RMSNORM) gr[j] = act[j] ? ((const f4*)a.gamma)[tid + j * TH] : f4{0.f, 0.f, 0.f, 0.f};
    }
    h4 w[U][KI];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const char* p = (r0 + u < r1) ? gemv_row_base<MAP>(w0, w1, w2, rpm, r0 + u, row_bytes) : xdummy;
#pragma unroll
        for (int j = 0; j < KI; ++j) w[u][j] = ld_nt_h4((const h4*)(p + loff[j]));
    }
    if (PRO == PRO_RMSNORM) rmsnorm_prologue<KI, TH>(xr, act, gr, a.K, sred);
    // inactive lanes (K not a multiple of 4*TH) multiply whatever they loaded by x = 0 - k_gemv_sa does the same; the sums agree as long as what they
    // loaded is finite, and a lane offset of 0 reads the row's first four weights (or the activation vector) in both
    for (uint32_t r = r0; r < r1; r += U) {
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t nr = r + U + u;
            const char* p = nr < r1 ? gemv_row_base<MAP>(w0, w1, w2, rpm, nr, row_bytes) : xdummy;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                const f4 c = widen4(w[u][j]);
                s = fmaf(c.x, xr[j].x, s);
                s = fmaf(c.y, xr[j].y, s);
                s = fmaf(c.z, xr[j].z, s);
                s = fmaf(c.w, xr[j].w, s);
                w[u][j] = ld_nt_h4((const h4*)(p + loff[j]));
            }
            acc[u] = s;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = wave_sum(acc[u]);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r + u < r1) red[(r - r0 + u) * NW + wave] = acc[u];
        }
    }
    __syncthreads();
    gemv_finish<EPI, NW>(a, red, r0, r1, fin, resid_pre, cs_pre, past_pre);
}

// k_gemv_rows over f16 weights: NC activation rows through the one-row kernel above; per activation row the arithmetic and its order are those of
// k_gemv_sa_h, hence of k_gemv_sa over the widened matrix.
template <int KI, int U, int TH, int NC, int PRO, int EPI, int MAP>
__global__ __launch_bounds__(TH) void k_gemv_rows_h(const GemvRowsArgs a) {
    LH_TOUCH_ARGS(a.w[0], a.x, a.rows, a.wg_q);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NW = TH / 64;
    double* sred = (double*)smem_raw;                       // [NC][NW]
    float* red = (float*)(smem_raw + NC * NW * 8);          // [weight rows of this workgroup][NC][NW] per-wave partial dot products
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t K4 = a.K >> 2;
    uint32_t r0, r1;
    wg_row_block(a.M, a.wg_q, a.wg_r, &r0, &r1);
    const char *w0 = (const char*)a.w[0], *w1 = (const char*)a.w[1], *w2 = (const char*)a.w[2];
    const char* xdummy = (const char*)a.x;                  // K floats: twice a row of K halves
    const uint32_t rpm = a.rows_per_mat;
    const uint64_t row_bytes = (uint64_t)a.K * 2;

    f4 xr[NC][KI];
    f4 gr[KI];
    bool act[KI];
    uint32_t loff[KI];
#pragma unroll
    for (int j = 0; j < KI; ++j) {
        act[j] = (uint32_t)(tid + j * TH) < K4;
        loff[j] = act[j] ? (uint32_t)(tid + j * TH) * 8u : 0u;
        if (PRO == PRO_RMSNORM) gr[j] = act[j] ? ((const f4*)a.gamma)[tid + j * TH] : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float* xc = a.x + (size_t)((uint32_t)c < a.n ? c : 0) * a.ldx;   // rows past n: a duplicate of row 0, results never stored
#pragma unroll
        for (int j = 0; j < KI; ++j) xr[c][j] = act[j] ? ((const f4*)xc)[tid + j * TH] : f4{0.f, 0.f, 0.f, 0.f};
    }
    h4 w[U][KI];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const char* p = (r0 + u < r1) ? gemv_row_base<MAP>(w0, w1, w2, rpm, r0 + u, row_bytes) : xdummy;
#pragma unroll
        for (int j = 0; j < KI; ++j) w[u][j] = ld_nt_h4((const h4*)(p + loff[j]));
    }
    if (PRO == PRO_RMSNORM) {   // k_gemv_rows' norm: per row the squares, the f64 order and the two roundings per element of rmsnorm_prologue
        double ss[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                if (act[j]) {
                    t += (double)__fmul_rn(xr[c][j].x, xr[c][j].x);
                    t += (double)__fmul_rn(xr[c][j].y, xr[c][j].y);
                    t += (double)__fmul_rn(xr[c][j].z, xr[c][j].z);
                    t += (double)__fmul_rn(xr[c][j].w, xr[c][j].w);
                }
            }
            ss[c] = t;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) ss[c] = wave_sum_f64(ss[c]);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) sred[c * NW + wave] = ss[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double tot = 0.0;
#pragma unroll
            for (int w2i = 0; w2i < NW; ++w2i) tot += sred[c * NW + w2i];
            const float scale = (float)(1.0 / sqrt(tot / (double)a.K + 1e-5));
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                if (act[j]) {
                    const f4 g = gr[j];
                    xr[c][j].x = __fmul_rn(g.x, __fmul_rn(xr[c][j].x, scale));
                    xr[c][j].y = __fmul_rn(g.y, __fmul_rn(xr[c][j].y, scale));
                    xr[c][j].z = __fmul_rn(g.z, __fmul_rn(xr[c][j].z, scale));
                    xr[c][j].w = __fmul_rn(g.w, __fmul_rn(xr[c][j].w, scale));
                }
            }
        }
    }
    for (uint32_t r = r0; r < r1; r += U) {
        float acc[U][NC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t nr = r + U + u;
            const char* p = nr < r1 ? gemv_row_base<MAP>(w0, w1, w2, rpm, nr, row_bytes) : xdummy;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[u][c] = 0.f;
#pragma unroll
            for (int j = 0; j < KI; ++j) {
                const f4 q = widen4(w[u][j]);       // widened once for all activation rows
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    float s = acc[u][c];
                    s = fmaf(q.x, xr[c][j].x, s);
                    s = fmaf(q.y, xr[c][j].y, s);
                    s = fmaf(q.z, xr[c][j].z, s);
                    s = fmaf(q.w, xr[c][j].w, s);
                    acc[u][c] = s;
                }
                w[u][j] = ld_nt_h4((const h4*)(p + loff[j]));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[u][c] = wave_sum(acc[u][c]);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (r + u < r1) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) red[((size_t)(r - r0 + u) * NC + c) * NW + wave] = acc[u][c];
                }
        }
    }
    __syncthreads();
    // epilogue: k_gemv_rows' (work item = weight row or pair x activation row; cross-wave sums in wave order)
    constexpr uint32_t PER = (EPI == EPI_STORE || EPI == EPI_RESID) ? 1u : 2u;
    const uint32_t nit = (r1 - r0 + PER - 1) / PER, nwork = nit * a.n;
    for (uint32_t wk = (uint32_t)tid; wk < nwork; wk += TH) {
        const uint32_t c = wk / nit, fin = (wk - c * nit) * PER;
        const uint32_t v = r0 + fin;
        const float* p0 = red + ((size_t)fin * NC + c) * NW;
        float s0 = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) s0 += p0[k];
        if (EPI == EPI_STORE) {
            a.y[(size_t)c * a.ldy + v] = s0;
        } else if (EPI == EPI_RESID) {
            a.y[(size_t)c * a.ldy + v] = __fadd_rn(s0, a.resid[(size_t)c * a.ldy + v]);
        } else {
            const float* p1 = p0 + (size_t)NC * NW;
            float s1 = 0.f;
#pragma unroll
            for (int k = 0; k < NW; ++k) s1 += p1[k];
            if (EPI == EPI_SILU_MUL) {
                a.y[(size_t)c * a.ldy + (v >> 1)] = __fmul_rn(silu_ref(s0), s1);
            } else {
                const uint32_t d = a.d;
                const uint32_t pos = a.rows ? a.rows[c].pos : a.past + c;
                float* kcb = a.rows ? a.rows[c].kc + a.kv_off : a.k_cache;
                float* vcb = a.rows ? a.rows[c].vc + a.kv_off : a.v_cache;
                if (v < 2 * d) {
                    const uint32_t e = v < d ? v : v - d;
                    const double2 cs = a.rope[(size_t)pos * (a.hd >> 1) + ((e % a.hd) >> 1)];
                    float o0, o1;
                    rope_rotate(s0, s1, cs, &o0, &o1);
                    float* dst = v < d ? a.q_out + (size_t)c * d + e : kcb + (size_t)pos * d + e;
                    dst[0] = o0;
                    dst[1] = o1;
                } else {
                    float* dst = vcb + (size_t)pos * d + (v - 2 * d);
                    dst[0] = s0;
                    dst[1] = s1;
                }
            }
        }
    }
}

// ---- conversions: plain grid-stride kernels, 16-byte accesses on the fp32 side (four elements per thread and step), a scalar tail ----
// exact widening (every half pattern; a NaN stays a NaN)
__global__ __launch_bounds__(256) void k_widen_f16(const _Float16* __restrict__ src, float* __restrict__ dst, uint64_t n) {
    const uint64_t n4 = n >> 2, stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) ((f4*)dst)[i] = widen4(((const h4*)src)[i]);
    for (uint64_t i = (n4 << 2) + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = (float)src[i];
}
// round to nearest even, overflow to +-inf, -0 kept (v_cvt_f16_f32 in the default rounding mode); *changed += elements whose value changed
__global__ __launch_bounds__(256) void k_narrow_f16(const float* __restrict__ src, _Float16* __restrict__ dst, uint64_t n, unsigned long long* changed) {
    const uint64_t n4 = n >> 2, stride = (uint64_t)gridDim.x * 256;
    uint32_t cnt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f4 v = ((const f4*)src)[i];
        const h4 h = __builtin_convertvector(v, h4);
        ((h4*)dst)[i] = h;
        const f4 b = widen4(h);
        cnt += (b.x != v.x && v.x == v.x) + (b.y != v.y && v.y == v.y) + (b.z != v.z && v.z == v.z) + (b.w != v.w && v.w == v.w);   // (a NaN stays a NaN: not counted)
    }
    for (uint64_t i = (n4 << 2) + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const _Float16 h = (_Float16)src[i];
        dst[i] = h;
        cnt += ((float)h != src[i] && src[i] == src[i]);
    }
    if (cnt) atomicAdd(changed, (unsigned long long)cnt);
}

}  // namespace lh
