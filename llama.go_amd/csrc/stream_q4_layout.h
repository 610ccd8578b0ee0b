// csrc/stream_q4_layout.h — where a nibble sits in the weight part of a ring image of k_stream_q4b (kernels_stream_q4b.h), and how four bytes of it become
// the bf16 operand of the MFMA: pure functions (no HIP), called by the kernel's DMA side AND by its reading side, exported as lh_stream_q4_image_off /
// lh_stream_q4_read_off / lh_stream_q4_operand and unit-tested without a GPU (tests/test_q4_stream_cpu.py, tests/stream_q4_layout_main.cpp).
//
// Layout.  Image row r (weight row r & 15 of tile slot r >> 4) holds the kc / 2 bytes of the chunk's nibbles: kc / 32 granules of 16 bytes, and granule g
// IS quant block g of the chunk (32 columns; byte b of the row = column 2 b in the low nibble, 2 b + 1 in the high one: kernels_q4.h).  Row pitch 64 / 128 /
// 256 bytes for kc = 128 / 256 / 512, dense: an LDS-DMA instruction writes lane i at base + 16 i, so no row can be padded and the permutation goes on the
// SOURCE address.  Granule g of row r is stored at position g ^ swz(r): an involution in g for a fixed row, so the DMA side (which picks the source granule
// for the position its lane lands on) and the reader call the same function.
// The operand read of one quant block kb is a ds_read_b32 per lane (r16, slot): dword `slot` of granule kb of each of 16 rows, 256 bytes.  A bank line is
// 256 bytes = 16 granules, so row r starts at granule (r * pitch / 16) % 16 of the line and the 16 rows must land on 16 different granules of it:
//   64-byte rows (kc = 128):  row r starts at 4 (r & 3); rows r, r + 4, r + 8, r + 12 alias  -> swz = (r >> 2) & 3: granule 4 (r & 3) + (kb ^ (r >> 2))
//   128-byte rows (kc = 256): row r starts at 8 (r & 1); every second row aliases           -> swz = (r >> 1) & 7: granule 8 (r & 1) + (kb ^ (r >> 1))
//   256-byte rows (kc = 512): every row starts at 0                                          -> swz = r & 15
// - the sixteen (r & 3, r >> 2) / (r & 1, r >> 1) / r are all different, so with bank = (address / 4) % 64 the 64 lanes touch the 64 banks once each.
//
// Conversion.  stream_q4_operand turns the dword of eight nibbles n0..n7 (nibble k = bits 4 k .. 4 k + 3 = column k of the lane's eight) into the four dwords
// k_stream_q8b's conversion yields for the int8 quants n_k - 8: element k = the bf16 of (float)(n_k - 8), elements 2 j and 2 j + 1 packed low / high.
// No integer -> float conversion: the nibble is masked IN PLACE into the mantissa of a float whose exponent makes that mantissa bit worth 1 -
// bits = (v & (15 << s)) | ((150 - s) << 23) is the fp32 2^(23 - s) + n exactly (s = 0, 4, 8, 12, 16: the nibble stays below the exponent field; the upper
// four nibbles after one shift of the dword by 16) - and ONE exact subtraction of 2^(23 - s) + 8 leaves (float)(n - 8), whose high half is its bf16 (|n - 8| <= 8:
// four significant bits).  The -8 is applied to every weight, not moved out of the sum.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LH_STREAM_Q4_FN __host__ __device__ inline
#else
#define LH_STREAM_Q4_FN inline
#endif

namespace lh {

LH_STREAM_Q4_FN uint32_t stream_q4_granule_pos(uint32_t kc, uint32_t r, uint32_t g) {
    return kc == 128 ? g ^ ((r >> 2) & 3u) : (kc == 256 ? g ^ ((r >> 1) & 7u) : g ^ (r & 15u));
}
// byte offset, in the weight part of an image, of granule g (quant block g of the chunk) of image row r
LH_STREAM_Q4_FN uint32_t stream_q4_granule_off(uint32_t kc, uint32_t r, uint32_t g) { return r * (kc / 2u) + stream_q4_granule_pos(kc, r, g) * 16u; }
// byte offset of the 4 bytes MFMA lane (r16, slot) reads of tile slot t for quant block kb of the chunk: the nibbles of columns 32 kb + 8 slot .. + 7
LH_STREAM_Q4_FN uint32_t stream_q4_read_off(uint32_t kc, uint32_t t, uint32_t r16, uint32_t kb, uint32_t slot) {
    return stream_q4_granule_off(kc, t * 16u + r16, kb) + slot * 4u;
}

// fp32 bits of (float)(n - 8) for the nibble n at bits s .. s + 3 of v (s = 0, 4, 8, 12, 16)
template <int S>
LH_STREAM_Q4_FN uint32_t stream_q4_f32_bits(uint32_t v) {
    static_assert(S == 0 || S == 4 || S == 8 || S == 12 || S == 16, "the nibble must stay below the exponent field");
    const uint32_t b = (v & (15u << S)) | ((uint32_t)(150 - S) << 23);
    float f;
    memcpy(&f, &b, 4);
    f -= (float)(1u << (23 - S)) + 8.0f;
    uint32_t o;
    memcpy(&o, &f, 4);
    return o;
}
// the high halves of two fp32 (= their bf16 where the low halves are zero) in one dword, `even` low
LH_STREAM_Q4_FN uint32_t stream_q4_pack(uint32_t even, uint32_t odd) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(odd, even, 0x07060302u);
#else
    return (even >> 16) | (odd & 0xffff0000u);
#endif
}
#if defined(__HIP_DEVICE_COMPILE__)
// The same two steps as the instructions they are meant to be.  Left to itself the compiler splits (v & mask) | exponent into v_and_b32 + v_or_b32 with two
// literals (a VOP3 takes none) and subtracts with one v_add_f32 per element: 27 vector instructions per eight weights.  Spelled out - v_and_or_b32 with the
// mask in an SGPR and the exponent word in a VGPR, the subtraction as a two-wide vector so that it becomes v_pk_add_f32 - it is 1 shift + 8 + 4 + 4 packs = 17.
typedef float stream_q4_f2 __attribute__((ext_vector_type(2)));
template <int S0, int S1>
__device__ inline uint32_t stream_q4_pair(uint32_t v, uint32_t w) {
    uint32_t b0, b1;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(b0) : "v"(v), "s"(15u << S0), "v"((uint32_t)(150 - S0) << 23));
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(b1) : "v"(w), "s"(15u << S1), "v"((uint32_t)(150 - S1) << 23));
    stream_q4_f2 f = {__builtin_bit_cast(float, b0), __builtin_bit_cast(float, b1)};
    f -= stream_q4_f2{(float)(1u << (23 - S0)) + 8.0f, (float)(1u << (23 - S1)) + 8.0f};
    const float fe = f.x, fo = f.y;   // (scalars first: __builtin_bit_cast of a vector ELEMENT reads element 0 for both)
    return stream_q4_pack(__builtin_bit_cast(uint32_t, fe), __builtin_bit_cast(uint32_t, fo));
}
#else
template <int S0, int S1>
inline uint32_t stream_q4_pair(uint32_t v, uint32_t w) { return stream_q4_pack(stream_q4_f32_bits<S0>(v), stream_q4_f32_bits<S1>(w)); }
#endif
// eight nibbles -> the bf16x8 operand of their int8 expansion (out[j] = elements 2 j, 2 j + 1)
LH_STREAM_Q4_FN void stream_q4_operand(uint32_t v, uint32_t out[4]) {
    const uint32_t u = v >> 16;
    out[0] = stream_q4_pair<0, 4>(v, v);
    out[1] = stream_q4_pair<8, 12>(v, v);
    out[2] = stream_q4_pair<16, 4>(v, u);
    out[3] = stream_q4_pair<8, 12>(u, u);
}
}  // namespace lh
