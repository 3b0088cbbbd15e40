// f29_pack.hpp -- the 32-byte packed form of the internal table format F29, and the range rule that makes it possible.
// Plain integer code on arrays: it compiles for the device (fe_device.hpp wraps it) and, unchanged, for the host
// (tests/cpp/test_f29_pack.cpp checks it against a big-integer restatement; tests/f29_pack_model.py is the same in Python).
//
// A bound-table entry is nine 29-bit limbs, value = sum l_i 2^(29 i), limbs 0..7 in [0, 2^29) and limb 8 SIGNED.  Packed, it is
// that value as a 256-bit two's-complement integer in eight 32-bit words (bit-contiguous): limb 8 contributes bits 232..255, so
// it must lie in [-2^23, 2^23), i.e. the value in [-2^255, 2^255) -- about +-1.104 p.  A canonical value packs to its own eight
// words: unpacking is fe_from_fr with an ARITHMETIC shift for limb 8.
//   unpack: limb i = ((word i-1 >> (32 - 3i)) | (word i << 3i)) & mask   (one funnel shift and one and, i = 1..7),
//           limb 0 = word 0 & mask, limb 8 = (int32) word 7 >> 8                                   -- 16 instructions
//   pack:   word k = (limb k >> 3k) | (limb k+1 << (29 - 3k))            (a shift and a shift-or, k = 1..7; k = 0 one shift-or)
//                                                                                                   -- 15 instructions
// The alternative that keeps the limbs in place and spreads limb 8 over the three spare bits of every word needs the same 15
// instructions to pack but 23 to unpack (eight ands, and limb 8 reassembled from eight 3-bit fields), and a canonical value
// would not be its own packed form.
//
// Range rule (f29_settle).  A bind computes v = e0 + t with t = r (e1 - e0) from fe_mul_bind, t in (-p - 2^230, 2^230): left
// alone the entries sink by up to p a round.  If v reads below -p / 2, p is added once -- the same field element, nearer zero.
// The test reads limb 8 of the un-normalised sum alone: limbs 0..7 of e0 and of t are each in [0, 2^29), so v lies in
// [l8 2^232, (l8 + 2) 2^232).  With H = floor(p / 2^233) (p / 2 = (H + 0.66) 2^232) the rule adds p where l8 < -(H + 1):
//   kept:  l8 >= -H - 1, v >= -(H + 1) 2^232 > -p / 2 - 2^232;      raised:  l8 <= -H - 2, v < -H 2^232, v + p < p / 2 + 2^232,
// i.e. the decision falls within 2^232 of -p / 2 on either side.  For sources in (-A, B) the result lies in
// (-max(p / 2 + 2^232, A + 2^230), max(B + 2^230, p / 2 + 2^232)); from canonical tables (A = 0, B = p), after k binds:
// (-p / 2 - 2^232 - (k - 1) 2^230, p + k 2^230), inside +-2^255 = +-1.104 p with 2^251 to spare for any k <= 40.
// The addition rides in the carry chain that brings limbs 0..7 into [0, 2^29) exactly, which the packed fields need anyway.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SC_F29_FN __host__ __device__ __forceinline__
#else
#define SC_F29_FN inline
#endif

namespace scd {

constexpr int32_t kF29Mask = 0x1fffffff;
constexpr int32_t kF29RuleTop = (0x0073eda7 >> 1) + 1; // H + 1, H = floor(p / 2^233): p is added where limb 8 reads below -(H + 1)

// p in radix 2^29
SC_F29_FN constexpr int32_t f29_p_limb(int i) {
    return i == 0 ? 0x00000001 : i == 1 ? 0x1ffffff8 : i == 2 ? 0x1f96ffbf : i == 3 ? 0x1b4805ff : i == 4 ? 0x1d80553b
         : i == 5 ? 0x0c0404d0 : i == 6 ? 0x1520cce7 : i == 7 ? 0x0a6533af : 0x0073eda7;
}

// eight words (a 256-bit two's-complement value) -> nine limbs, limbs 0..7 in [0, 2^29), limb 8 in [-2^23, 2^23)
SC_F29_FN void f29_unpack(const uint32_t (&w)[8], int32_t (&l)[9]) {
    l[0] = (int32_t)(w[0] & (uint32_t)kF29Mask);
#pragma unroll
    for (int i = 1; i < 8; ++i) l[i] = (int32_t)(((w[i - 1] >> (32 - 3 * i)) | (w[i] << (3 * i))) & (uint32_t)kF29Mask);
    l[8] = (int32_t)w[7] >> 8; // arithmetic: the sign of the value
}

// the inverse; limbs 0..7 MUST be in [0, 2^29) and limb 8 in [-2^23, 2^23) (f29_settle's output)
SC_F29_FN void f29_pack(const int32_t (&l)[9], uint32_t (&w)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = ((uint32_t)l[k] >> (3 * k)) | ((uint32_t)l[k + 1] << (29 - 3 * k));
}

// range rule + exact digits, in place: adds p where limb 8 reads below -kF29RuleTop (the value: about -p / 2), then propagates carries (limbs 0..7 into
// [0, 2^29), limb 8 takes the signed rest).  Input limbs 0..7 anywhere in [0, 2^30) (a lazy sum of two normalised elements).
SC_F29_FN void f29_settle(int32_t (&l)[9]) {
    const int32_t add = l[8] < -kF29RuleTop ? -1 : 0;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int32_t t = l[i] + (f29_p_limb(i) & add) + c;
        l[i] = t & kF29Mask;
        c = t >> 29; // arithmetic
    }
    l[8] = l[8] + (f29_p_limb(8) & add) + c;
}

} // namespace scd
