// lag_index.hpp -- index arithmetic of the lagging single-table products (kernels_lag.hip, the class epilogue of round 1 in
// kernels_big.hip).  Plain constexpr integer code: it compiles for the device and, unchanged, for the host
// (tests/cpp/test_lag_index.cpp checks every map against brute force).
//
// A table that only single-table products name contributes to a round message nothing but the sums of its even and of its odd entries.
// With C[c] = sum of T[i] over i = c (mod 2^m) -- T with its high nv - m variables summed out -- binding C round by round gives the same
// two sums as binding T, so T itself can lag: round 1 leaves C behind, rounds 2 .. m bind C alone (2^m entries, one block), and one pass
// (k_fix_deep) binds T with every challenge it missed before the first round that needs the table again.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SC_LAG_FN __host__ __device__ constexpr
#else
#define SC_LAG_FN constexpr
#endif

namespace scd {

constexpr int kLagMaxSkip = 4;               // rounds a table may lag (policy "lag_single")
constexpr int kLagMaxLevels = kLagMaxSkip + 1; // binds of one k_fix_deep pass
constexpr int kLagMaxM = kLagMaxSkip + 1;    // log2 of the largest class table
constexpr int kLagMaxClasses = 1 << kLagMaxM;

// ---- round 1: which class a lane's running sums belong to ----
// Lane tid of a 256-thread block walks pairs b = block * 256 + tid + i * stride, stride a multiple of 256: b mod 2^(m-1) = tid mod 2^(m-1)
// for m - 1 <= 8, so every `lo` (entry 2b) of the lane is in class 2 (tid mod 2^(m-1)) and every `hi` in that class + 1.
SC_LAG_FN uint32_t lag_class_lanes(int m) { return 1u << (m - 1); } // lanes with distinct classes; shuffle offsets 32 .. this one fold a wavefront
SC_LAG_FN uint32_t lag_class_lo(uint32_t tid, int m) { return 2u * (tid & (lag_class_lanes(m) - 1u)); }
SC_LAG_FN uint32_t lag_class_hi(uint32_t tid, int m) { return lag_class_lo(tid, m) + 1u; }
SC_LAG_FN uint32_t lag_class_of_entry(uint64_t entry, int m) { return (uint32_t)(entry & ((1u << m) - 1u)); }

// ---- k_fix_deep: a lane reads entries 4g .. 4g+3 (128 contiguous bytes) and binds levels 1 and 2 itself: it then holds entry g of the
// table bound twice.  Every further level pairs it with the lane lag_deep_xor(level) away.  So that no lane idles in those levels, a lane
// walks lag_deep_batch(levels) grid-stride iterations at once (slots 0 .. batch - 1, iteration i at g + i * stride, stride a multiple of
// 256) and every level halves its slots: of slots i and i + half, the lane whose lag_deep_bit is 0 finishes slot i -- it holds the
// pair's even entry and receives the odd one --, its partner slot i + half.  After the last level the lane holds one entry, of iteration
// lag_deep_iter(tid, levels): entry lag_deep_entry(g of that iteration, levels) of the bound table ----
SC_LAG_FN int lag_deep_batch(int levels) { return levels <= 2 ? 1 : 1 << (levels - 2); }
SC_LAG_FN uint32_t lag_deep_xor(int level) { return 1u << (level - 3); }                                 // level >= 3
SC_LAG_FN uint32_t lag_deep_bit(uint32_t tid, int level) { return (tid >> (level - 3)) & 1u; }            // level >= 3
SC_LAG_FN uint32_t lag_deep_iter(uint32_t tid, int levels) { // the low levels - 2 bits of the lane, most significant first
    uint32_t it = 0;
    for (int level = 3; level <= levels; ++level) it |= lag_deep_bit(tid, level) << (levels - level);
    return it;
}
SC_LAG_FN uint64_t lag_deep_entry(uint64_t g, int levels) { return levels == 1 ? 2 * g : g >> (levels - 2); } // (levels == 1: entries 2g and 2g + 1)

// position (in 16-byte units) of half `half` of entry `entry` in a table of the internal F29 format: fe_device.hpp's f29_chunk
SC_LAG_FN uint64_t lag_f29_chunk(uint64_t entry, int half) {
    return (entry >> 7) * 256 + (uint64_t)(2 * (int)(entry & 1) + half) * 64 + ((((entry >> 1) & 63) >> 1) | (((entry >> 1) & 1) << 5));
}

// ---- the class work area of one lagging product (device memory, 32-byte elements) ----
// [0, 2^m * grid): round 1's class partials, class-major; then two class tables of 2^m entries each (ping-pong between rounds)
SC_LAG_FN uint64_t lag_area_partials(int m, uint32_t grid) { return ((uint64_t)grid << m); }
SC_LAG_FN uint64_t lag_area_elems(int m, uint32_t grid) { return lag_area_partials(m, grid) + 2 * (1ull << m); }

} // namespace scd
