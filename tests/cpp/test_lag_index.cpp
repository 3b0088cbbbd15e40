// test_lag_index.cpp -- sumcheck_amd/csrc/lag_index.hpp on the host, against brute force: which class a lane's running sums of round 1
// belong to (and the class epilogue's shuffle tree and LDS combine, restated on integers), which entry of the bound table a lane of
// k_fix_deep ends up with and where it stores it.  Stand-alone; built with -fsanitize=address,undefined by tests/test_lag_index_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lag_index.hpp"

using namespace scd;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            if (g_fail++ < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                     \
    } while (0)

static const int kGrids[] = {192, 256, 341, 384, 512, 768, 1024}; // blocks per row of the merged round-1 launch (protocol.hip: split_grid)
constexpr int kBlock = 256;

static uint64_t value_of(uint64_t i) { return (i * 0x9e3779b97f4a7c15ull) >> 20; } // sums of < 2^22 of these stay below 2^64

// round 1's class epilogue on integers: per-lane sums of lo and hi, shuffle offsets 32 .. lag_class_lanes(m), waves combined per class
static void class_epilogue(int grid, int m, int iters) {
    const uint64_t stride = (uint64_t)grid * kBlock, n_pairs = stride * iters;
    std::vector<uint64_t> want(1u << m, 0), got(1u << m, 0);
    for (uint64_t e = 0; e < 2 * n_pairs; ++e) want[lag_class_of_entry(e, m)] += value_of(e);
    for (int blk = 0; blk < grid; ++blk) {
        uint64_t lo[kBlock] = {}, hi[kBlock] = {};
        for (int tid = 0; tid < kBlock; ++tid)
            for (uint64_t b = (uint64_t)blk * kBlock + tid; b < n_pairs; b += stride) {
                CHECK(lag_class_of_entry(2 * b, m) == lag_class_lo(tid, m));
                CHECK(lag_class_of_entry(2 * b + 1, m) == lag_class_hi(tid, m));
                lo[tid] += value_of(2 * b);
                hi[tid] += value_of(2 * b + 1);
            }
        const int lanes = (int)lag_class_lanes(m);
        std::vector<uint64_t> x((size_t)4 << m, 0); // [wave][class]
        for (int wave = 0; wave < kBlock / 64; ++wave) {
            uint64_t *l = lo + 64 * wave, *h = hi + 64 * wave;
            for (int off = 32; off >= lanes; off >>= 1) // shfl_down: lane i takes lane i + off (its own value past the wavefront's end)
                for (int i = 0; i < 64; ++i) {
                    l[i] += i + off < 64 ? l[i + off] : l[i];
                    h[i] += i + off < 64 ? h[i + off] : h[i];
                }
            for (int lane = 0; lane < lanes && lane < 64; ++lane) {
                x[((size_t)wave << m) + lag_class_lo(lane, m)] = l[lane];
                x[((size_t)wave << m) + lag_class_hi(lane, m)] = h[lane];
            }
        }
        for (int c = 0; c < (1 << m); ++c)
            for (int wave = 0; wave < kBlock / 64; ++wave) got[c] += x[((size_t)wave << m) + c];
    }
    for (int c = 0; c < (1 << m); ++c) CHECK(got[c] == want[c]);
}

// k_fix_deep on a table of indices: an entry of the table bound l times stands for 2^l consecutive original entries
struct Range {
    uint64_t first, count;
};
static Range bind(const Range &lo, const Range &hi) {
    CHECK(lo.first + lo.count == hi.first && lo.count == hi.count && lo.first % (2 * lo.count) == 0);
    return Range{lo.first, 2 * lo.count};
}
static void fix_deep(int grid, int levels, uint64_t n_groups) {
    const uint64_t n_out = (4 * n_groups) >> levels, stride = (uint64_t)grid * kBlock;
    const int n = lag_deep_batch(levels);
    CHECK(n_groups % (n * stride) == 0); // (the launcher's grid: a power of two)
    std::vector<int> written(n_out, 0);
    std::vector<int> chunk_used(2 * n_out, 0);
    for (uint64_t base = 0; base < n_groups; base += 64) { // a wavefront's first iteration: 64 consecutive lanes, aligned
        if ((base / stride) % n != 0) continue;            // (iterations 1 .. n - 1 of a batch belong to the step that started at iteration 0)
        std::vector<Range> v((size_t)64 * n);              // [lane][slot]
        for (int i = 0; i < 64; ++i)
            for (int s = 0; s < n; ++s) {
                const uint64_t g = base + i + s * stride;
                const Range a0 = bind(Range{4 * g, 1}, Range{4 * g + 1, 1}), a1 = bind(Range{4 * g + 2, 1}, Range{4 * g + 3, 1});
                if (levels == 1) {
                    const uint64_t e = lag_deep_entry(g, 1);
                    CHECK(a0.first == 2 * e && a1.first == 2 * (e + 1));
                    CHECK(e + 1 < n_out);
                    if (e + 1 < n_out) ++written[e], ++written[e + 1];
                    continue;
                }
                v[(size_t)i * n + s] = bind(a0, a1);
            }
        if (levels == 1) continue;
        for (int level = 3; level <= levels; ++level) {
            const int half = n >> (level - 2);
            std::vector<Range> got((size_t)64 * half);
            for (int i = 0; i < 64; ++i)
                for (int s = 0; s < half; ++s) { // shfl_xor: lane i receives what lane i ^ xor sends
                    const int src = i ^ (int)lag_deep_xor(level);
                    const bool src_odd = lag_deep_bit((uint32_t)((base + src) % kBlock), level) != 0;
                    got[(size_t)i * half + s] = src_odd ? v[(size_t)src * n + s] : v[(size_t)src * n + s + half];
                }
            for (int i = 0; i < 64; ++i)
                for (int s = 0; s < half; ++s) {
                    const bool odd = lag_deep_bit((uint32_t)((base + i) % kBlock), level) != 0;
                    v[(size_t)i * n + s] = odd ? bind(got[(size_t)i * half + s], v[(size_t)i * n + s + half]) : bind(v[(size_t)i * n + s], got[(size_t)i * half + s]);
                }
        }
        for (int i = 0; i < 64; ++i) {
            const uint64_t g = base + i + lag_deep_iter((uint32_t)((base + i) % kBlock), levels) * stride, e = lag_deep_entry(g, levels);
            CHECK(v[(size_t)i * n].first == (e << levels) && v[(size_t)i * n].count == (1ull << levels));
            CHECK(e < n_out);
            if (e < n_out) ++written[e];
        }
    }
    for (uint64_t e = 0; e < n_out; ++e) {
        CHECK(written[e] == 1);
        for (int half = 0; half < 2; ++half) { // fe_device.hpp: byte offset (e >> 7) * 4096 + (2 * (e & 1) + half) * 1024 + col(q) * 16, q = e >> 1
            const uint64_t q = e >> 1, col = ((q & 63) >> 1) | ((q & 1) << 5);
            const uint64_t bytes = (e >> 7) * 4096 + (2 * (e & 1) + half) * 1024 + col * 16;
            const uint64_t c = lag_f29_chunk(e, half);
            CHECK(c * 16 == bytes);
            CHECK(c < 2 * n_out);
            if (c < 2 * n_out) ++chunk_used[c];
        }
    }
    for (uint64_t c = 0; c < 2 * n_out; ++c) CHECK(chunk_used[c] == 1);
}

int main() {
    for (int grid : kGrids)
        for (int j = 3; j <= 6; ++j) {
            class_epilogue(grid, j - 1, 2);
        }
    // k_fix_deep's own grid: n_groups / (256 x batch) blocks, at most 1024 -- the smallest tables of a big round (2^16 entries) and larger ones
    for (int levels = 1; levels <= kLagMaxLevels; ++levels)
        for (int log_groups = 14; log_groups <= 19; ++log_groups) {
            const uint64_t n_groups = 1ull << log_groups, g = n_groups / ((uint64_t)kBlock * lag_deep_batch(levels));
            fix_deep((int)(g < 1024 ? g : 1024), levels, n_groups);
        }
    CHECK(lag_area_elems(kLagMaxM, 1024) == 32 * 1024 + 64);
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("ALL TESTS PASSED\n");
    return 0;
}
