// test_f29_pack.cpp -- the packed table format's host-compilable header (sumcheck_amd/csrc/f29_pack.hpp) against a straightforward
// big-integer restatement: the corners of the format and a few million random values through pack, unpack and the range rule.
// A stand-alone program (tests/test_f29_pack_host.py builds it with -fsanitize=address,undefined and runs it); CPU only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "f29_pack.hpp"

// ---- a 320-bit two's-complement integer, little-endian 64-bit words: add, shifted add of a small signed number, arithmetic shift -----------
struct Big {
    uint64_t w[5];
};
static Big big_from(int64_t v) {
    Big r;
    r.w[0] = (uint64_t)v;
    for (int i = 1; i < 5; ++i) r.w[i] = v < 0 ? ~0ULL : 0ULL;
    return r;
}
static Big big_add(const Big &a, const Big &b) {
    Big r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 5; ++i) {
        c += (unsigned __int128)a.w[i] + b.w[i];
        r.w[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
static Big big_neg(const Big &a) {
    Big r;
    for (int i = 0; i < 5; ++i) r.w[i] = ~a.w[i];
    return big_add(r, big_from(1));
}
static Big big_shl(const Big &a, int s) { // 0 <= s < 320
    Big r = {{0, 0, 0, 0, 0}};
    const int q = s / 64, o = s % 64;
    for (int i = 4; i >= q; --i) {
        r.w[i] = a.w[i - q] << o;
        if (o && i - q - 1 >= 0) r.w[i] |= a.w[i - q - 1] >> (64 - o);
    }
    return r;
}
static bool big_neg_p(const Big &a) { return a.w[4] >> 63; }
static Big big_sar(const Big &a, int s) {
    Big r;
    const uint64_t fill = big_neg_p(a) ? ~0ULL : 0ULL;
    const int q = s / 64, o = s % 64;
    for (int i = 0; i < 5; ++i) {
        const uint64_t lo = i + q < 5 ? a.w[i + q] : fill, hi = i + q + 1 < 5 ? a.w[i + q + 1] : fill;
        r.w[i] = o ? (lo >> o) | (hi << (64 - o)) : lo;
    }
    return r;
}
static bool big_eq(const Big &a, const Big &b) {
    for (int i = 0; i < 5; ++i)
        if (a.w[i] != b.w[i]) return false;
    return true;
}
static bool big_lt(const Big &a, const Big &b) { return big_neg_p(big_add(a, big_neg(b))); } // (no overflow: |values| < 2^270)

static Big value_of(const int32_t (&l)[9]) { // sum l_i 2^(29 i)
    Big v = big_from(0);
    for (int i = 0; i < 9; ++i) v = big_add(v, big_shl(big_from(l[i]), 29 * i));
    return v;
}
static void limbs_of(const Big &v, int32_t (&l)[9]) { // limbs 0..7 the digits, limb 8 the signed rest
    for (int i = 0; i < 8; ++i) l[i] = (int32_t)(big_sar(v, 29 * i).w[0] & 0x1fffffffu);
    l[8] = (int32_t)(int64_t)big_sar(v, 232).w[0];
}
static void words_of(const Big &v, uint32_t (&w)[8]) { // the low 256 bits
    for (int i = 0; i < 8; ++i) w[i] = (uint32_t)(v.w[i / 2] >> (32 * (i % 2)));
}
static Big from_words(const uint32_t (&w)[8]) { // 256-bit two's complement
    Big v = {{0, 0, 0, 0, 0}};
    for (int i = 0; i < 8; ++i) v.w[i / 2] |= (uint64_t)w[i] << (32 * (i % 2));
    v.w[4] = (w[7] >> 31) ? ~0ULL : 0ULL;
    return v;
}
static Big big_p() {
    int32_t pl[9];
    for (int i = 0; i < 9; ++i) pl[i] = scd::f29_p_limb(i);
    return value_of(pl);
}

static uint64_t rng_state = 0x5C20241008ULL;
static uint64_t rnd() { // SplitMix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

static long failures = 0;
#define CHECK(c, what)                                                         \
    do {                                                                       \
        if (!(c)) {                                                            \
            if (failures++ < 10) std::printf("FAIL line %d: %s\n", __LINE__, what); \
        }                                                                      \
    } while (0)

static void check_round_trip(const int32_t (&l)[9]) {
    const Big v = value_of(l);
    uint32_t w[8], want[8];
    scd::f29_pack(l, w);
    words_of(v, want);
    for (int i = 0; i < 8; ++i) CHECK(w[i] == want[i], "pack: the words are the value's two's-complement form");
    CHECK(big_eq(from_words(w), v), "packed value");
    int32_t back[9];
    scd::f29_unpack(w, back);
    for (int i = 0; i < 9; ++i) CHECK(back[i] == l[i], "unpack(pack(l)) == l");
}

static void check_settle(const int32_t (&l)[9], const Big &p) {
    const Big v = value_of(l);
    int32_t got[9], want[9];
    for (int i = 0; i < 9; ++i) got[i] = l[i];
    scd::f29_settle(got);
    const bool add = l[8] < -scd::kF29RuleTop;
    limbs_of(add ? big_add(v, p) : v, want);
    for (int i = 0; i < 9; ++i) CHECK(got[i] == want[i], "settle: value (+ p below the decision point) in exact digits");
    // the rule's two guarantees, from the value itself: kept values are above -p / 2 - 2^232, raised ones end below p / 2 + 2^232
    const Big half = big_sar(p, 1), slack = big_shl(big_from(1), 232);
    if (add) CHECK(big_lt(big_add(v, p), big_add(half, slack)), "a raised value ends below p / 2 + 2^232");
    else CHECK(big_lt(big_neg(big_add(half, slack)), v), "a kept value is above -p / 2 - 2^232");
}

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 3000000;
    const Big p = big_p(), one = big_from(1), lim = big_shl(one, 255);
    const int32_t mask = scd::kF29Mask, top_lo = -(1 << 23), top_hi = (1 << 23) - 1;
    {
        uint32_t w[8];
        words_of(p, w);
        CHECK(w[0] == 0x00000001u && w[7] == 0x73eda753u && w[6] == 0x299d7d48u, "p");
    }
    // corners: the ends of the range, around zero, +-p, +-p / 2 each +-1; limbs 0..7 all 0 / all 2^29 - 1 with limb 8 at both ends
    std::vector<Big> vals = {big_neg(lim), big_add(lim, big_neg(one)), big_from(0), big_from(-1), big_from(1)};
    const Big half = big_sar(p, 1);
    for (const Big &b : {p, big_neg(p), half, big_neg(half)})
        for (int d = -1; d <= 1; ++d) vals.push_back(big_add(b, big_from(d)));
    for (const Big &v : vals) {
        int32_t l[9];
        limbs_of(v, l);
        CHECK(big_eq(value_of(l), v), "limbs_of / value_of");
        CHECK(l[8] >= top_lo && l[8] <= top_hi, "a corner inside the format");
        check_round_trip(l);
    }
    for (int32_t low : {0, mask})
        for (int32_t top : {top_lo, top_hi}) {
            int32_t l[9];
            for (int i = 0; i < 8; ++i) l[i] = low;
            l[8] = top;
            check_round_trip(l);
        }
    // the range rule on both sides of its decision point, with the lower limbs at the ends of a lazy sum of two normalised elements
    for (int32_t dt = -2; dt <= 2; ++dt)
        for (int32_t low : {0, mask, 2 * mask}) {
            int32_t l[9];
            for (int i = 0; i < 8; ++i) l[i] = low;
            l[8] = -scd::kF29RuleTop + dt;
            check_settle(l, p);
        }
    for (long it = 0; it < n_random; ++it) {
        int32_t l[9];
        for (int i = 0; i < 8; ++i) l[i] = (int32_t)(rnd() & (uint64_t)mask);
        l[8] = (int32_t)(rnd() % (1u << 24)) + top_lo;
        check_round_trip(l);
        // a freshly bound entry: limbs 0..7 sums of two digits, limb 8 anywhere a source in the format plus a bind's term can put it,
        // every eighth draw within a few units of the decision point
        int32_t s[9];
        for (int i = 0; i < 8; ++i) s[i] = (int32_t)(rnd() & (uint64_t)mask) + (int32_t)(rnd() & (uint64_t)mask);
        s[8] = (it & 7) == 0 ? -scd::kF29RuleTop + (int32_t)(rnd() % 9) - 4 : (int32_t)(rnd() % (1u << 25)) - (1 << 24);
        check_settle(s, p);
    }
    if (failures) {
        std::printf("%ld FAILURES\n", failures);
        return 1;
    }
    std::printf("ALL TESTS PASSED (%ld random values)\n", n_random);
    return 0;
}
