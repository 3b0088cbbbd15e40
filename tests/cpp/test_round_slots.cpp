// test_round_slots.cpp -- sumcheck_amd/csrc/round_slots.hpp on the host: every list of one to three products of one to four factors over
// three tables, every prior table state, bind on and off, one launch for the round and one launch per product.  Buffers are (table, index)
// pairs and every buffer carries what a kernel would have left in it -- how many binds, in which format -- so the checks are the
// invariants a round must keep, not a second copy of the rule.  Stand-alone: g++ -fsanitize=address,undefined, prints ALL TESTS PASSED.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "round_slots.hpp"

struct Buf {
    int table = -1, idx = -1;
    bool operator==(const Buf &o) const { return table == o.table && idx == o.idx; }
};
struct Slot {
    Buf src, dst;
    uint32_t mode = 0, exp = 0, src_f29 = 0, dst_f29 = 0;
};
struct Table {
    Buf cur, buf[2];
    bool cur_f29 = false;
    int next = 0;
};
struct Product {
    std::vector<uint32_t> tables, exps;
};
constexpr int kTables = 3;

static long long g_checks = 0;
static const char *case_name();
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        ++g_checks;                                                                                  \
        if (!(cond)) {                                                                               \
            std::printf("FAILED %s:%d: %s  [case %s]\n", __FILE__, __LINE__, #cond, case_name());     \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)
static size_t g_id[7]; // the case at hand: products a, b, c of the list, prior states, bind, launch per product, F29 stores
static const char *case_name() {
    static char text[160];
    std::snprintf(text, sizeof(text), "products %zu %zu %zu, prior %zu, bind %zu, per product %zu, f29 %zu", g_id[0], g_id[1], g_id[2], g_id[3], g_id[4], g_id[5], g_id[6]);
    return text;
}
static Buf B(int table, int idx) {
    Buf b;
    b.table = table, b.idx = idx;
    return b;
}

// every product as Product stores it: distinct tables in first-occurrence order, a multiplicity each, one to four factors in all
static std::vector<Product> all_products() {
    std::vector<Product> out;
    for (int t0 = 0; t0 < kTables; ++t0)
        for (uint32_t e0 = 1; e0 <= 4; ++e0) {
            out.push_back({{(uint32_t)t0}, {e0}});
            for (int t1 = 0; t1 < kTables; ++t1)
                for (uint32_t e1 = 1; t1 != t0 && e0 + e1 <= 4; ++e1) {
                    out.push_back({{(uint32_t)t0, (uint32_t)t1}, {e0, e1}});
                    for (uint32_t e2 = 1; e0 + e1 + e2 <= 4; ++e2) out.push_back({{(uint32_t)t0, (uint32_t)t1, (uint32_t)(3 - t0 - t1)}, {e0, e1, e2}});
                }
        }
    return out;
}

struct World { // the tables of a handle and what their buffers hold
    Table tab[kTables];
    int binds[kTables][2]; // binds of THIS round a buffer's content has behind it (-1: nothing valid)
    bool f29[kTables][2];
    uint8_t bound[kTables];
};

// one launch: the slots of `n` products, checked against the world as it is when the launch starts, then carried out
struct Launch {
    Slot slot[12];
    int n = 0;
};
static void run_launch(World &w, const Launch &l, bool bind, bool use_f29, const Table *before, int *stores_of) {
    for (int i = 0; i < l.n; ++i) { // (c) no slot reads a buffer that a slot of the same launch stores to
        const Slot &a = l.slot[i];
        if (a.mode != 1) continue;
        for (int j = 0; j < l.n; ++j) CHECK(!(l.slot[j].src == a.dst));
        for (int j = 0; j < i; ++j) CHECK(!(l.slot[j].mode == 1 && l.slot[j].dst == a.dst));
    }
    for (int i = 0; i < l.n; ++i) {
        const Slot &s = l.slot[i];
        const int u = s.src.table;
        CHECK(s.exp == 1 && (s.mode == 0 || s.mode == 1 || s.mode == 3));
        const int held = w.binds[u][s.src.idx];
        CHECK(held >= 0);
        CHECK(held + (s.mode != 0 ? 1 : 0) == (bind ? 1 : 0));            // (d) the factor contributes the table with this round's bind, once
        if (s.mode != 0) CHECK(bind && s.src == before[u].cur);           // (d) modes 1 and 3 read the pre-round buffer
        CHECK(s.src_f29 == (w.f29[u][s.src.idx] ? 1u : 0u));              // (e) the format of the buffer that is read
        if (s.mode != 0) CHECK(s.dst_f29 == (use_f29 ? 1u : 0u));         // (e)
        if (s.mode == 1) {
            CHECK(s.dst.table == u && s.dst == before[u].buf[before[u].next]); // (b) into the spare buffer
            ++stores_of[u];
        }
    }
    for (int i = 0; i < l.n; ++i)
        if (l.slot[i].mode == 1) {
            w.binds[l.slot[i].dst.table][l.slot[i].dst.idx] = 1;
            w.f29[l.slot[i].dst.table][l.slot[i].dst.idx] = l.slot[i].dst_f29 != 0;
        }
}

static void run_case(const std::vector<const Product *> &prods, unsigned prior, bool bind, bool per_product, bool use_f29) {
    static World w;
    for (int u = 0; u < kTables; ++u) {
        Table &t = w.tab[u];
        t.buf[0] = B(u, 0), t.buf[1] = B(u, 1);
        const bool bound_before = bind && ((prior >> u) & 1u); // an earlier launch of the round (1) or k_fix_deep (2) has bound it
        t.next = u & 1;                                        // (either buffer may be the spare one)
        t.cur = t.buf[t.next ^ 1];
        t.cur_f29 = bound_before ? (use_f29 && u != 1) : u != 0; // table 1 bound by a canonical pass; table 0 never stored in F29 so far
        w.binds[u][t.next ^ 1] = bound_before ? 1 : 0;
        w.binds[u][t.next] = -1;
        w.f29[u][t.next ^ 1] = t.cur_f29;
        w.f29[u][t.next] = false;
        w.bound[u] = bound_before ? (u == 2 ? 2 : 1) : 0;
    }
    static Table before[kTables];
    static uint8_t bound_before[kTables];
    for (int u = 0; u < kTables; ++u) before[u] = w.tab[u], bound_before[u] = w.bound[u];
    int stores_of[kTables] = {0, 0, 0};
    bool named[kTables] = {false, false, false};
    auto cur = [&](uint32_t u) { return scd::TableBuf<Buf>{w.tab[u].cur, w.tab[u].cur_f29 ? 1u : 0u}; };
    auto store = [&](uint32_t u) { return scd::flip_table(w.tab[u], use_f29); };
    static Launch l; // (static: the sanitizer poisons a stack object's shadow at every scope entry, twelve million times over)
    static scd::LaunchStores<Buf> round_scope, product_scope;
    l.n = round_scope.n = 0;
    for (const Product *pr : prods) {
        for (uint32_t u : pr->tables) named[u] = true;
        product_scope.n = 0;
        uint32_t M = 0;
        for (uint32_t e : pr->exps) M += e;
        const int n = scd::fill_factor_slots(l.slot + l.n, pr->tables, pr->exps, bind, w.bound, per_product ? product_scope : round_scope, use_f29 ? 1u : 0u, cur, store);
        CHECK(n == (int)M);
        for (int f = 0, s = 0, rep = 0; f < n; ++f) { // one slot per factor, in the product's order
            CHECK(l.slot[l.n + f].src.table == (int)pr->tables[s]);
            if (++rep == (int)pr->exps[s]) ++s, rep = 0;
        }
        l.n += n;
        if (per_product) {
            run_launch(w, l, bind, use_f29, before, stores_of);
            l.n = 0;
        }
    }
    if (!per_product) run_launch(w, l, bind, use_f29, before, stores_of);
    for (int u = 0; u < kTables; ++u) {
        const Table &t = w.tab[u], &b = before[u];
        if (!bind || bound_before[u] || !named[u]) { // (a) and the tables a round leaves alone
            CHECK(stores_of[u] == 0 && t.cur == b.cur && t.next == b.next && t.cur_f29 == b.cur_f29 && w.bound[u] == bound_before[u]);
        } else { // (b) stored exactly once, and the table has moved to what was its spare buffer
            CHECK(stores_of[u] == 1 && t.cur == b.buf[b.next] && t.next == (b.next ^ 1) && t.cur_f29 == use_f29 && w.bound[u] == 1);
            CHECK(w.binds[u][t.cur.idx] == 1 && w.f29[u][t.cur.idx] == use_f29);
        }
    }
}

// the node-by-node builder: one slot per distinct table, the multiplicity in exp, a store for every table that is still unbound
static void test_table_slots(const std::vector<Product> &all) {
    for (size_t a = 0; a < all.size(); ++a)
        for (unsigned prior = 0; prior < 8; ++prior)
            for (int bind = 0; bind < 2; ++bind) {
                const Product &pr = all[a];
                g_id[0] = a, g_id[1] = g_id[2] = all.size(), g_id[3] = prior, g_id[4] = (size_t)bind, g_id[5] = 1, g_id[6] = 0; // (the node-by-node builder)
                Table tab[kTables];
                uint8_t bound[kTables];
                for (int u = 0; u < kTables; ++u) tab[u].buf[0] = B(u, 0), tab[u].buf[1] = B(u, 1), tab[u].cur = tab[u].buf[0], tab[u].next = 1, bound[u] = (prior >> u) & 1u;
                Slot slot[4];
                const int n = scd::fill_table_slots(slot, pr.tables, pr.exps, bind != 0, bound, [&](uint32_t u) { return tab[u].cur; },
                                                    [&](uint32_t u) { return scd::flip_table(tab[u], tab[u].cur_f29); });
                CHECK(n == (int)pr.tables.size());
                for (int s = 0; s < n; ++s) {
                    const uint32_t u = pr.tables[s];
                    const bool binds = bind && !((prior >> u) & 1u);
                    CHECK(slot[s].exp == pr.exps[s] && slot[s].mode == (binds ? 1u : 0u) && slot[s].src == B((int)u, 0));
                    CHECK(binds ? (slot[s].dst == B((int)u, 1) && tab[u].cur == slot[s].dst && tab[u].next == 0 && bound[u] == 1) : (slot[s].dst.table == -1 && tab[u].next == 1));
                }
            }
}

int main() {
    const std::vector<Product> all = all_products();
    std::printf("%zu products\n", all.size());
    if (all.size() != 72) return std::printf("FAILED: the enumeration of products\n"), 1;
    long long cases = 0;
    std::vector<const Product *> list;
    for (size_t a = 0; a < all.size(); ++a)
        for (size_t b = 0; b <= all.size(); ++b)     // (index all.size(): no such product)
            for (size_t c = 0; c <= all.size(); ++c) {
                if (b == all.size() && c != all.size()) continue;
                list.clear();
                list.push_back(&all[a]);
                if (b < all.size()) list.push_back(&all[b]);
                if (c < all.size()) list.push_back(&all[c]);
                for (unsigned prior = 0; prior < 8; ++prior)
                    for (int bind = prior == 0 ? 0 : 1; bind < 2; ++bind) // (a round that binds nothing has no table bound before: one prior state)
                        for (int per_product = 0; per_product < 2; ++per_product) {
                            const bool use_f29 = ((a + b + c + prior) & 1) != 0; // (F29 and canonical stores alternate over the cases: every list meets both)
                            const size_t id[7] = {a, b, c, prior, (size_t)bind, (size_t)per_product, (size_t)use_f29};
                            for (int i = 0; i < 7; ++i) g_id[i] = id[i];
                            run_case(list, prior, bind != 0, per_product != 0, use_f29);
                            ++cases;
                        }
            }
    test_table_slots(all);
    std::printf("%lld cases, %lld checks\nALL TESTS PASSED\n", cases, g_checks);
    return 0;
}
