// round_slots.hpp -- how the factors of a product become the argument slots (kernels.h: Slot) of a big-round launch: the one rule every
// launch plan of protocol.hip builds its slots by.  Plain C++, templated on the slot and pointer types: it compiles for the host without HIP
// (tests/cpp/test_round_slots.cpp enumerates it with (table, buffer) pairs for pointers).
//
// A binding round finds every table unbound in one buffer and leaves it bound in the other, and within ONE launch no slot may read a buffer
// that another slot stores to.  So the first factor on a table that is still unbound binds and stores it (mode 1); a later factor on a
// table stored by the SAME launch -- in this product or in another -- binds it again from the old buffer and stores nothing (mode 3); a
// factor on a table that an EARLIER launch of the round (or k_fix_deep) bound reads the new buffer as it is (mode 0), and so does every
// factor of a round that does not bind.
#pragma once
#include <cstdint>
#include <vector>

namespace scd {

struct SlotRule { // reads_old: the buffer the table held before the round (modes 1 and 3); otherwise the one it holds now
    uint32_t mode;
    bool reads_old, stores;
};
constexpr SlotRule slot_rule(bool bind, bool bound_before, bool stored_here) {
    return !bind || (bound_before && !stored_here) ? SlotRule{0, false, false} : stored_here ? SlotRule{3, true, false} : SlotRule{1, true, true};
}

template <class Src> struct TableBuf { // a buffer as a slot reads it: (src, src_f29)
    Src src;
    uint32_t f29;
};

// The tables that slots of ONE launch have stored so far, each with the buffer it held before.  bound[] (one per round) cannot say which
// launch bound a table; this can: one scope per round where the round is one launch, one scope per product where every product is a launch.
constexpr int kMaxLaunchStores = 48; // the slots of the largest launch (protocol.hip asserts it against kMaxRoundProds rows of four)
template <class Src> struct LaunchStores {
    uint32_t table[kMaxLaunchStores];
    TableBuf<Src> old[kMaxLaunchStores];
    int n = 0;
    const TableBuf<Src> *find(uint32_t u) const {
        for (int i = 0; i < n; ++i)
            if (table[i] == u) return &old[i];
        return nullptr;
    }
};

// the move every bind of a resident table ends with: the spare buffer becomes the current one.  Returns it.
template <class TableT> auto flip_table(TableT &t, bool f29) {
    auto dst = t.buf[t.next];
    t.cur = dst;
    t.cur_f29 = f29;
    t.next ^= 1;
    return dst;
}

// One slot per FACTOR of a product (tables[s], exps[s] times).  cur(u): the buffer table u holds now, as a TableBuf; store(u): where a bind
// of table u goes -- called once per stored table, and the caller moves the table there if its plan does (flip_table).  bound[u] != 0: the
// table has this round's bind already (not read unless `bind`); a store sets it to 1.  Returns the number of slots.
template <class SlotT, class Src, class Cur, class Store>
int fill_factor_slots(SlotT *slot, const std::vector<uint32_t> &tables, const std::vector<uint32_t> &exps, bool bind, uint8_t *bound, LaunchStores<Src> &stores,
                      uint32_t dst_f29, Cur cur, Store store) {
    int f = 0;
    for (size_t s = 0; s < tables.size(); ++s) {
        const uint32_t u = tables[s];
        for (uint32_t rep = 0; rep < exps[s]; ++rep, ++f) {
            SlotT &sl = slot[f];
            const TableBuf<Src> *old = bind ? stores.find(u) : nullptr;
            const SlotRule rule = slot_rule(bind, bind && bound[u] != 0, old != nullptr);
            const TableBuf<Src> from = rule.reads_old && old ? *old : cur(u);
            sl.exp = 1;
            sl.mode = rule.mode;
            sl.src = from.src;
            sl.src_f29 = from.f29;
            if (rule.mode != 0) sl.dst_f29 = dst_f29; // (mode 3 stores nothing: it keeps the value in the stored table's form)
            if (rule.stores) {
                stores.table[stores.n] = u;
                stores.old[stores.n++] = from;
                sl.dst = store(u);
                bound[u] = 1;
            }
        }
    }
    return f;
}

// The node-by-node kernels (k_prod_round_fe and the experiments build's) take one slot per distinct TABLE, exp its multiplicity, and read
// and store canonical tables only: no table repeats within a launch, so there is no mode 3 and no scope, and the formats are not theirs to
// set -- a second small function rather than flags on the rule above.  cur(u), store(u): plain pointers.
template <class SlotT, class Cur, class Store>
int fill_table_slots(SlotT *slot, const std::vector<uint32_t> &tables, const std::vector<uint32_t> &exps, bool bind, uint8_t *bound, Cur cur, Store store) {
    for (size_t s = 0; s < tables.size(); ++s) {
        const uint32_t u = tables[s];
        const SlotRule rule = slot_rule(bind, bind && bound[u] != 0, false);
        slot[s].exp = exps[s];
        slot[s].mode = rule.mode;
        slot[s].src = cur(u);
        if (rule.stores) {
            slot[s].dst = store(u);
            bound[u] = 1;
        }
    }
    return (int)tables.size();
}

} // namespace scd
