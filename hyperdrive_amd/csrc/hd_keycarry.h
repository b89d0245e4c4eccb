// hd_keycarry.h -- which known keys a set change keeps when it re-tiers the
// key tables (hd_fbtables.hip fb_map; DESIGN.md §4 "Where P comes from"):
// plain C++, no HIP, so the slot plan is tested without a GPU
// (tests/native/hd_keycarry_check.cpp runs this same text).
//
// A re-tier frees every table together with the key and state arrays and
// hands out slots from 1 again.  The keys the context knew are carried over
// that step in a device stash, one row per entry of the SNAPSHOT: the
// (signatory, slot) pairs and the slot states as they stood at the entry of
// hd_fb_map_signatories, before its first attempt.  A failed attempt has
// already moved slots of departed signatories to new ones while their states
// still say READY, so the live map may never be the source of a carry.
#pragma once
#include <stdint.h>
#include <string.h>

#include <utility>
#include <vector>

#include "hd_fixedbase.h"   // the slot states (HD_FB_EMPTY .. HD_FB_READY)

namespace hd {

// The snapshot: row r is signatory sig32[32 r ..] in slot slot[r]; state[]
// holds the states of slots 0 .. n_state - 1 and [f0, f1) is the foreign-key
// block.  A row's key is known when its slot lies in [1, n_state), outside
// the foreign block, and its state is LEARNED or READY.
struct KeySnapshot {
    const uint8_t* sig32;
    const uint32_t* slot;
    uint32_t n;
    const uint32_t* state;
    uint32_t n_state;
    uint32_t f0, f1;
};

inline bool key_snap_known(const KeySnapshot& s, uint32_t r) {
    const uint32_t sl = s.slot[r];
    if (sl < 1 || sl >= s.n_state || (sl >= s.f0 && sl < s.f1)) return false;
    return s.state[sl] == HD_FB_LEARNED || s.state[sl] == HD_FB_READY;
}

// index of sig in the sorted, distinct set (m rows of 32 bytes), or -1
inline int64_t key_sorted_find(const uint8_t* sorted32, uint32_t m, const uint8_t* sig) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const int c = memcmp(sorted32 + 32 * (size_t)mid, sig, 32);
        if (c == 0) return (int64_t)mid;
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

struct KeyCarryPlan {
    std::vector<int32_t> adm_slot;                       // new sorted index -> slot, -1: none
    std::vector<std::pair<uint32_t, uint32_t>> carry;    // (snapshot row, new slot), by new sorted index
    uint32_t used = 1;       // slots handed out, slot 0 included
    uint32_t carried = 0;    // = carry.size()
    uint32_t dropped = 0;    // known keys without a place: signatory left the set, or no slot
};

// Slots of the new sorted set in tables that start empty (slot 0 is G's and
// never assigned, slots end below max_slots): the signatories whose key the
// snapshot knows first, in sorted order among themselves, then the rest in
// sorted order.  A signatory the snapshot holds twice carries its first row.
inline void key_carry_plan(const KeySnapshot& s, const uint8_t* sorted32, uint32_t m, uint32_t max_slots,
                           KeyCarryPlan& out) {
    out.adm_slot.assign(m > 0 ? m : 1, -1);
    out.carry.clear();
    out.used = 1;
    out.carried = out.dropped = 0;
    std::vector<int64_t> row_of(m, -1);
    for (uint32_t r = 0; r < s.n; r++) {
        if (!key_snap_known(s, r)) continue;
        const int64_t k = key_sorted_find(sorted32, m, s.sig32 + 32 * (size_t)r);
        if (k < 0 || row_of[k] >= 0) out.dropped++;
        else row_of[k] = (int64_t)r;
    }
    for (uint32_t k = 0; k < m; k++) {
        if (row_of[k] < 0) continue;
        if (out.used < max_slots) {
            out.adm_slot[k] = (int32_t)out.used;
            out.carry.emplace_back((uint32_t)row_of[k], out.used++);
        } else {
            out.dropped++;
        }
    }
    out.carried = (uint32_t)out.carry.size();
    for (uint32_t k = 0; k < m && out.used < max_slots; k++)
        if (row_of[k] < 0) out.adm_slot[k] = (int32_t)out.used++;
}

// The known keys of the snapshot, and how many of them belong to a signatory
// of the new sorted set (what a set change at an unchanged width keeps in
// place: such a signatory keeps its slot).
inline void key_snap_count(const KeySnapshot& s, const uint8_t* sorted32, uint32_t m, uint32_t& known,
                           uint32_t& staying) {
    known = staying = 0;
    for (uint32_t r = 0; r < s.n; r++) {
        if (!key_snap_known(s, r)) continue;
        known++;
        staying += key_sorted_find(sorted32, m, s.sig32 + 32 * (size_t)r) >= 0 ? 1u : 0u;
    }
}

}  // namespace hd
