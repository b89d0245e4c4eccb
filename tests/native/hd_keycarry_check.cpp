// hd_keycarry_check.cpp -- the slot plan of a re-tiering set change
// (hyperdrive_amd/csrc/hd_keycarry.h) as a stand-alone host program, so that
// it runs as plain C++ under ASan + UBSan (tests/test_key_carry_host.py).
//
// stdin, any number of cases:
//   case <n_snap> <n_state> <f0> <f1> <m> <max_slots>
//   <64 hex digits> <slot>          n_snap snapshot rows
//   <state>                         n_state lines
//   <64 hex digits>                 m rows of the new set, sorted
// stdout per case:
//   plan <used> <carried> <dropped>
//   adm <slot of sorted index 0> ...
//   carry <row>:<slot> ...
//   count <known> <staying>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "../../hyperdrive_amd/csrc/hd_keycarry.h"

static bool unhex32(const std::string& h, uint8_t* out) {
    if (h.size() != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (sscanf(h.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

int main() {
    std::string word;
    while (std::cin >> word) {
        if (word != "case") return 2;
        uint32_t n_snap, n_state, f0, f1, m, max_slots;
        if (!(std::cin >> n_snap >> n_state >> f0 >> f1 >> m >> max_slots)) return 2;
        // exact sizes, no slack: an index one past an array is ASan's to catch
        std::vector<uint8_t> snap_sig(32 * (size_t)n_snap), sorted(32 * (size_t)m);
        std::vector<uint32_t> snap_slot(n_snap), state(n_state);
        for (uint32_t r = 0; r < n_snap; r++) {
            std::string h;
            if (!(std::cin >> h >> snap_slot[r]) || !unhex32(h, &snap_sig[32 * (size_t)r])) return 2;
        }
        for (uint32_t k = 0; k < n_state; k++)
            if (!(std::cin >> state[k])) return 2;
        for (uint32_t k = 0; k < m; k++) {
            std::string h;
            if (!(std::cin >> h) || !unhex32(h, &sorted[32 * (size_t)k])) return 2;
        }
        const hd::KeySnapshot s{snap_sig.data(), snap_slot.data(), n_snap, state.data(), n_state, f0, f1};
        hd::KeyCarryPlan p;
        hd::key_carry_plan(s, sorted.data(), m, max_slots, p);
        printf("plan %u %u %u\nadm", p.used, p.carried, p.dropped);
        for (uint32_t k = 0; k < m; k++) printf(" %d", p.adm_slot[k]);
        printf("\ncarry");
        for (const auto& c : p.carry) printf(" %u:%u", c.first, c.second);
        uint32_t known = 0, staying = 0;
        hd::key_snap_count(s, sorted.data(), m, known, staying);
        printf("\ncount %u %u\n", known, staying);
    }
    return 0;
}
