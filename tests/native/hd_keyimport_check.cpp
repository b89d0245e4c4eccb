// hd_keyimport_check.cpp -- host program over hd_keyimport.h: the row check of
// hd_import_keys (key_classify) as the gfx950 kernel runs it, compiled as
// plain C++ under ASan + UBSan and driven by tests/test_key_import_host.py.
//
// stdin, one command per line:
//   set <fmt> <n> <slots>   then n lines of 64 hex digits: the signatory array
//                           as hd_set_signatories takes it (any order,
//                           duplicates allowed); slots 1: every admitted
//                           signatory has an empty table slot, 0: no slot map
//   key <128 hex digits>    X || Y; prints "<status> <signer>"
// The admitted table is built as hd_set_signatories builds it: sorted, first
// of equal entries kept, hashed index by adm_index_build.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_keyimport.h"

using namespace hd;

static bool unhex(const std::string& s, uint8_t* out, size_t n) {
    if (s.size() != 2 * n) return false;
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(s.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

int main() {
    int fmt = 1;
    std::vector<uint32_t> words, ix;
    std::vector<int32_t> perm, slots;
    bool have_slots = false;
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "set") {
            size_t n;
            int sl;
            std::cin >> fmt >> n >> sl;
            std::vector<uint8_t> sigs(32 * n);
            for (size_t i = 0; i < n; i++) {
                std::string h;
                std::cin >> h;
                if (!unhex(h, &sigs[32 * i], 32)) return 2;
            }
            std::vector<uint32_t> order(n);
            for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
                return memcmp(&sigs[32 * (size_t)a], &sigs[32 * (size_t)b], 32) < 0;
            });
            words.clear();
            perm.clear();
            for (size_t k = 0; k < n; k++) {
                const uint8_t* s = &sigs[32 * (size_t)order[k]];
                if (!perm.empty() && memcmp(s, &sigs[32 * (size_t)perm.back()], 32) == 0) continue;
                for (int w = 0; w < 8; w++) words.push_back(load_be32(s + 4 * w));
                perm.push_back((int32_t)order[k]);
            }
            const uint32_t m = (uint32_t)perm.size();
            ix.assign(adm_index_slots(m), 0);
            adm_index_build(words.data(), m, ix.data(), (uint32_t)ix.size());
            have_slots = sl != 0;
            slots.resize(m);
            for (uint32_t k = 0; k < m; k++) slots[k] = (int32_t)k + 1;   // slot 0 is G's
        } else if (cmd == "key") {
            std::string h;
            std::cin >> h;
            // exactly 64 bytes on the heap: a read past the key is ASan's to find
            std::vector<uint8_t> key(64);
            if (!unhex(h, key.data(), 64)) return 2;
            const uint32_t m = (uint32_t)perm.size();
            const AdmIndex a{words.data(), ix.data(), (uint32_t)ix.size() - 1};
            ge q;
            int32_t idx, slot;
            const uint8_t st = key_classify(fmt, key.data(), a, m, have_slots ? slots.data() : nullptr, m + 1, q, idx, slot);
            if ((st == HD_KEY_IMPORTED) != (slot >= 1)) return 3;
            printf("%u %d\n", (unsigned)st, idx >= 0 ? (int)perm[idx] : -1);
        } else {
            return 2;
        }
    }
    return 0;
}
