// hd_preimage_check.cpp -- host check of the preimage table's key, equality
// predicate, hash and pid encoding (hyperdrive_amd/csrc/hd_dedup.h), the code
// k_pre_claim and k_fast_prep run.  Stand-alone: build with
// -fsanitize=address,undefined and run it; prints "ok" and exits 0, or names
// the first failed property and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_dedup.h"

using namespace hd;

namespace {

struct Arrays {
    size_t n;
    std::vector<uint8_t> type;
    std::vector<int64_t> height, round, vround;
    std::vector<uint8_t> value;   // exact size: the sanitizer sees any read past a row
    explicit Arrays(size_t n_) : n(n_), type(n_), height(n_), round(n_), vround(n_), value(32 * n_) {}
};

uint32_t rng_state = 0x2468ACEu;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

void fill(Arrays& a) {
    for (size_t i = 0; i < a.n; i++) {
        a.type[i] = (uint8_t)(1 + rnd() % 3);
        a.height[i] = (int64_t)rnd() << 24 | rnd();
        a.round[i] = rnd() & 7;
        a.vround[i] = (int64_t)(rnd() & 3) - 1;
    }
    for (auto& x : a.value) x = (uint8_t)rnd();
}

void copy_row(Arrays& a, size_t dst, size_t src) {
    a.type[dst] = a.type[src];
    a.height[dst] = a.height[src];
    a.round[dst] = a.round[src];
    a.vround[dst] = a.vround[src];
    memcpy(&a.value[32 * dst], &a.value[32 * src], 32);
}

DdPre key(const Arrays& a, size_t i, bool with_vround = true) {
    DdPre k;
    dd_pre_load(k, a.type[i] == T_PROPOSE, a.height.data(), a.round.data(), with_vround ? a.vround.data() : nullptr,
                a.value.data(), i);
    return k;
}

int fail(const char* what, long at = -1) {
    fprintf(stderr, "hd_preimage_check: %s (%ld)\n", what, at);
    return 1;
}

// byte b of the preimage fields, in the order height (8), round (8),
// valid_round (8), value (32): 56 bytes
void flip(Arrays& a, size_t i, int b, uint8_t mask) {
    if (b < 8) a.height[i] ^= (int64_t)((uint64_t)mask << (8 * b));
    else if (b < 16) a.round[i] ^= (int64_t)((uint64_t)mask << (8 * (b - 8)));
    else if (b < 24) a.vround[i] ^= (int64_t)((uint64_t)mask << (8 * (b - 16)));
    else a.value[32 * i + (b - 24)] ^= mask;
}

}  // namespace

int main() {
    const size_t n = 9;   // the last row's loads end at the arrays' ends
    Arrays a(n);
    fill(a);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++)
            if (dd_pre_equal(key(a, i), key(a, j)) != (i == j)) return fail("random rows", (long)(i * n + j));
    // an exact copy is equal and hashes alike; any single flipped bit of any
    // preimage byte is not equal -- of a vote, valid_round is no preimage byte
    for (int propose = 0; propose < 2; propose++)
        for (size_t dst : {(size_t)0, (size_t)4, n - 1}) {
            const size_t src = 2;
            for (int b = 0; b < 56; b++)
                for (int bit = 0; bit < 8; bit++) {
                    a.type[src] = propose ? T_PROPOSE : (bit & 1 ? T_PREVOTE : T_PRECOMMIT);
                    copy_row(a, dst, src);
                    if (!propose) a.type[dst] = bit & 1 ? T_PRECOMMIT : T_PREVOTE;   // the two vote types share
                    if (!dd_pre_equal(key(a, dst), key(a, src))) return fail("copy not equal", b);
                    if (dd_pre_hash(key(a, dst)) != dd_pre_hash(key(a, src))) return fail("copy hashes apart", b);
                    flip(a, dst, b, (uint8_t)(1u << bit));
                    const bool read = propose || b < 16 || b >= 24;
                    if (dd_pre_equal(key(a, dst), key(a, src)) == read) return fail("flipped byte", b);
                    // the hash reads every byte of height and round, value
                    // bytes 0-3 and 28-31, the low 31 bits of a propose's
                    // valid_round, and nothing else
                    const int vo = b - 24;
                    const bool hashed = b < 16 || (b >= 24 && (vo < 4 || vo >= 28)) ||
                                        (propose && b >= 16 && b < 20 && !(b == 19 && bit == 7));
                    const bool same = dd_pre_hash(key(a, dst)) == dd_pre_hash(key(a, src));
                    if (!hashed && !same) return fail("hash reads an undocumented byte", b);
                    if (hashed && same) return fail("hash ignores a documented byte", b);
                }
            fill(a);
        }
    // the near misses that must not share
    {
        Arrays m(n);
        fill(m);
        auto differ = [&](const char* what) {
            return dd_pre_equal(key(m, 0), key(m, n - 1)) ? fail(what) : 0;
        };
        m.type[2] = T_PREVOTE;
        copy_row(m, 0, 2);
        copy_row(m, n - 1, 2);
        if (!dd_pre_equal(key(m, 0), key(m, n - 1))) return fail("near-miss base not equal");
        m.value[32 * (n - 1) + 31] ^= 1;
        if (differ("values differing in the last byte")) return 1;
        copy_row(m, n - 1, 2);
        m.height[n - 1] ^= (int64_t)1 << 32;
        if (differ("heights differing in the high word")) return 1;
        if (dd_pre_hash(key(m, 0)) == dd_pre_hash(key(m, n - 1))) return fail("high height word not hashed");
        copy_row(m, n - 1, 2);
        m.round[n - 1] ^= (int64_t)1 << 32;
        if (differ("rounds differing in the high word")) return 1;
        if (dd_pre_hash(key(m, 0)) == dd_pre_hash(key(m, n - 1))) return fail("high round word not hashed");
        copy_row(m, n - 1, 2);
        m.type[n - 1] = T_PROPOSE;
        m.vround[n - 1] = 0;   // (a vote's key holds valid_round 0)
        if (differ("a propose and a vote")) return 1;
        m.type[0] = T_PROPOSE;
        m.vround[0] = -1;
        if (differ("proposes differing in valid_round")) return 1;
        m.vround[0] = 0;
        if (!dd_pre_equal(key(m, 0), key(m, n - 1))) return fail("equal proposes");
        // no valid_round array: a propose hashes -1, a vote still 0
        if (key(m, 0, false).valid_round != -1) return fail("propose without valid_round array");
        m.type[0] = T_PRECOMMIT;
        if (key(m, 0, false).valid_round != 0 || key(m, 0).valid_round != 0) return fail("vote valid_round");
    }
    // the pid encodings are disjoint for every index below HD_DD_MAX_N, and a
    // reference resolves through its claimant's word with one more load
    {
        const uint32_t top = HD_DD_MAX_N - 1u;
        if (dd_pid_is_ref(top) || dd_pid_is_none(top) || !dd_pid_is_ref(dd_pid_ref(top)) ||
            dd_pid_is_none(dd_pid_ref(top)) || dd_pid_claimant(dd_pid_ref(top)) != top || !dd_pid_is_none(HD_DD_FINAL) ||
            dd_pid_is_ref(HD_DD_FINAL))
            return fail("pid encoding");
        std::vector<uint32_t> pid = {5u, dd_pid_ref(0), HD_DD_FINAL, dd_pid_ref(4), 0u};
        if (dd_pid_resolve(pid.data(), 0) != 5u || dd_pid_resolve(pid.data(), 1) != 5u ||
            dd_pid_resolve(pid.data(), 3) != 0u || dd_pid_resolve(pid.data(), 4) != 0u ||
            !dd_pid_is_none(dd_pid_resolve(pid.data(), 2)))
            return fail("pid resolve");
    }
    puts("ok");
    return 0;
}
