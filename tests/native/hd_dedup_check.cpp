// hd_dedup_check.cpp -- host check of the repeat table's equality predicate
// and hash (hyperdrive_amd/csrc/hd_dedup.h), the code k_fast_prep runs.
// Stand-alone: build with -fsanitize=address,undefined and run it; prints
// "ok" and exits 0, or names the first failed property and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_dedup.h"

using namespace hd;

namespace {

struct Arrays {
    size_t n;
    std::vector<int64_t> height, round;
    std::vector<uint8_t> value, digest, from, sig;   // exact sizes: the sanitizer sees any read past a row
    explicit Arrays(size_t n_) : n(n_), height(n_), round(n_), value(32 * n_), digest(32 * n_), from(32 * n_), sig(65 * n_) {}
};

uint32_t rng_state = 0x12345u;
uint32_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

void fill(Arrays& a) {
    for (size_t i = 0; i < a.n; i++) {
        a.height[i] = (int64_t)rnd() << 20 | rnd();
        a.round[i] = rnd() & 7;
    }
    for (auto* v : {&a.value, &a.digest, &a.from, &a.sig})
        for (auto& x : *v) x = (uint8_t)rnd();
}

void copy_row(Arrays& a, size_t dst, size_t src) {
    a.height[dst] = a.height[src];
    a.round[dst] = a.round[src];
    memcpy(&a.value[32 * dst], &a.value[32 * src], 32);
    memcpy(&a.digest[32 * dst], &a.digest[32 * src], 32);
    memcpy(&a.from[32 * dst], &a.from[32 * src], 32);
    memcpy(&a.sig[65 * dst], &a.sig[65 * src], 65);
}

DdKey key(const Arrays& a, size_t i, bool with_digest) {
    DdKey k;
    dd_key_load(k, a.height.data(), a.round.data(), a.value.data(), with_digest ? a.digest.data() : nullptr,
                a.from.data(), a.sig.data(), i, a.n);
    return k;
}

int fail(const char* what, long at = -1) {
    fprintf(stderr, "hd_dedup_check: %s (%ld)\n", what, at);
    return 1;
}

// byte b of the fields the predicate reads, in the order height (8), round
// (8), value (32), from (32), sig (65): 145 bytes
void flip(Arrays& a, size_t i, int b, uint8_t mask) {
    if (b < 8) a.height[i] ^= (int64_t)((uint64_t)mask << (8 * b));
    else if (b < 16) a.round[i] ^= (int64_t)((uint64_t)mask << (8 * (b - 8)));
    else if (b < 48) a.value[32 * i + (b - 16)] ^= mask;
    else if (b < 80) a.from[32 * i + (b - 48)] ^= mask;
    else a.sig[65 * i + (b - 80)] ^= mask;
}

}  // namespace

int main() {
    // rows 0 .. n-1; the last row is the one whose loads end at the arrays' ends
    const size_t n = 9;
    Arrays a(n);
    fill(a);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++)
            for (int dg = 0; dg < 2; dg++)
                if (dd_key_equal(key(a, i, dg), key(a, j, dg)) != (i == j)) return fail("random rows", (long)(i * n + j));
    // an exact copy is equal; any single flipped bit of any byte is not, in
    // every position of the batch (first, middle, last row)
    for (size_t dst : {(size_t)0, (size_t)4, n - 1}) {
        const size_t src = dst == 2 ? 3 : 2;
        for (int b = 0; b < 145; b++)
            for (int bit = 0; bit < 8; bit++) {
                copy_row(a, dst, src);
                if (!dd_key_equal(key(a, dst, false), key(a, src, false))) return fail("copy not equal", b);
                if (dd_hash(key(a, dst, false)) != dd_hash(key(a, src, false))) return fail("copy hashes apart", b);
                flip(a, dst, b, (uint8_t)(1u << bit));
                if (dd_key_equal(key(a, dst, false), key(a, src, false))) return fail("flipped byte still equal", b);
                // the hash reads From bytes 0-3 and 28-31, signature bytes
                // 0-3, 28-31, 32-35 and 60-63, and nothing else
                const int fo = b - 48, so = b - 80;
                const bool hashed = (b >= 48 && b < 80 && (fo < 4 || fo >= 28)) ||
                                    (b >= 80 && (so < 4 || (so >= 28 && so < 36) || (so >= 60 && so < 64)));
                const bool same = dd_hash(key(a, dst, false)) == dd_hash(key(a, src, false));
                if (!hashed && !same) return fail("hash reads an undocumented byte", b);
                if (hashed && same) return fail("hash ignores a documented byte", b);
            }
        fill(a);
    }
    // digest mode: the digest row stands for (height, round, value), which
    // are not read (NULL there)
    {
        Arrays d(n);
        fill(d);
        copy_row(d, n - 1, 1);
        DdKey x, y;
        dd_key_load(x, nullptr, nullptr, nullptr, d.digest.data(), d.from.data(), d.sig.data(), n - 1, n);
        dd_key_load(y, nullptr, nullptr, nullptr, d.digest.data(), d.from.data(), d.sig.data(), 1, n);
        if (!dd_key_equal(x, y)) return fail("digest copy not equal");
        for (int b = 0; b < 32; b++) {
            d.digest[32 * (n - 1) + b] ^= 0x80;
            dd_key_load(x, nullptr, nullptr, nullptr, d.digest.data(), d.from.data(), d.sig.data(), n - 1, n);
            if (dd_key_equal(x, y)) return fail("flipped digest byte still equal", b);
            d.digest[32 * (n - 1) + b] ^= 0x80;
        }
    }
    // the table: a power of two, load <= 1/4 up to 2^29 messages, never 0
    for (uint32_t m : {1u, 63u, 255u, 256u, 257u, 8231u, 1u << 20, (1u << 24) + 1u, 1u << 29, HD_DD_MAX_N}) {
        const uint32_t w = dd_table_words(m);
        if (w < 1024u || (w & (w - 1u))) return fail("table size", (long)m);
        if (m <= (1u << 29) && (uint64_t)w < 4ull * m) return fail("table load", (long)m);
        if ((uint64_t)w >= 16ull * m && w > 1024u) return fail("table too large", (long)m);
    }
    // the ref encodings are disjoint for every index below HD_DD_MAX_N
    if (((HD_DD_REPEAT | (HD_DD_MAX_N - 1u)) >> 30) != 2u || (HD_DD_FINAL >> 30) != 3u || ((HD_DD_MAX_N - 1u) >> 30) != 0u)
        return fail("ref encoding");
    puts("ok");
    return 0;
}
