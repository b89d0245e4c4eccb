// hd_inv2_check.cpp -- host check of the lean inversions
// (hyperdrive_amd/csrc/hd_inv2.h): the up, mid and down passes the gfx950
// kernels run, lane by lane over plain arrays, for both domains (scalars
// mod n in Montgomery form, field elements mod p), K in {8, 16} x K2 in
// {8, 16}, against a direct divstep inversion of every live entry; then the
// one-level walk (inv2_lean) over the same inputs, checked the same way.
//
// Sizes N: 1, 64 K, 64 K + 1, 64 K K2 + 1 (the first with a second wave of
// inverting lanes).  Live masks: random, whole level-1 lanes dead, whole
// level-2 lanes dead, one live entry, none.  The rows have exactly the sizes
// the library allocates relative to T (9 T words per root row), so under
// -fsanitize=address an index past a row is an error; a dead entry's pre
// words must stay untouched.  Prints "ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../hyperdrive_amd/csrc/hd_inv2.h"

using namespace hd;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

static void fail(const char* what, const char* dom, int K, int K2, uint32_t N, int mask, long at) {
    fprintf(stderr, "hd_inv2_check: %s (%s K %d K2 %d N %u mask %d at %ld)\n", what, dom, K, K2, N, mask, at);
    exit(1);
}

static const uint32_t POISON = 0xA5A5A5A5u;
static const uint32_t MAXN = 16 * 16 * 64 + 1;

// an entry's input words (8 for a scalar, 9 for a field element) and the
// canonical words of its inverse by a direct inversion
struct ScDom {
    typedef sm D;
    static const int LW = 8;
    static const char* name() { return "s"; }
    static void random(uint32_t* w) {   // in [1, n): the top word of n is all ones
        for (int k = 0; k < 8; k++) w[k] = rnd();
        if (w[7] == 0xFFFFFFFFu) w[7] = 0xFFFFFFFEu;
        w[0] |= 1u;
        if (rnd() % 64 == 0) { memset(w, 0, 32); w[0] = 1 + rnd() % 3; }   // small values too
    }
    static void direct(uint32_t* out8, const uint32_t* w) {
        sc a, r;
        memcpy(a.v, w, 32);
        sc_inv_divsteps(r, a);
        memcpy(out8, r.v, 32);
    }
    // the pre row's entry (s^-1 R, < 2n) as canonical words of s^-1
    static void canon(uint32_t* out8, const uint32_t* e9) {
        sm x, one;
        memcpy(x.n, e9, 36);
        for (int k = 0; k < 9; k++) one.n[k] = k == 0;
        sm_mul(x, x, one);
        sc r;
        sm_to_sc(r, x);
        memcpy(out8, r.v, 32);
    }
};
struct FeDom {
    typedef fe D;
    static const int LW = 9;
    static const char* name() { return "Z"; }
    static void random(uint32_t* w) {
        uint32_t le[8];
        for (int k = 0; k < 8; k++) le[k] = rnd();
        if (le[7] == 0xFFFFFFFFu) le[7] = 0x7FFFFFFFu;   // below p
        le[0] |= 1u;
        if (rnd() % 64 == 0) { memset(le, 0, 32); le[0] = 1 + rnd() % 3; }
        fe z;
        fe_from_le(z, le);
        memcpy(w, z.n, 36);
    }
    static void direct(uint32_t* out8, const uint32_t* w) {
        fe a, r;
        memcpy(a.n, w, 36);
        fe_inv_divsteps(r, a);
        fe_normalize(r);
        fe_to_le(out8, r);
    }
    static void canon(uint32_t* out8, const uint32_t* e9) {
        fe x;
        memcpy(x.n, e9, 36);
        fe_normalize(x);
        fe_to_le(out8, x);
    }
};

template <class Dom>
struct Pool {
    std::vector<uint32_t> in, inv;   // MAXN x LW entry-major, MAXN x 8
    Pool() : in((size_t)MAXN * Dom::LW), inv((size_t)MAXN * 8) {
        for (uint32_t i = 0; i < MAXN; i++) {
            Dom::random(&in[(size_t)i * Dom::LW]);
            Dom::direct(&inv[(size_t)i * 8], &in[(size_t)i * Dom::LW]);
        }
    }
};

// mask: 0 random, 1 whole level-1 lanes dead, 2 whole level-2 lanes dead,
// 3 one live entry, 4 none
template <int K, int K2>
static void make_mask(std::vector<uint8_t>& live, uint32_t N, int mask) {
    const uint32_t T = split_lanes<K>(N), T2 = split_lanes<K2>(T);
    live.assign(N, 0);
    if (mask == 4) return;
    if (mask == 3) {
        live[rnd() % N] = 1;
        return;
    }
    for (uint32_t i = 0; i < N; i++) live[i] = rnd() % 10 < 7;
    if (mask == 1) {
        for (uint32_t t = 0; t < T; t++)
            if (t == 0 || t == T - 1 || rnd() % 3 == 0)
                for (uint32_t j = 0; j < (uint32_t)K; j++)
                    if (j * T + t < N) live[j * T + t] = 0;
    }
    if (mask == 2) {
        for (uint32_t u = 0; u < T2; u++)
            if (u == 0 || u == T2 - 1 || rnd() % 2 == 0)
                for (uint32_t j2 = 0; j2 < (uint32_t)K2; j2++) {
                    const uint32_t t = j2 * T2 + u;
                    if (t >= T) break;
                    for (uint32_t j = 0; j < (uint32_t)K; j++)
                        if (j * T + t < N) live[j * T + t] = 0;
                }
    }
}

template <class Dom, int K, int K2>
static long run(const Pool<Dom>& pool, uint32_t N, int mask) {
    typedef typename Dom::D D;
    const uint32_t n = N + 3;   // the rows' stride: the batch, not the slots in use
    const uint32_t nc = N, T = split_lanes<K>(nc), T2 = split_lanes<K2>(T);
    std::vector<uint8_t> live;
    make_mask<K, K2>(live, N, mask);
    // aux by slot (exactly nc entries: a read past the slots in use is an
    // error), the input row, pre, and the two root rows of 9 T words
    std::vector<uint32_t> aux(nc), in((size_t)Dom::LW * n), pre((size_t)9 * n, POISON);
    std::vector<uint32_t> roots((size_t)9 * T, POISON), rpre((size_t)9 * T, POISON);
    for (uint32_t i = 0; i < nc; i++) {
        aux[i] = (rnd() << 8) | (live[i] ? HD_FAST_LIVE : (rnd() % 2 ? 0x03u : 0xFEu));
        for (int k = 0; k < Dom::LW; k++)
            in[(size_t)k * n + i] = live[i] ? pool.in[(size_t)i * Dom::LW + k] : 0u;   // a dead entry: zero, never multiplied
    }
    for (uint32_t t = 0; t < T; t++) inv2_up<D, K>(t, T, nc, n, aux.data(), in.data(), pre.data(), roots.data());
    for (uint32_t u = 0; u < T2; u++) inv2_mid<D, K2>(u, T2, T, roots.data(), rpre.data());
    for (uint32_t t = 0; t < T; t++) inv2_down<D, K>(t, T, nc, n, aux.data(), in.data(), pre.data(), roots.data());
    // every live entry's inverse against the direct one, every dead entry's
    // pre words untouched; what[]: the two failures' names
    auto check = [&](const char* const what[2]) {
        long checked = 0;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t e[9];
            for (int k = 0; k < 9; k++) e[k] = pre[(size_t)k * n + i];
            if (i < nc && live[i]) {
                uint32_t got[8];
                Dom::canon(got, e);
                if (memcmp(got, &pool.inv[(size_t)i * 8], 32)) fail(what[0], Dom::name(), K, K2, N, mask, i);
                checked++;
            } else {
                for (int k = 0; k < 9; k++)
                    if (e[k] != POISON) fail(what[1], Dom::name(), K, K2, N, mask, i);
            }
        }
        return checked;
    };
    const char* const two[2] = {"inverse differs", "a dead entry was written"};
    const long checked = check(two);
    // the one-level walk (inv2_lean: k_fast_sinv_lean / k_fast_zinv_lean) on the same inputs
    pre.assign(pre.size(), POISON);
    for (uint32_t t = 0; t < T; t++) inv2_lean<D, K>(t, T, nc, n, aux.data(), in.data(), pre.data());
    const char* const one[2] = {"one level: inverse differs", "one level: a dead entry was written"};
    if (check(one) != checked) fail("one level: entries checked", Dom::name(), K, K2, N, mask, checked);
    return checked;
}

template <class Dom, int K, int K2>
static long run_sizes(const Pool<Dom>& pool) {
    const uint32_t sizes[4] = {1, (uint32_t)K * 64, (uint32_t)K * 64 + 1, (uint32_t)K * K2 * 64 + 1};
    long checked = 0;
    for (uint32_t N : sizes)
        for (int mask = 0; mask < 5; mask++) {
            const long c = run<Dom, K, K2>(pool, N, mask);
            if ((mask == 4 && c != 0) || (mask == 3 && c != 1)) fail("mask", Dom::name(), K, K2, N, mask, c);
            checked += c;
        }
    return checked;
}

template <class Dom>
static long run_domain() {
    const Pool<Dom> pool;
    return run_sizes<Dom, 8, 8>(pool) + run_sizes<Dom, 8, 16>(pool) + run_sizes<Dom, 16, 8>(pool) +
           run_sizes<Dom, 16, 16>(pool);
}

int main() {
    const long a = run_domain<ScDom>(), b = run_domain<FeDom>();
    if (a < 50000 || b < 50000) fail("too few entries checked", "both", 0, 0, 0, 0, a + b);
    printf("ok\n");
    return 0;
}
