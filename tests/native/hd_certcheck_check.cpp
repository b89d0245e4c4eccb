// hd_certcheck_check.cpp -- the plan and the per-message arithmetic of
// hd_check_certificates (hyperdrive_amd/csrc/hd_certcheck.h, the text
// k_cert_check compiles) as a stand-alone host program, so that they run as
// plain C++ under ASan + UBSan (tests/test_cert_host.py).
//
// The program replays the kernel lane by lane.  The grid, the table placement
// and the slice size come from cert_plan; block b takes certificates b,
// b + blocks, ...; a block is 4 wavefronts of 64 lanes, lane t of the block
// owns messages first + t, first + t + 256, ... of a segment.  Sweep 1 runs the
// lanes' atomicMin steps one after another in the asked order (0 ascending,
// 1 descending, 2 scattered), feeds each answer to cert_first, sums `good` and
// takes the minimum of `bad` per wavefront and then per block; sweep 2 is the
// restore.  Every column has exactly n entries, the bitmap exactly
// ceil(n / 32) words and every table exactly n_signers words, no slack: a
// read or write outside them is ASan's to catch.  A table that is not all
// CERT_EMPTY when its block is done (or, for small tables, after any
// certificate) ends the program with status 3.
//
// stdin, any number of commands:
//   case <n> <n_signers> <K> <V> <lds_limit> <order>
//     V lines:  <value, 64 hex digits>
//     n lines:  <type> <height> <round> <value id> <valid bit> <signer>
//     K lines:  <first> <count> <quorum> <type> <height> <round> <value id>
//     -> K lines: c <status> <good> <first_bad>
//   plan <n_signers> <K> <lds_limit>
//     -> p <in_lds> <blocks> <lds_bytes> <lds_entries> <slice_bytes> <scratch_bytes>
//          <CERT_LDS_CDNA4> <CERT_LDS_OWN> <CERT_GRID_LDS> <CERT_GRID_SCRATCH> <CERT_SCRATCH_CAP>
//   rowok <first> <count> <quorum> <type> <reserved 0> <reserved 1> <reserved 2> <n>
//     -> k <0|1>                                     (cert_row_ok)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_certcheck.h"

using namespace hd;

static_assert(sizeof(hd_cert) == 64, "hd_cert is 64 bytes");
static_assert(sizeof(hd_cert_result) == 16, "hd_cert_result is 16 bytes");

static bool hex32(const std::string& s, uint8_t* out) {
    if (s.size() != 64) return false;
    for (int k = 0; k < 32; k++) {
        unsigned x;
        if (sscanf(s.c_str() + 2 * k, "%2x", &x) != 1) return false;
        out[k] = (uint8_t)x;
    }
    return true;
}

// atomicMin / atomicCAS of one lane: returns the old word
static uint32_t atomic_min(uint32_t* p, uint32_t x) {
    const uint32_t old = *p;
    if (x < old) *p = x;
    return old;
}
static uint32_t atomic_cas(uint32_t* p, uint32_t expect, uint32_t x) {
    const uint32_t old = *p;
    if (cert_owns(old, expect)) *p = x;
    return old;
}

static bool all_empty(const uint32_t* tab, uint64_t words) {
    for (uint64_t e = 0; e < words; e++)
        if (tab[e] != CERT_EMPTY) return false;
    return true;
}

static int run_case() {
    uint32_t n, n_signers, K, V, lds_limit, order;
    if (!(std::cin >> n >> n_signers >> K >> V >> lds_limit >> order)) return 2;
    std::vector<uint8_t> vals(32 * (size_t)V);
    for (uint32_t v = 0; v < V; v++) {
        std::string h;
        if (!(std::cin >> h) || !hex32(h, vals.data() + 32 * (size_t)v)) return 2;
    }
    // exact heap arrays (new T[0] is a valid zero-size allocation)
    std::unique_ptr<uint8_t[]> type(new uint8_t[n]), value32(new uint8_t[32 * (size_t)n]);
    std::unique_ptr<int64_t[]> height(new int64_t[n]), round(new int64_t[n]);
    std::unique_ptr<int32_t[]> signer(new int32_t[n]);
    const uint32_t words = (n + 31) / 32;
    std::unique_ptr<uint32_t[]> bitmap(new uint32_t[words]);
    for (uint32_t w = 0; w < words; w++) bitmap[w] = 0;
    for (uint32_t i = 0; i < n; i++) {
        long long t, h, r, vid, ok, s;
        if (!(std::cin >> t >> h >> r >> vid >> ok >> s) || vid < 0 || vid >= V) return 2;
        type[i] = (uint8_t)t;
        height[i] = h;
        round[i] = r;
        memcpy(value32.get() + 32 * (size_t)i, vals.data() + 32 * (size_t)vid, 32);
        signer[i] = (int32_t)s;
        if (ok) bitmap[i >> 5] |= 1u << (i & 31);
    }
    std::unique_ptr<hd_cert[]> certs(new hd_cert[K]);
    std::unique_ptr<hd_cert_result[]> res(new hd_cert_result[K]);
    for (uint32_t k = 0; k < K; k++) {
        long long first, count, quorum, t, h, r, vid;
        if (!(std::cin >> first >> count >> quorum >> t >> h >> r >> vid) || vid < 0 || vid >= V) return 2;
        hd_cert& c = certs[k];
        memset(&c, 0, sizeof c);
        c.first = (uint32_t)first;
        c.count = (uint32_t)count;
        c.quorum = (uint32_t)quorum;
        c.type = (uint8_t)t;
        c.height = h;
        c.round = r;
        memcpy(c.value32, vals.data() + 32 * (size_t)vid, 32);
        if (!cert_row_ok(c, n)) return 4;   // the call would have refused it
    }

    const hd_cert_plan p = cert_plan(n_signers, K, lds_limit);
    if (K && p.blocks == 0) return 5;
    if (p.scratch_bytes != p.blocks * p.slice_bytes) return 5;
    if (p.in_lds ? (p.lds_bytes < 4ull * n_signers || p.lds_bytes + CERT_LDS_OWN > lds_limit + 12u || p.slice_bytes)
                 : (p.slice_bytes != 4ull * n_signers || p.lds_bytes))
        return 5;
    // the scratch placement: blocks slices of exactly n_signers words, EMPTY before the launch
    std::unique_ptr<uint32_t[]> scratch(new uint32_t[p.in_lds ? 0 : (size_t)(p.scratch_bytes / 4)]);
    if (!p.in_lds)
        for (uint64_t e = 0; e < p.scratch_bytes / 4; e++) scratch[e] = CERT_EMPTY;

    for (uint32_t b = 0; b < p.blocks; b++) {
        std::unique_ptr<uint32_t[]> lds;
        uint32_t* tab;
        if (p.in_lds) {
            lds.reset(new uint32_t[n_signers]);   // the words the kernel may touch, not the rounded-up allocation
            tab = lds.get();
            for (uint32_t e = 0; e < n_signers; e++) tab[e] = CERT_EMPTY;
        } else {
            tab = scratch.get() + (uint64_t)b * (p.slice_bytes / 4);
        }
        for (uint32_t k = b; k < K; k += p.blocks) {
            const hd_cert& c = certs[k];
            const CertKey key = cert_key(c);
            const uint32_t first = c.first, count = c.count;
            // sweep 1: the atomic steps of every lane, in the asked order
            std::vector<uint64_t> js(count);
            for (uint32_t j = 0; j < count; j++) js[j] = j;
            if (order == 1) std::reverse(js.begin(), js.end());
            if (order == 2)
                std::sort(js.begin(), js.end(), [](uint64_t a, uint64_t b2) {
                    const uint64_t ha = (a * 0x9E3779B97F4A7C15ull) >> 20, hb = (b2 * 0x9E3779B97F4A7C15ull) >> 20;
                    return ha != hb ? ha < hb : a < b2;
                });
            uint32_t good[CERT_BLOCK], bad[CERT_BLOCK];
            for (uint32_t t = 0; t < CERT_BLOCK; t++) good[t] = 0, bad[t] = HD_WHEN_NEVER;
            for (uint64_t j : js) {
                const uint32_t t = (uint32_t)(j % CERT_BLOCK), i = first + (uint32_t)j;
                uint32_t s;
                if (cert_class(key, type.get(), height.get(), round.get(), value32.get(), bitmap.get(), signer.get(),
                               n_signers, i, &s) == CERT_CLEAN)
                    cert_first(atomic_min(&tab[s], i), i, &good[t], &bad[t]);
                else
                    bad[t] = cert_min(bad[t], i);
            }
            // reduce: a wavefront's xor-shuffle sum / minimum is the sum / minimum over its lanes
            uint32_t s_good = 0, s_bad = CERT_EMPTY;
            for (uint32_t w = 0; w < CERT_BLOCK / CERT_WAVE; w++) {
                uint32_t g = 0, m = HD_WHEN_NEVER;
                for (uint32_t lane = 0; lane < CERT_WAVE; lane++) {
                    g += good[w * CERT_WAVE + lane];
                    m = cert_min(m, bad[w * CERT_WAVE + lane]);
                }
                s_good += g;
                s_bad = cert_min(s_bad, m);
            }
            // sweep 2: the restore
            for (uint64_t j : js) {
                const uint32_t i = first + (uint32_t)j;
                uint32_t s;
                if (cert_valid(bitmap.get(), signer.get(), i, n_signers, &s)) (void)atomic_cas(&tab[s], i, CERT_EMPTY);
            }
            if (n_signers <= 1024 && !all_empty(tab, n_signers)) return 3;
            uint32_t s, cls = CERT_CLEAN;
            if (s_bad != HD_WHEN_NEVER)
                cls = cert_class(key, type.get(), height.get(), round.get(), value32.get(), bitmap.get(), signer.get(),
                                 n_signers, s_bad, &s);
            res[k].status = cert_status(count, c.quorum, s_bad, cls);
            res[k].good = s_good;
            res[k].first_bad = s_bad;
            res[k].reserved = 0;
        }
        if (!all_empty(tab, n_signers)) return 3;
    }
    for (uint32_t k = 0; k < K; k++) printf("c %u %u %u\n", res[k].status, res[k].good, res[k].first_bad);
    return 0;
}

static int plan_case() {
    uint32_t n_signers, K, lds_limit;
    if (!(std::cin >> n_signers >> K >> lds_limit)) return 2;
    const hd_cert_plan p = cert_plan(n_signers, K, lds_limit);
    printf("p %u %u %u %u %llu %llu %u %u %u %u %llu\n", p.in_lds, p.blocks, p.lds_bytes, p.lds_entries,
           (unsigned long long)p.slice_bytes, (unsigned long long)p.scratch_bytes, (unsigned)CERT_LDS_CDNA4,
           (unsigned)CERT_LDS_OWN, (unsigned)CERT_GRID_LDS, (unsigned)CERT_GRID_SCRATCH,
           (unsigned long long)CERT_SCRATCH_CAP);
    return 0;
}

static int rowok_case() {
    hd_cert c;
    memset(&c, 0, sizeof c);
    unsigned t, r0, r1, r2;
    uint32_t n;
    if (!(std::cin >> c.first >> c.count >> c.quorum >> t >> r0 >> r1 >> r2 >> n)) return 2;
    c.type = (uint8_t)t;
    c.reserved[0] = (uint8_t)r0;
    c.reserved[1] = (uint8_t)r1;
    c.reserved[2] = (uint8_t)r2;
    printf("k %d\n", cert_row_ok(c, n) ? 1 : 0);
    return 0;
}

int main() {
    std::string word;
    while (std::cin >> word) {
        int rc = 2;
        if (word == "case") rc = run_case();
        else if (word == "plan") rc = plan_case();
        else if (word == "rowok") rc = rowok_case();
        if (rc) return rc;
    }
    return 0;
}
