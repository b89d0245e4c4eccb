// hd_certsets_check.cpp -- the set builder of hd_sigsets and the per-message
// arithmetic of hd_check_certificates_sets (hyperdrive_amd/csrc/hd_sigsets.h
// and hd_certcheck.h, the text k_cert_check_sets compiles) as a stand-alone
// host program, so that they run as plain C++ under ASan + UBSan
// (tests/test_certsets_host.py).
//
// The replay is hd_certcheck_check.cpp's: the grid, the table placement and the
// slice size come from cert_plan, called with the largest distinct count among
// the sets the certificates name; block b takes certificates b, b + blocks, ...;
// lane t of the block owns messages first + t, first + t + 256, ... and keeps
// the table index of its first CERTSET_KEEP messages for the restore, looking
// the later ones up again, as the kernel does.  Sweep 1 runs the lanes' atomicMin
// steps in the asked order (0 ascending, 1 descending, 2 scattered).  The sets
// are placed as hd_sigsets_add places them (sigset_build, sigset_place), in
// row and slot arrays of exactly the size used; every column has exactly n
// entries and every table exactly n_max words: a read or write outside them is
// ASan's to catch.  A table that is not all CERT_EMPTY when its block is done
// ends the program with status 3.
//
// stdin, any number of commands:
//   build <n> <P>
//     n lines:  <row, 64 hex digits>            P lines:  <probe, 64 hex digits>
//     -> b <n_distinct> <slots>
//        n_distinct lines: r <row>              (the sorted distinct rows)
//        n lines: i <index of input row>        P lines: q <index of probe, or -1>
//   case <n> <S> <K> <V> <F> <lds_limit> <order>
//     S sets:   <n_s> then n_s lines <row>
//     V lines:  <value>                         F lines:  <From>
//     n lines:  <type> <height> <round> <value id> <verdict byte> <From id>
//     K lines:  <first> <count> <quorum> <type> <height> <round> <value id> <set id>
//     -> K lines: c <status> <good> <first_bad>
//   place <rows_used> <slots_used> <n_sets> <m> <slots>
//     -> l <0|1> <word_off> <slot_off> <mask> <n>       (sigset_place)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_sigsets.h"

using namespace hd;

static_assert(sizeof(SigSetDesc) == 16, "a set's descriptor is four words");

static bool hex32(const std::string& s, uint8_t* out) {
    if (s.size() != 64) return false;
    for (int k = 0; k < 32; k++) {
        unsigned x;
        if (sscanf(s.c_str() + 2 * k, "%2x", &x) != 1) return false;
        out[k] = (uint8_t)x;
    }
    return true;
}

static bool read_rows(uint32_t n, std::unique_ptr<uint8_t[]>* out) {
    out->reset(new uint8_t[32 * (size_t)n]);
    for (uint32_t k = 0; k < n; k++) {
        std::string h;
        if (!(std::cin >> h) || !hex32(h, out->get() + 32 * (size_t)k)) return false;
    }
    return true;
}

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

static int build_case() {
    uint32_t n, P;
    if (!(std::cin >> n >> P)) return 2;
    std::unique_ptr<uint8_t[]> rows, probes;
    if (!read_rows(n, &rows) || !read_rows(P, &probes)) return 2;
    SigSetBuild b;
    if (!sigset_build(rows.get(), n, &b)) return 4;
    // exact copies: a lookup that leaves the rows or the slots is ASan's to catch
    std::unique_ptr<uint32_t[]> words(new uint32_t[b.words.size()]), slot(new uint32_t[b.slot.size()]);
    std::copy(b.words.begin(), b.words.end(), words.get());
    std::copy(b.slot.begin(), b.slot.end(), slot.get());
    const CertSet st{words.get(), slot.get(), (uint32_t)b.slot.size() - 1};
    printf("b %u %zu\n", b.n_distinct, b.slot.size());
    for (uint32_t k = 0; k < b.n_distinct; k++) {
        printf("r ");
        for (int w = 0; w < 8; w++) printf("%08x", words[8 * (size_t)k + w]);
        printf("\n");
    }
    // through the per-message function, every verdict byte authentic
    std::unique_ptr<uint8_t[]> ok(new uint8_t[std::max(n, P)]);
    for (uint32_t k = 0; k < std::max(n, P); k++) ok[k] = k & 1 ? V_VALID : V_NOT_ADMITTED;
    for (uint32_t k = 0; k < n + P; k++) {
        const uint8_t* base = k < n ? rows.get() : probes.get();
        uint32_t s = 0;
        const uint32_t cls = certset_member(st, ok.get(), base, k < n ? k : k - n, &s);
        if (cls != CERT_CLEAN && cls != CERT_NOT_MEMBER) return 6;
        printf("%c %d\n", k < n ? 'i' : 'q', cls == CERT_CLEAN ? (int)s : -1);
    }
    return 0;
}

static int place_case() {
    unsigned long long rows_used, slots_used, n_sets;
    uint32_t m, slots;
    if (!(std::cin >> rows_used >> slots_used >> n_sets >> m >> slots)) return 2;
    SigSetDesc d{0, 0, 0, 0};
    const bool ok = sigset_place(rows_used, slots_used, n_sets, m, slots, &d);
    printf("l %d %u %u %u %u\n", ok ? 1 : 0, d.word_off, d.slot_off, d.mask, d.n);
    return 0;
}

static int run_case() {
    uint32_t n, S, K, V, F, lds_limit, order;
    if (!(std::cin >> n >> S >> K >> V >> F >> lds_limit >> order)) return 2;
    // the sets, placed as hd_sigsets_add places them
    std::vector<SigSetDesc> desc;
    std::vector<uint32_t> all_words, all_slots;
    uint64_t rows_used = 0, slots_used = 0;
    for (uint32_t q = 0; q < S; q++) {
        uint32_t ns;
        std::unique_ptr<uint8_t[]> rows;
        if (!(std::cin >> ns) || !read_rows(ns, &rows)) return 2;
        SigSetBuild b;
        SigSetDesc d;
        if (!sigset_build(rows.get(), ns, &b)) return 4;
        if (!sigset_place(rows_used, slots_used, desc.size(), b.n_distinct, (uint32_t)b.slot.size(), &d)) return 4;
        if (d.word_off != all_words.size() || d.slot_off != all_slots.size()) return 5;
        all_words.insert(all_words.end(), b.words.begin(), b.words.end());
        all_slots.insert(all_slots.end(), b.slot.begin(), b.slot.end());
        rows_used += b.n_distinct;
        slots_used += b.slot.size();
        desc.push_back(d);
    }
    std::unique_ptr<uint32_t[]> words(new uint32_t[all_words.size()]), slots(new uint32_t[all_slots.size()]);
    std::copy(all_words.begin(), all_words.end(), words.get());
    std::copy(all_slots.begin(), all_slots.end(), slots.get());

    std::unique_ptr<uint8_t[]> vals, froms;
    if (!read_rows(V, &vals) || !read_rows(F, &froms)) return 2;
    std::unique_ptr<uint8_t[]> type(new uint8_t[n]), verdict(new uint8_t[n]), value32(new uint8_t[32 * (size_t)n]),
        from32(new uint8_t[32 * (size_t)n]);
    std::unique_ptr<int64_t[]> height(new int64_t[n]), round(new int64_t[n]);
    for (uint32_t i = 0; i < n; i++) {
        long long t, h, r, vid, vd, fid;
        if (!(std::cin >> t >> h >> r >> vid >> vd >> fid) || vid < 0 || vid >= V || fid < 0 || fid >= F) return 2;
        type[i] = (uint8_t)t;
        height[i] = h;
        round[i] = r;
        verdict[i] = (uint8_t)vd;
        memcpy(value32.get() + 32 * (size_t)i, vals.get() + 32 * (size_t)vid, 32);
        memcpy(from32.get() + 32 * (size_t)i, froms.get() + 32 * (size_t)fid, 32);
    }
    std::unique_ptr<hd_cert[]> certs(new hd_cert[K]);
    std::unique_ptr<uint32_t[]> set_of(new uint32_t[K]);
    std::unique_ptr<hd_cert_result[]> res(new hd_cert_result[K]);
    uint32_t n_max = 0;
    for (uint32_t k = 0; k < K; k++) {
        long long first, count, quorum, t, h, r, vid, sid;
        if (!(std::cin >> first >> count >> quorum >> t >> h >> r >> vid >> sid) || vid < 0 || vid >= V) return 2;
        hd_cert& c = certs[k];
        memset(&c, 0, sizeof c);
        c.first = (uint32_t)first;
        c.count = (uint32_t)count;
        c.quorum = (uint32_t)quorum;
        c.type = (uint8_t)t;
        c.height = h;
        c.round = r;
        memcpy(c.value32, vals.get() + 32 * (size_t)vid, 32);
        if (!cert_row_ok(c, n) || sid < 0 || sid >= (long long)desc.size()) return 4;   // the call would have refused it
        set_of[k] = (uint32_t)sid;
        n_max = std::max(n_max, desc[sid].n);
    }

    const hd_cert_plan p = cert_plan(n_max, K, lds_limit);
    if (K && p.blocks == 0) return 5;
    if (!p.in_lds && p.slice_bytes != 4ull * n_max) return 5;
    std::unique_ptr<uint32_t[]> scratch(new uint32_t[p.in_lds ? 0 : (size_t)(p.scratch_bytes / 4)]);
    if (!p.in_lds)
        for (uint64_t e = 0; e < p.scratch_bytes / 4; e++) scratch[e] = CERT_EMPTY;

    for (uint32_t b = 0; b < p.blocks; b++) {
        std::unique_ptr<uint32_t[]> lds;
        uint32_t* tab;
        if (p.in_lds) {
            lds.reset(new uint32_t[n_max]);   // the words the kernel may touch, not the rounded-up allocation
            tab = lds.get();
            for (uint32_t e = 0; e < n_max; e++) tab[e] = CERT_EMPTY;
        } else {
            tab = scratch.get() + (uint64_t)b * (p.slice_bytes / 4);
        }
        for (uint32_t k = b; k < K; k += p.blocks) {
            const hd_cert& c = certs[k];
            const CertKey key = cert_key(c);
            const CertSet st = certset_of(words.get(), slots.get(), desc[set_of[k]]);
            const uint32_t first = c.first, count = c.count;
            std::vector<uint64_t> js(count);
            for (uint32_t j = 0; j < count; j++) js[j] = j;
            if (order == 1) std::reverse(js.begin(), js.end());
            if (order == 2)
                std::sort(js.begin(), js.end(), [](uint64_t a, uint64_t b2) {
                    const uint64_t ha = (a * 0x9E3779B97F4A7C15ull) >> 20, hb = (b2 * 0x9E3779B97F4A7C15ull) >> 20;
                    return ha != hb ? ha < hb : a < b2;
                });
            uint32_t good[CERT_BLOCK], bad[CERT_BLOCK], keep[CERT_BLOCK][CERTSET_KEEP];
            for (uint32_t t = 0; t < CERT_BLOCK; t++) {
                good[t] = 0, bad[t] = HD_WHEN_NEVER;
                for (uint32_t r = 0; r < CERTSET_KEEP; r++) keep[t][r] = CERT_EMPTY;
            }
            // sweep 1
            for (uint64_t j : js) {
                const uint32_t t = (uint32_t)(j % CERT_BLOCK), i = first + (uint32_t)j;
                uint32_t s;
                if (certset_class(key, type.get(), height.get(), round.get(), value32.get(), st, verdict.get(),
                                  from32.get(), i, &s) == CERT_CLEAN) {
                    if (s >= desc[set_of[k]].n) return 6;   // the table index lies in the certificate's set
                    cert_first(atomic_min(&tab[s], i), i, &good[t], &bad[t]);
                    if (j / CERT_BLOCK < CERTSET_KEEP) keep[t][j / CERT_BLOCK] = s;
                } else {
                    bad[t] = cert_min(bad[t], i);
                }
            }
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
            // sweep 2: the restore, from the kept indices first
            for (uint64_t j : js) {
                const uint32_t t = (uint32_t)(j % CERT_BLOCK), i = first + (uint32_t)j;
                if (j / CERT_BLOCK < CERTSET_KEEP) {
                    const uint32_t s = keep[t][j / CERT_BLOCK];
                    if (s != CERT_EMPTY) (void)atomic_cas(&tab[s], i, CERT_EMPTY);
                } else {
                    uint32_t s;
                    if (certset_member(st, verdict.get(), from32.get(), i, &s) == CERT_CLEAN)
                        (void)atomic_cas(&tab[s], i, CERT_EMPTY);
                }
            }
            if (n_max <= 1024 && !all_empty(tab, n_max)) return 3;
            uint32_t s, cls = CERT_CLEAN;
            if (s_bad != HD_WHEN_NEVER)
                cls = certset_class(key, type.get(), height.get(), round.get(), value32.get(), st, verdict.get(),
                                    from32.get(), s_bad, &s);
            res[k].status = certset_status(count, c.quorum, s_bad, cls);
            res[k].good = s_good;
            res[k].first_bad = s_bad;
            res[k].reserved = 0;
        }
        if (!all_empty(tab, n_max)) return 3;
    }
    for (uint32_t k = 0; k < K; k++) printf("c %u %u %u\n", res[k].status, res[k].good, res[k].first_bad);
    return 0;
}

int main() {
    std::string word;
    while (std::cin >> word) {
        int rc = 2;
        if (word == "case") rc = run_case();
        else if (word == "build") rc = build_case();
        else if (word == "place") rc = place_case();
        if (rc) return rc;
    }
    return 0;
}
