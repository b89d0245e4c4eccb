// hd_logselect_check.cpp -- the filter and the rank arithmetic of hd_log_select
// (hyperdrive_amd/csrc/hd_logselect.h, the text k_log_sel_count and
// k_log_sel_emit compile) as a stand-alone host program, so that they run as
// plain C++ under ASan + UBSan (tests/test_select_host.py).
//
// The program replays the two passes lane by lane: a block is 4 wavefronts of
// 64 lanes, a wavefront's ballot is built from its lanes' match bits, the
// xor-shuffle sum of a wavefront is the sum over its lanes.  The match flags
// have exactly L entries and the output exactly min(limit or infinity, cap)
// slots, no slack: a read at or beyond L, or a store at or beyond cap, is
// ASan's to catch.
//
// stdin, any number of commands:
//   rank <L> <pos_lo> <pos_hi> <limit> <cap> <L characters 0/1, or - when L = 0>
//     -> r <total> <n> <position of slot 0> ...      (min(n, room) positions)
//   match <type_mask> <flags> <round_lo> <round_hi> <value hex> <from hex>
//         <type> <round> <value hex> <from hex>
//     -> m <0|1>
//   filter <type_mask> <flags> <reserved>
//     -> f <0|1>                                     (log_filter_ok)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../hyperdrive_amd/csrc/hd_logselect.h"

using namespace hd;

static bool hex32(const std::string& s, uint8_t* out) {
    if (s.size() != 64) return false;
    for (int k = 0; k < 32; k++) {
        unsigned x;
        if (sscanf(s.c_str() + 2 * k, "%2x", &x) != 1) return false;
        out[k] = (uint8_t)x;
    }
    return true;
}

// the match bits of wavefront w of block b, as __ballot gives them
static uint64_t ballot_of(const std::vector<uint8_t>& flags, uint32_t lo, uint32_t end, uint32_t b, uint32_t w) {
    uint64_t bal = 0;
    for (uint32_t lane = 0; lane < LOG_SEL_WAVE; lane++) {
        const uint32_t q = lo + b * LOG_SEL_BLOCK + w * LOG_SEL_WAVE + lane;
        if (q < end && flags[q]) bal |= 1ull << lane;   // flags[q] only below end <= L, as the kernel reads its rows
    }
    return bal;
}

static int rank_case() {
    uint32_t L, lo, pos_hi, limit, cap;
    std::string bits;
    if (!(std::cin >> L >> lo >> pos_hi >> limit >> cap >> bits)) return 2;
    if (L == 0) bits.clear();
    if (bits.size() != L) return 2;
    std::vector<uint8_t> flags(L);
    for (uint32_t q = 0; q < L; q++) flags[q] = bits[q] == '1';
    const uint32_t end = log_sel_end(pos_hi, L), nb = log_sel_blocks(lo, end);
    const uint32_t room = log_sel_room(limit, cap);
    std::vector<uint32_t> blk(nb), out(room), hits(room);
    uint32_t total = 0, n = 0;
    // k_log_sel_count
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t wn[LOG_SEL_WAVES];
        for (uint32_t w = 0; w < LOG_SEL_WAVES; w++) wn[w] = (uint32_t)__builtin_popcountll(ballot_of(flags, lo, end, b, w));
        blk[b] = wn[0] + wn[1] + wn[2] + wn[3];
    }
    // k_log_sel_emit
    for (uint32_t b = 0; b < nb; b++) {
        uint32_t part[LOG_SEL_WAVES], wn[LOG_SEL_WAVES];
        uint64_t bal[LOG_SEL_WAVES];
        for (uint32_t w = 0; w < LOG_SEL_WAVES; w++) {
            uint32_t sn = 0;
            for (uint32_t lane = 0; lane < LOG_SEL_WAVE; lane++) sn += log_sel_partial(blk.data(), b, w * LOG_SEL_WAVE + lane);
            part[w] = sn;
            bal[w] = ballot_of(flags, lo, end, b, w);
            wn[w] = (uint32_t)__builtin_popcountll(bal[w]);
        }
        const uint32_t off = part[0] + part[1] + part[2] + part[3];
        if (b == nb - 1) {
            total = off + wn[0] + wn[1] + wn[2] + wn[3];
            n = log_sel_n(total, limit);
        }
        for (uint32_t w = 0; w < LOG_SEL_WAVES; w++)
            for (uint32_t lane = 0; lane < LOG_SEL_WAVE; lane++) {
                if (!((bal[w] >> lane) & 1ull)) continue;
                const uint32_t j = log_sel_rank(off, wn, w, bal[w], lane);
                if (j >= room) continue;
                out.data()[j] = lo + b * LOG_SEL_BLOCK + w * LOG_SEL_WAVE + lane;
                hits.data()[j]++;
            }
    }
    const uint32_t stored = n < room ? n : room;
    for (uint32_t j = 0; j < room; j++)
        if (hits[j] != (j < stored ? 1u : 0u)) return 3;   // every returned slot once, no other slot at all
    printf("r %u %u", total, n);
    for (uint32_t j = 0; j < stored; j++) printf(" %u", out[j]);
    printf("\n");
    return 0;
}

static int match_case() {
    hd_log_filter f;
    memset(&f, 0, sizeof f);
    long long rlo, rhi, round;
    uint32_t type;
    std::string fv, ff, ev, ef;
    if (!(std::cin >> f.type_mask >> f.flags >> rlo >> rhi >> fv >> ff >> type >> round >> ev >> ef)) return 2;
    f.round_lo = rlo;
    f.round_hi = rhi;
    // exact 32-byte buffers on the heap: a compare that runs past byte 31 is ASan's to catch
    std::vector<uint8_t> value(32), from(32);
    if (!hex32(fv, f.value32) || !hex32(ff, f.from32) || !hex32(ev, value.data()) || !hex32(ef, from.data())) return 2;
    printf("m %d\n", log_match(f, type, (int64_t)round, value.data(), from.data()) ? 1 : 0);
    return 0;
}

static int filter_case() {
    hd_log_filter f;
    memset(&f, 0, sizeof f);
    if (!(std::cin >> f.type_mask >> f.flags >> f.reserved)) return 2;
    printf("f %d\n", log_filter_ok(f) ? 1 : 0);
    return 0;
}

int main() {
    std::string word;
    while (std::cin >> word) {
        int rc = 2;
        if (word == "rank") rc = rank_case();
        else if (word == "match") rc = match_case();
        else if (word == "filter") rc = filter_case();
        if (rc) return rc;
    }
    return 0;
}
