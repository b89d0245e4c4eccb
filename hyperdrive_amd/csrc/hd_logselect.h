// hd_logselect.h -- the filter and the rank arithmetic of hd_log_select
// (hd_log.hip k_log_sel_count / k_log_sel_emit; DESIGN.md §4 "The retained
// log"): plain C++, so both are tested without a GPU
// (tests/native/hd_logselect_check.cpp runs this same text).
//
// The selection is ordered: match number j, counted in ascending position,
// goes to output slot j.  One lane looks at one position; a block is 256
// lanes in 4 wavefronts of 64.  A lane's slot is
//
//   the matches of the blocks before its block          (log_sel_partial, summed)
// + the matches of the wavefronts before it in the block (wn[0 .. w-1])
// + the matches of the lanes before it in its wavefront  (the ballot's low bits)
//
// and a lane stores only when that slot is below log_sel_room(limit, cap), so
// no store lands at or beyond cap whatever the counts are.
#pragma once
#include <stdint.h>

#include "../../include/hd_log.h"
#include "hd_common.h"

namespace hd {

enum : uint32_t { LOG_SEL_BLOCK = 256, LOG_SEL_WAVE = 64, LOG_SEL_WAVES = LOG_SEL_BLOCK / LOG_SEL_WAVE };
enum : uint32_t { LOG_SEL_TYPES = 0xEu, LOG_SEL_FLAGS = HD_LOG_SEL_VALUE | HD_LOG_SEL_FROM };

// what hd_log_select refuses before any device work
HD bool log_filter_ok(const hd_log_filter& f) {
    return f.type_mask != 0 && (f.type_mask & ~(uint32_t)LOG_SEL_TYPES) == 0 &&
           (f.flags & ~(uint32_t)LOG_SEL_FLAGS) == 0 && f.reserved == 0;
}

HD uint64_t log_sel_load64(const uint8_t* p) {
    uint64_t x;
    __builtin_memcpy(&x, p, 8);
    return x;
}

// all 32 bytes
HD bool log_sel_eq32(const uint8_t* a, const uint8_t* b) {
    uint64_t d = 0;
    for (int k = 0; k < 4; k++) d |= log_sel_load64(a + 8 * k) ^ log_sel_load64(b + 8 * k);
    return d == 0;
}

// Does an entry of this type, round, value and From pass the filter?  (The
// position range is the caller's: a lane outside it never gets here.)
HD bool log_match(const hd_log_filter& f, uint32_t type, int64_t round, const uint8_t* value32,
                  const uint8_t* from32) {
    if (type > 31u || !((f.type_mask >> type) & 1u)) return false;
    if (round < f.round_lo || round > f.round_hi) return false;
    if ((f.flags & HD_LOG_SEL_VALUE) && !log_sel_eq32(value32, f.value32)) return false;
    if ((f.flags & HD_LOG_SEL_FROM) && !log_sel_eq32(from32, f.from32)) return false;
    return true;
}

// The positions looked at: [pos_lo, log_sel_end) -- pos_hi clipped to the L
// retained entries, so a row at or beyond L (scratch of the last insert) is
// never read.  Empty when the result is <= pos_lo.
HD uint32_t log_sel_end(uint32_t pos_hi, uint32_t L) { return pos_hi < L ? pos_hi : L; }
HD uint32_t log_sel_blocks(uint32_t lo, uint32_t end) {
    return end > lo ? (end - lo + LOG_SEL_BLOCK - 1) / LOG_SEL_BLOCK : 0;
}

// slots a call may fill: min(limit or infinity, cap)
HD uint32_t log_sel_room(uint32_t limit, uint32_t cap) { return limit != 0 && limit < cap ? limit : cap; }
// matches a call returns: min(total, limit or infinity)
HD uint32_t log_sel_n(uint32_t total, uint32_t limit) { return limit != 0 && limit < total ? limit : total; }

// Thread t's share of the matches of the blocks before block b: counts
// t, t + 256, ... below b.  The 256 shares add up to the block's offset.
HD uint32_t log_sel_partial(const uint32_t* blk, uint32_t b, uint32_t t) {
    uint32_t s = 0;
    for (uint32_t k = t; k < b; k += LOG_SEL_BLOCK) s += blk[k];
    return s;
}

// The slot of lane `lane` of wavefront w: off is the block's offset, wn the
// block's per-wavefront match counts, ballot the wavefront's match bits.
HD uint32_t log_sel_rank(uint32_t off, const uint32_t* wn, uint32_t w, uint64_t ballot, uint32_t lane) {
    uint32_t r = off;
    for (uint32_t k = 0; k < w; k++) r += wn[k];
    return r + (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}

}  // namespace hd
