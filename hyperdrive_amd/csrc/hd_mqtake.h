// hd_mqtake.h -- which sender queue a delivered row of a consume comes from
// (hd_mq.hip k_mq_take_rows; DESIGN.md §4 "Rows around the path"): plain C++,
// so the locate is tested without a GPU (tests/native/hd_mqtake_check.cpp
// runs this same text).
//
// k_mq_plan leaves off[s] = the delivered rows of the senders before s (an
// exclusive scan in sender order, non-decreasing).  A sender that delivers
// nothing -- outside procsAllowed, or with nothing at or below the consumed
// height -- has the offset of the next one, so offsets repeat and "an s with
// off[s] <= k" is not enough: row k belongs to the LAST such s.  That one
// delivers: its successor's offset (or the total, after the last sender) is
// above k, so its own count is not zero.
#pragma once
#include <stdint.h>

#include "hd_common.h"

namespace hd {

// The sender of delivered row k: the last s in [0, ns) with off[s] <= k.
// Needs ns >= 1 and k < the delivered total (then off[0] = 0 <= k).  Row k is
// entry head[s] + (k - off[s]) of the pool.
HD uint32_t mq_take_locate(const uint32_t* off, uint32_t ns, uint32_t k) {
    uint32_t a = 0, b = ns;   // off[a] <= k; b == ns or off[b] > k
    while (b - a > 1) {
        const uint32_t m = a + (b - a) / 2;
        if (off[m] <= k) a = m;
        else b = m;
    }
    return a;
}

}  // namespace hd
