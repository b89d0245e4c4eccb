// hd_dedup.h -- repeat detection of the known-key check (k_fast_prep,
// hd_fastverify.hip; DESIGN.md §4 "repeats").
//
// NewPrevoteHash and NewPrecommitHash hash byte-identical preimages (SURVEY
// F6: process/message.go:172-186 vs 270-284 -- sha256_vote takes no type) and
// signing is deterministic RFC6979, so a signatory that prevotes
// and then precommits the same value at (height, round) sends the same 65
// signature bytes twice; a replay of a valid message is an exact repeat too.
// The known-key check's verdict, recovered signatory and signer index are a
// function of (digest, From, signature, admitted set) alone, so the check of
// a vote whose (height, round, value, From, signature) equal an earlier
// vote's in the batch is that vote's check.
//
// Per verify call a table of message indices (open addressing, linear
// probing, HD_DD_EMPTY = free) holds the votes that entered the check.  A
// vote hashes words of its signature and From (dd_hash), claims the first
// free slot of its probe sequence with one compare-and-swap, and on a claimed
// slot compares its own input fields with the claimant's (dd_key_equal: every
// byte the check reads).  A full match makes it a repeat of the claimant; a
// mismatch probes on; after HD_DD_PROBES slots it gives up and is checked as
// a distinct message, so a crafted collision flood costs what it cost before.
// Nothing is ever merged on the hash alone.
//
// Calls with a caller-supplied digest (hd_verify_batch_digest_device) key on
// the digest row in place of (height, round, value): the three arrays may be
// absent there, and the digest is what the check reads.
#pragma once
#include "hd_common.h"

namespace hd {

#define HD_DD_PROBES 8u             // slots a vote tries before it counts as distinct
#define HD_DD_EMPTY 0xFFFFFFFFu     // table word: free
// ref[i], the per-message word readers resolve a message's rows through:
//   < 2^30              the message's compact slot (a distinct live message)
//   HD_DD_REPEAT | j    a repeat of message j (ref[j] is j's compact slot)
//   HD_DD_FINAL | code  not in the check: early verdict or HD_NEEDS_SLOW
#define HD_DD_REPEAT 0x80000000u
#define HD_DD_FINAL 0xC0000000u
#define HD_DD_INDEX 0x3FFFFFFFu
#define HD_DD_MAX_N (1u << 30)      // batch sizes the encoding covers

// Every input of a vote's known-key check.  value: the 32 value bytes, or the
// digest row of a call with caller-supplied digests (height = round = 0 then).
struct DdKey {
    int64_t height, round;
    uint32_t value[8], from[8], r[8], s[8];
    uint32_t v;   // the recovery byte, all 8 bits
};

HD bool dd_key_equal(const DdKey& a, const DdKey& b) {
    uint32_t d = (uint32_t)(a.height != b.height) | (uint32_t)(a.round != b.round) | (a.v ^ b.v);
    HD_UNROLL for (int k = 0; k < 8; k++)
        d |= (a.value[k] ^ b.value[k]) | (a.from[k] ^ b.from[k]) | (a.r[k] ^ b.r[k]) | (a.s[k] ^ b.s[k]);
    return d == 0;
}

// The key of message i of a batch of n.  digest32: the caller's digest rows,
// or NULL (then height / round / value32 are read).
HD void dd_key_load(DdKey& k, const int64_t* height, const int64_t* round, const uint8_t* value32,
                    const uint8_t* digest32, const uint8_t* from32, const uint8_t* sig65, size_t i, size_t n) {
    if (digest32) {
        k.height = k.round = 0;
        load_row32_be(k.value, digest32, i);
    } else {
        k.height = height[i];
        k.round = round[i];
        load_row32_be(k.value, value32, i);
    }
    load_row32_be(k.from, from32, i);
    load_sig65(k.r, k.s, k.v, sig65, i, n);
}

// The table hash.  It reads the first and last word of r, of s and of From
// (signature bytes 0-3, 28-31, 32-35, 60-63; From bytes 0-3, 28-31) and
// nothing else: r alone would let one signature's R collide every message
// that reuses it, and From spreads one replayed signature over senders.
HD uint32_t dd_hash(const DdKey& k) {
    uint32_t h = k.r[0] * 0x9E3779B1u;
    h = (h ^ k.r[7]) * 0x85EBCA6Bu;
    h = (h ^ (h >> 15) ^ k.s[0]) * 0xC2B2AE35u;
    h = (h ^ k.s[7]) * 0x27D4EB2Fu;
    h = (h ^ (h >> 13) ^ k.from[0]) * 0x165667B1u;
    h = (h ^ k.from[7]) * 0x9E3779B1u;
    return h ^ (h >> 16);
}

// Table words for a batch of n: a power of two >= 4 n (load <= 1/4), >= 1024.
HD uint32_t dd_table_words(uint32_t n) {
    uint32_t w = 1024u;
    while (w < 4u * (uint64_t)n && w < 0x80000000u) w <<= 1;
    return w;
}

}  // namespace hd
