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
HD uint32_t dd_hash_words(uint32_t r0, uint32_t r7, uint32_t s0, uint32_t s7, uint32_t f0, uint32_t f7) {
    uint32_t h = r0 * 0x9E3779B1u;
    h = (h ^ r7) * 0x85EBCA6Bu;
    h = (h ^ (h >> 15) ^ s0) * 0xC2B2AE35u;
    h = (h ^ s7) * 0x27D4EB2Fu;
    h = (h ^ (h >> 13) ^ f0) * 0x165667B1u;
    h = (h ^ f7) * 0x9E3779B1u;
    return h ^ (h >> 16);
}
HD uint32_t dd_hash(const DdKey& k) { return dd_hash_words(k.r[0], k.r[7], k.s[0], k.s[7], k.from[0], k.from[7]); }

// Table words for a batch of n: a power of two >= 4 n (load <= 1/4), >= 1024.
HD uint32_t dd_table_words(uint32_t n) {
    uint32_t w = 1024u;
    while (w < 4u * (uint64_t)n && w < 0x80000000u) w <<= 1;
    return w;
}

// ---- shared preimages (k_pre_claim / k_pre_hash; DESIGN.md §4 "preimages") --
// The digest of a message is SHA-256 over (height, round, value) for a vote
// and over (height, round, valid_round, value) for a propose: no type beyond
// that, no sender.  Every signatory of a round signs the same preimage, so a
// call hashes each distinct preimage once.  A second table of message indices
// (same scheme as above: one compare-and-swap on the first free slot of
// HD_DD_PROBES, a full compare on a claimed slot, its own claimant past the
// cutoff) gives every typed message a preimage id.
// pid[i], the per-message word k_fast_prep resolves a digest row through:
//   < 2^30              the message's own preimage id (it is the claimant)
//   HD_DD_REPEAT | j    the preimage of message j (pid[j] is j's id)
//   HD_DD_FINAL         no preimage: a type outside 1..3
struct DdPre {
    uint32_t is_propose;   // 0 or 1
    int64_t valid_round;   // of a propose, else 0
    int64_t height, round;
    uint32_t value[8];
};

// vround may be NULL: a propose then hashes valid_round -1, as k_fast_prep does
HD void dd_pre_load(DdPre& k, bool is_propose, const int64_t* height, const int64_t* round, const int64_t* vround,
                    const uint8_t* value32, size_t i) {
    k.is_propose = is_propose ? 1u : 0u;
    k.valid_round = is_propose ? (vround ? vround[i] : -1) : 0;
    k.height = height[i];
    k.round = round[i];
    load_row32_be(k.value, value32, i);
}

// every byte of the preimage, and which of the two preimage forms it is
HD bool dd_pre_equal(const DdPre& a, const DdPre& b) {
    uint32_t d = (a.is_propose ^ b.is_propose) | (uint32_t)(a.valid_round != b.valid_round) |
                 (uint32_t)(a.height != b.height) | (uint32_t)(a.round != b.round);
    HD_UNROLL for (int k = 0; k < 8; k++) d |= a.value[k] ^ b.value[k];
    return d == 0;
}

// The preimage table's hash: both halves of height and of round, the first
// and last value word (bytes 0-3, 28-31), the form and the low half of
// valid_round.  Heights and rounds that differ in their high words only, and
// the canonical / nil / random values of one round, land on different probe
// sequences; the compare decides in any case.
HD uint32_t dd_pre_hash(const DdPre& k) {
    uint32_t h = ((uint32_t)(uint64_t)k.height) * 0x9E3779B1u;
    h = (h ^ (uint32_t)((uint64_t)k.height >> 32)) * 0x85EBCA6Bu;
    h = (h ^ (h >> 15) ^ (uint32_t)(uint64_t)k.round) * 0xC2B2AE35u;
    h = (h ^ (uint32_t)((uint64_t)k.round >> 32)) * 0x27D4EB2Fu;
    h = (h ^ (h >> 13) ^ k.value[0]) * 0x165667B1u;
    h = (h ^ k.value[7]) * 0x9E3779B1u;
    h = (h ^ (h >> 14) ^ k.is_propose ^ ((uint32_t)(uint64_t)k.valid_round << 1)) * 0x85EBCA6Bu;
    return h ^ (h >> 16);
}

// the claimant's id word behind pid word q (q's own when it is an id); the
// caller loads pid[dd_pid_claimant(q)] when dd_pid_is_ref(q)
HD bool dd_pid_is_ref(uint32_t q) { return (q >> 30) == 2u; }
HD bool dd_pid_is_none(uint32_t q) { return (q >> 30) == 3u; }
HD uint32_t dd_pid_claimant(uint32_t q) { return q & HD_DD_INDEX; }
HD uint32_t dd_pid_ref(uint32_t claimant) { return HD_DD_REPEAT | claimant; }
HD uint32_t dd_pid_resolve(const uint32_t* pid, uint32_t i) {
    uint32_t q = pid[i];
    if (dd_pid_is_ref(q)) q = pid[dd_pid_claimant(q)];
    return q;
}

}  // namespace hd
