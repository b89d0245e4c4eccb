// hd_certcheck.h -- the plan and the per-message arithmetic of
// hd_check_certificates (hd_certcheck.hip k_cert_check; include/hd_cert.h
// states the semantics; DESIGN.md §4 "The certificate check"): plain C++, so
// all of it is tested without a GPU (tests/native/hd_certcheck_check.cpp runs
// this same text lane by lane).
//
// One block of 256 lanes takes one certificate at a time (certificates
// blockIdx, blockIdx + grid, ...) and owns a table of one word per signatory,
// CERT_EMPTY everywhere between certificates.  Per certificate:
//
//   sweep 1  every lane classifies its messages (cert_class).  A clean message
//            does old = atomicMin(table[signer], index) and cert_first reads the
//            answer: old == EMPTY is the signer's first arrival (good + 1);
//            old < index makes this message a repeat; old > index makes message
//            `old` one.  Whatever the lane order, the signer's lowest clean
//            index ends up in the table, every other clean message of that
//            signer has been named a repeat by exactly one lane, and the entry
//            left EMPTY exactly once: good, and the minimum over the offenders,
//            are pure functions of the inputs.
//   reduce   good by sum, first_bad by min: wavefront, then block.
//   sweep 2  the restore: the message whose index the table holds (cert_owns)
//            puts EMPTY back -- a compare-and-swap, so only the entries this
//            certificate wrote are written.
//   finish   one lane classifies message first_bad again for the status.
#pragma once
#include <stdint.h>

#include "../../include/hd_cert.h"
#include "hd_common.h"

namespace hd {

enum : uint32_t { CERT_BLOCK = 256, CERT_WAVE = 64, CERT_EMPTY = 0xFFFFFFFFu };
// What one workgroup may allocate on CDNA4 (160 KiB LDS per CU, all of it
// available to a single workgroup); the kernel's own words (the certificate's
// row and the two accumulators) come out of the same allocation.
enum : uint32_t { CERT_LDS_CDNA4 = 160u * 1024u, CERT_LDS_OWN = 256u };
// Grid caps: 8 blocks a CU on the LDS placement; on the scratch placement one
// block a CU, and fewer while the slices would exceed CERT_SCRATCH_CAP.
enum : uint32_t { CERT_GRID_LDS = 2048u, CERT_GRID_SCRATCH = 256u };
enum : uint64_t { CERT_SCRATCH_CAP = 64ull << 20 };

// classes of a message (0 is clean; a clean message may still be a repeat)
enum : uint32_t { CERT_CLEAN = 0, CERT_NOT_VALID = 1, CERT_WRONG = 2 };

// the largest n_signers whose table lives in LDS
HD uint32_t cert_lds_entries(uint32_t lds_limit) {
    return lds_limit > CERT_LDS_OWN ? (lds_limit - CERT_LDS_OWN) / 4u : 0u;
}

HD hd_cert_plan cert_plan(uint32_t n_signers, uint32_t K, uint32_t lds_limit) {
    hd_cert_plan p;
    p.lds_entries = cert_lds_entries(lds_limit);
    p.in_lds = n_signers <= p.lds_entries ? 1u : 0u;
    if (p.in_lds) {
        p.lds_bytes = (4u * n_signers + 15u) & ~15u;   // <= lds_limit - CERT_LDS_OWN + 12
        p.slice_bytes = 0;
        p.blocks = K < CERT_GRID_LDS ? K : (uint32_t)CERT_GRID_LDS;
    } else {
        p.lds_bytes = 0;
        p.slice_bytes = 4ull * n_signers;
        uint64_t cap = CERT_SCRATCH_CAP / p.slice_bytes;   // slice_bytes > 0: n_signers > lds_entries >= 0
        if (cap < 1) cap = 1;
        if (cap > CERT_GRID_SCRATCH) cap = CERT_GRID_SCRATCH;
        p.blocks = K < cap ? K : (uint32_t)cap;
    }
    p.scratch_bytes = p.blocks * p.slice_bytes;
    return p;
}

// what hd_check_certificates refuses before any device work (n: the batch size)
HD bool cert_row_ok(const hd_cert& c, uint32_t n) {
    return (uint64_t)c.first + c.count <= n && c.quorum != 0 &&
           (c.type == HD_TYPE_PREVOTE || c.type == HD_TYPE_PRECOMMIT) &&
           (c.reserved[0] | c.reserved[1] | c.reserved[2]) == 0;
}

// The certificate's fields as a lane keeps them: the value as 8 big-endian
// words, the form load_row32_be gives a message's value in.
struct CertKey {
    uint32_t type;
    int64_t height, round;
    uint32_t value[8];
};
HD CertKey cert_key(const hd_cert& c) {
    CertKey k;
    k.type = c.type;
    k.height = c.height;
    k.round = c.round;
    for (int w = 0; w < 8; w++) {   // value32 sits at byte 32 of the row: aligned words
        uint32_t le;
        __builtin_memcpy(&le, c.value32 + 4 * w, 4);
        k.value[w] = bswap32(le);
    }
    return k;
}

// Message i's bit of the bitmap and its signer index: true, with the table
// index in *s, only when the bit is set and the index lies in [0, n_signers).
HD bool cert_valid(const uint32_t* bitmap, const int32_t* signer, uint32_t i, uint32_t n_signers, uint32_t* s) {
    if (!((bitmap[i >> 5] >> (i & 31u)) & 1u)) return false;
    const int32_t x = signer[i];
    if (x < 0 || (uint32_t)x >= n_signers) return false;
    *s = (uint32_t)x;
    return true;
}

HD bool cert_fields(const CertKey& k, const uint8_t* type, const int64_t* height, const int64_t* round,
                    const uint8_t* value32, uint32_t i) {
    if (type[i] != k.type || height[i] != k.height || round[i] != k.round) return false;
    uint32_t w[8];
    load_row32_be(w, value32, i);
    uint32_t d = 0;
    for (int j = 0; j < 8; j++) d |= w[j] ^ k.value[j];
    return d == 0;
}

// the class of message i; *s is its table index when the class is CERT_CLEAN
HD uint32_t cert_class(const CertKey& k, const uint8_t* type, const int64_t* height, const int64_t* round,
                       const uint8_t* value32, const uint32_t* bitmap, const int32_t* signer, uint32_t n_signers,
                       uint32_t i, uint32_t* s) {
    if (!cert_valid(bitmap, signer, i, n_signers, s)) return CERT_NOT_VALID;
    if (!cert_fields(k, type, height, round, value32, i)) return CERT_WRONG;
    return CERT_CLEAN;
}

HD uint32_t cert_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// A clean message i after old = atomicMin(&table[s], i): the lane's share of
// good and of the lowest offender.
HD void cert_first(uint32_t old, uint32_t i, uint32_t* good, uint32_t* bad) {
    if (old == CERT_EMPTY) *good += 1;          // this signer's entry left EMPTY here, and only here
    else if (old < i) *bad = cert_min(*bad, i);   // a lower clean message of the signer: i repeats it
    else *bad = cert_min(*bad, old);              // i is lower: `old`, which held the entry, is the repeat
}

// Sweep 2: does message i own table[s], that is, must it put EMPTY back?  The
// kernel does both at once with atomicCAS(&table[s], i, CERT_EMPTY).
HD bool cert_owns(uint32_t entry, uint32_t i) { return entry == i; }

// cls_bad: the class of message `bad` (read only when bad != HD_WHEN_NEVER);
// a clean lowest offender is a repeat
HD uint32_t cert_status(uint32_t count, uint32_t quorum, uint32_t bad, uint32_t cls_bad) {
    if (count < quorum) return HD_CERT_SHORT;
    if (bad == HD_WHEN_NEVER) return HD_CERT_OK;
    return cls_bad == CERT_NOT_VALID ? HD_CERT_BAD_SIGNATURE
                                     : cls_bad == CERT_WRONG ? HD_CERT_WRONG_FIELD : HD_CERT_REPEATED_SENDER;
}

}  // namespace hd
