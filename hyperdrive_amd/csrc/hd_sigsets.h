// hd_sigsets.h -- the set builder of hd_sigsets (include/hd_sigsets.h) and the
// per-message arithmetic of hd_check_certificates_sets (hd_certcheck.hip
// k_cert_check_sets; include/hd_cert.h states the semantics; DESIGN.md §4 "The
// certificate check"): plain C++, so all of it is tested without a GPU
// (tests/native/hd_certsets_check.cpp runs this same text lane by lane).
//
// The sweeps are hd_certcheck.h's: cert_first, cert_owns and cert_status are
// used as they stand.  What differs is how a message gets its table index:
// not from the verification's signer column but from the hashed index of the
// set its certificate names (adm_index_find: one or two dependent slot loads
// and one 32-byte compare), and the table has one word per distinct entry of
// that set.  A lane keeps the index of its first CERTSET_KEEP messages for the
// restore; a longer segment looks the later ones up again.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/hd_sigsets.h"
#include "hd_certcheck.h"
#include "hd_verify_msg.h"

namespace hd {

// one more class of a message, beside hd_certcheck.h's
enum : uint32_t { CERT_NOT_MEMBER = 3 };
// indices a lane keeps between sweep 1 and the restore: segments of up to
// CERTSET_KEEP * CERT_BLOCK messages make one lookup per message
enum : uint32_t { CERTSET_KEEP = 4 };

// a set on the device: rows [word_off / 8, word_off / 8 + n) of the row array,
// slots [slot_off, slot_off + mask + 1) of the slot array
struct SigSetDesc {
    uint32_t word_off, slot_off, mask, n;
};

// ---- the builder (host) -------------------------------------------------------------
struct SigSetBuild {
    std::vector<uint32_t> words;   // n_distinct sorted rows, 8 big-endian words each
    std::vector<uint32_t> slot;    // adm_index_slots(n_distinct) slots
    uint32_t n_distinct = 0;
};
// false: more distinct rows than an object may hold (nothing else is checked here)
HD_HOSTONLY bool sigset_build(const uint8_t* sigs32, uint32_t n, SigSetBuild* out) {
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return memcmp(sigs32 + 32 * (size_t)a, sigs32 + 32 * (size_t)b, 32) < 0;
    });
    out->words.clear();
    const uint8_t* last = nullptr;
    uint32_t m = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint8_t* s = sigs32 + 32 * (size_t)order[k];
        if (last && memcmp(s, last, 32) == 0) continue;
        for (int w = 0; w < 8; w++) out->words.push_back(load_be32(s + 4 * w));
        last = s;
        m++;
    }
    out->n_distinct = m;
    if (m > HD_SIGSETS_MAX_ROWS) return false;   // before adm_index_slots: 4 m stays within 32 bits
    const uint32_t slots = adm_index_slots(m);
    out->slot.assign(slots, 0);
    adm_index_build(out->words.data(), m, out->slot.data(), slots);
    return true;
}

// Where a set of m distinct rows and `slots` slots goes behind what an object
// already holds; false beyond the limits of include/hd_sigsets.h.
HD_HOSTONLY bool sigset_place(uint64_t rows_used, uint64_t slots_used, uint64_t n_sets, uint32_t m, uint32_t slots,
                              SigSetDesc* d) {
    if (n_sets >= HD_SIGSETS_MAX_SETS || rows_used + m > HD_SIGSETS_MAX_ROWS) return false;
    if (slots_used + slots > 0xFFFFFFFFull) return false;   // cannot happen within the two limits above
    d->word_off = (uint32_t)(8 * rows_used);   // < 2^30
    d->slot_off = (uint32_t)slots_used;
    d->mask = slots - 1;
    d->n = m;
    return true;
}

// ---- the per-message arithmetic -----------------------------------------------------
// what the ingress treats as authenticated: the signature is From's,
// whether or not From is in the context's admitted set
HD bool certset_authentic(uint8_t verdict) { return verdict == V_VALID || verdict == V_NOT_ADMITTED; }

// the set of one certificate as a lane holds it
struct CertSet {
    const uint32_t* adm;    // its sorted rows
    const uint32_t* slot;   // its slots
    uint32_t mask;
};
HD CertSet certset_of(const uint32_t* words, const uint32_t* slots, const SigSetDesc& d) {
    return CertSet{words + d.word_off, slots + d.slot_off, d.mask};
}

// Message i by verdict byte, set and From alone: CERT_NOT_VALID, CERT_NOT_MEMBER
// or CERT_CLEAN with the From's position in the set's sorted distinct rows in *s.
HD uint32_t certset_member(const CertSet& st, const uint8_t* verdict, const uint8_t* from32, uint32_t i, uint32_t* s) {
    if (!certset_authentic(verdict[i])) return CERT_NOT_VALID;
    uint32_t f[8];
    load_row32_be(f, from32, i);
    const int32_t x = adm_index_find(st.adm, st.slot, st.mask, f);   // an empty set: 16 empty slots, -1 at once
    if (x < 0) return CERT_NOT_MEMBER;
    *s = (uint32_t)x;
    return CERT_CLEAN;
}

// the class of message i; *s is its table index when the class is CERT_CLEAN
HD uint32_t certset_class(const CertKey& k, const uint8_t* type, const int64_t* height, const int64_t* round,
                          const uint8_t* value32, const CertSet& st, const uint8_t* verdict, const uint8_t* from32,
                          uint32_t i, uint32_t* s) {
    const uint32_t c = certset_member(st, verdict, from32, i, s);
    if (c != CERT_CLEAN) return c;
    return cert_fields(k, type, height, round, value32, i) ? (uint32_t)CERT_CLEAN : (uint32_t)CERT_WRONG;
}

// cert_status with the one class it does not know
HD uint32_t certset_status(uint32_t count, uint32_t quorum, uint32_t bad, uint32_t cls_bad) {
    const uint32_t st = cert_status(count, quorum, bad, cls_bad == CERT_NOT_MEMBER ? (uint32_t)CERT_NOT_VALID : cls_bad);
    return st == HD_CERT_BAD_SIGNATURE && cls_bad == CERT_NOT_MEMBER ? (uint32_t)HD_CERT_NOT_MEMBER : st;
}

}  // namespace hd

// The object (hd_sigsets.hip owns it; hd_certcheck.hip reads it).  The host
// keeps every descriptor and row count; the device arrays grow by copy, so a
// set's offsets never change.
struct hd_sigsets {
    hd_ctx* ctx = nullptr;   // compared, never followed, once the context may be gone
    int device = 0;
    uint32_t* d_words = nullptr;
    uint32_t* d_slots = nullptr;
    hd::SigSetDesc* d_desc = nullptr;
    size_t cap_words = 0, cap_slots = 0, cap_desc = 0;   // bytes
    uint64_t rows_used = 0, slots_used = 0;
    std::vector<hd::SigSetDesc> desc;
    std::vector<uint32_t> n_rows;
};
