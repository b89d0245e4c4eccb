// hd_keyimport.h -- one row of hd_import_keys (include/hd_verify.h), written
// once for both builds: the gfx950 kernel of hd_keyimport.hip and the host
// program of tests/native/hd_keyimport_check.cpp run this same text.
//
// A caller's public key is never believed: a signatory is SHA-256 of the
// key's encoding, so the key either hashes to an admitted signatory or it is
// not imported.  The encodings do not all cover both coordinates (the
// compressed one holds X and the parity of Y only), so the curve equation is
// checked first: on the curve, X and the parity fix Y.
#pragma once
#include "../../include/hd_verify.h"
#include "hd_fixedbase.h"
#include "hd_sha256.h"
#include "hd_verify_msg.h"

namespace hd {

// a 32-byte big-endian string (8 big-endian words) >= p, by its bytes
HD bool key_be_ge_p(const uint32_t w[8]) {
    const uint32_t top = w[0] & w[1] & w[2] & w[3] & w[4] & w[5];
    return top == 0xFFFFFFFFu && (w[6] == 0xFFFFFFFFu || (w[6] == 0xFFFFFFFEu && w[7] >= 0xFFFFFC2Fu));
}

// X || Y (32-byte big-endian each) -> an affine point.  false: a coordinate
// is >= p or Y^2 != X^3 + 7 ((0, 0) included: 0 != 7).
HD bool key_parse(ge& q, uint32_t x_be[8], uint32_t y_be[8], const uint8_t* key64) {
    load_row32_be(x_be, key64, 0);
    load_row32_be(y_be, key64, 1);
    if (key_be_ge_p(x_be) || key_be_ge_p(y_be)) return false;
    fe_from_be(q.x, x_be);
    fe_from_be(q.y, y_be);
    fe x2, x3, y2, seven, rhs;
    fe_sqr(x2, q.x);
    fe_mul(x3, x2, q.x);
    fe_set_u32(seven, 7);
    fe_add(rhs, x3, seven);
    fe_sqr(y2, q.y);
    return fe_eq(rhs, y2);   // normalises the difference before the compare
}

// What a key is to a context, short of its slot's state: HD_KEY_BAD_POINT,
// HD_KEY_NOT_ADMITTED, HD_KEY_NO_SLOT, or HD_KEY_IMPORTED for a key with a
// slot (the caller then reads the slot's state: HD_KEY_KNOWN when it already
// holds a key).  idx: the sorted admitted index (-1 unless admitted), slot:
// the table slot (-1 unless the status is HD_KEY_IMPORTED).  adm_slot NULL:
// no slot map (fast path off, or the last table mapping failed).
HD uint8_t key_classify(int fmt, const uint8_t* key64, const AdmIndex& ix, uint32_t n_adm, const int32_t* adm_slot,
                        uint32_t nslots, ge& q, int32_t& idx, int32_t& slot) {
    idx = -1;
    slot = -1;
    uint32_t x_be[8], y_be[8], sig[8];
    if (!key_parse(q, x_be, y_be, key64)) return HD_KEY_BAD_POINT;
    sha256_pubkey(sig, fmt, x_be, y_be, y_be[7] & 1u);
    idx = n_adm ? adm_index_find(ix, sig) : -1;
    if (idx < 0) return HD_KEY_NOT_ADMITTED;
    const int32_t sl = adm_slot ? adm_slot[idx] : -1;
    if (sl < 1 || (uint32_t)sl >= nslots) return HD_KEY_NO_SLOT;   // over the slot cap: no table
    slot = sl;
    return HD_KEY_IMPORTED;
}

}  // namespace hd
