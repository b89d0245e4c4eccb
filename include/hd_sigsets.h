/* hd_sigsets.h -- signatory sets resident on the device, apart from the
 * context's admitted set.
 *
 * The reference rebuilds procsAllowed at every ResetHeight
 * (replica/replica.go:136-144), so the certificates a lagging peer receives
 * for many heights fall under several signatory sets, of different sizes and
 * with different f.  An hd_sigsets keeps any number of such sets on the device;
 * hd_check_certificates_sets (hd_cert.h) decides the membership of every
 * certificate against the set that certificate names.  Nothing here reads or
 * changes the context's admitted set (hd_set_signatories), its key tables or
 * its foreign-key block, and a hd_set_signatories on the context between calls
 * changes no output of a check against these sets.
 *
 * Per set the device holds the distinct rows sorted ascending (8 big-endian
 * words each), their hashed index (the admitted table's: open addressing at
 * load factor <= 1/4, keyed by the first 16 bytes of a row) and a descriptor
 * of four words: word offset, slot offset, slot mask, distinct count.
 *
 * Limits.  The offsets are 32-bit: an object holds at most
 * HD_SIGSETS_MAX_ROWS distinct rows over all of its sets and at most
 * HD_SIGSETS_MAX_SETS sets; an add beyond either is HD_EINVAL.
 *
 * One caller thread per object, as for the context; an add or a clear must
 * not run while a check that names the object is in flight (the checks return
 * synchronised). */
#ifndef HD_SIGSETS_H
#define HD_SIGSETS_H

#include "hd_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HD_SIGSETS_MAX_ROWS (1u << 27)   /* distinct rows, summed over the sets */
#define HD_SIGSETS_MAX_SETS (1u << 20)

typedef struct hd_sigsets hd_sigsets;

int hd_sigsets_create(hd_ctx* ctx, hd_sigsets** out);
/* the context may be destroyed before or after its sets */
int hd_sigsets_destroy(hd_sigsets* s);
/* Appends one set of n x 32 bytes: rows in any order, duplicates allowed (as
 * hd_set_signatories); n == 0 is a legal, empty set (sigs32 may then be NULL).
 * *set_id receives the set's id: ids count up from 0 in order of add, and
 * earlier ids stay valid.  HD_EINVAL for NULL arguments or beyond the limits;
 * HD_ENOMEM leaves the object as it was. */
int hd_sigsets_add(hd_sigsets* s, const uint8_t* sigs32, uint32_t n, uint32_t* set_id);
/* forgets every set (the next add returns id 0) and keeps the allocations */
int hd_sigsets_clear(hd_sigsets* s);
/* the rows given to add and how many of them are distinct (either may be
 * NULL); HD_EINVAL for an unknown set_id */
int hd_sigsets_info(const hd_sigsets* s, uint32_t set_id, uint32_t* n_rows, uint32_t* n_distinct);

#ifdef __cplusplus
}
#endif
#endif /* HD_SIGSETS_H */
