/* hd_cert.h -- check many quorum certificates on the device.
 *
 * A quorum certificate is the 2f+1 signed votes behind a firing of commit or
 * prevote_validround (DecideLog.certificate / hd_log_select cut one from the
 * retained log; hd_log_select_device -> hd_marshal_batch_device put it on the
 * wire for a lagging peer).  The reference leaves resynchronisation to its
 * caller (mq/mq.go:16, replica/replica.go:222-235); this is the receiving
 * side: K certificates, each a segment [first, first + count) of one verified
 * batch, are decided in one launch straight after the verification.
 *
 * Semantics.  Each message of a segment has exactly one class, tested in this
 * order:
 *   1. not valid:   its bit of the valid bitmap is clear, or its signer index
 *                   is outside [0, n_signers)
 *   2. wrong field: type, height, round or value32 differs from the
 *                   certificate's
 *   3. repeat:      a clean message with a lower index in the same segment
 *                   has the same signer (clean: valid and matching the fields)
 * Classes 1-3 are offending.  `good` is the number of clean non-repeats (the
 * distinct signatories among the clean messages), `first_bad` the lowest
 * offending batch index (HD_WHEN_NEVER: none), and `status` is SHORT when
 * count < quorum, otherwise the class of message first_bad, otherwise OK.
 * good and first_bad are filled for every status.  A message that is not
 * clean never makes a later message a repeat.  Segments may overlap and may be
 * given in any order; an empty segment is SHORT with good 0.  Every output is
 * a pure function of the inputs. */
#ifndef HD_CERT_H
#define HD_CERT_H

#include "hd_sigsets.h"
#include "hd_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HD_CERT_OK               0
#define HD_CERT_SHORT            1   /* count < quorum */
#define HD_CERT_BAD_SIGNATURE    2   /* lowest offending message is not VALID */
#define HD_CERT_WRONG_FIELD      3   /* ... has another type, height, round or value */
#define HD_CERT_REPEATED_SENDER  4   /* ... repeats the signatory of a lower clean message */
#define HD_CERT_NOT_MEMBER       5   /* hd_check_certificates_sets only: lowest offending message is
                                        authentic, its From outside the certificate's set */

typedef struct {            /* 64 bytes */
    uint32_t first, count;  /* messages [first, first + count) of the batch */
    uint32_t quorum;        /* 2f+1; 0 is HD_EINVAL */
    uint8_t  type;          /* HD_TYPE_PREVOTE or HD_TYPE_PRECOMMIT, else HD_EINVAL */
    uint8_t  reserved[3];   /* 0 */
    int64_t  height, round;
    uint8_t  value32[32];
} hd_cert;

typedef struct {            /* 16 bytes */
    uint32_t status;        /* HD_CERT_* */
    uint32_t good;          /* distinct signatories among the clean messages */
    uint32_t first_bad;     /* batch index of the lowest offending message, or HD_WHEN_NEVER */
    uint32_t reserved;
} hd_cert_result;

/* Device form.  dbatch (type, height, round, value32 are read), d_valid_bitmap
 * and d_signer are the device outputs of hd_verify_batch_device for that batch;
 * n_signers bounds the signer index: the n given to hd_set_signatories.  certs
 * and results are host arrays of K rows.  The call uploads the K rows on
 * `stream` (NULL: the context's), makes one launch for all K, downloads K rows
 * and synchronises the stream once.
 * HD_EINVAL, before any device work and with `results` untouched, for NULL
 * arguments (the columns, the bitmap and d_signer may be NULL only when
 * dbatch->n is 0), a height, round, d_signer or bitmap pointer that is not
 * aligned to its element, first + count > dbatch->n, quorum 0, a type other
 * than Prevote / Precommit, or non-zero reserved bytes in any row.  K == 0 is
 * HD_OK.  The checks of one context share its table scratch: one call at a
 * time (the call returns synchronised, so one caller thread per context, the
 * library's rule, is enough). */
int hd_check_certificates_device(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                 const int32_t* d_signer, uint32_t n_signers, const hd_cert* certs, uint32_t K,
                                 hd_cert_result* results, void* stream);

/* Host form: one upload of `batch`, the context's verification (as
 * hd_process_batch runs it) against the context's signatory set -- whose size
 * is the bound of the signer index -- then the same check on the context's
 * stream; the only synchronisation is the download.  verdict: n bytes
 * (HD_VERDICT_*) or NULL; it tells why a BAD_SIGNATURE message failed.  Errors
 * as the device form, plus HD_EINVAL for a NULL column of a batch of n > 0. */
int hd_check_certificates(hd_ctx* ctx, const hd_batch* batch, const hd_cert* certs, uint32_t K,
                          hd_cert_result* results, uint8_t* verdict);

/* Where the check keeps its per-signer table and how large a grid it launches
 * (hyperdrive_amd/csrc/hd_certcheck.h cert_plan; diagnostics only).  The table
 * has one word per signatory.  It lives in LDS while 4 * n_signers bytes plus
 * the kernel's own words fit what one workgroup may allocate (lds_limit: the
 * smaller of CDNA4's 160 KiB and the current device's sharedMemPerBlock, or
 * the former without a device); above that each block owns a slice of device
 * scratch kept by the context, and the grid is capped so that the scratch
 * stays within 64 MiB (or one slice). */
typedef struct {
    uint32_t in_lds;         /* 1: LDS; 0: device scratch */
    uint32_t blocks;         /* grid (0 only when K == 0) */
    uint32_t lds_bytes;      /* dynamic LDS per block (0 on the scratch placement) */
    uint32_t lds_entries;    /* the largest n_signers whose table lives in LDS */
    uint64_t slice_bytes;    /* scratch per block (0 on the LDS placement) */
    uint64_t scratch_bytes;  /* blocks * slice_bytes */
} hd_cert_plan;
int hd_cert_plan_info(uint32_t n_signers, uint32_t K, hd_cert_plan* plan);

/* ---- several signatory sets in one call -----------------------------------
 * A peer that has fallen behind receives certificates for many heights, and
 * the reference rebuilds procsAllowed at every ResetHeight
 * (replica/replica.go:136-144): those certificates fall under several
 * signatory sets.  Here certificate k is checked under set set_of[k] of an
 * hd_sigsets (hd_sigsets.h), not under the context's admitted set, which the
 * call neither reads for membership nor changes.
 *
 * Semantics.  Each message of a segment has exactly one class, tested in this
 * order:
 *   1. not authentic: its verdict byte is neither HD_VERDICT_VALID nor
 *                     HD_VERDICT_NOT_ADMITTED (the two the ingress treats as
 *                     authenticated: the signature is From's, whatever the
 *                     context's set says about From)
 *   2. not a member:  its from32 is not an entry of set set_of[k]
 *   3. wrong field:   type, height, round or value32 differs from the
 *                     certificate's
 *   4. repeat:        a clean message with a lower index in the same segment
 *                     has the same From -- the same position in the set's
 *                     sorted distinct rows (clean: authentic, a member and
 *                     matching the fields)
 * Classes 1-4 are offending.  good, first_bad and SHORT are exactly as above;
 * status is SHORT when count < quorum, otherwise the class of message
 * first_bad (BAD_SIGNATURE, NOT_MEMBER, WRONG_FIELD, REPEATED_SENDER),
 * otherwise OK.  A message that is not clean never makes a later message a
 * repeat.  Certificates of different sets may overlap and come in any order;
 * an empty set makes every authentic message NOT_MEMBER.  Every output is a
 * pure function of the inputs.
 *
 * The per-signer table has one word per distinct entry of the certificate's
 * set; its placement (hd_cert_plan_info) is decided once per call, by the
 * largest distinct count among the sets the call names.
 *
 * Device form.  dbatch (type, height, round, value32 and from32 are read) and
 * d_verdict, the n verdict bytes hd_verify_batch_device or
 * hd_authenticate_batch_device wrote for that batch.  certs, set_of and
 * results are host arrays of K rows.  One upload of the K rows and their K set
 * ids on `stream` (NULL: the context's), one launch, one download, one
 * synchronisation.  There is no bitmap and no signer array: a signer index
 * names a row of one admitted set and means nothing across sets.
 * HD_EINVAL, before any device work and with `results` untouched, for what
 * hd_check_certificates_device refuses (d_verdict in the place of the bitmap),
 * a NULL sets, set_of or from32, a set_of[k] that `sets` does not hold, `sets`
 * created on another context, or a value32 or from32 that is not 16-byte
 * aligned.  K == 0 is HD_OK.  One call at a time per context, as above. */
int hd_check_certificates_sets_device(hd_ctx* ctx, const hd_sigsets* sets, const hd_batch* dbatch,
                                      const uint8_t* d_verdict, const hd_cert* certs, const uint32_t* set_of,
                                      uint32_t K, hd_cert_result* results, void* stream);

/* Host form: one upload of `batch`, hd_verify_batch_device for the verdicts
 * only -- against whatever set the context has: VALID and NOT_ADMITTED are both
 * authentic -- then the same check on the context's stream; the only
 * synchronisation is the download.  verdict: n bytes (HD_VERDICT_*) or NULL; it
 * tells why a BAD_SIGNATURE message failed.  Errors as the device form, plus
 * HD_EINVAL for a NULL column of a batch of n > 0. */
int hd_check_certificates_sets(hd_ctx* ctx, const hd_sigsets* sets, const hd_batch* batch, const hd_cert* certs,
                               const uint32_t* set_of, uint32_t K, hd_cert_result* results, uint8_t* verdict);

#ifdef __cplusplus
}
#endif
#endif /* HD_CERT_H */
