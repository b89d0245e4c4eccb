/* hd_log.h -- a height's vote and propose logs kept on the device across
 * decide calls.
 *
 * hd_decide_ordered answers "which quorum rules hold and at which message did
 * each fire" for one batch in isolation.  The reference's Process keeps its
 * ProposeLogs / PrevoteLogs / PrecommitLogs / TraceLogs from insert to insert
 * and empties them only when the height changes (process/process.go:710-725);
 * a height's messages arrive over many flushes.  An hd_log is that state for
 * one height: it accepts batch after batch and after each one returns exactly
 * what hd_decide_ordered would return for the whole stream so far.
 *
 * The log retains, in arrival order, every message the reference would have
 * in its logs: each logged vote (dup == 0) and each logged propose
 * (pclass == 0), with the fields decide reads (type, height, round,
 * valid_round, value, From, value_ok).  Equal ignores the signature, so a log
 * keeps none unless hd_log_keep_signatures asks for it; with it each entry is
 * the whole message, signature included, first-wins like every other field: a
 * vote that arrives again with other signature bytes is a duplicate and the
 * entry keeps the first copy's 65 bytes.  An entry's position never changes
 * while the height lasts.  An insert replays
 * [retained entries | batch] through the ordered decide passes: first-wins is
 * "lowest index", every retained entry is the only one of its key and lies
 * below every new message, so each is logged again and the outcome is the
 * one-shot outcome of the whole stream.
 *
 * Indices (rep, propose, when, exact_until) are in joined coordinates: a value
 * below `base` (the entries before the call) is a log position, which the
 * caller has seen in an earlier call's logpos; a value >= base is message
 * (value - base) of this batch.  A rule fired in this call exactly when its
 * `when` is >= base.  Rows are reported for every round of the height that has
 * anything logged, in the order of each round's first logged item.
 *
 * What the log holds can be read back (hd_log_read): a replica snapshots a
 * height's logs with its State and, after a restart, inserts the rows it read
 * -- with their value_ok and verdict VALID -- into a fresh log of the same
 * height, f and schedule, which then holds the same entries at the same
 * positions.  hd_log_insert_evidence returns, with each catch record, both
 * whole messages the reference's Catcher takes, so the caller keeps no copy of
 * the log to turn a log position back into a message.
 *
 * A log uses its context's tally scratch: its calls and the context's
 * tallies and decides go on one stream (the rule for tallies).  A set change
 * on the context between inserts is allowed and changes no output. */
#ifndef HD_LOG_H
#define HD_LOG_H

#include "hd_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hd_log hd_log;

int hd_log_create(hd_ctx* ctx, hd_log** out);
/* the context may be destroyed before or after its logs */
int hd_log_destroy(hd_log* log);
/* Empties the log and sets the height, f (the thresholds are 2f+1 and f+1),
 * the round-robin schedule (n_sched x 32 bytes, copied to the device; NULL: no
 * turn check) and the most entries the log may hold (0: no limit).  A new log
 * is at height 0 with f = 0 and no schedule. */
int hd_log_reset(hd_log* log, int64_t height, uint32_t f, const uint8_t* sched32, uint32_t n_sched,
                 uint32_t max_entries);
/* either output may be NULL */
int hd_log_len(const hd_log* log, int64_t* height, uint32_t* entries);

typedef struct {
    uint32_t base;      /* entries before this insert */
    uint32_t kept;      /* entries this insert added  */
    uint32_t relogged;  /* retained entries logged again by the replay: must equal base */
    uint32_t* logpos;   /* n words or NULL: each message's log position, or HD_WHEN_NEVER */
} hd_log_info;

/* One insert.  A message is a candidate when its verdict is VALID and its
 * height is the log's; any other message comes out as dup 3 / pclass 3 (the
 * reference's inserts reject another height first, process.go:759, 824, 861).
 * out->pclass and out->dup (each optional) have n entries, for this batch's
 * messages only; out->cap and order->cap count rows (order->cap >= out->cap).
 * A batch of n = 0 reports the log as it stands (zero rows on an empty log).
 *
 * HD_EINVAL for NULL arguments or base + n >= 2^30, before any device work;
 * HD_ECAP with out->n set when out->cap is too small; HD_ECAP with info->kept
 * set when the insert would exceed max_entries; HD_EDEVICE when relogged !=
 * base.  Any error leaves the log as it was before the call.
 *
 * Host buffers; value_ok n bytes or NULL. */
int hd_log_insert(hd_log* log, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                  hd_decide_out* out, hd_decide_order* order, hd_log_info* info);
/* Device batch, valid bitmap (hd_verify_batch_device's; bit i is message i of
 * this batch) and value_ok; host outputs; synchronises `stream` (NULL: the
 * context's). */
int hd_log_insert_device_bitmap(hd_log* log, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                const uint8_t* d_value_ok, hd_decide_out* out, hd_decide_order* order,
                                hd_log_info* info, void* stream);

/* The same inserts plus the catch list (hd_catch_out, hd_verify.h) of this
 * batch's messages, in joined coordinates like every other index: a record's
 * index is base + i for message i of this batch; its against is a log position
 * < base when the logged message was kept by an earlier insert (that call's
 * logpos named it), and base + j for message j of this batch otherwise.  A
 * retained entry is never an offender -- it is the only message of its key --
 * and a conflicting message that a later insert brings again is reported
 * again, as the reference would catch it again.  An insert of n = 0 has zero
 * records.  out, order and info are filled exactly as the insert without the
 * list fills them; out->dup and out->pclass may be NULL.
 *
 * HD_EINVAL for a NULL hd_catch_out or cap > 0 with a NULL array; HD_ECAP with
 * caught->n set to the need when the records do not fit (out->n is set too if
 * the rows do not fit either); HD_EDEVICE if a record named a retained entry as
 * its offender.  Like every error these leave the log as it was, so the same
 * insert repeated with enough room succeeds. */
int hd_log_insert_catch(hd_log* log, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                        hd_decide_out* out, hd_decide_order* order, hd_log_info* info, hd_catch_out* caught);
int hd_log_insert_catch_device_bitmap(hd_log* log, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                      const uint8_t* d_value_ok, hd_decide_out* out, hd_decide_order* order,
                                      hd_log_info* info, hd_catch_out* caught, void* stream);

/* Keep each entry's 65 signature bytes (on != 0) or not (0, the default).
 * Allowed only while the log is empty, HD_EINVAL otherwise; the setting
 * survives hd_log_reset.  On a log that keeps signatures every insert of
 * n > 0 messages needs batch->sig65 (HD_EINVAL before any device work). */
int hd_log_keep_signatures(hd_log* log, int on);

/* Rows of whole messages in caller-allocated host columns of cap rows each. */
typedef struct {
    uint32_t cap, n;
    uint8_t* type;
    int64_t *height, *round, *valid_round;
    uint8_t *value32, *from32, *value_ok;
    uint8_t* sig65;         /* NULL: not gathered, not downloaded */
} hd_log_rows;

/* Reads n entries into out: entries first .. first + n - 1 when pos is NULL,
 * else entries pos[0 .. n-1] (host array; any order, repeats allowed).
 * valid_round comes back as stored: the caller's value, or -1 where the
 * inserted batch had no valid_round array.  One gather on the device, one
 * download, one synchronisation of the context's stream; the log is unchanged.
 *
 * HD_EINVAL before any device work for a NULL struct or array (sig65 apart;
 * cap == 0 needs no arrays), cap < n, any position >= entries, or sig65 on a
 * log that keeps no signatures.  n == 0 is HD_OK with out->n = 0. */
int hd_log_read(hd_log* log, const uint32_t* pos, uint32_t first, uint32_t n, hd_log_rows* out);

/* The inserts with the catch list, plus the evidence: row k of offender and
 * row k of against are the whole messages of catch record k (a retained entry
 * from the log, a message of this batch from the batch), gathered on the device
 * in the same call.  The against row of an out-of-turn propose (against ==
 * HD_WHEN_NEVER) is all zero bytes.  Both row sets need cap >= caught->cap
 * (HD_EINVAL otherwise), so the only capacity error is the catch list's own;
 * sig65 in either needs a log that keeps signatures.  Everything else -- the
 * outputs, the errors, the log left as it was by any error -- is
 * hd_log_insert_catch[_device_bitmap]'s. */
typedef struct {
    hd_log_rows offender, against;
} hd_evidence_out;

int hd_log_insert_evidence(hd_log* log, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                           hd_decide_out* out, hd_decide_order* order, hd_log_info* info, hd_catch_out* caught,
                           hd_evidence_out* evidence);
int hd_log_insert_evidence_device_bitmap(hd_log* log, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                         const uint8_t* d_value_ok, hd_decide_out* out, hd_decide_order* order,
                                         hd_log_info* info, hd_catch_out* caught, hd_evidence_out* evidence,
                                         void* stream);

/* ---- keyed reads ------------------------------------------------------------
 * The reference keeps its logs as maps and reads them by key: ProposeLogs[r],
 * PrevoteLogs[r][from], every precommit of round r for value v
 * (process/state.go:44-57).  hd_log_select is that read on the device: the
 * entries of the asked types whose round lies in [round_lo, round_hi] and,
 * when asked, whose value and From equal the filter's, in arrival order
 * (ascending position).  With limit = k it returns the first k of them -- the
 * 2f+1 votes behind a firing of commit are limit = 2f+1 over the positions up
 * to the firing.  The log is unchanged. */
#define HD_LOG_SEL_VALUE 1u
#define HD_LOG_SEL_FROM 2u

typedef struct {
    int64_t  round_lo, round_hi;   /* inclusive; lo > hi selects nothing */
    uint32_t type_mask;            /* bit t: entries of type t, t = 1 Propose, 2 Prevote, 3 Precommit */
    uint32_t flags;                /* HD_LOG_SEL_VALUE: value32 must equal; HD_LOG_SEL_FROM: from32 must equal */
    uint32_t pos_lo, pos_hi;       /* positions [pos_lo, pos_hi); pos_hi is clipped to the log's entries */
    uint32_t limit;                /* 0: every match; k: the first k matches in arrival order */
    uint32_t reserved;             /* 0 */
    uint8_t  value32[32], from32[32];
} hd_log_filter;

typedef struct {
    uint32_t total;   /* matches inside [pos_lo, pos_hi), whatever limit and cap are */
    uint32_t n;       /* returned: min(total, limit or infinity) */
} hd_log_selected;

/* Host outputs.  pos_out: cap words or NULL; rows: NULL, or columns of
 * rows->cap >= cap rows (sig65 only on a log that keeps signatures).  cap == 0
 * with NULL outputs is the count-only form: nothing but the 8-byte header
 * comes down.  One synchronisation of the context's stream while n stays
 * within the staged guess (256 rows, or a quarter more than the last call
 * returned; as the evidence block does it); a larger selection takes a second
 * copy.
 *
 * HD_EINVAL before any device work for a NULL log, filter or sel, a type_mask
 * of 0 or with bits outside 1..3, unknown flags, reserved != 0, rows without
 * its arrays, rows->cap < cap, or sig65 on a log that keeps no signatures.
 * HD_ECAP when n > cap and an output was asked for: sel holds the need,
 * nothing was written, and the same call with enough room succeeds.  An empty
 * log, an empty position range and round_lo > round_hi are HD_OK with zero
 * matches. */
int hd_log_select(hd_log* log, const hd_log_filter* flt, uint32_t* pos_out, uint32_t cap, hd_log_rows* rows,
                  hd_log_selected* sel);

/* Device outputs: d_out's columns (valid_round and sig65 may be NULL;
 * adv_class is ignored), d_value_ok and d_pos (each may be NULL) hold cap
 * rows; rows [0, sel->n) are written on `stream` (NULL: the context's), which
 * is synchronised once to return the counts; no row at or beyond cap is ever
 * written.  value32 and from32 must be 16-byte aligned and the int64 columns
 * 8-byte aligned (HD_EINVAL otherwise; torch and hipMalloc buffers are).
 * d_out may be NULL when cap == 0 (the count-only form).  The columns are
 * inputs of hd_marshal_batch_device, hd_verify_batch_device and the
 * *_device_bitmap calls as they stand.  Errors as hd_log_select. */
int hd_log_select_device(hd_log* log, const hd_log_filter* flt, const hd_batch_out* d_out, uint8_t* d_value_ok,
                         uint32_t* d_pos, uint32_t cap, hd_log_selected* sel, void* stream);

#ifdef __cplusplus
}
#endif
#endif
