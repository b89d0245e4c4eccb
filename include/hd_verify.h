/*
 * hd_verify.h -- C ABI of the MI355X batch authenticator + tallier for
 * hyperdrive consensus messages (libhdverify.so).
 *
 * Plain C: pointers and sizes only, no HIP/torch types in the signatures, so
 * that hyperdrive's Go packages can bind it through cgo (INTEGRATION.md shows
 * the binding).  What each entry point replaces in the reference
 * (tuanggolt/hyperdrive @ /root/reference):
 *
 *   hd_verify_batch     the authentication precondition the reference leaves to
 *                       its caller before Replica.Propose/Prevote/Precommit
 *                       (replica/replica.go:153-181; "assumes that the sender
 *                       has already been authenticated", mq/mq.go:85-101,
 *                       process/process.go:95-98): per message
 *                       NewProposeHash / NewPrevoteHash / NewPrecommitHash
 *                       (process/message.go:53-78, 165-186, 263-284) ->
 *                       id.Signature.Signatory(&hash) (message_test.go:152) ->
 *                       Signatory.Equal(From) (message_test.go:154) ->
 *                       procsAllowed[From] (mq/mq.go:49-51).
 *   hd_set_signatories  building procsAllowed from the signatory set
 *                       (replica/replica.go:69-72) and its rebuild on
 *                       ResetHeight (replica/replica.go:136-144).
 *   hd_tally            the first-wins vote logs (process/process.go:823-892)
 *                       and the counting loops of the 2f+1 / f+1 rules
 *                       (process.go:486-494, 534, 574-582, 626-632, 658,
 *                       696-702, 751), for every (height, round) of a batch.
 *   hd_decide           the same plus the propose log (insertPropose,
 *                       process.go:758-819) and the rules' count predicates
 *                       themselves, one row per (height, round).
 *   hd_decide_ordered   the same plus, per rule, the message at which it first
 *                       holds when the batch is inserted one message at a
 *                       time (the rules are tried after every insert,
 *                       process.go:229-269).
 *   hd_decide_catch     either of the two plus the Catcher's calls: each double
 *                       vote, double propose and out-of-turn propose with the
 *                       logged message it contradicts (process.go:771-793,
 *                       838-841, 875-878).
 *   hd_log (hd_log.h)   the same across calls: a height's logs kept on the
 *                       device until the height changes (process.go:710-725).
 *
 * Ownership: all host buffers are caller-owned; the library copies what it
 * needs and keeps no pointer after a call returns.  Device buffers passed to
 * the *_device variants are caller-owned device memory (HBM) on the ctx's
 * device.  Threading: one hd_ctx per caller thread (the reference's Process is
 * single-goroutine, process.go:100-101); distinct contexts may share a device.
 * Errors: per-message failures are verdicts, never error returns; a negative
 * return is an HD_E* code (invalid argument, allocation, device failure).
 */
#ifndef HD_VERIFY_H
#define HD_VERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---------------------------------------------------- */
#define HD_OK 0
#define HD_EINVAL (-1)   /* bad argument (NULL pointer, size mismatch)       */
#define HD_ENOMEM (-2)   /* host or device allocation failed                 */
#define HD_EDEVICE (-3)  /* HIP runtime / kernel failure                     */
#define HD_ECAP (-4)     /* hd_tally_out capacity too small (n_* hold need)  */
#define HD_EAGAIN (-5)   /* hd_tally_collect: more groups than were staged;
                            run hd_tally_device_bitmap on the same inputs   */

/* ---- message types (process/message.go:11-22) ------------------------ */
#define HD_TYPE_PROPOSE 1
#define HD_TYPE_PREVOTE 2
#define HD_TYPE_PRECOMMIT 3

/* ---- per-message verdicts -------------------------------------------- */
#define HD_VERDICT_VALID 0              /* recovered signatory == From, From admitted */
#define HD_VERDICT_BAD_RECID 1          /* V >= 4 (go-ethereum checkSignature)       */
#define HD_VERDICT_BAD_RS 2             /* r or s == 0 or >= n                         */
#define HD_VERDICT_NO_POINT 3           /* x = r (+n) not a curve x-coordinate        */
#define HD_VERDICT_INFINITY 4           /* recovered point at infinity                */
#define HD_VERDICT_SIGNATORY_MISMATCH 5 /* recovered signatory != From                */
#define HD_VERDICT_NOT_ADMITTED 6       /* From not in the admitted signatory set     */
#define HD_VERDICT_BAD_TYPE 7           /* type not Propose/Prevote/Precommit         */
#define HD_VERDICT_NOT_AUTHENTIC 8      /* hd_authenticate_batch_device only: From's
                                           known key does not verify the signature;
                                           the recovery that would name the reason
                                           (NO_POINT, INFINITY or SIGNATORY_MISMATCH)
                                           was skipped                                 */

typedef struct hd_ctx hd_ctx;

/* Structure-of-arrays batch.  Strings are raw bytes: value32 = process.Value
 * ([32]byte), from32 = id.Signatory ([32]byte), sig65 = id.Signature
 * (R || S || V, [65]byte).  valid_round may be NULL when the batch carries no
 * Proposes (then -1 = InvalidRound is used). */
typedef struct {
    uint32_t n;
    const uint8_t* type;
    const int64_t* height;
    const int64_t* round;
    const int64_t* valid_round;
    const uint8_t* value32;
    const uint8_t* from32;
    const uint8_t* sig65;
} hd_batch;

/* ---- context --------------------------------------------------------- */
int hd_ctx_create(int device, hd_ctx** out);
/* Destroy first waits for the context's own stream, its verify calls, and the
 * last work of every caller stream that used its scratch or tables (routes,
 * tallies, digests, codec, generator); other work on the device is not waited
 * for.
 * Streams: a `stream` argument of NULL means the context's own stream, which
 * is created non-blocking: it is NOT ordered after work on the legacy NULL
 * stream (e.g. torch's default stream).  Device inputs produced on another
 * stream must be ordered by the caller (pass that stream, or an event). */
int hd_ctx_destroy(hd_ctx* ctx);
/* The pubkey encoding id.NewSignatory hashes [renproject/id v0.4.2; not
 * confirmable in this container, SURVEY §8(c)]:
 *   HD_PUBKEY_COMPRESSED   (1, default) SHA-256(02|03 || X), 33 bytes
 *   HD_PUBKEY_UNCOMPRESSED (0)          SHA-256(04 || X || Y), 65 bytes
 *   HD_PUBKEY_RAW64        (2)          SHA-256(X || Y), 64 bytes (X, Y 32-byte big-endian)
 *   HD_PUBKEY_XY_STRIPPED  (3)          SHA-256(X.Bytes() || Y.Bytes()), Go big.Int minimal
 *                                       big-endian encodings (leading zero bytes dropped), <= 64 bytes
 * Changing it drops the learned keys of the known-key fast path. */
#define HD_PUBKEY_UNCOMPRESSED 0
#define HD_PUBKEY_COMPRESSED 1
#define HD_PUBKEY_RAW64 2
#define HD_PUBKEY_XY_STRIPPED 3
int hd_ctx_set_pubkey_format(hd_ctx* ctx, int format);
/* Admitted set = procsAllowed.  sigs32: n x 32 bytes, any order, duplicates
 * allowed.  Signer indices reported by the library index this array.
 * Blocking: waits for the context's device work in flight (a verify call
 * still learning keys must not see its slots reassigned), so call it between
 * batches, as ResetHeight does (replica/replica.go:136-144).
 * Known keys (fast path below): every key the context knows, learned or
 * imported, of a signatory that stays admitted is still known on return,
 * whatever the change does to the key tables.  At an unchanged table width
 * its tables stay as they are.  When the new set size makes the context pick
 * another width (narrower or wider), or a table allocation fails and the
 * change retries at the next narrower width, the keys are carried over on the
 * device and their tables are rebuilt at the new width inside this call: the
 * next verify call finds them built.  A carried key that gets no slot at the
 * new width (budget) is dropped.  Three exceptions, which forget every key:
 * a forced width (HD_VAR_KEY_WIDTH != 0) that differs from the current one; a
 * pubkey format change (hd_ctx_set_pubkey_format); and a set change that
 * fails (HD_ENOMEM at every width).  The foreign-key block is emptied on
 * every set change.  No output of a verify or authenticate call depends on
 * any of this. */
int hd_set_signatories(hd_ctx* ctx, const uint8_t* sigs32, uint32_t n);
typedef struct {
    int width_before, width_after;   /* table widths in bits */
    uint32_t kept;      /* keys left READY in place, tables untouched */
    uint32_t carried;   /* keys rebuilt at another width or after a failed allocation */
    uint32_t dropped;   /* known keys lost: signatory left the set, or no slot */
} hd_set_change_info;
/* what the context's last hd_set_signatories did to its known keys;
 * all zero before the first one or with the fast path off */
int hd_ctx_set_change_info(hd_ctx* ctx, hd_set_change_info* out);
/* Public keys of admitted signatories, supplied by the caller (a replica
 * holds its peers' keys, or exported them before it stopped), so that the
 * known-key fast path below does not start cold after a restart or a format
 * change (a set change keeps the keys by itself, see hd_set_signatories).
 * The keys are not trusted: a signatory is SHA-256
 * of its key's encoding, so each key is checked to lie on the curve, hashed
 * in the context's pubkey format and looked up in the admitted set; a key
 * that hashes to no admitted signatory is not stored.  An import changes no
 * output of any verify or authenticate call: it only makes a signatory's key
 * known before its first VALID message instead of after it.
 * Both calls wait for the context's device work in flight and are synchronous
 * (call them between batches, as hd_set_signatories).  Imported keys are kept
 * and dropped exactly as learned ones: kept across hd_set_signatories for
 * signatories that stay admitted, a change of table width included; dropped
 * by a pubkey format change, by a set change to another forced width
 * (HD_VAR_KEY_WIDTH) and by a set change that fails. */
#define HD_KEY_IMPORTED     0  /* slot was empty: key stored, tables built               */
#define HD_KEY_KNOWN        1  /* slot already had a key (necessarily this one)          */
#define HD_KEY_NOT_ADMITTED 2  /* SHA-256(encoding) is not in the admitted set           */
#define HD_KEY_NO_SLOT      3  /* admitted, but no table slot (budget, fast path off,
                                  or the last table mapping failed)                      */
#define HD_KEY_BAD_POINT    4  /* X or Y >= p, or Y^2 != X^3 + 7 (includes (0,0))        */
/* keys64: n x 64 bytes, X || Y, 32-byte big-endian each, on host memory,
 * whatever the pubkey format (the format only decides how the key is hashed).
 * status: n bytes (HD_KEY_*), decided by the slots' states before the call:
 * rows that repeat one key report the same status.  signer: n int32 or NULL:
 * index into the array last given to hd_set_signatories (as the verify calls
 * report it), -1 unless status <= 3 and the key is admitted.  On return every
 * IMPORTED key's tables are built.  HD_EINVAL, before any device work, for a
 * NULL keys64 or status with n > 0; n == 0 is HD_OK. */
int hd_import_keys(hd_ctx* ctx, const uint8_t* keys64, uint32_t n, uint8_t* status, int32_t* signer);
/* For each of the n_adm entries of the array last given to hd_set_signatories
 * (duplicates included): known[i] = 1 and keys64[64 i ..] = X || Y when that
 * signatory's slot holds a key (learned or imported), else 0 and 64 zero
 * bytes.  *n_out = n_adm.  cap < n_adm: HD_ECAP with *n_out = n_adm, nothing
 * written.  Right after a set change it reports the keys that change kept or
 * carried (hd_set_signatories); nothing known after one of its three
 * exceptions: another forced width, a format change, a failed mapping. */
int hd_export_keys(hd_ctx* ctx, uint8_t* keys64, uint8_t* known, uint32_t cap, uint32_t* n_out);
/* Known-key fast path (on by default; HD_VERIFY_FASTPATH=0 in the
 * environment turns it off for new contexts).  The first message of an
 * admitted signatory that verifies VALID through the full recovery teaches
 * the context that signatory's public key; later messages claiming that
 * signatory are checked against the key with fixed-base tables
 * (R == s^-1 (m G + r P)) and only fall back to the full recovery when the
 * check fails.  Verdicts, recovered signatories, signer indices and bitmaps
 * are identical either way.  Keys are kept across hd_set_signatories for
 * signatories that stay admitted (a change of table width included; the
 * exceptions are listed there) and dropped when the pubkey format changes. */
int hd_ctx_set_fastpath(hd_ctx* ctx, int enable);
/* known_keys: admitted signatories whose key tables are built;
 * last_fallback: messages of the last verify call that took the full
 * recovery (either may be NULL; synchronises the device) */
int hd_ctx_fastpath_stats(hd_ctx* ctx, uint32_t* known_keys, uint32_t* last_fallback);
/* Foreign-key slots (HD_VAR_FOREIGN_KEYS): ready_slots = foreign slots whose
 * tables are built; evictions = slotless Froms promoted so far into the slot
 * of a colder foreign key (a From with more recoveries since the last check
 * than twice the slot holder's known-key checks + 4; hd_fbtables.hip
 * fb_evict); checks = eviction checks so far (each waited for the context's
 * earlier verify calls).  Any may be NULL; synchronises the context's calls. */
int hd_ctx_foreign_stats(hd_ctx* ctx, uint32_t* ready_slots, uint32_t* evictions, uint32_t* checks);
/* Repeats of the known-key check (HD_VAR_DEDUP), cumulative since context
 * creation, from device counters: checked = messages that entered the check
 * (known key, valid type, signature in range), repeats = those of them that
 * were exact repeats of an earlier message of their call and were served from
 * its check.  checked - repeats is the number of checks executed.  Either may
 * be NULL; synchronises the context's calls. */
int hd_ctx_dedup_stats(hd_ctx* ctx, uint64_t* checked, uint64_t* repeats);
/* Shared preimages of the known-key check (HD_VAR_PRE_SHARE), cumulative since
 * context creation, from device counters: typed = messages with a type in
 * 1..3 of the calls that shared preimages (those without caller digests),
 * distinct = the preimages those calls hashed (one SHA-256 each, two blocks
 * for a propose).  Either may be NULL; synchronises the context's calls. */
int hd_ctx_preimage_stats(hd_ctx* ctx, uint64_t* typed, uint64_t* distinct);
/* Verify calls that took the overlap path (HD_VAR_SUM_CAP, HD_VAR_LEAN_INV,
 * HD_VAR_SUM_CHAIN), cumulative since context creation, counted on the host
 * when the call is submitted: capped = calls whose k_fast_sums was launched
 * with the LDS reservation, lean = calls that launched the lean inversion
 * kernels, chained = calls whose k_fast_sums was made to wait for the
 * previous call's.  Any pointer may be NULL; host-only. */
int hd_ctx_overlap_stats(hd_ctx* ctx, uint32_t* capped, uint32_t* lean, uint32_t* chained);
/* Levels of the lean inversions (the calls hd_ctx_overlap_stats counts as
 * lean).  2, the default: each of the two inversions runs as three kernels
 * (up, mid, down), and one divstep inversion serves 8 or 16 lanes' products
 * (16 unless the environment variable HD_INV_K2 is 8 at context creation)
 * as well as each lane's 8 or 16 slots.  1: the one lean kernel per inversion,
 * one divstep inversion per lane.  The outputs of a call are the same either
 * way.  set = 1 or 2 sets the value for the calls submitted from then on,
 * set = -1 only reads it; returns the value in force, or HD_EINVAL for a NULL
 * context or any other set.  Taken at context creation from the environment
 * variable HD_INV_LEVELS (1 or 2).  Not a variant key: the call plan and the
 * variant table do not know it.  Host-only. */
int hd_ctx_inv_levels(hd_ctx* ctx, int set);
/* Lean calls by the form of their inversions, cumulative since context
 * creation, counted on the host when the call is submitted: out[0] = calls
 * that launched the two-level form, out[1] = calls that launched the
 * one-level lean kernels (their sum is hd_ctx_overlap_stats' lean).
 * HD_EINVAL for a NULL argument; host-only. */
int hd_ctx_inv_stats(hd_ctx* ctx, uint64_t out[2]);
/* Shape of the known-key check as the context runs it now (for cost models):
 * g_windows / key_windows: fixed-base windows of the G table and of the
 * per-key tables (one table point each; the first is loaded, the rest are
 * mixed additions); msgs_per_inversion: messages that share one inversion of
 * each kind in the last verify call (the split check takes 16 from 2^19
 * expected distinct checked messages up, else 8: the batch size times the
 * share of distinct messages in the latest finished call, so with calls in
 * flight the value can depend on which of them has finished; HD_VAR_SPLIT_K
 * pins it; 2 for the paired kernel).
 * Host-only (no device access); any pointer may be NULL. */
int hd_ctx_fastpath_geometry(hd_ctx* ctx, int* g_windows, int* key_windows, int* msgs_per_inversion);
/* Device-time profile for roofline reports.  While enabled, every verify
 * call of the context records HIP events on its stream around the whole call
 * and around the known-key check's sums kernel (k_fast_sums, the dominant
 * kernel).  hd_ctx_profile_read waits for the recorded events, returns the
 * calls recorded since the last read with their summed milliseconds (either
 * pointer may be NULL; sums_ms covers the calls that ran the kernel, counted
 * in *sums_launches) and clears the record. */
int hd_ctx_profile(hd_ctx* ctx, int enable);
/* Kernel variants of a context, for A/B measurements and for the tests that
 * run every compiled instantiation against the golden fixtures.  Defaults
 * come from the environment at context creation (the variable in brackets);
 * HD_EINVAL for an unknown key or value. */
#define HD_VAR_VERIFY_WAVES 0   /* k_verify register budget, waves per SIMD: 2, 3 (default) or 4 (compressed
                                   pubkeys; the other formats run the 3-wave build) [HD_VERIFY_WAVES] */
#define HD_VAR_SUM_WAVES 1      /* k_fast_sums waves per SIMD: 2, 3 or 4 (128 VGPRs, table points loaded when
                                   used); 0 (default) 4 for batches under two rounds at 3, else 3 [HD_SUM_WAVES] */
#define HD_VAR_SPLIT_K 4        /* messages per inversion of the known-key check: -1 by the number of distinct
                                   checked messages (default), 8 or 16 [HD_FAST_K] */
#define HD_VAR_RECOVER_G 5      /* the full recovery's u1 G: 0 from the fixed-base G table (default), 1 from the
                                   GLV ladder's own 12-bit table [HD_RECOVER_GLV_G] */
#define HD_VAR_KEY_WIDTH 7      /* per-key table windows: 0 by the table budget (default: 22 while every key's
                                   1.48 GB table fits, else 20 (407 MB), else 16 (36 MB), else 13 (5 MB); the
                                   budget is HD_FB_MAX_BYTES or 64 GiB per device, shared by the
                                   process's contexts and bounded by the free memory), or 13, 16, 20, 22;
                                   applies from the next hd_set_signatories [HD_FB_PW] */
#define HD_VAR_WAVE_PRIO 8      /* wave issue priority (s_setprio 0..3) of the known-key check's short kernels
                                   (prep, s / Z inversions, comparison, lift, the leftovers' k_verify): above
                                   k_fast_sums' 0 they keep
                                   their SIMD share while the next call's sums waves share the SIMD
                                   [HD_WAVE_PRIO] */
#define HD_VAR_FOREIGN_KEYS 10  /* table slots (0..64) reserved for authenticated Froms outside the admitted set:
                                   a NOT_ADMITTED recovery teaches the context its key, and later messages of
                                   that From take the known-key check (verdict NOT_ADMITTED, identical to the
                                   recovery's); applies from the next hd_set_signatories (reserved once per
                                   context, when the table budget allows; a later 0 stops using the block); 16 (default),
                                   0 = off [HD_FOREIGN_KEYS] */
#define HD_VAR_SLOW_LIFT 11     /* the known-key check's leftovers: 1 (default) a lift kernel first (x^3 + 7 a
                                   square, else NO_POINT), then the full recovery over the rest; 0 the full
                                   recovery over every leftover (it checks the lift itself) [HD_SLOW_LIFT] */
#define HD_VAR_DEDUP 12         /* repeats in the known-key check: 1 (default) a vote whose height, round,
                                   value, From and 65 signature bytes equal an earlier live vote's of the
                                   same call (the Prevote / Precommit pair of one signatory and value, a
                                   replay) is checked once and every copy gets that check's outputs; 0 no
                                   message is ever marked a repeat (same kernels, same compaction)
                                   [HD_DEDUP] */
#define HD_VAR_PRE_SHARE 15     /* digests of the known-key check: 1 (default) a call without caller digests
                                   hashes each distinct preimage (height, round, value; valid_round too for a
                                   propose) once and every message reads its digest by preimage id; 0 every
                                   message hashes its own (the operator's switch: no adaptive rule)
                                   [HD_PRE_SHARE] */
#define HD_VAR_SUM_CAP 9        /* residency of the 3-wave k_fast_sums: 1 (default) a dynamic-LDS reservation
                                   admits two 256-lane blocks per CU, two waves per SIMD (2 x 168 of 512
                                   VGPRs), so waves of other calls' short kernels fit beside a running sums;
                                   0 three waves per SIMD.  The 2- and 4-wave forms are never capped.  On by
                                   default with keys 13 and 14: the three together measured +2-3 % on 1M C2,
                                   each alone, cap + chain and cap + lean nothing.  None of the three applies to a call
                                   that follows one which left more than 1 / 128 of its messages over from
                                   the known-key check: 30 % adversarial traffic measured 10 % slower with
                                   them.  The rule reads a count the device writes as earlier calls run, so
                                   with such calls in flight a call's path (its speed, never its outputs)
                                   can differ from run to run; hd_ctx_overlap_stats counts the calls that
                                   took it [HD_SUM_CAP] */
#define HD_VAR_LEAN_INV 13      /* the two inversion kernels of calls that take the 2- or 3-wave sums: 1
                                   (default) linear walks whose prefix products go through the rows (97
                                   VGPRs: a wave fits beside a capped sums); 0 K inputs and prefixes, or a
                                   product tree, in registers (368 / 397 VGPRs).  Calls that take the 4-wave
                                   sums (small batches) keep the register forms.  Default and measurement:
                                   see key 9 [HD_LEAN_INV] */
#define HD_VAR_SUM_CHAIN 14     /* k_fast_sums of consecutive calls of a context: 1 (default) a call's sums
                                   waits (on the device) for the previous call's sums when the two calls are
                                   on different streams, so one call's sums runs at a time and the other
                                   calls' short kernels run beside it; 0 no such wait.  Calls that take the
                                   4-wave sums neither wait nor are waited for.  Default and measurement:
                                   see key 9 [HD_SUM_CHAIN] */
/* Keys 3 and 6 (the digit pass and the paired kernel's waves) were measured
 * without gain and removed in round 5: set returns HD_EINVAL for them, get
 * returns their fixed value.  (The cap, the lean inversions and the chain,
 * removed with them, came back in round 12 under their old keys.)  Key 2,
 * k_fast_sums' table-point prefetch depth, went the same way: depth 2 spilt
 * and measured 1-3 % slower, so the depth is fixed
 * (one addition ahead; the 4-wave form loads when used) and get returns 1. */
#define HD_VAR__COUNT 16
int hd_ctx_set_variant(hd_ctx* ctx, int which, int value);
int hd_ctx_get_variant(hd_ctx* ctx, int which, int* value);
int hd_ctx_profile_read(hd_ctx* ctx, uint32_t* calls, double* verify_ms, uint32_t* sums_launches, double* sums_ms);

/* ---- verification ------------------------------------------------------
 * verdict:     n bytes (HD_VERDICT_*), required.
 * recovered32: n x 32 bytes or NULL: recovered signatory (zeros when the
 *              recovery itself failed).
 * valid_bitmap: ceil(n/32) words or NULL: bit i set iff verdict[i] == VALID.
 * Host pointers; synchronous. */
int hd_verify_batch(hd_ctx* ctx, const hd_batch* batch, uint8_t* verdict, uint8_t* recovered32,
                    uint32_t* valid_bitmap);

/* Same, with every pointer (batch fields and outputs) in device memory of the
 * ctx's device; signer (n x int32 or NULL) receives the index of From in the
 * hd_set_signatories array for VALID messages, -1 otherwise.  Enqueued on
 * `stream` (a hipStream_t, NULL = the ctx's stream); asynchronous.  The
 * context keeps three scratch sets used round robin.  Once every admitted
 * signatory's key tables are built, calls issued on different streams run
 * concurrently on the device (a call waits only for the last call that used
 * its scratch set), so a caller that alternates two streams fills the SIMDs
 * one call's low-occupancy kernels leave idle; while keys are still being
 * learned, a call on another stream first waits for the previous call. */
int hd_verify_batch_device(hd_ctx* ctx, const hd_batch* dbatch, uint8_t* d_verdict, uint8_t* d_recovered32,
                           int32_t* d_signer, uint32_t* d_valid_bitmap, void* stream);

/* Authentication only, for the replica ingress: the reference buffers a
 * message only once it is authenticated (process/process.go:95-98,
 * mq/mq.go:85-101) and drops it otherwise, whatever the reason.  Same inputs
 * and ordering as hd_verify_batch_device with verdicts only.  VALID and
 * NOT_ADMITTED are exactly hd_verify_batch_device's; every other message gets
 * a verdict that is neither of them: the same as hd_verify_batch_device's, or
 * HD_VERDICT_NOT_AUTHENTIC where From's key is known and the known-key check
 * fails (then the recovered key is not From's, so the message is not
 * authentic; the full recovery that would classify it is skipped). */
int hd_authenticate_batch_device(hd_ctx* ctx, const hd_batch* dbatch, uint8_t* d_verdict, void* stream);

/* Asynchronous host-buffer verification (the cgo caller's path,
 * replica/replica.go:156-181, without its synchronous upload -> verify ->
 * download): hd_verify_submit queues the upload of `batch`, the verification
 * and the download of the outputs on one of the context's HD_HOST_SLOTS
 * pipelines and returns a ticket; hd_verify_wait(ticket) blocks until the
 * outputs are in the caller's buffers.  Consecutive submits overlap: batch
 * k+1's upload runs under batch k's kernels, and the two pipelines' verify
 * calls under each other.  Inputs in pinned memory (hd_host_alloc) are
 * uploaded by DMA straight from the caller's buffers; pageable inputs are
 * first copied into pinned staging by host threads.  The input buffers must
 * stay unchanged, and the output buffers valid, until the ticket's wait
 * returns.  A submit that reuses a pipeline first completes its previous
 * ticket.  Tickets start at 1; waiting on a completed ticket returns at once. */
#define HD_HOST_SLOTS 3   /* a caller keeps up to 3 in flight: upload, verify and output store of three
                             batches overlap (2 in flight serialise upload + verify + store); more
                             pipelines than the device's 4 hardware queues (with the context's own
                             stream) would share queues and serialise behind each other */
int hd_verify_submit(hd_ctx* ctx, const hd_batch* batch, uint8_t* verdict, uint8_t* recovered32,
                     uint32_t* valid_bitmap, uint64_t* ticket);
int hd_verify_wait(hd_ctx* ctx, uint64_t ticket);
/* Compact host batch (PCIe-lean form of hd_verify_submit, 86 B per vote
 * instead of 146 B).  A replica knows its signatory set and a batch carries
 * few distinct values, so From and value cross PCIe as 16-bit indices:
 *   from_idx[i] <  n_sig: From = row from_idx[i] of the array last passed to
 *                         hd_set_signatories (caller order, duplicates kept;
 *                         n_sig = its length)
 *   from_idx[i] >= n_sig: From = escape32 row from_idx[i] - n_sig (senders
 *                         outside the set, e.g. the NOT_ADMITTED ones)
 *   value_idx[i]:         value = values32 row value_idx[i]
 * The rows are expanded on the device, then verified as hd_verify_submit
 * verifies the expanded batch: verdicts, recovered signatories and bitmaps
 * are byte-identical.  HD_EINVAL (nothing queued) when an index names no
 * row, n_sig + n_escape > 65536 or n_values is 0 or > 65536.  Same ticket
 * semantics as hd_verify_submit; the dictionaries must stay unchanged until
 * the ticket's wait returns too. */
typedef struct {
    uint32_t n;
    const uint8_t* type;
    const int64_t* height;
    const int64_t* round;
    const int64_t* valid_round;   /* NULL: no Proposes (-1 = InvalidRound) */
    const uint16_t* from_idx;     /* n */
    const uint16_t* value_idx;    /* n */
    const uint8_t* sig65;         /* n x 65 */
    uint32_t n_escape;
    const uint8_t* escape32;      /* n_escape x 32 (may be NULL when 0) */
    uint32_t n_values;
    const uint8_t* values32;      /* n_values x 32 */
} hd_batch_compact;
int hd_verify_submit_compact(hd_ctx* ctx, const hd_batch_compact* batch, uint8_t* verdict, uint8_t* recovered32,
                             uint32_t* valid_bitmap, uint64_t* ticket);
/* pinned (page-locked) host memory for inputs the caller fills directly */
int hd_host_alloc(size_t bytes, void** out);
int hd_host_free(void* p);

/* A stream on a hardware queue of its own (a CU-mask stream with every CU
 * set), for a caller's verify or tally streams.  Ordinary streams share the
 * device's few hardware queues (GPU_MAX_HW_QUEUES, 4) round robin, and a
 * cross-stream wait queued in a shared queue holds back the other streams
 * mapped to it.  Destroy with hd_stream_destroy. */
int hd_stream_create_dedicated(hd_ctx* ctx, void** stream);
int hd_stream_destroy(hd_ctx* ctx, void* stream);

/* ---- tally --------------------------------------------------------------
 * Input: a batch and its verdicts.  Candidates are VALID Prevotes and
 * Precommits.  Per (height, round, type, signer) the lowest batch index wins
 * (first-wins, process.go:834-847); later ones are duplicates: identical
 * value -> dropped silently, different value -> what the reference hands to
 * Catcher.CatchDoublePrevote/Precommit (process.go:838-843, 875-880).
 * All output arrays are caller-owned with the given capacities.
 * Values are grouped by their 32 bytes themselves (count_rep names a message
 * carrying the value), so the caller-interned value_id argument SURVEY §8(b)
 * sketches is not needed and not taken. */
typedef struct {
    /* (height, round, type, value) groups, in the batch order of each group's
     * first message (deterministic) */
    uint32_t cap_counts;
    uint32_t n_counts;
    int64_t* count_height;
    int64_t* count_round;
    uint8_t* count_type;
    uint32_t* count_rep;   /* batch index of a message with that value */
    uint32_t* count_n;     /* number of first-wins votes for the value  */
    /* (height, round) groups, in the batch order of each round's first
     * candidate */
    uint32_t cap_hr;
    uint32_t n_hr;
    int64_t* hr_height;
    int64_t* hr_round;
    uint32_t* hr_prevotes;   /* len(PrevoteLogs[r])   */
    uint32_t* hr_precommits; /* len(PrecommitLogs[r]) */
    uint32_t* hr_any;        /* distinct vote signers (TraceLogs[r] without proposes) */
    /* n bytes or NULL: 0 logged, 1 identical duplicate, 2 conflicting
     * duplicate (double vote), 3 not a candidate (of this partition) */
    uint8_t* dup;
    /* cap_hr entries or NULL: batch index of each round's first candidate */
    uint32_t* hr_rep;
} hd_tally_out;

int hd_tally(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, hd_tally_out* out);

/* Same on device-resident inputs (pointers as in hd_verify_batch_device).
 * The logs are keyed by From itself, which equals the recovered signatory of
 * every VALID message.  Results land in the host arrays of `out`;
 * synchronises `stream`. */
int hd_tally_device(hd_ctx* ctx, const hd_batch* dbatch, const uint8_t* d_verdict, hd_tally_out* out, void* stream);

/* Same, with validity given as the valid bitmap of hd_verify_batch_device
 * (e.g. after an all-gather of per-GPU bitmaps over RCCL). */
int hd_tally_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap, hd_tally_out* out,
                           void* stream);

/* Asynchronous form of hd_tally_device_bitmap, for a caller that pipelines
 * batches (the cgo binding's VerifyBatchAsync, bench.py): the tally's kernels
 * and ONE download of its results into the ticket's pinned stage are queued on
 * `stream`, and nothing is waited for.  Once the stream has passed that point
 * (an event recorded after this call, or a stream sync), hd_tally_collect
 * fills `out` exactly as hd_tally_device_bitmap would.  The inputs must stay
 * unchanged until then.  The tallies of one context share device scratch, so
 * issue them all on ONE stream (they then run in its order).  Collect waits
 * (on the host, for the ticket's event) until the download has landed.
 *  - The rows are staged at capacities guessed from earlier tallies (the
 *    largest counts seen + 1/4).  A batch with more groups makes collect return
 *    HD_EAGAIN with nothing written; run hd_tally_device_bitmap on the same
 *    inputs instead.  Collect raises the guesses, so the next submit stages more.
 *  - stage / stage_cap: pinned host memory (hd_host_alloc) of at least
 *    hd_tally_stage_bytes(ctx, n, dup) bytes; a smaller stage makes the
 *    submit return HD_ECAP with `need` set.
 *  - dup != 0 stages the per-message classification too (out->dup of collect).
 * The partitioned and routed tallies (several GPUs) stay synchronous. */
typedef struct {
    void* stage;        /* caller: pinned host buffer                          */
    size_t stage_cap;   /* caller: its size in bytes                           */
    int dup;            /* caller: stage the classification                    */
    uint32_t n;         /* set by the submit: the batch size                   */
    uint32_t H, Cg;     /* set by the submit: staged row capacities            */
    size_t need;        /* set by the submit: stage bytes this submit needed   */
    void* done;         /* library: an event recorded after the download
                           (created by the first submit; hd_tally_ticket_release) */
} hd_tally_ticket;
int hd_tally_device_bitmap_async(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                 hd_tally_ticket* ticket, void* stream);
int hd_tally_collect(hd_ctx* ctx, const hd_tally_ticket* ticket, hd_tally_out* out);   /* waits for `done` */
int hd_tally_ticket_release(hd_tally_ticket* ticket);
size_t hd_tally_stage_bytes(hd_ctx* ctx, uint32_t n, int dup);

/* Partitioned tally for G GPUs: only candidates with
 * hd_tally_partition_of(height, round, nparts) == part are tallied.
 * First-wins is per (height, round, type, signer), so the owner of an
 * (height, round) sees every duplicate of its keys and the partitions' groups
 * are exactly the unpartitioned tally's: their union, ordered by count_rep /
 * hr_rep, is the single-GPU output, and dup merges by taking the minimum over
 * partitions (a non-owner reports 3). */
int hd_tally_device_bitmap_part(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap, uint32_t part,
                                uint32_t nparts, hd_tally_out* out, void* stream);
/* the partition of an (height, round) among nparts (host function) */
uint32_t hd_tally_partition_of(int64_t height, int64_t round, uint32_t nparts);

/* verify + tally with one upload of the batch */
int hd_process_batch(hd_ctx* ctx, const hd_batch* batch, uint8_t* verdict, uint8_t* recovered32,
                     uint32_t* valid_bitmap, hd_tally_out* tally);

/* ---- decide: every round's quorum rules, proposes included ---------------
 * The tally above plus the propose log of process.go:758-819 and the count
 * predicates that read it, one row per (height, round), all on the device.
 *
 * Vote logs: exactly hd_tally's (first-wins per (h, r, type, From)).
 *
 * Propose log per (h, r).  A propose is ELIGIBLE when it is VALID, its round
 * is > -1 (process.go:763) and, with a schedule, its height is > 0 and its
 * From is sched32[(uint64(h) + uint64(r)) % n_sched] (scheduler.go:52;
 * process.go:770-781).  Without a schedule (sched32 NULL) there is no turn
 * check.  Among a round's eligible proposes the lowest batch index is LOGGED
 * (process.go:788-795, 804, 811).  pclass[i]:
 *   0  logged
 *   1  eligible and Equal to the logged one (message.go:83-89: height, round,
 *      valid_round, value, From -- not the signature): dropped silently
 *   2  eligible and not Equal: Catcher.CatchDoublePropose(this, logged)
 *   3  not a propose candidate (not a propose, not VALID, round <= -1, or
 *      height <= 0 with a schedule)
 *   4  VALID propose out of turn: Catcher.CatchOutOfTurnPropose
 * The logged propose is valid (process.go:803) when its value is not NilValue
 * and value_ok[i] is nonzero (value_ok stands in for validator.Valid, run by
 * the caller before the call; NULL: every non-nil value is valid).  A valid
 * logged propose adds its From to the round's trace (813-816); an invalid one
 * is logged but not traced.
 *
 * One row per (h, r) that has a vote candidate or a logged propose, in the
 * batch order of the round's first such message.  bits (thresholds from f):
 *   bit 0 timeout_prevote            prevotes >= 2f+1                  (534)
 *   bit 1 precommit_nil              pv_nil >= 2f+1                (626-632)
 *   bit 2 timeout_precommit_reached  precommits >= 2f+1                (658)
 *   bit 3 timeout_precommit_exact    precommits == 2f+1           (310, 658)
 *   bit 4 skip                       trace >= f+1                      (751)
 *   bit 5 precommit_value            valid propose, pv_value >= 2f+1 (574-582)
 *   bit 6 commit                     valid propose, pc_value >= 2f+1 (696-702)
 *   bit 7 prevote_validround         propose with valid_round > -1,
 *                                    pv_validround >= 2f+1         (486-494)
 * The bits are count predicates over the batch's final logs.  The automaton's
 * step and once-flag gating stays with the caller, and so does the
 * `valid_round < CurrentRound` guard of process.go:481: bit 7 is computed for
 * any valid_round > -1, the propose's own round and later ones included. */
typedef struct {
    uint32_t f;               /* the thresholds are 2f+1 and f+1 */
    uint32_t n_sched;         /* entries of sched32 */
    const uint8_t* sched32;   /* n_sched x 32 bytes (the round-robin order), or NULL */
    const uint8_t* value_ok;  /* n bytes, or NULL */
} hd_decide_in;

typedef struct {
    uint32_t cap;             /* capacity of the row arrays */
    uint32_t n;               /* rows (the need, when HD_ECAP) */
    int64_t* height;
    int64_t* round;
    uint32_t* rep;            /* batch index of the round's first vote candidate or logged propose */
    uint32_t* propose;        /* batch index of the logged propose, or 0xFFFFFFFF */
    uint32_t* prevotes;       /* len(PrevoteLogs[r])   */
    uint32_t* precommits;     /* len(PrecommitLogs[r]) */
    uint32_t* trace;          /* len(TraceLogs[r]): distinct vote signers, +1 for a valid logged
                                 propose whose From is not among them */
    uint32_t* pv_value;       /* first-wins prevotes / precommits of this round for the logged */
    uint32_t* pc_value;       /*   propose's value (0 without a propose) */
    uint32_t* pv_nil;         /* first-wins prevotes for NilValue */
    uint32_t* pv_validround;  /* first-wins prevotes of (h, propose.valid_round) for the propose's
                                 value when a propose is logged and valid_round > -1, else 0 */
    uint8_t* flags;           /* bit 0 a propose is logged, bit 1 it is valid, bit 2 it was traced
                                 and its signer was new to the trace (never set without bit 1) */
    uint8_t* bits;            /* the eight predicates above */
    uint8_t* pclass;          /* n bytes or NULL: the propose classes above */
    uint8_t* dup;             /* n bytes or NULL: hd_tally_out.dup */
} hd_decide_out;

/* Host buffers (as hd_tally); in->sched32 and in->value_ok are host pointers.
 * Whole batch only.  HD_EINVAL for NULL arguments, before any device work;
 * HD_ECAP with out->n set when out->cap is too small. */
int hd_decide(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in,
              hd_decide_out* out);
/* Device inputs (the batch, the valid bitmap of hd_verify_batch_device,
 * in->sched32 and in->value_ok are device pointers), host outputs;
 * synchronises `stream`. */
int hd_decide_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                            const hd_decide_in* in, hd_decide_out* out, void* stream);

/* ---- decide, ordered: the message at which each rule fires ----------------
 * The reference inserts one message at a time and tries its rules after every
 * insert (process.go:229-269); hd_decide's bits describe only the batch's
 * final logs.  The ordered form adds, per row and predicate, the batch index
 * at which the predicate FIRST holds when the batch is inserted in batch
 * order.  The log after messages 0..i is the final log restricted to indices
 * <= i (first-wins is "lowest batch index"), so with q2 = 2f+1, q1 = f+1 (in
 * 64 bits), p the logged propose's index and "k-th" the k-th smallest index:
 *   when[0]  q2-th logged prevote of the round
 *   when[1]  q2-th logged prevote of the round for NilValue
 *   when[2]  q2-th logged precommit of the round
 *   when[3]  == when[2]: the equality first holds there; it holds on the
 *            prefixes ending in [when[3], exact_until), exact_until being the
 *            (q2+1)-th logged precommit of the round
 *   when[4]  q1-th smallest trace entry; a signer's entry is the lowest of its
 *            logged prevote, its logged precommit and, for the From of a valid
 *            logged propose, p
 *   when[5]  valid propose: max(p, q2-th logged prevote for its value)
 *   when[6]  valid propose: max(p, q2-th logged precommit for its value)
 *   when[7]  propose with valid_round > -1: max(p, q2-th logged prevote of
 *            (h, valid_round) for its value) -- possibly a message of another
 *            round
 * HD_WHEN_NEVER where the predicate never holds.  For every bit but 3,
 * when[k] != HD_WHEN_NEVER exactly when hd_decide's bit k is set; bit 3 is
 * set exactly when when[3] != HD_WHEN_NEVER and exact_until == HD_WHEN_NEVER.
 * Sorting the non-NEVER entries by index gives the order in which to feed the
 * automaton.  Row j belongs to row j of the hd_decide_out, which is filled
 * exactly as hd_decide fills it.  Errors as hd_decide; order->cap < out->cap
 * (or a batch of 2^30 messages or more) is HD_EINVAL before any device work. */
#define HD_WHEN_NEVER 0xFFFFFFFFu
typedef struct {
    uint32_t cap;          /* rows of the arrays below; must be >= out->cap */
    uint32_t* when;        /* cap x 8, row-major: when[8*j + k] for row j, bit k */
    uint32_t* exact_until; /* cap */
} hd_decide_order;
int hd_decide_ordered(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in,
                      hd_decide_out* out, hd_decide_order* order);
int hd_decide_ordered_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                    const hd_decide_in* in, hd_decide_out* out, hd_decide_order* order,
                                    void* stream);

/* ---- decide, catch: each offence with the logged message it contradicts ----
 * The reference reports misbehaviour from inside its inserts: the offender and,
 * for three of the four calls, the logged message it contradicts
 * (Catcher.CatchDoublePropose / CatchDoublePrevote / CatchDoublePrecommit /
 * CatchOutOfTurnPropose, process.go:771-793, 838-841, 875-878).  The catch
 * list is those calls for a whole batch: one record (index, kind, against)
 * per message with dup == 2 or pclass 2 or 4, in ascending index -- the order
 * of the reference's calls, since it inserts one message at a time.
 *   kind 1, 2  index is a double Prevote / Precommit (dup == 2); against is the
 *              logged vote of the same (height, round, From): the dup == 0
 *              message of that key
 *   kind 3     index is a double propose (pclass == 2); against is the logged
 *              propose of its round (the row's `propose`)
 *   kind 4     index is an out-of-turn propose (pclass == 4); against is
 *              HD_WHEN_NEVER
 * Identical copies (dup == 1, pclass == 1) have no record.  against < index in
 * every record that names one.
 *
 * hd_decide_catch is hd_decide (order NULL) or hd_decide_ordered (order given)
 * plus the list: out and order are filled exactly as those calls fill them.
 * out->dup and out->pclass may be NULL while the list is asked for; neither
 * is then downloaded.  A votes-only caller passes in->sched32 = NULL.
 * HD_EINVAL, before any device work, for a NULL hd_catch_out or cap > 0 with
 * a NULL array (cap == 0 with NULL arrays only counts); HD_ECAP with caught->n
 * set to the need when n > cap -- if out->cap is too small as well, out->n is
 * set too.  An empty batch has zero records. */
#define HD_CATCH_DOUBLE_PREVOTE   1
#define HD_CATCH_DOUBLE_PRECOMMIT 2
#define HD_CATCH_DOUBLE_PROPOSE   3
#define HD_CATCH_OUT_OF_TURN      4
typedef struct {
    uint32_t cap;       /* capacity of the arrays (0 with NULL arrays: count only) */
    uint32_t n;         /* records (the need, when HD_ECAP) */
    uint32_t* index;    /* ascending */
    uint32_t* against;  /* HD_WHEN_NEVER for kind 4 */
    uint8_t*  kind;
} hd_catch_out;
int hd_decide_catch(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in,
                    hd_decide_out* out, hd_decide_order* order, hd_catch_out* caught);
int hd_decide_catch_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                  const hd_decide_in* in, hd_decide_out* out, hd_decide_order* order,
                                  hd_catch_out* caught, void* stream);

/* ---- multi-GPU in one process ----------------------
 * A context per device plus an RCCL communicator over the devices
 * (ncclCommInitAll); for one caller (a Replica) that owns several GPUs.
 * hd_multi_verify_batch = hd_process_batch over the devices: message i is
 * uploaded to and verified on the device whose contiguous 32-aligned shard
 * holds i (each device receives 1/G of the batch over PCIe); with `tally`
 * non-NULL each device routes its shard's candidates to the owners of their
 * rounds (hd_route_candidates_device) with one grouped ncclSend / ncclRecv
 * over xGMI, every owner tallies what it received (hd_tally_routed_device)
 * and the host merges the disjoint tables into the single-device output
 * (same rows, same order).  Host buffers, synchronous; outputs as
 * hd_verify_batch / hd_tally.  devices: ngpus ordinals (NULL: 0 ..
 * ngpus-1); a device listed twice gets two contexts and the exchange uses
 * device copies (RCCL takes one rank per device).  Not thread-safe (one
 * hd_multi per caller thread). */
typedef struct hd_multi hd_multi;
int hd_multi_create(int ngpus, const int* devices, hd_multi** out);
int hd_multi_destroy(hd_multi* m);
/* number of devices; whether the exchange runs over RCCL (else copies) */
int hd_multi_size(hd_multi* m, int* ngpus, int* uses_rccl);
/* the context of device slot k (fast-path stats etc.), NULL if out of range */
hd_ctx* hd_multi_ctx(hd_multi* m, int k);
/* hd_set_signatories on every context: each keeps or carries its own known
 * keys as that call states, with the same three exceptions (another forced
 * width, a format change, a failed mapping); hd_ctx_set_change_info of
 * hd_multi_ctx(m, k) says what context k did. */
int hd_multi_set_signatories(hd_multi* m, const uint8_t* sigs32, uint32_t n);
int hd_multi_set_pubkey_format(hd_multi* m, int format);
/* hd_import_keys on every context; HD_EDEVICE when the contexts disagree on a
 * status.  hd_export_keys over the contexts: known ORed, each key from the
 * first context that has it. */
int hd_multi_import_keys(hd_multi* m, const uint8_t* keys64, uint32_t n, uint8_t* status, int32_t* signer);
int hd_multi_export_keys(hd_multi* m, uint8_t* keys64, uint8_t* known, uint32_t cap, uint32_t* n_out);
int hd_multi_verify_batch(hd_multi* m, const hd_batch* batch, uint8_t* verdict, uint8_t* recovered32,
                          uint32_t* valid_bitmap, hd_tally_out* tally);

/* ---- synthetic workload (seeded; benchmarks/tests) --------
 * kind 0: votes (signer = i % S, type = 2 + (i/S)%2, h = 1 + i/(2S), r = 0)
 * kind 1: rounds (h = 1; per round 1 Propose + S Prevotes + S Precommits)
 * adv_pct: percentage of messages corrupted by the adversarial classes. */
int hd_gen_keys(hd_ctx* ctx, uint32_t S, uint8_t* signatories32, uint8_t* foreign32);
typedef struct {
    uint8_t* type;
    int64_t* height;
    int64_t* round;
    int64_t* valid_round;
    uint8_t* value32;
    uint8_t* from32;
    uint8_t* sig65;
    int8_t* adv_class; /* may be NULL */
} hd_batch_out;
/* device pointers; messages start .. start+n-1 of the workload. */
int hd_gen_batch_device(hd_ctx* ctx, uint32_t kind, uint64_t start, uint32_t n, uint32_t S, uint32_t adv_pct,
                        const uint8_t* d_signatories32, const uint8_t* d_foreign32, const hd_batch_out* d_out,
                        void* stream);

/* ---- multi-GPU tally routing (the C4 data path) -----------
 * The tally of a batch sharded over G GPUs without replicating the batch:
 * hd_route_candidates_device turns the candidates of one device's shard --
 * VALID Prevotes / Precommits per d_valid_bitmap, global index base_index + i
 * -- into HD_ROUTE_ROW_BYTES rows in d_rows (16-byte aligned, cap_rows rows),
 * grouped by the owner rank of their round (hd_tally_partition_of(h, r,
 * nparts), nparts <= 64) and in index order inside each group; counts[nparts]
 * (host) gets the group sizes (group o starts at row sum(counts[0..o))).
 * Synchronous (one small download); HD_ECAP when cap_rows is too small;
 * HD_EINVAL (nothing written) when a candidate's From is not in the context's
 * current admitted set (the set changed since verification): a row names its
 * signer by admitted index, so such a vote could not be told apart from
 * another non-admitted signer's on the owner.
 * The rows cross xGMI (grouped ncclSend/Recv or an all-to-all); the owner
 * concatenates what it received in source-rank order (= global index order)
 * and calls hd_unroute_device: a device batch (type, height, round, value32,
 * From rebuilt from the admitted set; valid_round -1 if given) and each
 * row's global index; hd_tally_routed_device then tallies it (every row is a
 * candidate; count_rep / hr_rep are global indices; dup is per received row).
 * The owners' tables are disjoint and their union ordered by count_rep /
 * hr_rep is the single-GPU tally.  All contexts need the same admitted set. */
#define HD_ROUTE_ROW_BYTES 64
int hd_route_candidates_device(hd_ctx* ctx, const hd_batch* dshard, const uint32_t* d_valid_bitmap,
                               uint32_t base_index, uint32_t nparts, uint8_t* d_rows, uint32_t cap_rows,
                               uint32_t* counts, void* stream);
/* The same, routing only candidates whose (height, round) is one of the
 * n_rounds pairs (d_round_h[k], d_round_r[k]), sorted lexicographically (as
 * signed int64): the rounds that appear in more than one shard.  A round
 * present in one shard only is complete there, so that shard tallies it
 * itself (hd_tally_device_bitmap, reps + base_index) and keeps only those
 * rows of its local tables; only the shared rounds cross xGMI, to their
 * owners (hd_tally_partition_of).  n_rounds = 0 routes nothing. */
int hd_route_candidates_listed_device(hd_ctx* ctx, const hd_batch* dshard, const uint32_t* d_valid_bitmap,
                                      uint32_t base_index, uint32_t nparts, const int64_t* d_round_h,
                                      const int64_t* d_round_r, uint32_t n_rounds, uint8_t* d_rows,
                                      uint32_t cap_rows, uint32_t* counts, void* stream);
int hd_unroute_device(hd_ctx* ctx, const uint8_t* d_rows, uint32_t n, const hd_batch_out* d_out, uint32_t* d_gidx,
                      void* stream);
int hd_tally_routed_device(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_gidx, hd_tally_out* out,
                           void* stream);

/* ---- misc ------------------------------------------------------------- */
const char* hd_strerror(int code);
/* last HIP error text recorded by the ctx (empty if none) */
const char* hd_ctx_last_error(hd_ctx* ctx);
/* ABI version, bumped on any signature change */
int hd_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* HD_VERIFY_H */
