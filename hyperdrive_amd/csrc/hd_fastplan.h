// hd_fastplan.h -- the variant table, and which kernels one call of the known-key check
// (hd_fastverify.hip) launches: plain C++, no HIP, so both are tested without a GPU (tests/test_fastplan.py).
#pragma once
#include <stdint.h>

#include "../../include/hd_verify.h"
#include "hd_fixedbase.h"   // the table widths (HD_FB_W, HD_FB_WW, HD_FB_WX, HD_FB_WN)

// One row per HD_VAR_* key (include/hd_verify.h states each variant's meaning), in key order: the
// variable that sets the default at context creation, the default, and the values
// hd_ctx_set_variant accepts -- lo..hi, or what `ok` says where that is no range.
struct HdVarRow {
    int key;
    const char* env;   // NULL: none
    int dflt, lo, hi;
    bool (*ok)(int);
};
inline const HdVarRow HD_VARIANTS[HD_VAR__COUNT] = {
    {HD_VAR_VERIFY_WAVES, "HD_VERIFY_WAVES", 3, 2, 4, nullptr},
    {HD_VAR_SUM_WAVES, "HD_SUM_WAVES", 0, 0, 0, [](int v) { return v == 0 || (v >= 2 && v <= 4); }},
    // key 2 (k_fast_sums prefetch depth; 2 spilt and lost) and keys 3, 6 (round 5: no
    // gain measured) are retired: set rejects, get reads
    {2, nullptr, 1, 1, 0, nullptr},
    {3, nullptr, 0, 1, 0, nullptr},
    {HD_VAR_SPLIT_K, "HD_FAST_K", -1, 0, 0, [](int v) { return v == -1 || v == 8 || v == 16; }},
    {HD_VAR_RECOVER_G, "HD_RECOVER_GLV_G", 0, 0, 1, nullptr},   // (the variable's presence means 1: hd_ctx_create)
    {6, nullptr, 2, 1, 0, nullptr},
    {HD_VAR_KEY_WIDTH, "HD_FB_PW", 0, 0, 0,
     [](int v) { return v == 0 || v == HD_FB_W || v == HD_FB_WW || v == HD_FB_WN || v == HD_FB_WX; }},
    {HD_VAR_WAVE_PRIO, "HD_WAVE_PRIO", 0, 0, 3, nullptr},
    {HD_VAR_SUM_CAP, "HD_SUM_CAP", 1, 0, 1, nullptr},
    {HD_VAR_FOREIGN_KEYS, "HD_FOREIGN_KEYS", 16, 0, 64, nullptr},
    {HD_VAR_SLOW_LIFT, "HD_SLOW_LIFT", 1, 0, 1, nullptr},
    {HD_VAR_DEDUP, "HD_DEDUP", 1, 0, 1, nullptr},
    {HD_VAR_LEAN_INV, "HD_LEAN_INV", 1, 0, 1, nullptr},
    {HD_VAR_SUM_CHAIN, "HD_SUM_CHAIN", 1, 0, 1, nullptr},
    {HD_VAR_PRE_SHARE, "HD_PRE_SHARE", 1, 0, 1, nullptr},
};
inline bool hd_var_accepts(int key, int value) {
    if (key < 0 || key >= HD_VAR__COUNT) return false;
    const HdVarRow& r = HD_VARIANTS[key];
    return r.ok ? r.ok(value) : value >= r.lo && value <= r.hi;
}

// What fb_plan_call decides from: the context's variants and CU count, the call, and one snapshot
// of the figures earlier calls left (FbWork::est_host; UINT32_MAX = none seen yet): [0] the leftovers
// of the known-key check, [1] those past the lift, [2] the distinct live messages and [3] the batch
// size of the latest finished call.  The device writes them as earlier calls run, so with calls in
// flight a plan -- the call's speed, never its outputs -- is not reproducible from run to run.
struct FbPlanIn {
    const int* var;   // hd_ctx::var
    int n_cu;
    uint32_t n;
    bool auth, caller_digests;   // hd_authenticate_batch_device; the caller supplied the digests
    uint32_t est[4];
};

// Everything decided per call (but the window width, FbWork::wp, and the capped block's LDS bytes).
struct FbCallPlan {
    int k, waves;     // messages per inversion (8 or 16); k_fast_sums waves per SIMD asked for (2, 3, 4)
    // The k_fast_sums<WAVES, WP> launched: sums_waves alone names the form.  sums_pf reports the prefetch
    // depth that form has (0 or 1, as the kernel derives it from WAVES) to the host build's plan export
    // (hdh_fb_plan, tests/native/hd_host_check.cpp), whose layout the plan tests read; no launch reads it.
    int sums_waves, sums_pf;
    bool overlap, capped, lean, chain, share, dedup, lift;   // (capped, lean and chain need overlap)
    uint32_t full, lift_blocks, slow_blocks;   // fallback grids: over the whole batch, k_slow_lift's, k_verify's
};

// Blocks of a grid-stride fallback kernel (k_slow_lift, k_verify over a
// list) for the latest list length seen: 1.25x its blocks, at least 64 (a
// sudden burst of leftovers costs a few grid-stride rounds once), at most
// `full`.
inline uint32_t fb_fallback_blocks(uint32_t est, uint32_t full) {
    if (est == 0xFFFFFFFFu) return full;
    const uint64_t want = ((uint64_t)est * 5 / 4 + 255) / 256, least = full < 64u ? full : 64u;
    return (uint32_t)(want < least ? least : want > full ? full : want);
}

inline FbCallPlan fb_plan_call(const FbPlanIn& in) {
    const int* var = in.var;
    const uint32_t n = in.n, none = 0xFFFFFFFFu;
    const uint64_t cu = in.n_cu > 1 ? (uint64_t)in.n_cu : 1u;
    FbCallPlan p{};
    // Messages per inversion of the known-key check (HD_VAR_SPLIT_K): 8 or 16;
    // -1 (default) by size: 16 from 2^19 expected slots up, else 8 (before
    // round 7: from 2^20 - 2^16 messages up, 65,536 lanes, one wave per SIMD).  The inversion kernels are bound by their
    // dependent ALU chains; halving the inversions outweighs the lost second wave
    // per SIMD (1M C2 messages, one box, scalars and prefixes in registers:
    // k_fast_sinv 102 -> 91 us, k_fast_zinv 91 -> 76 us from K = 8 to 16; with the
    // rows in HBM between steps K = 4 / 8 / 16 gave 177 / 111 / 90 and 166 / 102
    // / 85 us)
    // The lanes are the distinct live messages, not the batch (repeats take no
    // slot).  The rule looks at this call's n times the slot share of the latest
    // finished call (its slots and its n, which k_fast_sinv stores into pinned
    // memory: no host sync), so a call of another size after it is still judged
    // by its own size.  Any K is correct; a stale share only picks the other one.
    // Before any call has finished the share is 1.
    uint64_t lanes = n;
    const uint32_t seen = in.est[2], of = in.est[3];
    // (a call in which nothing entered the check -- keys still unknown -- says nothing about the share)
    if (seen != none && of != none && seen != 0 && seen <= of) lanes = (uint64_t)n * seen / of;
    // Round 7, C2 with repeats merged (~623k slots, 609 waves at K = 16): K = 16
    // 1,063 M msgs/s against 1,044-1,048 M at K = 8, so the rule's threshold
    // came down from 2^20 - 2^16 to 2^19 slots; C3's 128k messages measured
    // K = 8 faster (round 6), and nothing between the two has been measured.
    p.k = var[HD_VAR_SPLIT_K] > 0 ? var[HD_VAR_SPLIT_K] : lanes >= (1u << 19) ? 16 : 8;
    // k_fast_sums waves per SIMD for a batch of n (HD_VAR_SUM_WAVES).
    // 0 (the default): 4 waves per SIMD for a batch that fills fewer than two
    // rounds at 3 (C3's 128k messages: +5 %; measured 3 % slower per 1M, where
    // 3 waves keep the loaded-ahead table points)
    p.waves = var[HD_VAR_SUM_WAVES] ? var[HD_VAR_SUM_WAVES] : (uint64_t)n < 2ull * 3 * 4 * 64 * cu ? 4 : 3;
    // Whether a call of n messages takes the overlap path (HD_VAR_SUM_CAP,
    // HD_VAR_LEAN_INV, HD_VAR_SUM_CHAIN, each where its variant is on): not with
    // the 4-wave sums (small batches), and not while the latest call left more
    // than 1 / 128 of its size over from the known-key check (est[0]; none
    // seen yet counts as none).  Those recoveries' waves sit on the SIMDs for
    // more than a sums' length, and with one capped sums at a time the chip runs
    // short of work beside them: C5 (30 % adversarial) measured 10 % slower on
    // the overlap path, so such traffic keeps the path without it (DESIGN 5,
    // round 12).  Authentication calls (the ingress, whose pushes alternate with
    // the message queue's many short kernels) keep that path too: the ingress
    // line measured 1-8 % slower on the overlap path in three pairs of runs.
    p.overlap = !in.auth && p.waves != 4 && (in.est[0] == none || (uint64_t)in.est[0] * 128 <= n);
    // (the cap is the 3-wave forms' only; whether a chained call's wait is
    // placed depends on the event calls at launch time)
    p.capped = var[HD_VAR_SUM_CAP] && p.overlap && p.waves == 3;
    p.lean = var[HD_VAR_LEAN_INV] && p.overlap;
    p.chain = var[HD_VAR_SUM_CHAIN] && p.overlap;
    p.sums_waves = p.waves;
    p.sums_pf = p.sums_waves == 4 ? 0 : 1;   // the 4-wave form loads its points when used
    p.share = var[HD_VAR_PRE_SHARE] && !in.caller_digests;
    p.dedup = var[HD_VAR_DEDUP] != 0;
    p.lift = var[HD_VAR_SLOW_LIFT] != 0;
    const uint64_t blocks = ((uint64_t)n + 255) / 256;
    p.full = (uint32_t)(blocks < 4 * cu ? blocks : 4 * cu);
    // the lift walks the check's leftovers, k_verify what passed the lift (or the leftovers, without one)
    p.lift_blocks = fb_fallback_blocks(in.est[0], p.full);
    p.slow_blocks = fb_fallback_blocks(in.est[p.lift ? 1 : 0], p.full);
    return p;
}
