// hd_fbwork.h -- what the units of the known-key check share: FbWork, the row structs the
// kernels pass between each other, and the functions that cross units.  hd_fastverify.hip is one call,
// hd_fastsums.hip k_fast_sums, hd_fastinv.hip the inversion kernels, hd_fbtables.hip the tables and their slots.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "hd_dedup.h"
#include "hd_fixedbase.h"
#include "hd_internal.h"

struct FbWork {
    const hd::gp* gtab = nullptr;   // the shared G table of the device (fb_g_table)
    uint32_t nslots = 0;        // slots with a table (whole chunks); slot 0 is unused
    uint32_t max_slots = 0;     // from HD_FB_MAX_BYTES (slot 0 included)
    // Per-key tables live in chunks of HD_FB_CHUNK slots that are allocated
    // when the admitted set first needs them and never moved: a set change
    // that adds keys allocates only new chunks (no regrow, no copy of the
    // tables already built).  tabs[slot] points at the slot's table.
    hd::gp** tabs = nullptr;        // device: max_slots table pointers
    std::vector<hd::gp*> chunks;    // host: the chunk allocations
    hd::ge* base = nullptr;         // max_slots x HD_FB_NWIN window bases
    hd::ge* pub = nullptr;          // max_slots keys
    uint32_t* state = nullptr;  // max_slots HD_FB_* states
    int32_t* adm_slot = nullptr;  // admitted sorted index -> slot
    bool map_ok = true;           // the last hd_fb_map_signatories succeeded (else: full recovery only)
    size_t cap_adm_slot = 0;
    uint32_t* list = nullptr;     // slot work list (max_slots)
    uint32_t* counts = nullptr;   // [0] slots to build (the table builder's)
    uint32_t* zr = nullptr;       // the table builder's z ratios (k_fb_runs: HD_FB_RUN x 9 words per thread)
    // Per-call scratch, HD_FB_NSCRATCH sets used round robin, so that verify
    // calls issued on different streams can run concurrently on the device:
    // the next call's one-message-per-lane kernels fill the SIMDs that this
    // call's inversion kernels (n / K lanes), the last partial round of its
    // k_fast_sums and its fallback recovery leave idle.
    struct Scratch {
        uint32_t* rows = nullptr;     // the split check's per-message rows (SplitRows, 63 words per message)
        size_t cap_rows = 0;
        // the two-level lean inversions' roots and roots-prefix rows (RootRows),
        // 9 words x split_lanes<8>(n) each; the s pass and the Z pass of a call
        // use them one after the other
        uint32_t* roots = nullptr;
        size_t cap_roots = 0;
        // the repeat table (hd_dedup.h): dd_table_words(n) message indices,
        // then the preimage table, as many: one allocation, cleared by one
        // memset over the tables the call uses
        uint32_t* dtab = nullptr;
        size_t cap_dtab = 0;
        // shared preimages: n digest rows (32 bytes, by preimage id), then
        // pid (n words, by message), then plist (n words, by id: the claimant)
        uint8_t* pre = nullptr;
        size_t cap_pre = 0;
        uint32_t* slow = nullptr;     // message index list: the known-key check's leftovers
        size_t cap_slow = 0;
        // device words: [0] leftovers (slow's length), [1] after k_slow_lift,
        // [2] distinct live messages (the compact slots in use), [3] repeats;
        // [2] and [3] are one 64-bit word to k_fast_prep's atomic; [4] distinct
        // preimages (the ids in use), [5] messages without a type 1..3
        // (k_pre_claim); 8 words
        uint32_t* count = nullptr;
        uint32_t* slow2 = nullptr;    // the leftovers that pass the lift: the full recovery's list
        size_t cap_slow2 = 0;
        hipEvent_t done = nullptr;    // recorded after the last call that used this set
        hipStream_t stream = nullptr; // that call's stream
        bool used = false;
    };
    static constexpr int NSCRATCH = 3;
    Scratch sc[NSCRATCH];
    int next = 0;                 // the set the next call takes
    int last_set = -1;            // the set of the last call (hd_ctx_fastpath_stats)
    // Mapped slots whose key is not READY, in pinned host memory the device
    // also writes (k_fb_ready subtracts what it finished): 0 means nothing
    // can be learned any more, so a verify call launches no table-build
    // kernels.  Set exactly (after a device sync) whenever the admitted set
    // or the key format changes; UINT32_MAX = unknown.
    uint32_t* nr_host = nullptr;
    uint32_t* nr_dev = nullptr;
    // The fallback list lengths of the latest calls ([0] leftovers of the
    // check, [1] those past the lift), stored by k_slow_lift / k_verify into
    // pinned host memory: they size the next calls' fallback grids (both
    // kernels walk their list grid-stride, so any size is correct; a grid
    // sized by the last list instead of the batch keeps ~2,000 blocks that
    // would only start and exit from queueing for SIMD slots behind a
    // concurrent call's k_fast_sums).  UINT32_MAX = none seen yet.
    // [2], [3]: the distinct live messages and the batch size of the latest
    // call (k_fast_sinv stores them); their ratio picks the next calls'
    // messages per inversion (fb_plan_call; a call reads the four once).
    uint32_t* est_host = nullptr;
    uint32_t* est_dev = nullptr;
    // hd_ctx_dedup_stats: [0] messages that entered the known-key check, [1]
    // those served as repeats, since context creation (device, 64-bit)
    unsigned long long* dstats = nullptr;
    // hd_ctx_preimage_stats: [0] typed messages of the calls that shared
    // preimages, [1] the distinct preimages they hashed (device, 64-bit)
    unsigned long long* pstats = nullptr;
    // Ordering between calls (hd_fb_verify): a call waits (on the device) for
    // the last call that used its scratch set.  While keys can still be
    // learned (nr_host != 0), or on the first call after the last key became
    // READY, a call also waits for the previous call, whatever its stream:
    // learning writes the shared tables, states and builder scratch.  In the
    // steady state (every mapped key READY, nothing written but per-call
    // scratch and the caller's outputs) calls on different streams overlap.
    hipEvent_t done = nullptr;    // recorded after every call
    hipStream_t last = nullptr;
    bool any = false;
    bool steady = false;          // the previous call ran with nothing to learn
    // HD_VAR_SUM_CHAIN: a call's k_fast_sums waits for the previous call's
    // when that call launched one on another stream, so one call's sums runs
    // at a time and the other calls' short kernels run beside it instead of
    // in lockstep with each other.  done is recorded right after a
    // chained launch; prev says that the previous call recorded it (a
    // call without a launch -- no admitted set, an early error return --
    // leaves it false, and the next call does not wait).  A wait only ever
    // names work submitted earlier, so the order between calls stays acyclic.
    // The event is older than the call events (done, Scratch::done) of its
    // call, so whoever waits for those has waited for it.
    struct SumsChain {
        hipEvent_t done = nullptr;
        hipStream_t last = nullptr;
        bool prev = false, now = false;
        // start of a call: what the previous call launched; this call has
        // launched nothing yet, whichever way it returns
        void begin_call() { prev = now; now = false; }
        // before a chained call's sums: whether s was made to wait.  Without
        // the event (creation failed) the call runs unchained.
        bool wait(hipStream_t s) {
            if (!done && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) done = nullptr;
            return done && prev && last != s && hipStreamWaitEvent(s, done, 0) == hipSuccess;
        }
        // after a chained call's sums
        void record(hipStream_t s) {
            now = done && hipEventRecord(done, s) == hipSuccess;
            if (now) last = s;
        }
    } sums;
    uint32_t n_capped = 0, n_lean = 0, n_chained = 0;   // hd_ctx_overlap_stats
    // hd_ctx_inv_levels: the lean inversions in two levels (2) or as the one
    // kernel each (1); inv_k2: roots per inverting lane (HD_INV_K2: 8 or 16).
    // n_inv: lean calls that launched the two-level form, the one-level form.
    int inv_levels = 2, inv_k2 = 16;
    uint64_t n_inv[2] = {0, 0};
    // hd_ctx_profile: event pairs around whole calls and around k_fast_sums
    bool prof = false;
    std::vector<hipEvent_t> ev_call, ev_sums;
    size_t n_call = 0, n_sums = 0;   // pairs in use
    std::unordered_map<std::string, uint32_t> slot_of;  // signatory -> slot
    std::vector<uint32_t> free_slots;
    hd_set_change_info change{0, 0, 0, 0, 0};   // hd_ctx_set_change_info: the last hd_fb_map_signatories
    uint32_t used = 1;            // slots handed out so far (slot 0 = G)
    int wp = HD_FB_W;             // window width of the per-key tables (HD_FB_W or HD_FB_WW)
    int last_k = 8;               // messages per inversion of the last split check (FbCallPlan::k)
    double budget = 0;            // table bytes allowed (HD_FB_MAX_BYTES), shared per device
    size_t bytes = 0;             // table bytes this context holds
    // Foreign keys (HD_VAR_FOREIGN_KEYS): fres slots fbase .. reserved once
    // (a contiguous block, kept across set changes) for authenticated Froms
    // outside the admitted set, of which the first fcap are in use (fcap is
    // re-read from the variant at every set change: 0 turns learning off,
    // the block stays reserved); fdict maps such a From to its slot (emptied
    // on every set change).  k_verify stores the claim count into fpend_host;
    // a change since fseen makes the next call build the new tables.
    uint32_t* fdict = nullptr;
    uint32_t* fnext = nullptr;
    uint32_t fbase = 0, fcap = 0, fres = 0;
    uint32_t* fpend_host = nullptr;   // [0] claim count, [1] the fmiss flag (SlowCtl)
    uint32_t* fpend_dev = nullptr;
    uint32_t fseen = 0;
    // Slot eviction (fb_evict): fhit[0, 64) counts each foreign slot's
    // known-key checks, fhit[64, 64 + HD_FD_BUCKETS) the recoveries of each
    // slotless dictionary entry (fbhit), fkey the slotless entries' keys.
    // fwait / fcalls: calls between checks while misses are flagged
    // (doubling, up to HD_FD_EVICT_WAIT_MAX, while checks swap nothing).
    uint32_t* fhit = nullptr;
    hd::ge* fkey = nullptr;
    uint32_t fwait = 1, fcalls = 0;
    bool fforce = false;   // build the LEARNED slots at this call's end (an eviction re-keyed one)
    uint32_t evictions = 0;
    uint32_t evict_checks = 0;   // fb_evict passes that waited for the context's calls
    uint32_t evict_aborts = 0;   // passes whose new dictionary had no bucket for a slot holder
};

#define FBCHK(expr, what)                                \
    do {                                                 \
        hipError_t e_ = (expr);                          \
        if (e_ != hipSuccess) return hd_ctx_fail(ctx, e_, what); \
    } while (0)

namespace hd {

// Repeats and compaction (hd_dedup.h).  k_fast_prep gives every
// distinct live message a compact slot c from a device counter and writes its
// rows at c (all rows keep the batch's stride n); a vote that repeats an
// earlier live vote of the batch byte for byte takes no slot.  ref[i] names
// message i's slot, the message it repeats, or its early code (dd_resolve).
// The three middle kernels run over slots [0, live), live read from the
// counter: their grids are sized for n and the surplus waves exit at once;
// the inversion kernels derive T from live, so their waves are full.
// k_fast_cmp stays one lane per message in index order (the bitmap ballot):
// lane i resolves its slot through ref and compares from that slot's rows, so
// every copy of a repeated message gets the outputs its own check would give.
// Which of two equal messages claims the slot, and the order of the compact
// slots, vary from run to run; no output depends on either.
struct SplitRows {
    uint32_t* aux;   // n, by slot: table slot << 8 | code
    int32_t* idx;    // n, by message: admitted (sorted) index
    uint32_t* ref;   // n, by message: compact slot | HD_DD_REPEAT + message | HD_DD_FINAL + code
    uint32_t* u1;    // 8n, by slot: m
    uint32_t* u2;    // 8n, by slot: r
    uint32_t* s;     // 8n, by slot: s
    uint32_t* pre;   // 9n, by slot: prefix products of s, then s^-1 R (radix 2^29); later of Z, then Z^-1
    uint32_t* xyz;   // 27n, by slot: the XYZZ sum as (X ZZZ, Y ZZ, Z = ZZ ZZZ) (gxz_finish)
    uint32_t* cnt;   // Scratch::count: [2] live slots, [3] repeats of this call
    int prio;        // wave priority of the short kernels (HD_VAR_WAVE_PRIO)
};

// the code of message i and, when it has rows, its compact slot (two loads
// for a repeat; valid after k_fast_prep's kernel boundary)
HD uint32_t dd_resolve(const SplitRows& rows, uint32_t i, uint32_t& c, bool& has_slot) {
    uint32_t rf = rows.ref[i];
    has_slot = (rf >> 30) != 3u;
    c = 0;
    if (!has_slot) return rf & 0xFFu;
    if (rf & HD_DD_REPEAT) rf = rows.ref[rf & HD_DD_INDEX];
    c = rf;
    return rows.aux[c] & 0xFFu;
}

// s_setprio takes an immediate: a uniform branch per level
HD void wave_prio(int p) {
    if (p == 1) __builtin_amdgcn_s_setprio(1);
    else if (p == 2) __builtin_amdgcn_s_setprio(2);
    else if (p >= 3) __builtin_amdgcn_s_setprio(3);
}

// a Booth digit of window w as a reference into the base's table: entry
// index | HD_REF_NEG for a negative digit, HD_REF_ZERO for 0 (entry 0 of the
// window is then read and discarded)
#define HD_REF_NEG 0x80000000u
#define HD_REF_ZERO 0x40000000u
#define HD_REF_IDX 0x3FFFFFFFu
template <int W>
HD uint32_t fb_ref(int d, int w) {
    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
    const uint32_t base = (uint32_t)w * FbL<W>::N;
    return d == 0 ? (base | HD_REF_ZERO) : ((base + ad - 1) | (d < 0 ? HD_REF_NEG : 0u));
}

// the shared preimages of a call (k_pre_claim, k_pre_hash, k_fast_prep<true>: hd_fastverify.hip)
struct PreRows {
    uint8_t* dig;      // n rows of 32 bytes, by id: the digest, big-endian (a caller's digest row format)
    uint32_t* pid;     // n, by message (hd_dedup.h)
    uint32_t* plist;   // n, by id: the claimant's message index
    uint32_t* cnt;     // Scratch::count: [4] ids in use, [5] messages of this call without a type 1..3
};

// the two-level lean inversions' rows (hd_fastinv.hip; Scratch::roots)
struct RootRows {
    uint32_t* roots;   // 9 T: the lanes' products, then their inverses
    uint32_t* rpre;    // 9 T: prefix products of the roots
};

}  // namespace hd

// f(std::integral_constant) over the compiled per-key table widths (any other
// wp: HD_FB_W) and over the messages per inversion (8 unless 16)
template <typename F>
auto with_width(int wp, F f) {
    if (wp == HD_FB_WX) return f(std::integral_constant<int, HD_FB_WX>{});
    if (wp == HD_FB_WW) return f(std::integral_constant<int, HD_FB_WW>{});
    if (wp == HD_FB_WN) return f(std::integral_constant<int, HD_FB_WN>{});
    return f(std::integral_constant<int, HD_FB_W>{});
}
template <typename F>
auto with_k(int k, F f) {
    return k == 16 ? f(std::integral_constant<int, 16>{}) : f(std::integral_constant<int, 8>{});
}

// windows of a per-key table of width wp
inline int fb_nwin(int wp) { return with_width(wp, [](auto w) { return (int)hd::FbL<decltype(w)::value>::NWIN; }); }

// hd_fbtables.hip
int fb_learn(hd_ctx* ctx, hipStream_t s);
bool fb_foreign_pending(const FbWork* f);
int fb_evict(hd_ctx* ctx, bool* changed);
// hd_fastsums.hip: the plan's k_fast_sums form at table width wp, `blocks` blocks of 256 lanes
void fb_launch_sums(const FbCallPlan& p, int wp, uint32_t blocks, hipStream_t s, uint32_t n, const hd::gp* gtab,
                    const hd::gp* const* tabs, const hd::SplitRows& rows);
// hd_fastinv.hip: the s and the Z inversion of a call of n messages, p.k per lane, in the form the plan,
// inv_levels and inv_k2 (FbWork) select; est, stats: FbWork::est_dev + 2 and dstats, for the s pass's first lane
void fb_launch_sinv(const FbCallPlan& p, int inv_levels, int inv_k2, hipStream_t s, uint32_t n,
                    const hd::SplitRows& rows, const hd::RootRows& rr, uint32_t* est, unsigned long long* stats);
void fb_launch_zinv(const FbCallPlan& p, int inv_levels, int inv_k2, hipStream_t s, uint32_t n,
                    const hd::SplitRows& rows, const hd::RootRows& rr);
