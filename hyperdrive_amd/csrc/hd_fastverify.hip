// hd_fastverify.hip -- the known-key fast path of hd_verify_batch_device and
// the tables it runs on (hd_fixedbase.h).
//
// Per batch, stream-ordered, no host synchronisation:
//   k_fast_prep / k_fast_sinv / k_fast_sums / k_fast_zinv / k_fast_cmp
//                   the split known-key check (the default, see "the split
//                   check" below): a message whose claimed From is an
//                   admitted signatory with a known key is checked with two
//                   fixed-base multiplications (23 mixed additions, no
//                   doublings, no square root); VALID / early exact verdicts
//                   are final, everything else is appended to a list
//   k_verify        (hd_verify.hip) the full libsecp256k1-semantics recovery
//                   over that list only; VALID messages of signatories without
//                   a known key publish the recovered key to their slot
//   k_fb_list / k_fb_bases / k_fb_runs / k_fb_ready
//                   (hd_fbtables.hip) build the tables of newly learned keys;
//                   with nothing learned each exits at once
// This unit is one call: the one-message-per-lane kernels, the order of
// launches, events and stream waits, the per-call entry points.  FbWork and
// the row structs: hd_fbwork.h; k_fast_sums: hd_fastsums.hip; the inversion
// kernels: hd_fastinv.hip; tables, slots, widths, foreign keys: hd_fbtables.hip.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/hd_verify.h"
#include "hd_fbwork.h"
#include "hd_inv2.h"
#include "hd_verify_msg.h"

using namespace hd;

namespace {

// message i of a device batch, fields on demand (as DevSrc in hd_verify.hip)
struct FastSrc {
    const DevBatch& b;
    uint32_t i;
    const uint8_t* dg;
    __device__ __forceinline__ uint32_t type() const { return b.type[i]; }
    __device__ __forceinline__ uint32_t value(int w) const { return load_be32(b.value32 + 32 * (size_t)i + 4 * w); }
    __device__ __forceinline__ uint32_t from(int w) const { return load_be32(b.from32 + 32 * (size_t)i + 4 * w); }
    __device__ __forceinline__ uint32_t sig_r(int w) const { return load_be32(b.sig65 + 65 * (size_t)i + 4 * w); }
    __device__ __forceinline__ uint32_t sig_s(int w) const { return load_be32(b.sig65 + 65 * (size_t)i + 32 + 4 * w); }
    __device__ __forceinline__ uint32_t sig_v() const { return b.sig65[65 * (size_t)i + 64]; }
    // whole fields with wide loads (hd_common.h)
    __device__ __forceinline__ void sig(uint32_t r_be[8], uint32_t s_be[8], uint32_t& v) const {
        load_sig65(r_be, s_be, v, b.sig65, i, b.n);
    }
    __device__ __forceinline__ void from_words(uint32_t w[8]) const { load_row32_be(w, b.from32, i); }
    __device__ __forceinline__ void value_words(uint32_t w[8]) const { load_row32_be(w, b.value32, i); }
};

// ---- the split check: K messages per lane share each inversion ----------
// The known-key check in five kernels: the two inversions (of s mod n, of Z
// mod p) serve K messages of a lane each (Montgomery's trick over K), and
// everything else runs one message per lane, so that only the inversion
// kernels have the low occupancy of n / K lanes.  Per-message state sits in word-major HBM rows
// between them (lane t reads word w of message i at w * n + i, coalesced):
//   k_fast_prep     one per lane: lookup, digest, early checks; m, r, s
//   k_fast_sinv     K per lane: prefix products of s, one inversion mod n,
//                   s^-1 of each message
//   k_fast_sums     one per lane: u1 = m / s, u2 = r / s as window digits
//                   (into LDS), then u1 G + u2 P (the first window's point
//                   loaded, one XYZZ mixed addition per further window)
//   k_fast_zinv     K per lane: prefix products of Z, one inversion mod p,
//                   Z^-1 of each message
//   k_fast_cmp      one per lane: the comparison, the outputs, the valid
//                   bitmap and the fallback list
// Message i of lane t of an inversion kernel is i = j T + t (j < K,
// T = ceil(n / K)), so every step j of a wave touches consecutive messages.
// The verdicts are the ones verify_fast2 (hd_fixedbase.h, host-tested) gives:
// same early checks, same sums, same comparison.
// (HD_FAST_LIVE, the aux code "keep going", and soa_load / soa_store, a word-major
// row's entry: hd_inv2.h; SplitRows, the rows, with repeats and compaction,
// and PreRows: hd_fbwork.h)
//
// Shared preimages (hd_dedup.h).  A call that computes its own
// digests hashes each distinct preimage once: k_pre_claim gives every typed
// message a preimage id (pid), k_pre_hash hashes one preimage per lane over
// the ids in use, and k_fast_prep<true> reads its digest row by id.  Skipping
// the hash lane by lane in k_fast_prep would save nothing (a wave with one
// hashing lane issues the whole compression): the hashing lanes are compacted
// here as the sums' slots are.

// one message per lane: the preimage table's probe, the ids and pid.  Blocks
// of HD_PRE_BLOCK lanes: the blocks' atomics all land on the one id counter,
// so a block is as large as a block can be and adds to the second counter
// only what is rare (1M messages, alone on the chip: 117 us with two atomics
// per block of 256, 105 us so).
#define HD_PRE_BLOCK 1024
__global__ __launch_bounds__(HD_PRE_BLOCK) void k_pre_claim(DevBatch b, PreRows pre, uint32_t* __restrict__ ptab,
                                                   uint32_t pmask, int prio) {
    wave_prio(prio);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool present = i < b.n;   // (no early exit: the block's lanes meet at the id counter below)
    const uint32_t type = present ? b.type[i] : 0u;
    const bool typed = type >= 1 && type <= 3;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t rep = HD_DD_EMPTY, h = 0;
    DdPre me;
    me.is_propose = 0;
    me.valid_round = me.height = me.round = 0;
    HD_UNROLL for (int k = 0; k < 8; k++) me.value[k] = 0;
    if (typed) {
        dd_pre_load(me, type == T_PROPOSE, b.height, b.round, b.valid_round, b.value32, i);
        h = dd_pre_hash(me);
    }
    // The probe of one lane: true when the message found its preimage or
    // claimed a slot, false past the cutoff.  The fields compared are the
    // caller's input arrays, which no kernel writes: no ordering with the
    // claimant's lane is needed.
    auto probe = [&]() -> bool {
        HD_NOUNROLL for (uint32_t p = 0; p < HD_DD_PROBES; p++) {
            const uint32_t cur = atomicCAS(&ptab[(h + p) & pmask], HD_DD_EMPTY, i);
            if (cur == HD_DD_EMPTY) return true;   // claimed
            DdPre other;
            dd_pre_load(other, b.type[cur] == T_PROPOSE, b.height, b.round, b.valid_round, b.value32, cur);
            if (dd_pre_equal(me, other)) {
                rep = cur;
                return true;
            }
        }
        return false;
    };
    // Consecutive messages mostly share a preimage (a round's votes arrive
    // together), and 64 lanes that compare-and-swap one address serialise at
    // the memory side.  So only the head of a run probes: a lane whose
    // preimage differs from the lane's before it (every byte compared), or
    // the wave's first lane.  The lanes of its run take its claimant, or it
    // as theirs; when it gave up at the cutoff they count on their own, as
    // their own probes would have ended.
    auto up = [&](uint32_t x) { return (uint32_t)__shfl_up((int)x, 1); };
    auto up64 = [&](int64_t x) {
        return (int64_t)((uint64_t)up((uint32_t)((uint64_t)x >> 32)) << 32 | up((uint32_t)(uint64_t)x));
    };
    DdPre pk;
    pk.is_propose = up(me.is_propose);
    pk.valid_round = up64(me.valid_round);
    pk.height = up64(me.height);
    pk.round = up64(me.round);
    HD_UNROLL for (int k = 0; k < 8; k++) pk.value[k] = up(me.value[k]);
    const bool prev_typed = up(typed ? 1u : 0u) != 0u;
    const bool head = typed && (lane == 0 || !prev_typed || !dd_pre_equal(me, pk));
    uint32_t found = 0;
    if (head) found = probe() ? 1u : 0u;
    // a typed lane that is no head follows a typed lane with an equal key:
    // the run reaches back to a head (the first lane, when typed, is one)
    const unsigned long long hm = __ballot(head) & ((2ull << lane) - 1ull);
    const int hl = hm ? 63 - __clzll((long long)hm) : 0;
    const uint32_t hrep = (uint32_t)__shfl((int)rep, hl), hfound = (uint32_t)__shfl((int)found, hl);
    if (typed && !head && hfound) rep = hrep == HD_DD_EMPTY ? i - lane + (uint32_t)hl : hrep;
    // ids: one atomic per block adds its claimants (returned: the block's
    // first id), another its messages without a type 1..3, if any (the typed
    // ones are the rest of n); a lane's id follows from the ballots
    const bool claimant = typed && rep == HD_DD_EMPTY;
    __shared__ uint32_t s_cnt[HD_PRE_BLOCK / 64], s_base;
    const unsigned long long bc = __ballot(claimant), bu = __ballot(present && !typed);
    if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(bc) | (uint32_t)__popcll(bu) << 16;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < HD_PRE_BLOCK / 64; w++) t += s_cnt[w];   // (<= 1024 each half: no carry)
        s_base = 0;
        if (t & 0xFFFFu) s_base = atomicAdd(pre.cnt + 4, t & 0xFFFFu);
        if (t >> 16) atomicAdd(pre.cnt + 5, t >> 16);
    }
    __syncthreads();
    if (!present) return;
    if (claimant) {
        uint32_t id = s_base + (uint32_t)__popcll(bc & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wv; w++) id += s_cnt[w] & 0xFFFFu;
        pre.plist[id] = i;
        pre.pid[i] = id;
    } else {
        pre.pid[i] = typed ? dd_pid_ref(rep) : HD_DD_FINAL;
    }
}

// one distinct preimage per lane: the grid is sized for n and the waves past
// the ids in use exit here.  (stats: the first lane adds the call to the
// context's cumulative counters.)
__global__ __launch_bounds__(256) void k_pre_hash(DevBatch b, PreRows pre, unsigned long long* __restrict__ stats,
                                                  int prio) {
    wave_prio(prio);
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nd = pre.cnt[4];
    if (id == 0) {
        const uint32_t typed = b.n - pre.cnt[5];
        if (typed) atomicAdd(&stats[0], (unsigned long long)typed);
        if (nd) atomicAdd(&stats[1], (unsigned long long)nd);
    }
    if (id >= nd) return;
    const uint32_t i = pre.plist[id];
    uint32_t value[8], out[8];
    load_row32_be(value, b.value32, i);
    if (b.type[i] == T_PROPOSE)
        sha256_propose(out, b.height[i], b.round[i], b.valid_round ? b.valid_round[i] : -1, value);
    else
        sha256_vote(out, b.height[i], b.round[i], value);
    store_row32_be(pre.dig, id, out);
}

// one message per lane (occupancy hides the lookup's dependent loads): type,
// admitted lookup, key state, digest, the early checks; m and r to the rows.
// SHARE: the digest is the row of the message's preimage id (PreRows; no SHA
// code in the kernel), and the id stands for (height, round, value) in the
// repeat compare: equal ids are equal preimages, and equal preimages that
// missed each other at the preimage table's cutoff are merely not merged.
template <bool SHARE>
__global__ __launch_bounds__(256) void k_fast_prep(DevBatch b, const uint8_t* __restrict__ digest_in,
                                                   const uint32_t* __restrict__ state,
                                                   const int32_t* __restrict__ adm_slot, AdmIndex ix,
                                                   uint32_t n_adm, SplitRows rows, const uint32_t* __restrict__ fdict,
                                                   uint32_t* __restrict__ fhit, uint32_t fbase,
                                                   uint32_t* __restrict__ dtab, uint32_t dmask, PreRows pre) {
    wave_prio(rows.prio);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = b.n;
    const bool present = i < n;   // (no early exit: the block's lanes meet at the slot counter below)
    FastSrc src{b, present ? i : 0u, digest_in};
    const uint32_t type = present ? src.type() : 0u;
    uint32_t code = HD_NEEDS_SLOW, slot = 0, rep = HD_DD_EMPTY;
    int32_t idx = -1;
    sc r, s, m;
    if (!present) {
    } else if (type < 1 || type > 3) {
        code = V_BAD_TYPE;
    } else {
        uint32_t from_be[8];
        src.from_words(from_be);
        idx = n_adm ? adm_index_find(ix, from_be) : -1;
        int32_t sl = idx >= 0 ? adm_slot[idx] : -1;
        if (idx < 0 && fdict) {
            // an authenticated From outside the admitted set with a known key:
            // the check's success means NOT_ADMITTED (idx -2 marks it)
            sl = fdict_find(fdict, from_be);
            if (sl >= 0) idx = -2;
        }
        if (sl >= 0 && state[sl] == HD_FB_READY) {
            slot = (uint32_t)sl;
            if (idx == -2) atomicAdd(&fhit[sl - (int32_t)fbase], 1u);   // a foreign slot's use (fb_evict)
            FastIn in;
            // this message's inputs, as the repeat table compares them: the
            // preimage id stands for (height, round, value) when shared
            DdKey me;
            uint32_t my_id = 0;
            me.height = me.round = 0;
            if constexpr (SHARE) {
                my_id = dd_pid_resolve(pre.pid, i);
                load_row32_be(in.digest_be, pre.dig, my_id);
            } else if (digest_in) {
                load_row32_be(in.digest_be, digest_in, i);
                HD_UNROLL for (int k = 0; k < 8; k++) me.value[k] = in.digest_be[k];
            } else {
                src.value_words(me.value);
                me.height = b.height[i];
                me.round = b.round[i];
                if (type == T_PROPOSE)
                    sha256_propose(in.digest_be, me.height, me.round, b.valid_round ? b.valid_round[i] : -1, me.value);
                else
                    sha256_vote(in.digest_be, me.height, me.round, me.value);
            }
            src.sig(in.r_be, in.s_be, in.v);
            in.ready = true;
            fe x;
            uint8_t o;
            if (fast_prefix(o, r, s, m, x, in)) {
                code = HD_FAST_LIVE;
                // A vote looks for an equal earlier vote (hd_dedup.h).  The
                // table holds live votes only, so a match is a message with
                // rows; the fields compared are the caller's input arrays,
                // which no kernel writes, so the compare needs no ordering
                // with the claimant's lane.  Proposes are never merged (their
                // preimage has valid_round).  dtab is NULL with HD_VAR_DEDUP 0.
                if (dtab && type != T_PROPOSE) {
                    if constexpr (!SHARE) {
                        HD_UNROLL for (int k = 0; k < 8; k++) {
                            me.from[k] = from_be[k];
                            me.r[k] = in.r_be[k];
                            me.s[k] = in.s_be[k];
                        }
                        me.v = in.v;
                    }
                    const uint32_t h = dd_hash_words(in.r_be[0], in.r_be[7], in.s_be[0], in.s_be[7], from_be[0], from_be[7]);
                    HD_NOUNROLL for (uint32_t p = 0; p < HD_DD_PROBES; p++) {
                        const uint32_t cur = atomicCAS(&dtab[(h + p) & dmask], HD_DD_EMPTY, i);
                        if (cur == HD_DD_EMPTY) break;   // claimed: distinct
                        bool eq;
                        if constexpr (SHARE) {
                            // dd_key_equal's compare with the ids in place of
                            // (height, round, value), field by field against
                            // this lane's live registers: the differences are
                            // ORed as the claimant's words arrive
                            uint32_t d = dd_pid_resolve(pre.pid, cur) ^ my_id, w[8], w2[8], v2;
                            load_row32_be(w, b.from32, cur);
                            HD_UNROLL for (int k = 0; k < 8; k++) d |= w[k] ^ from_be[k];
                            load_sig65(w, w2, v2, b.sig65, cur, n);
                            HD_UNROLL for (int k = 0; k < 8; k++) d |= (w[k] ^ in.r_be[k]) | (w2[k] ^ in.s_be[k]);
                            eq = (d | (v2 ^ in.v)) == 0;
                        } else {
                            DdKey other;
                            dd_key_load(other, b.height, b.round, b.value32, digest_in, b.from32, b.sig65, cur, n);
                            eq = dd_key_equal(me, other);
                        }
                        if (eq) {
                            rep = cur;
                            break;
                        }
                    }
                }
            } else {
                code = o;
            }
        }
    }
    // Compact slots: one 64-bit atomic per block adds its distinct live
    // messages (low word, returned: the block's first slot) and its repeats
    // (high word); a lane's slot follows from the ballots.
    const bool live = code == HD_FAST_LIVE;
    const bool distinct = live && rep == HD_DD_EMPTY;
    __shared__ uint32_t s_cnt[4], s_base;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long bd = __ballot(distinct), br = __ballot(live && !distinct);
    if (lane == 0) s_cnt[wv] = (uint32_t)__popcll(bd) | (uint32_t)__popcll(br) << 16;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];   // (<= 256 each half: no carry)
        s_base = 0;
        if (t)
            s_base = (uint32_t)atomicAdd((unsigned long long*)(rows.cnt + 2),
                                         (unsigned long long)(t & 0xFFFFu) | (unsigned long long)(t >> 16) << 32);
    }
    __syncthreads();
    if (!present) return;
    if (distinct) {
        uint32_t c = s_base + (uint32_t)__popcll(bd & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wv; w++) c += s_cnt[w] & 0xFFFFu;
        rows.aux[c] = slot << 8 | HD_FAST_LIVE;
        soa_store(rows.u1, n, c, m.v);
        soa_store(rows.u2, n, c, r.v);
        soa_store(rows.s, n, c, s.v);
        rows.ref[i] = c;
    } else {
        rows.ref[i] = live ? (HD_DD_REPEAT | rep) : (HD_DD_FINAL | code);
    }
    rows.idx[i] = idx;
}

// x = r (+ n when v & 2) as a field element: the x coordinate of R (the range
// checks of sig_prefix passed in k_fast_prep)
HD void fast_rx(fe& x, const sc& r, uint32_t v) {
    uint32_t xw[8];
    HD_UNROLL for (int k = 0; k < 8; k++) xw[k] = r.v[k];
    if (v & 2) {
        const uint32_t N[8] = {HD_N0, HD_N1, HD_N2, HD_N3, HD_N4, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        uint64_t c = 0;
        HD_UNROLL for (int k = 0; k < 8; k++) { c += (uint64_t)xw[k] + N[k]; xw[k] = (uint32_t)c; c >>= 32; }
    }
    fe_from_le(x, xw);
}

// The comparison of message i (zi: the inverse of its stored ZZ ZZZ, read
// from the rows when null), its outputs when its verdict is final, its
// place on the fallback list, and its bit of the valid bitmap.  Every lane
// of the wavefront calls it together (ballots) for 64 consecutive, 64-aligned
// message indices; `present` is false past the batch.
__device__ __forceinline__ void cmp_one(const DevBatch& b, const SplitRows& rows, const int32_t* __restrict__ adm_perm,
                       uint8_t* __restrict__ verdict, uint8_t* __restrict__ rec32, int32_t* __restrict__ signer,
                       uint32_t* __restrict__ slow, uint32_t* __restrict__ n_slow, uint32_t* __restrict__ bitmap,
                       bool auth, uint32_t i, bool present, const fe* zi) {
    const uint32_t n = b.n;
    uint8_t v = HD_NEEDS_SLOW;
    if (present) {
        // the rows of message i are its slot's: its own, or those of the
        // message it repeats (same inputs, so the same comparison; a repeat
        // redoes the two products instead of a second pass copying outputs)
        uint32_t c;
        bool has_slot;
        v = (uint8_t)dd_resolve(rows, i, c, has_slot);
        if (v == HD_FAST_LIVE) {
            fe xn, yn, w, x;
            soa_load(xn.n, rows.xyz, n, c);
            soa_load(yn.n, rows.xyz + 9 * (size_t)n, n, c);
            if (zi) w = *zi;
            else soa_load(w.n, rows.pre, n, c);
            sc r;
            soa_load(r.v, rows.u2, n, c);
            const uint32_t sv = b.sig65[65 * (size_t)i + 64];
            fast_rx(x, r, sv);
            v = fast_final_xz(xn, yn, w, x, sv);
            // authentication only: From's key does not give R, so the
            // recovered key is not From's -- final, without the recovery
            if (auth && v == HD_NEEDS_SLOW) v = V_NOT_AUTHENTIC;
            if (v == V_VALID && rows.idx[i] == -2) v = V_NOT_ADMITTED;   // a foreign key's check
        }
        if (v != HD_NEEDS_SLOW) {
            const bool ok = v == V_VALID;
            verdict[i] = v;
            if (rec32) {
                uint32_t f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (ok || (v == V_NOT_ADMITTED && rows.idx[i] == -2)) load_row32_be(f, b.from32, i);
                store_row32_be(rec32, i, f);
            }
            if (signer) signer[i] = ok ? adm_perm[rows.idx[i]] : -1;
        }
    }
    const bool to_slow = present && v == HD_NEEDS_SLOW;
    const unsigned long long bal = __ballot(to_slow);
    const uint32_t lane = threadIdx.x & 63u;
    if (bal) {
        const uint32_t leader = (uint32_t)__ffsll((long long)bal) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(n_slow, (uint32_t)__popcll(bal));
        base = __shfl(base, (int)leader);
        if (to_slow) slow[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1))] = i;
    }
    if (bitmap) {
        const unsigned long long ok = __ballot(present && v == V_VALID);
        const uint32_t i0 = i - lane;   // multiple of 64
        if (lane == 0 && i0 < n) {
            bitmap[i0 >> 5] = (uint32_t)ok;
            if (i0 + 32 < n) bitmap[(i0 >> 5) + 1] = (uint32_t)(ok >> 32);
        }
    }
}

// One message per lane over a grid of whole wavefronts: the comparison of a
// live message, the outputs of every message that has its final verdict, the
// fallback list, and the valid bitmap -- a wavefront covers 64 consecutive
// messages, two bitmap words written from one ballot.  Messages handed to the
// full recovery get bit 0 here; k_verify sets theirs.
__global__ __launch_bounds__(256) void k_fast_cmp(DevBatch b, SplitRows rows, const int32_t* __restrict__ adm_perm,
                                                  uint8_t* __restrict__ verdict, uint8_t* __restrict__ rec32,
                                                  int32_t* __restrict__ signer, uint32_t* __restrict__ slow,
                                                  uint32_t* __restrict__ n_slow, uint32_t* __restrict__ bitmap,
                                                  bool auth) {
    wave_prio(rows.prio);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    cmp_one(b, rows, adm_perm, verdict, rec32, signer, slow, n_slow, bitmap, auth, i, i < b.n, nullptr);
}

// Before the full recovery of the leftovers: the reference's first checks
// and the lift of R (V >= 4, r / s range,
// r + n >= p, x^3 + 7 a square), in recover_m's order.  A message that fails
// one has its final verdict (nothing recovered) for one square-root chain,
// ~7 % of a recovery -- the "x not on the curve" adversarial class, and the
// malformed signatures of signatories without a known key; the rest go to
// the compacted list `out` (*n_out) that k_verify walks.  Leftovers are ~10 %
// of a 30 %-adversarial batch, so the saving is in the recovery's throughput
// cost, which overlapping calls expose.
//
// Round 4: a leftover that went through the known-key check (aux code still
// HD_FAST_LIVE, so m and s are in the rows) and lifts is tested for the
// INFINITY verdict with the fixed-base G table (fb_is_infinity: R == (m / s) G).
// That class -- cheap for anyone to craft (R = k G, s = m / k) -- then costs a
// scalar inversion and 11 additions instead of a full recovery each.
__global__ __launch_bounds__(256) void k_slow_lift(DevBatch b, const uint32_t* __restrict__ list,
                                                   const uint32_t* __restrict__ count, uint8_t* __restrict__ verdict,
                                                   uint8_t* __restrict__ rec32, int32_t* __restrict__ signer,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ n_out,
                                                   int prio, uint32_t* __restrict__ est, SplitRows rows,
                                                   const gp* __restrict__ gtab) {
    wave_prio(prio);
    const uint32_t total = *count, stride = gridDim.x * blockDim.x;
    if (est && blockIdx.x == 0 && threadIdx.x == 0) est[0] = total;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t base = blockIdx.x * blockDim.x; base < total; base += stride) {
        const uint32_t p = base + threadIdx.x;
        bool keep = false;
        uint32_t i = 0;
        if (p < total) {
            i = list[p];
            uint32_t r_be[8], s_be[8], v;
            load_sig65(r_be, s_be, v, b.sig65, i, b.n);
            sc r, s;
            fe x;
            uint8_t pre = sig_prefix(r, s, x, r_be, s_be, v);
            if (pre == V_VALID) {
                fe y2, y, seven;
                fe_sqr(y2, x);
                fe_mul(y2, y2, x);
                fe_set_u32(seven, 7);
                fe_add(y2, y2, seven);
                if (!fe_sqrt(y, y2)) {
                    pre = V_NO_POINT;
                } else if (gtab && rows.aux) {
                    // (a repeat on the list reads its m at the slot of the message it repeats)
                    uint32_t c;
                    bool has_slot;
                    if (dd_resolve(rows, i, c, has_slot) == HD_FAST_LIVE) {
                        ge R;
                        R.x = x;
                        R.y = y;
                        if (fe_is_odd(y) != ((v & 1u) != 0)) fe_neg(R.y, y);
                        sc m;   // (s is sig_prefix's; m as k_fast_prep left it)
                        soa_load(m.v, rows.u1, b.n, c);
                        if (fb_is_infinity<HD_FB_WG>(m, s, R, GpTab{gtab})) pre = V_INFINITY;
                    }
                }
            }
            keep = pre == V_VALID;
            if (!keep) {
                verdict[i] = pre;
                if (rec32) {
                    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    store_row32_be(rec32, i, z);
                }
                if (signer) signer[i] = -1;
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (bal) {
            const uint32_t leader = (uint32_t)__ffsll((long long)bal) - 1;
            uint32_t o = 0;
            if (lane == leader) o = atomicAdd(n_out, (uint32_t)__popcll(bal));
            o = __shfl(o, (int)leader);
            if (keep) out[o + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = i;
        }
    }
}

}  // namespace

// the next free event pair of a profile record (created on first use), or
// NULL when profiling is off or the event could not be created
static hipEvent_t* fb_prof_pair(std::vector<hipEvent_t>& ev, size_t& used, bool on) {
    if (!on) return nullptr;
    if (2 * (used + 1) > ev.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess) return nullptr;
        if (hipEventCreate(&b) != hipSuccess) {
            (void)hipEventDestroy(a);
            return nullptr;
        }
        ev.push_back(a);
        ev.push_back(b);
    }
    return &ev[2 * used++];
}

// One call's split check: prep, s inversion, chain wait, sums, Z inversion, cmp.
static void launch_split(hd_ctx* ctx, const DevBatch& b, const uint8_t* d_digest, uint8_t* d_verdict,
                         uint8_t* d_rec32, int32_t* d_signer, uint32_t* d_bitmap, const SplitRows& rows,
                         const FbWork::Scratch& sc, hipStream_t s, bool auth, const FbCallPlan& p) {
    FbWork* f = ctx->fb;
    const uint32_t n = b.n;
    // The middle kernels run over the slots in use, which only the device
    // knows: their grids cover n slots and the surplus waves exit at once.
    const uint32_t nb = (n + 255) / 256;
    // HD_VAR_DEDUP 0: no table, so no message is ever marked a repeat; slots,
    // ref and every kernel are the same
    const uint32_t tw = dd_table_words(n);
    uint32_t* dtab = p.dedup ? sc.dtab : nullptr;
    const uint32_t* fdict = f->fcap ? f->fdict : nullptr;
    if (p.share) {
        // HD_VAR_PRE_SHARE 1 and no caller digests: each distinct preimage is
        // hashed once (k_pre_claim, k_pre_hash), k_fast_prep reads the rows
        const PreRows pre{sc.pre, (uint32_t*)(sc.pre + 32 * (size_t)n), (uint32_t*)(sc.pre + 36 * (size_t)n), sc.count};
        k_pre_claim<<<(n + HD_PRE_BLOCK - 1) / HD_PRE_BLOCK, HD_PRE_BLOCK, 0, s>>>(b, pre, sc.dtab + tw, tw - 1u, rows.prio);
        k_pre_hash<<<nb, 256, 0, s>>>(b, pre, f->pstats, rows.prio);
        k_fast_prep<true><<<nb, 256, 0, s>>>(b, nullptr, f->state, f->adm_slot, hd_adm_index(ctx), ctx->n_adm, rows,
                                             fdict, f->fhit, f->fbase, dtab, tw - 1u, pre);
    } else {
        k_fast_prep<false><<<nb, 256, 0, s>>>(b, d_digest, f->state, f->adm_slot, hd_adm_index(ctx), ctx->n_adm, rows,
                                              fdict, f->fhit, f->fbase, dtab, tw - 1u, PreRows{});
    }
    // hd_ctx_inv_levels 2: the root rows hold split_lanes<8>(n) lanes each; T <= split_lanes<K>(n) <= that
    const bool two = p.lean && f->inv_levels == 2;
    const RootRows rr{sc.roots, two ? sc.roots + 9 * (size_t)split_lanes<8>(n) : nullptr};
    fb_launch_sinv(p, f->inv_levels, f->inv_k2, s, n, rows, rr, f->est_dev + 2, f->dstats);
    // HD_VAR_SUM_CHAIN (see FbWork): behind the previous call's sums when it
    // ran on another stream; before the profile pair, so the pair times the
    // kernel and not the wait.  (The 4-wave sums of a small batch stays out: fb_plan_call.)
    if (p.chain && f->sums.wait(s)) f->n_chained++;
    hipEvent_t* pe = fb_prof_pair(f->ev_sums, f->n_sums, f->prof);
    if (pe) (void)hipEventRecord(pe[0], s);
    fb_launch_sums(p, f->wp, nb, s, n, f->gtab, f->tabs, rows);
    if (pe) (void)hipEventRecord(pe[1], s);
    if (p.chain) f->sums.record(s);
    fb_launch_zinv(p, f->inv_levels, f->inv_k2, s, n, rows, rr);
    if (p.lean) f->n_inv[two ? 0 : 1]++;
    // whole blocks of 256: every wavefront's 64 messages are one bitmap word pair
    k_fast_cmp<<<nb, 256, 0, s>>>(b, rows, ctx->d_adm_perm, d_verdict, d_rec32, d_signer, sc.slow, sc.count,
                                  d_bitmap, auth);
}

static int fb_verify_impl(hd_ctx* ctx, const DevBatch& b, const uint8_t* d_digest, uint8_t* d_verdict,
                          uint8_t* d_rec32, int32_t* d_signer, uint32_t* d_bitmap, FbWork::Scratch& sc,
                          hipStream_t s, bool auth);

int hd_fb_verify(hd_ctx* ctx, const DevBatch& b, const uint8_t* d_digest, uint8_t* d_verdict, uint8_t* d_rec32,
                 int32_t* d_signer, uint32_t* d_bitmap, hipStream_t s, bool auth) {
    FbWork* f = ctx->fb;
    f->sums.begin_call();
    if (!f->done) FBCHK(hipEventCreateWithFlags(&f->done, hipEventDisableTiming), "fb event");
    const int j = f->next;
    f->next = (j + 1) % FbWork::NSCRATCH;
    FbWork::Scratch& sc = f->sc[j];
    if (!sc.done) FBCHK(hipEventCreateWithFlags(&sc.done, hipEventDisableTiming), "fb scratch event");
    if (!sc.count) FBCHK(hipMalloc(&sc.count, 32), "fb scratch count");
    // foreign slots re-keyed (fb_evict; it waited for every earlier call)
    bool evicted = false;
    int re = fb_evict(ctx, &evicted);
    if (re) return re;
    // see FbWork: in the steady state only this set's previous user orders
    // this call; otherwise the previous call does, on whatever stream
    const bool steady = !evicted && f->nr_host && *(volatile uint32_t*)f->nr_host == 0 && !fb_foreign_pending(f);
    if (sc.used && sc.stream != s) FBCHK(hipStreamWaitEvent(s, sc.done, 0), "fb scratch order");
    if (f->any && f->last != s && !(steady && f->steady)) FBCHK(hipStreamWaitEvent(s, f->done, 0), "fb stream order");
    hipEvent_t* pe = fb_prof_pair(f->ev_call, f->n_call, f->prof);
    if (pe) (void)hipEventRecord(pe[0], s);
    const int rc = fb_verify_impl(ctx, b, d_digest, d_verdict, d_rec32, d_signer, d_bitmap, sc, s, auth);
    if (pe) (void)hipEventRecord(pe[1], s);
    FBCHK(hipEventRecord(sc.done, s), "fb scratch record");
    FBCHK(hipEventRecord(f->done, s), "fb event record");
    sc.used = true;
    sc.stream = s;
    f->last_set = j;
    f->last = s;
    f->any = true;
    f->steady = steady;
    return rc;
}

// Every verify call of this context has finished (the host waits on the
// call events; other contexts and streams are not waited for).
int hd_fb_quiesce(hd_ctx* ctx) {
    FbWork* f = ctx->fb;
    if (!f) return HD_OK;
    for (auto& sc : f->sc)
        if (sc.used) FBCHK(hipEventSynchronize(sc.done), "fb quiesce");
    if (f->any) FBCHK(hipEventSynchronize(f->done), "fb quiesce");
    return HD_OK;
}

static int fb_verify_impl(hd_ctx* ctx, const DevBatch& b, const uint8_t* d_digest, uint8_t* d_verdict,
                          uint8_t* d_rec32, int32_t* d_signer, uint32_t* d_bitmap, FbWork::Scratch& sc,
                          hipStream_t s, bool auth) {
    FbWork* f = ctx->fb;
    int rc = hd_dev_grow(ctx, (void**)&sc.slow, &sc.cap_slow, 4 * (size_t)b.n);
    if (rc) return rc;
    const uint32_t blocks = (b.n + 255) / 256;
    rc = hd_dev_grow(ctx, (void**)&sc.slow2, &sc.cap_slow2, 4 * (size_t)b.n);
    if (rc) return rc;
    FBCHK(hipMemsetAsync(sc.count, 0, 32, s), "fb count reset");
    if (ctx->n_adm > 0 && f->adm_slot && f->map_ok) {
        if (b.n > HD_DD_MAX_N) {   // ref's encoding (hd_dedup.h); the rows of such a batch exceed the device anyway
            ctx->last_error = "known-key check: more than 2^30 messages in one call";
            return HD_EINVAL;
        }
        const size_t row_words = 63;   // per message
        rc = hd_dev_grow(ctx, (void**)&sc.rows, &sc.cap_rows, 4 * row_words * (size_t)b.n);
        if (rc) return rc;
        const uint32_t n = b.n;
        // the call's plan, from one snapshot of the figures earlier calls left
        // ([2] before [3], the order k_fast_sinv's stores are written for)
        const volatile uint32_t* est = f->est_host;
        const FbCallPlan p = fb_plan_call(FbPlanIn{ctx->var, ctx->n_cu, n, auth, d_digest != nullptr,
                                                   {est[0], est[1], est[2], est[3]}});
        // the repeat table, then the preimage table: one allocation, and one
        // clear over the tables this call uses
        if (p.dedup || p.share) {
            const size_t tab_bytes = 4 * (size_t)dd_table_words(n);
            rc = hd_dev_grow(ctx, (void**)&sc.dtab, &sc.cap_dtab, 2 * tab_bytes);
            if (rc) return rc;
            const size_t first = p.dedup ? 0 : tab_bytes, last = p.share ? 2 * tab_bytes : tab_bytes;
            FBCHK(hipMemsetAsync((uint8_t*)sc.dtab + first, 0xFF, last - first, s), "fb table clear");
        }
        if (p.share) {
            rc = hd_dev_grow(ctx, (void**)&sc.pre, &sc.cap_pre, 40 * (size_t)n);
            if (rc) return rc;
        }
        if (p.lean && f->inv_levels == 2) {   // RootRows: two rows of 9 words per level-1 lane
            rc = hd_dev_grow(ctx, (void**)&sc.roots, &sc.cap_roots, 4 * 18 * (size_t)split_lanes<8>(n));
            if (rc) return rc;
        }
        SplitRows rows;
        rows.aux = sc.rows;
        rows.idx = (int32_t*)(sc.rows + (size_t)n);
        rows.u1 = sc.rows + 2 * (size_t)n;
        rows.u2 = sc.rows + 10 * (size_t)n;
        rows.s = sc.rows + 18 * (size_t)n;
        rows.pre = sc.rows + 26 * (size_t)n;
        rows.xyz = sc.rows + 35 * (size_t)n;
        rows.ref = sc.rows + 62 * (size_t)n;
        rows.cnt = sc.count;
        rows.prio = ctx->var[HD_VAR_WAVE_PRIO];
        launch_split(ctx, b, d_digest, d_verdict, d_rec32, d_signer, d_bitmap, rows, sc, s, auth, p);
        f->last_k = p.k;
        f->n_capped += p.capped;   // hd_ctx_overlap_stats (n_chained: where the wait is placed)
        f->n_lean += p.lean;
        FBCHK(hipGetLastError(), "split check launch");
        // k_fast_cmp wrote the valid bitmap; the slow path sets the bits of
        // its VALID messages
        // HD_VAR_SLOW_LIFT: the lift kernel first (its NO_POINT verdicts leave
        // the list), or k_verify over the whole leftover list (it lifts too).
        // A leftover list is usually under one wave per SIMD, so k_verify's
        // time is one recovery's latency whatever the list length, and the
        // separate lift only adds its own chain in series.
        if (p.lift) {
            k_slow_lift<<<p.lift_blocks, 256, 0, s>>>(b, sc.slow, sc.count, d_verdict, d_rec32, d_signer, sc.slow2,
                                                      sc.count + 1, rows.prio, f->est_dev, rows, f->gtab);
            FBCHK(hipGetLastError(), "k_slow_lift");
        }
        const SlowCtl ctl{p.lift ? sc.slow2 : sc.slow, p.lift ? sc.count + 1 : sc.count, f->adm_slot, f->state, f->pub,
                          d_bitmap, p.lift ? f->est_dev + 1 : f->est_dev, rows.prio,
                          f->fcap ? f->fdict : nullptr, f->fnext, f->fbase, f->fcap, f->fpend_dev,
                          f->fcap ? f->fhit + 64 : nullptr, f->fkey, f->fpend_dev + 1};
        rc = hd_launch_slow(ctx, b, d_digest, d_verdict, d_rec32, d_signer, nullptr, ctl, p.slow_blocks, s);
        if (rc) return rc;
        return fb_learn(ctx, s);
    }
    // no admitted set: every message takes the full recovery (it ends in
    // NOT_ADMITTED at best), nothing to learn
    const SlowCtl none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, nullptr};
    return hd_launch_slow(ctx, b, d_digest, d_verdict, d_rec32, d_signer, d_bitmap, none, blocks, s);
}

extern "C" {

int hd_ctx_set_fastpath(hd_ctx* ctx, int enable) {
    if (!ctx) return HD_EINVAL;
    if (enable && !ctx->fb) {
        (void)hipSetDevice(ctx->device);
        int rc = hd_fb_init(ctx);
        if (rc) return rc;
        // map the current admitted set (sorted words -> bytes)
        if (ctx->n_adm) {
            std::vector<uint32_t> words(8 * (size_t)ctx->n_adm);
            FBCHK(hipMemcpy(words.data(), ctx->d_adm, 32 * (size_t)ctx->n_adm, hipMemcpyDeviceToHost), "adm read");
            std::vector<uint8_t> sorted(32 * (size_t)ctx->n_adm);
            for (size_t k = 0; k < words.size(); k++) store_be32(&sorted[4 * k], words[k]);
            rc = hd_fb_map_signatories(ctx, sorted.data(), ctx->n_adm);
            if (rc) return rc;
        }
    }
    ctx->fastpath = enable != 0;
    return HD_OK;
}

int hd_ctx_fastpath_geometry(hd_ctx* ctx, int* g_windows, int* key_windows, int* msgs_per_inversion) {
    if (!ctx) return HD_EINVAL;
    const int k = ctx->fb ? ctx->fb->last_k : 8;
    if (g_windows) *g_windows = FbL<HD_FB_WG>::NWIN;
    if (key_windows) *key_windows = fb_nwin(ctx->fb ? ctx->fb->wp : HD_FB_W);
    if (msgs_per_inversion) *msgs_per_inversion = k > 0 ? k : 2;
    return HD_OK;
}

int hd_ctx_profile(hd_ctx* ctx, int enable) {
    if (!ctx) return HD_EINVAL;
    if (!ctx->fb) return enable ? HD_EINVAL : HD_OK;   // the profile covers the known-key path's calls
    ctx->fb->prof = enable != 0;
    return HD_OK;
}

int hd_ctx_profile_read(hd_ctx* ctx, uint32_t* calls, double* verify_ms, uint32_t* sums_launches, double* sums_ms) {
    if (!ctx) return HD_EINVAL;
    double tc = 0, ts = 0;
    uint32_t nc = 0, ns = 0;
    if (ctx->fb) {
        FbWork* f = ctx->fb;
        (void)hipSetDevice(ctx->device);
        for (size_t k = 0; k < f->n_call; k++) {
            float ms = 0;
            FBCHK(hipEventSynchronize(f->ev_call[2 * k + 1]), "profile sync");
            FBCHK(hipEventElapsedTime(&ms, f->ev_call[2 * k], f->ev_call[2 * k + 1]), "profile read");
            tc += ms;
        }
        for (size_t k = 0; k < f->n_sums; k++) {
            float ms = 0;
            FBCHK(hipEventSynchronize(f->ev_sums[2 * k + 1]), "profile sync");
            FBCHK(hipEventElapsedTime(&ms, f->ev_sums[2 * k], f->ev_sums[2 * k + 1]), "profile read");
            ts += ms;
        }
        nc = (uint32_t)f->n_call;
        ns = (uint32_t)f->n_sums;
        f->n_call = f->n_sums = 0;
    }
    if (calls) *calls = nc;
    if (verify_ms) *verify_ms = tc;
    if (sums_launches) *sums_launches = ns;
    if (sums_ms) *sums_ms = ts;
    return HD_OK;
}

int hd_ctx_dedup_stats(hd_ctx* ctx, uint64_t* checked, uint64_t* repeats) {
    if (!ctx) return HD_EINVAL;
    if (checked) *checked = 0;
    if (repeats) *repeats = 0;
    if (!ctx->fb || !ctx->fb->dstats) return HD_OK;
    (void)hipSetDevice(ctx->device);
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    unsigned long long st[2] = {0, 0};
    FBCHK(hipMemcpy(st, ctx->fb->dstats, 16, hipMemcpyDeviceToHost), "repeat counters read");
    if (checked) *checked = st[0];
    if (repeats) *repeats = st[1];
    return HD_OK;
}

int hd_ctx_preimage_stats(hd_ctx* ctx, uint64_t* typed, uint64_t* distinct) {
    if (!ctx) return HD_EINVAL;
    if (typed) *typed = 0;
    if (distinct) *distinct = 0;
    if (!ctx->fb || !ctx->fb->pstats) return HD_OK;
    (void)hipSetDevice(ctx->device);
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    unsigned long long st[2] = {0, 0};
    FBCHK(hipMemcpy(st, ctx->fb->pstats, 16, hipMemcpyDeviceToHost), "preimage counters read");
    if (typed) *typed = st[0];
    if (distinct) *distinct = st[1];
    return HD_OK;
}

int hd_ctx_inv_levels(hd_ctx* ctx, int set) {
    if (!ctx || !ctx->fb || (set != -1 && set != 1 && set != 2)) return HD_EINVAL;
    if (set != -1) ctx->fb->inv_levels = set;
    return ctx->fb->inv_levels;
}

int hd_ctx_inv_stats(hd_ctx* ctx, uint64_t out[2]) {
    if (!ctx || !out) return HD_EINVAL;
    const FbWork* f = ctx->fb;
    out[0] = f ? f->n_inv[0] : 0;
    out[1] = f ? f->n_inv[1] : 0;
    return HD_OK;
}

int hd_ctx_overlap_stats(hd_ctx* ctx, uint32_t* capped, uint32_t* lean, uint32_t* chained) {
    if (!ctx) return HD_EINVAL;
    const FbWork* f = ctx->fb;
    if (capped) *capped = f ? f->n_capped : 0;
    if (lean) *lean = f ? f->n_lean : 0;
    if (chained) *chained = f ? f->n_chained : 0;
    return HD_OK;
}

}  // extern "C"
