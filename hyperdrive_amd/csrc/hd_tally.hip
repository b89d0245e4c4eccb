// hd_tally.hip -- GPU tally of authenticated votes: the first-wins vote logs
// of process/process.go:823-892 and the counts the 2f+1 / f+1 rules read
// (process.go:486-494, 534, 574-582, 626-632, 658, 696-702, 751), for every
// (height, round) in a batch at once.
//
// Candidates are VALID Prevotes / Precommits.  Three group-bys:
//
//   G  (h, r)                 open-addressing hash table in HBM, one slot per
//                             round: distinct prevote and precommit signers,
//                             signers with both (probed once per wavefront:
//                             lanes of a wavefront usually share their round)
//   logs (h, r, type, From)   first-wins vote logs (process.go:834-847): for an
//                             admitted From a dense cell (round rank, type,
//                             admitted index) of an L2-resident word array,
//                             first-wins = atomicMin of the batch index; a From
//                             outside the admitted set takes the hashed table D
//   C  (G slot, type, value)  count of first-wins votes per value
//                             (process.go:574-579 and the other count loops)
//
// A hash slot's `claim` word holds the LOWEST batch index of its key: a new
// key claims an empty slot by CAS, an equal key with a lower index lowers it
// by atomicMin.  Keys are never copied -- a probe compares against the
// claimer's fields in the (immutable) batch, so there is no torn-key window.
// The distinct signers of a round over both types (TraceLogs[r] restricted to
// votes, process.go:744-754) are prevotes + precommits - signers with both.
// Counts are integer atomics, hence deterministic; outputs are ordered by the
// batch index of each group's first message (first-item bitmaps and their
// popcount prefixes, no sort).
// Non-winners compare their value with the winner's: identical -> dropped
// silently, different -> the double vote handed to Catcher.CatchDouble*
// (process.go:838-843, 875-880).
//
// hd_decide (the end of this file) runs the same passes with the propose log
// of process.go:758-819 beside them -- a fourth claim table P keyed (h, r) --
// and turns each round's counts into one row with the eight predicate bits.
// hd_decide_ordered adds a sort of the logged votes by (round, batch index)
// and a per-row walk that finds the message at which each predicate first
// holds in batch order.  hd_decide_catch adds the list of offences, each with
// the logged message it contradicts (two passes before the tables are cleaned).
#include <hip/hip_runtime.h>

#include <chrono>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <type_traits>
#include <vector>

#include "hd_internal.h"
#include "hd_verify_msg.h"

using namespace hd;

static const uint32_t kEmpty = 0xFFFFFFFFu;

struct TallyWork {
    DevBuf b[24];   // one per TSlot (static_assert below the enum)
    void* host = nullptr;   // pinned download stage (hipHostMalloc)
    size_t host_cap = 0;
    uint32_t* scalar = nullptr;   // pinned word (a partition's candidate count)
    // staged row capacities (the last call's counts + 1/4); atomic: an async
    // collect may raise them while another thread submits
    std::atomic<uint32_t> guess_hr{1024}, guess_cnt{1024};
    // the tables clean themselves (k_tally_emit): cleared only when their
    // allocation or capacity changes, or a call did not queue all its launches
    struct Clean {
        bool dirty = false;
        const void* p = nullptr;
        uint32_t k = 0;
    } tab, ptab;   // ptab: hd_decide's propose claim table (cleaned by k_decide_clean)
    std::atomic<uint32_t> guess_dec{1024};   // hd_decide: the staged row capacity
    std::atomic<uint32_t> guess_catch{1024}; // hd_decide_catch: the staged record capacity
};
// T_G: the hash tables and call counters; T_C: the dense log cells; T_D /
// T_SORTK / T_TMP: a partition's candidate compaction; T_GSLOT / T_DSLOT /
// T_CSLOT: per-item round slot, log reference and count slot; T_BITS: the
// first-item bitmaps and their prefixes; T_SEL: the output stage; T_NSEL: the
// overflow rows; T_DUP: a routed batch's classification when it is scattered
// on the device instead of staged; T_CHECK: HD_TALLY_CHECK's counters;
// hd_decide: T_P the propose claim table, T_PSLOT per-item propose slot,
// T_DSTAGE / T_DOVF its output stage and overflow rows, T_SCHED / T_VOK the
// host form's uploaded schedule and value_ok bytes; hd_decide_ordered: T_WKEY /
// T_WVAL the per-item sort keys and batch indices (unsorted | sorted), T_WTMP
// the radix sort's temporary storage; hd_decide_catch: T_CATCH the overflow
// records and, when the caller takes no classes, the classes' scratch
enum TSlot { T_G, T_D, T_C, T_GSLOT, T_DSLOT, T_NSEL, T_SEL, T_SORTK, T_TMP, T_DUP, T_ROUTE, T_CHECK,
             T_CSLOT, T_BITS, T_P, T_PSLOT, T_DSTAGE, T_DOVF, T_SCHED, T_VOK, T_WKEY, T_WVAL, T_WTMP, T_CATCH, T_COUNT };
static_assert(T_COUNT == sizeof(TallyWork::b) / sizeof(DevBuf), "a buffer for every TSlot");

// table layouts (structure of arrays inside one allocation, capacity cap)
struct GTab {   // (h, r)
    uint32_t* claim;
    uint32_t* nprev;
    uint32_t* nprec;
    uint32_t* nboth;
    uint32_t* gid;   // the round's number (creation order): its dense log cells
};
struct CTab {   // (G slot, type, value)
    uint32_t* claim;
    uint32_t* n;
};
struct TallyCtr {   // 64 B, zero between calls (k_tally_emit resets it)
    uint32_t n_rounds;   // rounds numbered so far (k_tally_rounds)
    uint32_t pad[15];
};


HD uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

HD uint64_t hash_hr(int64_t h, int64_t r) {
    return mix64((uint64_t)h * 0x9E3779B97F4A7C15ull ^ mix64((uint64_t)r));
}
// partition of a round among nparts (the high half of its hash; the table
// probes use the low bits)
HD uint32_t part_of(uint64_t hhr, uint32_t nparts) { return nparts > 1 ? (uint32_t)((hhr >> 32) % nparts) : 0u; }

struct Part {
    uint32_t part, nparts;
};

// verdict and bitmap both NULL: every Prevote / Precommit is a candidate (a
// batch of routed candidates, hd_unroute_device)
__device__ __forceinline__ bool candidate(const DevBatch& b, const uint8_t* verdict, const uint32_t* bitmap,
                                          uint32_t i, Part p) {
    const uint8_t t = b.type[i];
    if (t != T_PREVOTE && t != T_PRECOMMIT) return false;
    if (verdict && verdict[i] != V_VALID) return false;
    if (bitmap && !((bitmap[i >> 5] >> (i & 31)) & 1u)) return false;
    return p.nparts <= 1 || part_of(hash_hr(b.height[i], b.round[i]), p.nparts) == p.part;
}

__device__ __forceinline__ bool eq32(const uint8_t* a, const uint8_t* b) {
    const uint4* x = reinterpret_cast<const uint4*>(a);
    const uint4* y = reinterpret_cast<const uint4*>(b);
    const uint4 x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[1];
    return ((x0.x ^ y0.x) | (x0.y ^ y0.y) | (x0.z ^ y0.z) | (x0.w ^ y0.w) | (x1.x ^ y1.x) | (x1.y ^ y1.y) |
            (x1.z ^ y1.z) | (x1.w ^ y1.w)) == 0;
}

// Claim-or-find.  Returns the slot and whether this call created it; the
// slot's claim word ends up holding the lowest index of its key.
template <typename Eq>
__device__ __forceinline__ uint32_t probe(uint32_t* claim, uint32_t mask, uint64_t hash, uint32_t i, Eq eq,
                                          bool& created) {
    uint32_t s = (uint32_t)hash & mask;
    while (true) {
        uint32_t c = claim[s];
        if (c == kEmpty) {
            c = atomicCAS(&claim[s], kEmpty, i);
            if (c == kEmpty) {
                created = true;
                return s;
            }
        }
        if (eq(c)) {
            if (i < c) atomicMin(&claim[s], i);
            created = false;
            return s;
        }
        s = (s + 1) & mask;
    }
}
// Read-only lookup (the table is complete): the slot of a key that exists.
template <typename Eq>
__device__ __forceinline__ uint32_t find(const uint32_t* claim, uint32_t mask, uint64_t hash, Eq eq) {
    uint32_t s = (uint32_t)hash & mask;
    while (true) {
        const uint32_t c = claim[s];
        if (c == kEmpty) return kEmpty;
        if (eq(c)) return s;
        s = (s + 1) & mask;
    }
}

// Adds one wavefront's 0/1 increments to a counter array.  Lanes of a
// wavefront usually share their slot (batches arrive in height order), so
// the lanes whose slot equals the first active lane's add with one atomic
// (ballot + popcount over the active lanes only); the others fall back to
// their own.
__device__ __forceinline__ void wave_add(uint32_t* ctr, uint32_t slot, bool inc) {
    const unsigned long long act = __ballot(true);
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)act) - 1;
    const uint32_t s0 = __shfl(slot, leader, 64);
    const bool mine = slot == s0;
    const uint32_t v = (uint32_t)__popcll(__ballot(mine && inc));
    if (lane == leader && v) atomicAdd(&ctr[s0], v);
    if (!mine && inc) atomicAdd(&ctr[slot], 1u);
}

// Lanes of a wavefront usually share their round (batches arrive in height
// order): the first active lane -- the lowest batch index among them -- probes
// for every lane whose key equals its key and broadcasts the slot; the
// others probe on their own.  Skipping the followers' probes keeps the
// first-wins claim exact: their indices are higher than the leader's.  This
// turns up to 64 same-address CAS / atomicMin per wavefront into one.
__device__ __forceinline__ int first_active_lane() {
    return __ffsll((long long)__ballot(true)) - 1;
}
__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src, 64), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

__device__ __forceinline__ uint64_t hash_log(uint64_t hhr, const uint8_t* from, uint32_t t) {
    return mix64(hhr ^ *reinterpret_cast<const uint64_t*>(from) ^ (uint64_t)t);
}

// Items.  The whole-batch tally walks every message (item p = batch index
// p); a partition's tally first compacts its candidates into cand[] (in
// batch order, k_tally_flag + the ordered compaction below), so that every
// later pass and every index array is sized by the partition's candidates,
// not by the replicated batch (G ranks x the per-GPU batch).  Claim words
// hold item numbers, which order like batch indices.
__device__ __forceinline__ uint32_t msg_of(const uint32_t* cand, uint32_t p) { return cand ? cand[p] : p; }

// a partition's candidates: at[i] = i, others empty; dup of the others = 3
__global__ __launch_bounds__(256) void k_tally_flag(DevBatch b, const uint8_t* __restrict__ verdict,
                                                    const uint32_t* __restrict__ bitmap, Part p,
                                                    uint32_t* __restrict__ at, uint8_t* __restrict__ dup) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < b.n; i += gridDim.x * blockDim.x) {
        const bool c = candidate(b, verdict, bitmap, i, p);
        at[i] = c ? i : kEmpty;
        if (dup && !c) dup[i] = 3;
    }
}

// pass 1: every candidate -> its round (G slot).  Lanes of a wavefront
// usually share their round, so the first candidate lane probes for all lanes
// with its (h, r) (shfl64).  Without cand[] the pass also filters the
// candidates.  The lane that creates a round's slot numbers the round
// (gid, in creation order) and its wavefront clears the round's 2S dense log
// cells, so the cells need no clearing pass.  The loop is wavefront-uniform
// (every lane reaches the ballots).
__global__ void k_tally_rounds(DevBatch b, const uint32_t* __restrict__ cand, uint32_t m,
                               const uint8_t* __restrict__ verdict, const uint32_t* __restrict__ bitmap, Part p,
                               GTab G, uint32_t mask, uint32_t* __restrict__ gslot, uint8_t* __restrict__ dup,
                               TallyCtr* ctr, uint32_t* __restrict__ Dd, uint32_t per, uint32_t nd) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * blockDim.x; base < m; base += stride) {
        const uint32_t q = base + threadIdx.x;
        bool c = q < m;
        const uint32_t i = c ? msg_of(cand, q) : 0u;
        if (c && !cand && !candidate(b, verdict, bitmap, i, p)) {
            if (dup) dup[i] = 3;
            gslot[q] = kEmpty;
            c = false;
        }
        const unsigned long long act = __ballot(c);
        if (!act) continue;
        const int lead = __ffsll((long long)act) - 1;
        const int64_t h = c ? b.height[i] : 0, r = c ? b.round[i] : 0;
        const int64_t hl = shfl64(h, lead), rl = shfl64(r, lead);   // every lane takes part in the shuffles
        const bool follower = c && lane != lead && hl == h && rl == r;
        uint32_t g = kEmpty, id = kEmpty;
        bool created = false;
        if (c && !follower) {
            g = probe(G.claim, mask, hash_hr(h, r), q,
                      [&](uint32_t o) {
                          const uint32_t io = msg_of(cand, o);
                          return b.height[io] == h && b.round[io] == r;
                      },
                      created);
            if (created) {
                id = atomicAdd(&ctr->n_rounds, 1u);
                G.gid[g] = id;
            }
        }
        const uint32_t gl = (uint32_t)__shfl((int)g, lead, 64);
        if (c) gslot[q] = follower ? gl : g;
        // the new rounds' dense cells, one round at a time by the whole wavefront
        unsigned long long cr = __ballot(created && id < nd);
        while (cr) {
            const int l = __ffsll((long long)cr) - 1;
            const uint32_t idl = (uint32_t)__shfl((int)id, l, 64);
            uint32_t* cells = Dd + (size_t)idl * per;
            for (uint32_t k = lane; k < per; k += 64) cells[k] = kEmpty;
            cr &= cr - 1;
        }
    }
}

// Dense vote logs.  A candidate's log key (h, r, type, From) is, for an
// admitted From, the cell (round number, type, admitted index) of an array of
// nd x 2 x S words -- a few MB, L2-resident -- and first-wins is one
// atomicMin of the item number into that cell: no hashing, no key compares
// against the batch.  A From outside the context's admitted set (possible
// when the caller's verdicts predate a set change), or a round numbered past
// the dense cells (a batch of very many rounds), takes the hashed table D
// instead; a signatory's prevote and precommit of a round always take the
// same path.  ref[q]: the cell index, or HD_REF_HASHED | the D slot.
#define HD_REF_HASHED 0x80000000u
__global__ void k_tally_logs(DevBatch b, const uint32_t* __restrict__ cand, uint32_t m,
                             const uint32_t* __restrict__ gslot, const uint32_t* __restrict__ gid,
                             AdmIndex ix, uint32_t S, uint32_t* __restrict__ Dd, uint32_t nd,
                             uint32_t* __restrict__ D, uint32_t mask, uint32_t* __restrict__ ref) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += stride) {
        const uint32_t g = gslot[q];
        if (g == kEmpty) continue;
        const uint32_t i = msg_of(cand, q);
        const uint8_t t = b.type[i];
        const uint8_t* from = b.from32 + 32 * (size_t)i;
        const uint32_t rid = gid[g];
        int32_t signer = -1;
        if (rid < nd) {
            uint32_t from_be[8];
            load_row32_be(from_be, b.from32, i);
            signer = adm_index_find(ix, from_be);
        }
        if (signer >= 0) {
            const uint32_t cell = (rid * 2u + (t == T_PRECOMMIT ? 1u : 0u)) * S + (uint32_t)signer;
            atomicMin(&Dd[cell], q);
            ref[q] = cell;
        } else {
            const int64_t h = b.height[i], r = b.round[i];
            bool created;
            const uint32_t d = probe(D, mask, hash_log(hash_hr(h, r), from, t), q,
                                     [&](uint32_t o) {
                                         const uint32_t io = msg_of(cand, o);
                                         return b.type[io] == t && b.height[io] == h && b.round[io] == r &&
                                                eq32(b.from32 + 32 * (size_t)io, from);
                                     },
                                     created);
            ref[q] = HD_REF_HASHED | d;
        }
    }
}

// the C table's key hash: (G slot, type, value)
__device__ __forceinline__ uint64_t hash_count(const uint8_t* value, uint32_t g, uint8_t t) {
    const uint64_t hv = *reinterpret_cast<const uint64_t*>(value) ^ *reinterpret_cast<const uint64_t*>(value + 8);
    return mix64(hv ^ ((uint64_t)g << 1 | (t & 1u)));
}

// Per-value counts of a wavefront's winners: the distinct (round, type,
// value) keys among the active lanes are handled one at a time -- the lowest
// lane holding a key (the lowest item, so first-wins of the claim word stays
// exact) probes C once and adds the number of lanes with that key in one
// atomic.  A batch's votes repeat few values per round, so this is a few
// probes and atomics per wavefront instead of one per lane on a handful of
// hot words.  Returns the C slot of this lane's key.
__device__ __forceinline__ uint32_t count_value(CTab C, uint32_t mask, const DevBatch& b, const uint32_t* cand,
                                                const uint32_t* gslot, uint32_t g, uint8_t t, uint32_t q,
                                                const uint8_t* value) {
    const uint4* vw = reinterpret_cast<const uint4*>(value);
    const uint4 v0 = vw[0], v1 = vw[1];
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(true);
    uint32_t mine = 0;   // on a key's lowest lane: the number of lanes with the key
    int my_lead = lane;  // the lowest lane with this lane's key
    while (pending) {
        const int lead = __ffsll((long long)pending) - 1;
        uint32_t diff = (uint32_t)__shfl((int)g, lead, 64) ^ g;
        diff |= (uint32_t)__shfl((int)t, lead, 64) ^ t;
        diff |= (uint32_t)__shfl((int)v0.x, lead, 64) ^ v0.x;
        diff |= (uint32_t)__shfl((int)v0.y, lead, 64) ^ v0.y;
        diff |= (uint32_t)__shfl((int)v0.z, lead, 64) ^ v0.z;
        diff |= (uint32_t)__shfl((int)v0.w, lead, 64) ^ v0.w;
        diff |= (uint32_t)__shfl((int)v1.x, lead, 64) ^ v1.x;
        diff |= (uint32_t)__shfl((int)v1.y, lead, 64) ^ v1.y;
        diff |= (uint32_t)__shfl((int)v1.z, lead, 64) ^ v1.z;
        diff |= (uint32_t)__shfl((int)v1.w, lead, 64) ^ v1.w;
        const unsigned long long same = __ballot(diff == 0 && ((pending >> lane) & 1ull));
        if ((same >> lane) & 1ull) my_lead = lead;
        if (lane == lead) mine = (uint32_t)__popcll(same);
        pending &= ~same;
    }
    // the keys' lowest lanes probe C together (their keys differ), instead of
    // one after another inside the loop above
    uint32_t c = kEmpty;
    if (mine) {
        bool created;
        c = probe(C.claim, mask, hash_count(value, g, t), q,
                  [&](uint32_t o) {
                      const uint32_t io = msg_of(cand, o);
                      return gslot[o] == g && b.type[io] == t && eq32(b.value32 + 32 * (size_t)io, value);
                  },
                  created);
        atomicAdd(&C.n[c], mine);
    }
    return (uint32_t)__shfl((int)c, my_lead, 64);
}

// pass 3: each log entry's winner (the lowest item of its key) counts as a
// distinct signer of its type in the round and counts its value (C); a
// prevote winner whose signer also has a precommit log in the round counts
// in nboth.  The other candidates are classified against the winner's value.
// cslot[q]: a winner's C slot, kEmpty for the other candidates.
__global__ void k_tally_values(DevBatch b, const uint32_t* __restrict__ cand, uint32_t m,
                               const uint32_t* __restrict__ Dd, uint32_t S, const uint32_t* __restrict__ D,
                               GTab G, CTab C, uint32_t mask, const uint32_t* __restrict__ gslot,
                               const uint32_t* __restrict__ ref, uint32_t* __restrict__ cslot,
                               uint8_t* __restrict__ dup) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += stride) {
        const uint32_t g = gslot[q];
        if (g == kEmpty) continue;
        const uint32_t i = msg_of(cand, q);
        const uint32_t rf = ref[q];
        const bool hashed = (rf & HD_REF_HASHED) != 0;
        const uint32_t w = hashed ? D[rf & ~HD_REF_HASHED] : Dd[rf];
        const uint8_t* value = b.value32 + 32 * (size_t)i;
        if (w != q) {
            if (dup) dup[i] = eq32(b.value32 + 32 * (size_t)msg_of(cand, w), value) ? 1 : 2;
            cslot[q] = kEmpty;
            continue;
        }
        if (dup) dup[i] = 0;
        const uint8_t t = b.type[i];
        wave_add(G.nprev, g, t == T_PREVOTE);
        wave_add(G.nprec, g, t == T_PRECOMMIT);
        bool both = false;
        if (t == T_PREVOTE) {
            if (!hashed) {
                both = Dd[rf + S] != kEmpty;   // the same signer's precommit cell of the round
            } else {
                const int64_t h = b.height[i], r = b.round[i];
                const uint8_t* from = b.from32 + 32 * (size_t)i;
                const uint32_t o = find(D, mask, hash_log(hash_hr(h, r), from, T_PRECOMMIT), [&](uint32_t c) {
                    const uint32_t ic = msg_of(cand, c);
                    return b.type[ic] == T_PRECOMMIT && b.height[ic] == h && b.round[ic] == r &&
                           eq32(b.from32 + 32 * (size_t)ic, from);
                });
                both = o != kEmpty;
            }
        }
        wave_add(G.nboth, g, both);
        cslot[q] = count_value(C, mask, b, cand, gslot, g, t, q, value);
    }
}

// Output order: the groups of each table by their first item.  A group's
// first item is the one its slot's claim word holds; the per-item flags
// "first of its round" / "first of its (round, type, value)" are bitmaps
// Bg / Bc, one bit per item, and an item's output position is the number of
// flags before it.  Both passes below give each block IPB consecutive items
// (IPB / 32 bitmap words it alone writes; IPB = 256 .. 2048, the largest
// that still gives about four blocks per CU, tally_ipb()):
//   k_tally_firsts  the block's flags as whole words (two ballots per
//                   wavefront: no atomics, nothing to clear), their popcount
//                   prefix within the block, and the block's totals;
//   k_tally_emit    each block first sums the totals of the blocks before it
//                   (its offsets; the last block also writes the group counts
//                   into the stage header), then every first item writes its
//                   group's row at its position (rows past the staged
//                   capacity go to the overflow columns) and resets its table
//                   slots, so the tables are clean for the next call without
//                   a clearing pass.
// The offsets are summed by every emit block rather than scanned once by the
// last block of k_tally_firsts: that scan needed a ticket counter, and the
// device-scope release each block made before taking its ticket writes back
// the block's XCD L2 -- dirty with the verify kernels' rows when the tally
// runs beside them (39 us for 501 blocks of a 128k batch, against ~5 us
// for the sums, nb^2 / 2 L2-resident words).
#define HD_TALLY_IPB_MAX 2048u   // items per block (8 per thread)

template <uint32_t IPB>
__global__ __launch_bounds__(256) void k_tally_firsts(uint32_t m, const uint32_t* __restrict__ gslot,
                                                      const uint32_t* __restrict__ cslot, const uint32_t* G_claim,
                                                      const uint32_t* C_claim, uint32_t* __restrict__ Bg,
                                                      uint32_t* __restrict__ Bc, uint32_t* __restrict__ pre_g,
                                                      uint32_t* __restrict__ pre_c, uint32_t* __restrict__ blk) {
    constexpr uint32_t W = IPB / 32;   // words per block (<= 64: one wavefront scans them)
    __shared__ uint32_t wg[W], wc[W];
    const uint32_t nb = gridDim.x;
    const uint32_t lo = blockIdx.x * IPB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t k = 0; k < IPB / 256; k++) {
        const uint32_t q = lo + k * 256 + threadIdx.x;
        bool fg = false, fc = false;
        if (q < m) {
            const uint32_t g = gslot[q];
            if (g != kEmpty) {
                fg = G_claim[g] == q;
                const uint32_t c = cslot[q];
                fc = c != kEmpty && C_claim[c] == q;
            }
        }
        const unsigned long long bg = __ballot(fg), bc = __ballot(fc);
        if (lane == 0) {
            const uint32_t w = k * 8 + wave * 2;
            wg[w] = (uint32_t)bg;
            wg[w + 1] = (uint32_t)(bg >> 32);
            wc[w] = (uint32_t)bc;
            wc[w + 1] = (uint32_t)(bc >> 32);
        }
    }
    __syncthreads();
    if (threadIdx.x < W) {   // one lane per word (wavefront 0)
        const uint32_t t = threadIdx.x, gw = wg[t], cw = wc[t];
        uint32_t ig = (uint32_t)__popc(gw), ic = (uint32_t)__popc(cw);
        for (int d = 1; d < 64; d <<= 1) {   // inclusive scan across the wavefront
            const uint32_t yg = (uint32_t)__shfl_up((int)ig, d, 64), yc = (uint32_t)__shfl_up((int)ic, d, 64);
            if ((int)t >= d) {
                ig += yg;
                ic += yc;
            }
        }
        const size_t wi = (size_t)blockIdx.x * W + t;
        Bg[wi] = gw;
        Bc[wi] = cw;
        pre_g[wi] = ig - (uint32_t)__popc(gw);
        pre_c[wi] = ic - (uint32_t)__popc(cw);
        if (t == W - 1) {
            blk[blockIdx.x] = ig;
            blk[nb + blockIdx.x] = ic;
        }
    }
}

// the output rows of one call, column arrays at capacities (H, Cg) in the
// stage and (m - H, m - Cg) in the overflow
struct TallyCols {
    int64_t *o_h, *o_r, *c_h, *c_r;
    uint32_t *o_prev, *o_prec, *o_any, *o_rep, *c_rep, *c_n;
    uint8_t* c_t;
};

// Column tables.  A block of rows at capacity `cap` is a structure of arrays: column after column in the
// table's order, each width * cap bytes.  One table per row kind names, per column, the kernels' pointer
// (TallyCols / DecideCols) and the caller's array (hd_tally_out / hd_decide_out), so the layout the kernels
// write, the row size and every copy out of a block come from one list.
struct Col {
    size_t width, dev, out;   // bytes per row; offset of the column's pointer in the kernels' struct, in the out struct
};
template <size_t W, size_t WO>
constexpr Col col_of(size_t dev, size_t out) {
    static_assert(W == WO, "the kernels' and the caller's column hold the same type");
    return Col{W, dev, out};
}
#define HD_COL(D, d, O, o) col_of<sizeof(*D::d), sizeof(*O::o)>(offsetof(D, d), offsetof(O, o))
template <size_t N>
constexpr size_t row_bytes(const Col (&cols)[N]) {
    size_t b = 0;
    for (size_t k = 0; k < N; k++) b += cols[k].width;
    return b;
}
// the kernels' pointers of the block at (base, cap), into the struct at x
template <size_t N>
HD_HOSTONLY void cols_layout(const Col (&cols)[N], char* base, size_t cap, void* x) {
    for (const Col& c : cols) {
        memcpy(static_cast<char*>(x) + c.dev, &base, sizeof base);
        base += c.width * cap;
    }
}
// `rows` rows of every column of the block at (base, cap) into the caller's arrays of `out`, from row `at`
// on; a NULL array is skipped.  copy(dst, src, bytes) returns a hipError_t: copy_host from a downloaded
// stage, copy_down(s) from the overflow block on the device.
template <size_t N, typename Copy>
HD_HOSTONLY int cols_copy(hd_ctx* ctx, const Col (&cols)[N], const char* base, size_t cap, size_t rows, size_t at,
                          const void* out, Copy copy) {
    for (const Col& c : cols) {
        char* dst;
        memcpy(&dst, static_cast<const char*>(out) + c.out, sizeof dst);
        if (dst && rows)
            if (hipError_t e = copy(dst + c.width * at, base, c.width * rows)) return hd_ctx_fail(ctx, e, "row copy");
        base += c.width * cap;
    }
    return HD_OK;
}
HD_HOSTONLY hipError_t copy_host(void* dst, const void* src, size_t bytes) { return memcpy(dst, src, bytes), hipSuccess; }
// a download queued on s (the caller synchronises once)
HD_HOSTONLY auto copy_down(hipStream_t s) {
    return [s](void* dst, const void* src, size_t n) { return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s); };
}
HD_HOSTONLY size_t pad64(size_t n) { return (n + 63) & ~(size_t)63; }

// the tally's per-round rows, then its per-value rows at a capacity of their own
constexpr Col kRoundCols[] = {
    HD_COL(TallyCols, o_h, hd_tally_out, hr_height),      HD_COL(TallyCols, o_r, hd_tally_out, hr_round),
    HD_COL(TallyCols, o_prev, hd_tally_out, hr_prevotes), HD_COL(TallyCols, o_prec, hd_tally_out, hr_precommits),
    HD_COL(TallyCols, o_any, hd_tally_out, hr_any),       HD_COL(TallyCols, o_rep, hd_tally_out, hr_rep),
};
constexpr Col kValueCols[] = {
    HD_COL(TallyCols, c_h, hd_tally_out, count_height), HD_COL(TallyCols, c_r, hd_tally_out, count_round),
    HD_COL(TallyCols, c_rep, hd_tally_out, count_rep),  HD_COL(TallyCols, c_n, hd_tally_out, count_n),
    HD_COL(TallyCols, c_t, hd_tally_out, count_type),
};
constexpr size_t kRoundRow = row_bytes(kRoundCols), kValueRow = row_bytes(kValueCols);
static_assert(kRoundRow == 2 * 8 + 4 * 4 && kValueRow == 2 * 8 + 2 * 4 + 1, "tally row bytes");
static_assert(sizeof(kRoundCols) / sizeof(Col) + sizeof(kValueCols) / sizeof(Col) == sizeof(TallyCols) / sizeof(void*),
              "every TallyCols pointer is a column of one table");

HD_HOSTONLY TallyCols tally_cols(char* base, uint32_t h, uint32_t c) {
    TallyCols x;
    cols_layout(kRoundCols, base, h, &x);
    cols_layout(kValueCols, base + kRoundRow * h, c, &x);
    return x;
}
// the rows of such a pair of blocks into out, from rows (at_hr, at_cnt) on
template <typename Copy>
HD_HOSTONLY int tally_rows_copy(hd_ctx* ctx, const char* base, uint32_t h, uint32_t c, uint32_t n_hr, uint32_t n_cnt,
                                uint32_t at_hr, uint32_t at_cnt, const hd_tally_out* out, Copy copy) {
    if (int rc = cols_copy(ctx, kRoundCols, base, h, n_hr, at_hr, out, copy)) return rc;
    return cols_copy(ctx, kValueCols, base + kRoundRow * h, c, n_cnt, at_cnt, out, copy);
}

template <uint32_t IPB>
__global__ __launch_bounds__(256) void k_tally_emit(DevBatch b, const uint32_t* __restrict__ cand, uint32_t m,
                                                    const uint32_t* __restrict__ gidx, const uint32_t* __restrict__ gslot,
                                                    const uint32_t* __restrict__ cslot, const uint32_t* __restrict__ ref,
                                                    GTab G, CTab C, uint32_t* __restrict__ D,
                                                    const uint32_t* __restrict__ Bg, const uint32_t* __restrict__ Bc,
                                                    const uint32_t* __restrict__ pre_g, const uint32_t* __restrict__ pre_c,
                                                    const uint32_t* __restrict__ blk, TallyCols st, uint32_t H,
                                                    uint32_t Cg, TallyCols ov, TallyCtr* ctr, uint32_t* stage_hdr) {
    const uint32_t nb = gridDim.x;
    // this block's offsets: the totals of the blocks before it
    __shared__ uint32_t part[2][4];
    uint32_t sg = 0, sc = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256) {
        sg += blk[k];
        sc += blk[nb + k];
    }
    for (int d = 32; d > 0; d >>= 1) {
        sg += (uint32_t)__shfl_xor((int)sg, d, 64);
        sc += (uint32_t)__shfl_xor((int)sc, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = sg;
        part[1][threadIdx.x >> 6] = sc;
    }
    __syncthreads();
    const uint32_t og = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    const uint32_t oc = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (threadIdx.x == 0) {
        if (blockIdx.x == nb - 1) {
            stage_hdr[0] = og + blk[nb - 1];        // rounds (hr rows)
            stage_hdr[1] = oc + blk[2 * nb - 1];    // (round, type, value) groups
            stage_hdr[2] = 0;                       // an async ticket's completion word (k_tally_signal)
        }
        if (blockIdx.x == 0) ctr->n_rounds = 0;     // k_tally_rounds' numbering, for the next call
    }
    const uint32_t lo = blockIdx.x * IPB;
    for (uint32_t k = 0; k < IPB / 256; k++) {
        const uint32_t q = lo + k * 256 + threadIdx.x;
        if (q >= m) break;
        const uint32_t g = gslot[q];
        if (g == kEmpty) continue;
        const uint32_t i = msg_of(cand, q), w = q >> 5, below = (1u << (q & 31)) - 1u;
        const uint32_t gw = Bg[w], cw = Bc[w];
        if ((gw >> (q & 31)) & 1u) {   // the round's first candidate: its hr row
            const uint32_t pos = og + pre_g[w] + (uint32_t)__popc(gw & below);
            const TallyCols& x = pos < H ? st : ov;
            const uint32_t j = pos < H ? pos : pos - H;
            const uint32_t np = G.nprev[g], nc = G.nprec[g], nbo = G.nboth[g];
            x.o_h[j] = b.height[i];
            x.o_r[j] = b.round[i];
            x.o_prev[j] = np;
            x.o_prec[j] = nc;
            x.o_any[j] = np + nc - nbo;
            x.o_rep[j] = gidx ? gidx[i] : i;
            G.claim[g] = kEmpty;
            G.nprev[g] = G.nprec[g] = G.nboth[g] = 0;
        }
        if ((cw >> (q & 31)) & 1u) {   // the (round, type, value) group's first winner: its count row
            const uint32_t c = cslot[q];
            const uint32_t pos = oc + pre_c[w] + (uint32_t)__popc(cw & below);
            const TallyCols& x = pos < Cg ? st : ov;
            const uint32_t j = pos < Cg ? pos : pos - Cg;
            x.c_h[j] = b.height[i];
            x.c_r[j] = b.round[i];
            x.c_t[j] = b.type[i];
            x.c_rep[j] = gidx ? gidx[i] : i;
            x.c_n[j] = C.n[c];
            C.claim[c] = kEmpty;
            C.n[c] = 0;
        }
        const uint32_t rf = ref[q];
        if ((rf & HD_REF_HASHED) && D[rf & ~HD_REF_HASHED] == q) D[rf & ~HD_REF_HASHED] = kEmpty;   // the log's winner
    }
}

// An async tally's completion, after its download on the same stream: word 2
// of the caller's pinned stage (mapped) becomes 1.  hd_tally_collect polls it
// instead of synchronising an event: a thread blocked in hipEventSynchronize
// slowed the verify launches of the submitting thread 4x (c3_host_probe,
// HD_BENCH_ASYNC_TALLY=1: 0.18 ms per verify enqueue against 0.04).
__global__ void k_tally_signal(uint32_t* word) {
    if (threadIdx.x == 0) __hip_atomic_store(word, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// HD_TALLY_CHECK after k_tally_emit: the tables are clean again
__global__ void k_tally_check_clean(uint32_t cap, const uint32_t* __restrict__ tabs, TallyCtr* ctr, uint32_t* bad) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += gridDim.x * blockDim.x) {
        bool ok = true;
        for (int k = 0; k < 3; k++) ok &= tabs[(size_t)k * cap + s] == kEmpty;
        for (int k = 3; k < 7; k++) ok &= tabs[(size_t)k * cap + s] == 0u;
        if (!ok && atomicAdd(bad, 1u) == 0) printf("hd tally check: slot %u not clean after the emit\n", s);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && ctr->n_rounds) atomicAdd(bad, 1u);
}

// ------------------------------------------------- consistency check (debug)
// HD_TALLY_CHECK=1 in the environment: after k_tally_values, three kernels
// re-derive the tables' invariants and the host compares them (a violation is
// HD_EDEVICE with the counters in the context's last error, and the first
// offending slot printed by the device):
//   * every candidate's log cell holds an item of the same cell, no later than
//     itself (a stale or foreign cell would silently drop a winner);
//   * every non-empty dense cell / hashed D slot holds an item that maps to it;
//   * no two C (or D) slots hold the same key: the probe from the key of a
//     slot's claimer finds that slot first;
//   * every C claimer is a winner;
//   * winners == sum over G of (prevotes + precommits) == sum over C of n
//     == non-empty dense cells + D claims.
struct TallyCheck {
    uint32_t winners, cells, d_claims, sum_g, sum_c, stale, bad_cell, dup_key, bad_claim, pad[7];
};

__device__ __forceinline__ uint32_t cell_value(const uint32_t* Dd, const uint32_t* D, uint32_t rf) {
    return (rf & HD_REF_HASHED) ? D[rf & ~HD_REF_HASHED] : Dd[rf];
}

__global__ void k_tally_check_items(uint32_t m, const uint32_t* __restrict__ gslot, const uint32_t* __restrict__ ref,
                                    const uint32_t* __restrict__ Dd, const uint32_t* __restrict__ D,
                                    TallyCheck* chk) {
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += gridDim.x * blockDim.x) {
        if (gslot[q] == kEmpty) continue;
        const uint32_t rf = ref[q], w = cell_value(Dd, D, rf);
        if (w == q) {
            atomicAdd(&chk->winners, 1u);
        } else if (w == kEmpty || w > q || gslot[w] == kEmpty || ref[w] != rf) {
            if (atomicAdd(&chk->stale, 1u) == 0)
                printf("hd tally check: item %u ref %08x holds %u (ref %08x)\n", q, rf, w,
                       w < m ? ref[w] : 0xFFFFFFFFu);
        }
    }
}

__global__ void k_tally_check_cells(const uint32_t* __restrict__ Dd, const TallyCtr* ctr, uint32_t per, uint32_t nd,
                                    uint32_t m, const uint32_t* __restrict__ ref, TallyCheck* chk) {
    if (!Dd) return;
    const size_t cells = (size_t)min(ctr->n_rounds, nd) * per;   // the rounds numbered into dense cells
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < cells; c += (size_t)gridDim.x * blockDim.x) {
        const uint32_t w = Dd[c];
        if (w == kEmpty) continue;
        atomicAdd(&chk->cells, 1u);
        if (w >= m || ref[w] != (uint32_t)c)
            if (atomicAdd(&chk->bad_cell, 1u) == 0)
                printf("hd tally check: dense cell %lu holds item %u\n", (unsigned long)c, w);
    }
}

__global__ void k_tally_check_slots(DevBatch b, const uint32_t* __restrict__ cand, uint32_t m, uint32_t cap,
                                    GTab G, CTab C, const uint32_t* __restrict__ D, const uint32_t* __restrict__ Dd,
                                    const uint32_t* __restrict__ gslot, const uint32_t* __restrict__ ref,
                                    TallyCheck* chk) {
    const uint32_t mask = cap - 1;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += gridDim.x * blockDim.x) {
        if (G.claim[s] != kEmpty) atomicAdd(&chk->sum_g, G.nprev[s] + G.nprec[s]);
        const uint32_t c = C.claim[s];
        if (c != kEmpty) {
            atomicAdd(&chk->sum_c, C.n[s]);
            const uint32_t ic = msg_of(cand, c), g = gslot[c];
            const uint8_t t = b.type[ic];
            const uint8_t* value = b.value32 + 32 * (size_t)ic;
            if (c >= m || g == kEmpty || cell_value(Dd, D, ref[c]) != c)
                if (atomicAdd(&chk->bad_claim, 1u) == 0) printf("hd tally check: C slot %u claimer %u\n", s, c);
            const uint32_t f = find(C.claim, mask, hash_count(value, g, t), [&](uint32_t o) {
                const uint32_t io = msg_of(cand, o);
                return gslot[o] == g && b.type[io] == t && eq32(b.value32 + 32 * (size_t)io, value);
            });
            if (f != s)
                if (atomicAdd(&chk->dup_key, 1u) == 0)
                    printf("hd tally check: C slots %u and %u hold one key (claimers %u, %u)\n", f, s,
                           f == kEmpty ? kEmpty : C.claim[f], c);
        }
        const uint32_t d = D[s];
        if (d != kEmpty) {
            atomicAdd(&chk->d_claims, 1u);
            const uint32_t id = msg_of(cand, d);
            const uint8_t t = b.type[id];
            const int64_t h = b.height[id], r = b.round[id];
            const uint8_t* from = b.from32 + 32 * (size_t)id;
            const uint32_t f = find(D, mask, hash_log(hash_hr(h, r), from, t), [&](uint32_t o) {
                const uint32_t io = msg_of(cand, o);
                return b.type[io] == t && b.height[io] == h && b.round[io] == r &&
                       eq32(b.from32 + 32 * (size_t)io, from);
            });
            if (f != s)
                if (atomicAdd(&chk->dup_key, 1u) == 0) printf("hd tally check: D slots %u and %u hold one key\n", f, s);
        }
    }
}

// ordered compaction of at (n entries) in chunks of HD_CHUNK (a partition's
// candidates, in batch order): per-chunk counts, then each chunk writes from
// the sum of the counts before it (a block reads at most n / HD_CHUNK words)
#define HD_CHUNK 8192
__global__ __launch_bounds__(256) void k_tally_chunk_counts(uint32_t n, const uint32_t* __restrict__ at,
                                                            uint32_t* __restrict__ cnt) {
    typedef hipcub::BlockReduce<uint32_t, 256> Red;
    __shared__ typename Red::TempStorage ts;
    const uint32_t lo = blockIdx.x * HD_CHUNK, hi = min(n, lo + HD_CHUNK);
    uint32_t m = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) m += at[i] != kEmpty ? 1u : 0u;
    const uint32_t t = Red(ts).Sum(m);
    if (threadIdx.x == 0) cnt[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void k_tally_chunk_write(uint32_t n, const uint32_t* __restrict__ at,
                                                           const uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ order,
                                                           uint32_t* __restrict__ rank_of,
                                                           uint32_t* __restrict__ total) {
    typedef hipcub::BlockScan<uint32_t, 256> Scan;
    typedef hipcub::BlockReduce<uint32_t, 256> Red;
    __shared__ typename Scan::TempStorage ts;
    __shared__ typename Red::TempStorage rs;
    __shared__ uint32_t base;
    const uint32_t nch = (n + HD_CHUNK - 1) / HD_CHUNK;
    uint32_t bsum = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256) bsum += cnt[k];
    bsum = Red(rs).Sum(bsum);
    if (threadIdx.x == 0) {
        base = bsum;
        if (blockIdx.x == nch - 1) *total = bsum + cnt[blockIdx.x];
    }
    __syncthreads();
    constexpr uint32_t PER = HD_CHUNK / 256;   // contiguous entries per thread, in order
    const uint32_t lo = blockIdx.x * HD_CHUNK + threadIdx.x * PER;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < PER; k++) mine += (lo + k < n && at[lo + k] != kEmpty) ? 1u : 0u;
    uint32_t off = 0;
    Scan(ts).ExclusiveSum(mine, off);
    uint32_t o = base + off;
    for (uint32_t k = 0; k < PER && mine; k++) {
        const uint32_t i = lo + k;
        if (i < n) {
            const uint32_t v = at[i];
            if (v != kEmpty) {
                order[o] = v;
                if (rank_of) rank_of[v] = o;
                o++;
            }
        }
    }
}

// ---------------------------------------------------------- routing (C4)
// The multi-GPU tally without a replicated batch: each device turns the
// candidates of ITS shard (VALID Prevotes / Precommits) into 64-byte route
// rows, grouped by the rank that owns the candidate's round
// (hd_tally_partition_of) and in index order inside a group; the groups
// cross xGMI (one grouped send/recv or all-to-all); the owner rebuilds a
// batch from the rows it received -- concatenated in source-rank order,
// which is global index order, since shards are contiguous index ranges --
// and tallies it (every row a candidate) with the reps mapped back to global
// indices.  First-wins is per (height, round, type, signer), so the owner of
// a round sees every candidate of its keys, in the order of the whole batch.
struct RouteRow {          // 64 B
    int64_t h, r;
    uint4 value[2];        // the 32 value bytes as stored
    uint32_t gidx;         // global batch index
    uint32_t signer_type;  // admitted (sorted) index << 8 | type
    uint32_t pad[2];
};
static_assert(sizeof(RouteRow) == 64, "route row");
#define HD_ROUTE_MAX_PARTS 64u

// Optional round filter of the route kernels: only candidates whose (h, r)
// is in a sorted list (lexicographic, signed) are routed -- the rounds that
// appear in more than one shard (hd_route_candidates_listed_device); every
// other round is tallied where it is.
struct RoundList {
    const int64_t* h;
    const int64_t* r;
    uint32_t n;
};
__device__ __forceinline__ bool round_listed(const RoundList& l, int64_t h, int64_t r) {
    if (!l.h) return true;
    uint32_t lo = 0, hi = l.n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const int64_t mh = l.h[mid], mr = l.r[mid];
        if (mh < h || (mh == h && mr < r)) lo = mid + 1;
        else hi = mid;
    }
    return lo < l.n && l.h[lo] == h && l.r[lo] == r;
}

// per block and owner: the number of candidates (o-major: cnt[o * nb + blk]);
// *outside counts candidates whose From is not in the context's admitted set
// (possible when the set changed since verification): a row carries the
// admitted index, not the From, so such a candidate cannot be routed
__global__ __launch_bounds__(256) void k_route_count(DevBatch b, const uint32_t* __restrict__ bitmap, uint32_t nparts,
                                                     AdmIndex ix, uint32_t n_adm, uint32_t* __restrict__ cnt,
                                                     uint32_t* __restrict__ outside, RoundList rl) {
    __shared__ uint32_t c[HD_ROUTE_MAX_PARTS];
    if (threadIdx.x < nparts) c[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b.n && candidate(b, nullptr, bitmap, i, Part{0, 1}) && round_listed(rl, b.height[i], b.round[i])) {
        atomicAdd(&c[part_of(hash_hr(b.height[i], b.round[i]), nparts)], 1u);
        uint32_t from_be[8];
        load_row32_be(from_be, b.from32, i);
        const int32_t sg = n_adm ? adm_index_find(ix, from_be) : -1;
        if (sg < 0) atomicAdd(outside, 1u);
    }
    __syncthreads();
    if (threadIdx.x < nparts) cnt[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = c[threadIdx.x];
}

// the rows: block blk's candidates of owner o start at off[o * nb + blk]
// (the exclusive scan of k_route_count's counts), ranked inside the block by
// wavefront ballots, so each owner's rows keep the batch order
__global__ __launch_bounds__(256) void k_route_write(DevBatch b, const uint32_t* __restrict__ bitmap, uint32_t nparts,
                                                     uint32_t base, const uint32_t* __restrict__ off,
                                                     AdmIndex ix, uint32_t n_adm, RouteRow* __restrict__ rows,
                                                     RoundList rl) {
    __shared__ uint32_t wcnt[4][HD_ROUTE_MAX_PARTS];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool c = i < b.n && candidate(b, nullptr, bitmap, i, Part{0, 1}) && round_listed(rl, b.height[i], b.round[i]);
    const uint32_t o = c ? part_of(hash_hr(b.height[i], b.round[i]), nparts) : 0xFFFFFFFFu;
    uint32_t rank = 0;
    for (uint32_t k = 0; k < nparts; k++) {
        const unsigned long long bal = __ballot(o == k);
        if (o == k) rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[w][k] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (!c) return;
    uint32_t pos = off[(size_t)o * gridDim.x + blockIdx.x] + rank;
    for (uint32_t v = 0; v < w; v++) pos += wcnt[v][o];
    uint32_t from_be[8];
    load_row32_be(from_be, b.from32, i);
    const int32_t sg = n_adm ? adm_index_find(ix, from_be) : -1;
    RouteRow row;
    row.h = b.height[i];
    row.r = b.round[i];
    const uint4* vp = reinterpret_cast<const uint4*>(b.value32 + 32 * (size_t)i);
    row.value[0] = vp[0];
    row.value[1] = vp[1];
    row.gidx = base + i;
    // a VALID message's From is admitted (NOT_ADMITTED otherwise); a batch
    // with a candidate outside the current set was refused before this kernel
    row.signer_type = ((uint32_t)(sg >= 0 ? sg : 0xFFFFFF) << 8) | b.type[i];
    row.pad[0] = row.pad[1] = 0;
    rows[pos] = row;
}

// the owners' starts: starts[o] = off[o * nb], starts[nparts] = the total
__global__ void k_route_starts(const uint32_t* __restrict__ off, const uint32_t* __restrict__ cnt, uint32_t nparts,
                               uint32_t nb, uint32_t* __restrict__ starts) {
    const uint32_t o = threadIdx.x;
    if (o < nparts) starts[o] = off[(size_t)o * nb];
    if (o == 0) {
        const size_t last = (size_t)nparts * nb - 1;
        starts[nparts] = off[last] + cnt[last];
    }
}

// received rows -> a batch (From rebuilt from the admitted set) + gidx
__global__ __launch_bounds__(256) void k_unroute(const RouteRow* __restrict__ rows, uint32_t n,
                                                 const uint32_t* __restrict__ adm, uint32_t n_adm, hd_batch_out o,
                                                 uint32_t* __restrict__ gidx) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const RouteRow row = rows[j];
    const uint32_t sg = row.signer_type >> 8;
    o.type[j] = (uint8_t)(row.signer_type & 0xFFu);
    ((int64_t*)o.height)[j] = row.h;
    ((int64_t*)o.round)[j] = row.r;
    if (o.valid_round) ((int64_t*)o.valid_round)[j] = -1;
    uint4* vp = reinterpret_cast<uint4*>(o.value32 + 32 * (size_t)j);
    vp[0] = row.value[0];
    vp[1] = row.value[1];
    uint32_t f[8];
    HD_UNROLL for (int k = 0; k < 8; k++) f[k] = sg < n_adm ? adm[8 * (size_t)sg + k] : 0xFFFFFFFFu;
    store_row32_be(o.from32, j, f);
    gidx[j] = row.gidx;
}

// ---------------------------------------------------------------- host side
#define TCHK(expr, what)                                         \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return hd_ctx_fail(ctx, _e, what); \
    } while (0)

static void* tbuf(hd_ctx* ctx, int slot, size_t bytes, int* rc) {
    DevBuf& b = ctx->tally->b[slot];
    int r = hd_dev_grow(ctx, &b.p, &b.cap, bytes);
    if (r) {
        *rc = r;
        return nullptr;
    }
    return b.p;
}

void hd_tally_release(hd_ctx* ctx) {
    if (!ctx || !ctx->tally) return;
    for (auto& b : ctx->tally->b)
        if (b.p) (void)hipFree(b.p);
    if (ctx->tally->host) (void)hipHostFree(ctx->tally->host);
    if (ctx->tally->scalar) (void)hipHostFree(ctx->tally->scalar);
    delete ctx->tally;
    ctx->tally = nullptr;
}

static inline uint32_t nblk(uint32_t n) { return (n + 255) / 256; }
// items per block of the order passes: the largest power of two in 256 ..
// HD_TALLY_IPB_MAX that leaves about four blocks per CU (a 128k-message batch
// at 2048 ran 63 blocks, latency-bound on a quarter of the chip)
static inline uint32_t tally_ipb(uint32_t m, uint32_t n_cu) {
    uint32_t ipb = HD_TALLY_IPB_MAX;
    while (ipb > 256u && (m + ipb - 1) / ipb < 4u * n_cu) ipb >>= 1;
    return ipb;
}

// dense log cells allowed (words): rounds numbered past nd = this / 2S take
// the hashed table (e.g. a batch of a million single-message rounds)
#define HD_TALLY_DENSE_MAX (64ull << 20)

// dup_global[gidx[j]] = dup[j] (a routed batch's classification at its
// global indices, in the owner's device memory: hd_multi)
__global__ __launch_bounds__(256) void k_dup_scatter(uint32_t n, const uint8_t* __restrict__ dup,
                                                     const uint32_t* __restrict__ gidx, uint8_t* __restrict__ dup_global) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) dup_global[gidx[j]] = dup[j];
}

// the stage layout: [n_hr, n_cnt | classification (n bytes, when staged) |
// per-round rows (kRoundCols, capacity h) | per-value rows (kValueCols, capacity c)]
static size_t tally_rows_off(uint32_t n, bool dup) { return 64 + pad64(dup ? n : 0); }
static size_t tally_stage_bytes(uint32_t n, bool dup, uint32_t h, uint32_t c) {
    return tally_rows_off(n, dup) + kRoundRow * h + kValueRow * c + 64;
}

// A call's one download: `bytes` of the device stage into the context's pinned stage (grown with a quarter
// to spare), and the synchronisation.  Returns the host copy, or NULL with the error in *rc.
static const char* tally_download(hd_ctx* ctx, const void* d_stage, size_t bytes, hipStream_t s, int* rc) {
    TallyWork* tw = ctx->tally;
    hipError_t e = hipSuccess;
    if (tw->host_cap < bytes) {
        if (tw->host) (void)hipHostFree(tw->host);
        tw->host = nullptr;
        tw->host_cap = 0;
        e = hipHostMalloc(&tw->host, bytes + (bytes >> 2), hipHostMallocDefault);
        if (e == hipSuccess) tw->host_cap = bytes + (bytes >> 2);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(tw->host, d_stage, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) return (const char*)tw->host;
    *rc = hd_ctx_fail(ctx, e, "tally stage download");
    return nullptr;
}

// the order passes' run-time items per block as a compile-time one: f(std::integral_constant<uint32_t, IPB>)
template <typename F>
static void with_ipb(uint32_t ipb, F f) {
    switch (ipb) {
        case 256u: f(std::integral_constant<uint32_t, 256u>{}); break;
        case 512u: f(std::integral_constant<uint32_t, 512u>{}); break;
        case 1024u: f(std::integral_constant<uint32_t, 1024u>{}); break;
        case 2048u: f(std::integral_constant<uint32_t, 2048u>{}); break;
    }
}

// The tables and per-item scratch of one call over m items.  The tally, the decide and (through
// hd_decide_run) the retained log run on the context's one set of buffers and hand each other clean
// tables, so the sizes, the slicing and the clear are decided here and nowhere else.
struct TallyPlan {
    uint32_t grid;        // blocks of the probe passes
    uint32_t cap, mask;   // slots of each hash table (a power of two), cap - 1
    uint32_t ipb, nbo;    // items per block and blocks of the order passes
    uint32_t* tabs;       // the table allocation (the clean check reads it whole)
    GTab G;
    CTab C;
    uint32_t* d;          // the hashed log table D
    TallyCtr* ctr;        // the call counters, after the tables
    uint32_t *gslot, *ref, *cslot;             // per item: round slot, log reference, count slot
    uint32_t *Bg, *Bc, *pre_g, *pre_c, *blk;   // first-item bitmaps, their prefixes, block totals
    uint32_t S, nd;       // admitted signatories; rounds with dense log cells
    uint32_t* Dd;         // the dense cells (nd x 2 x S words), NULL without admitted signatories
    uint32_t *P, *pslot;  // hd_decide: the propose claim table and the per-item propose slot
};

// Sizes and allocates the plan and queues the clear the tables need.  The kernels leave them clean
// (k_tally_emit, k_decide_clean), so that is on first use, at a new allocation or capacity, or after a call
// that did not queue all its launches: the tables count as dirty from here until tally_plan_done.
// `propose` adds hd_decide's table P, with a clear state of its own.
static int tally_plan(hd_ctx* ctx, uint32_t m, bool propose, hipStream_t s, TallyPlan& p) {
    TallyWork* tw = ctx->tally;
    // blocks per CU of the probe passes (HD_TALLY_BPC, default 16)
    static const uint32_t bpc = getenv("HD_TALLY_BPC") ? (uint32_t)std::max(1, atoi(getenv("HD_TALLY_BPC"))) : 16u;
    p = TallyPlan{};
    p.grid = std::min<uint32_t>(nblk(m), (uint32_t)ctx->n_cu * bpc);
    // the tables hold at most one key per item, load factor <= 1/2 so probes terminate
    p.cap = 1024;
    while (p.cap < 2 * m) p.cap <<= 1;
    p.mask = p.cap - 1;
    p.ipb = tally_ipb(m, (uint32_t)ctx->n_cu);
    p.nbo = (m + p.ipb - 1) / p.ipb;
    const size_t nw = (size_t)p.nbo * (p.ipb / 32), K = p.cap;
    int rc = 0;
    // one allocation for the tables, K words each: the claim words (G, C, D:
    // empty), the counters (G x 3, C: zero), the round numbers (gid); then the
    // call counters (TallyCtr)
    char* tb = (char*)tbuf(ctx, T_G, 4 * 8 * K + sizeof(TallyCtr), &rc);
    p.gslot = (uint32_t*)tbuf(ctx, T_GSLOT, 4 * (size_t)m, &rc);
    p.ref = (uint32_t*)tbuf(ctx, T_DSLOT, 4 * (size_t)m, &rc);
    p.cslot = (uint32_t*)tbuf(ctx, T_CSLOT, 4 * (size_t)m, &rc);
    // Bg | Bc | pre_g | pre_c (nw words each) | block totals (2 nbo)
    uint32_t* bits = (uint32_t*)tbuf(ctx, T_BITS, 4 * (4 * nw + 2 * (size_t)p.nbo), &rc);
    if (propose) {
        p.P = (uint32_t*)tbuf(ctx, T_P, 4 * K, &rc);
        p.pslot = (uint32_t*)tbuf(ctx, T_PSLOT, 4 * (size_t)m, &rc);
    }
    // dense log cells (nd rounds x 2 x S) for admitted signatories, the hashed
    // D table for the rest: room for every item's round up to HD_TALLY_DENSE_MAX words
    p.S = ctx->n_adm;
    const size_t dcap = p.S > 0 ? std::min<size_t>(HD_TALLY_DENSE_MAX, (size_t)m * 2 * p.S) : 0;
    p.nd = p.S > 0 ? (uint32_t)(dcap / (2 * (size_t)p.S)) : 0u;
    p.Dd = dcap ? (uint32_t*)tbuf(ctx, T_C, 4 * dcap, &rc) : nullptr;
    if (rc) return rc;
    uint32_t* tabs = p.tabs = (uint32_t*)tb;
    p.G = GTab{tabs, tabs + 3 * K, tabs + 4 * K, tabs + 5 * K, tabs + 7 * K};
    p.C = CTab{tabs + K, tabs + 6 * K};
    p.d = tabs + 2 * K;
    p.ctr = reinterpret_cast<TallyCtr*>(tb + 4 * 8 * K);
    p.Bg = bits, p.Bc = bits + nw, p.pre_g = bits + 2 * nw, p.pre_c = bits + 3 * nw, p.blk = bits + 4 * nw;
    auto stale = [&](const TallyWork::Clean& c, const void* at) { return c.dirty || c.p != at || c.k != p.cap; };
    if (stale(tw->tab, tb)) {
        TCHK(hipMemsetAsync(tabs, 0xFF, 4 * 3 * K, s), "clear claims");
        TCHK(hipMemsetAsync(tabs + 3 * K, 0, 4 * 4 * K, s), "clear counters");
        TCHK(hipMemsetAsync(p.ctr, 0, sizeof(TallyCtr), s), "clear call counters");
    }
    if (propose && stale(tw->ptab, p.P)) TCHK(hipMemsetAsync(p.P, 0xFF, 4 * K, s), "clear propose claims");
    tw->tab = {true, tb, p.cap};
    if (propose) tw->ptab = {true, p.P, p.cap};
    return HD_OK;
}
// every launch of the plan's call is queued: its kernels leave the tables clean
static void tally_plan_done(hd_ctx* ctx, const TallyPlan& p) {
    ctx->tally->tab.dirty = false;
    if (p.P) ctx->tally->ptab.dirty = false;
}

// HD_TALLY_CHECK: the invariants of the tables just built (k_tally_check_*),
// read back at once (a synchronisation: debug only)
static int tally_check(hd_ctx* ctx, const DevBatch& b, const uint32_t* cand, uint32_t m, const TallyPlan& p,
                       hipStream_t s) {
    int rc = 0;
    TallyCheck* chk = (TallyCheck*)tbuf(ctx, T_CHECK, sizeof(TallyCheck), &rc);
    if (rc) return rc;
    TCHK(hipMemsetAsync(chk, 0, sizeof(TallyCheck), s), "tally check clear");
    const uint32_t grid = std::min<uint32_t>(nblk(std::max(m, p.cap)), (uint32_t)ctx->n_cu * 8u);
    k_tally_check_items<<<grid, 256, 0, s>>>(m, p.gslot, p.ref, p.Dd, p.d, chk);
    k_tally_check_cells<<<grid, 256, 0, s>>>(p.Dd, p.ctr, 2 * p.S, p.nd, m, p.ref, chk);
    k_tally_check_slots<<<grid, 256, 0, s>>>(b, cand, m, p.cap, p.G, p.C, p.d, p.Dd, p.gslot, p.ref, chk);
    TCHK(hipGetLastError(), "tally check kernels");
    TallyCheck h{};
    TCHK(hipMemcpyAsync(&h, chk, sizeof h, hipMemcpyDeviceToHost, s), "tally check download");
    TCHK(hipStreamSynchronize(s), "tally check sync");
    const bool ok = h.stale == 0 && h.bad_cell == 0 && h.dup_key == 0 && h.bad_claim == 0 && h.winners == h.sum_g &&
                    h.winners == h.sum_c && h.winners == h.cells + h.d_claims;
    if (ok) return HD_OK;
    char buf[320];
    snprintf(buf, sizeof buf,
             "tally check failed: winners %u, sum G %u, sum C %u, dense cells %u + D claims %u, stale %u, "
             "bad cells %u, duplicate keys %u, bad C claimers %u (m %u, cap %u)",
             h.winners, h.sum_g, h.sum_c, h.cells, h.d_claims, h.stale, h.bad_cell, h.dup_key, h.bad_claim, m, p.cap);
    ctx->last_error = buf;
    return HD_EDEVICE;
}

// HD_TALLY_CHECK after the emit: every table slot and the counters are clean
static int tally_check_clean(hd_ctx* ctx, const TallyPlan& p, hipStream_t s) {
    int rc = 0;
    uint32_t* bad = (uint32_t*)tbuf(ctx, T_CHECK, sizeof(TallyCheck), &rc);
    if (rc) return rc;
    TCHK(hipMemsetAsync(bad, 0, 4, s), "tally clean check clear");
    k_tally_check_clean<<<std::min<uint32_t>(nblk(p.cap), (uint32_t)ctx->n_cu * 8u), 256, 0, s>>>(p.cap, p.tabs, p.ctr,
                                                                                                  bad);
    uint32_t h = 0;
    TCHK(hipMemcpyAsync(&h, bad, 4, hipMemcpyDeviceToHost, s), "tally clean check download");
    TCHK(hipStreamSynchronize(s), "tally clean check sync");
    if (h == 0) return HD_OK;
    ctx->last_error = "tally check failed: " + std::to_string(h) + " table slots not clean after the emit";
    return HD_EDEVICE;
}

// the device address of an async stage's completion word (word 2), or NULL
// when the stage is not mapped pinned memory (collect then waits on the event)
static uint32_t* ticket_signal(void* stage) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, stage, 0) != hipSuccess || !dp) {
        (void)hipGetLastError();
        return nullptr;
    }
    return reinterpret_cast<uint32_t*>(dp) + 2;
}

// gidx (optional): the batch's messages' global indices -- the rep outputs
// are mapped through it (a routed batch, hd_tally_routed_device); with
// dup_global the per-message classification is scattered there through gidx
// on the device instead of being downloaded (out->dup unused).  With `tk`
// (hd_tally_device_bitmap_async) nothing is waited for: the stage goes to the
// ticket's pinned buffer and hd_tally_collect unpacks it later.
//
// Launches per call: k_tally_rounds, k_tally_logs, k_tally_values,
// k_tally_firsts, k_tally_emit and one download (a partition adds its
// candidate compaction and one host read; a routed owner's scatter one
// kernel).  The hash tables and counters clean themselves (k_tally_emit), the
// dense cells are cleared by the round that takes them (k_tally_rounds), and
// the bitmaps are written whole: nothing is cleared per call unless
// tally_plan finds the tables new, resized or left by an unfinished call.
static int tally_device(hd_ctx* ctx, const hd_batch* hb, const uint8_t* d_verdict, const uint32_t* d_bitmap,
                        Part part, hd_tally_out* out, hipStream_t s, const uint32_t* gidx = nullptr,
                        uint8_t* dup_global = nullptr, hd_tally_ticket* tk = nullptr) {
    const uint32_t n = hb->n;
    if (!ctx->tally) ctx->tally = new TallyWork();
    DevBatch b{n, hb->type, hb->height, hb->round, hb->valid_round, hb->value32, hb->from32, hb->sig65};
    int rc = 0;
    const bool check = [] {
        const char* e = getenv("HD_TALLY_CHECK");
        return e && atoi(e) != 0;
    }();
    // The output stage (tally_stage_bytes) is downloaded with ONE copy after
    // ONE host sync.  Its row capacities H and Cg are the previous call's
    // counts plus a margin; rows past them land in overflow columns on the
    // device, downloaded by a second round of copies when needed.
    TallyWork* tw = ctx->tally;
    // the classification is staged for download only when the caller reads it
    // (out->dup, or the ticket's dup); a routed owner's scatter (dup_global)
    // keeps it in device scratch of its own
    const bool stage_dup = tk ? tk->dup != 0 : out->dup != nullptr;
    const uint32_t H = tw->guess_hr, Cg = tw->guess_cnt;
    const size_t dup_off = 64, rows_off = tally_rows_off(n, stage_dup), total = tally_stage_bytes(n, stage_dup, H, Cg);
    if (tk) {
        if (part.nparts != 1 || gidx || dup_global) return HD_EINVAL;
        tk->n = n;
        tk->H = H;
        tk->Cg = Cg;
        tk->need = total;
        if (!tk->stage || tk->stage_cap < tk->need) return HD_ECAP;
    }
    char* st = (char*)tbuf(ctx, T_SEL, total, &rc);
    uint8_t* d_dup = stage_dup ? (uint8_t*)(st + dup_off) : nullptr;
    if (!stage_dup && dup_global) d_dup = (uint8_t*)tbuf(ctx, T_DUP, n, &rc);
    if (rc) return rc;
    // Items: the whole batch, or a partition's candidates compacted in batch
    // order (the rest of the tally then scales with the partition, not with
    // the replicated batch).
    uint32_t m = n;
    const uint32_t* cand = nullptr;
    if (part.nparts > 1) {
        uint32_t* at = (uint32_t*)tbuf(ctx, T_SORTK, 4 * (size_t)n, &rc);
        uint32_t* ccnt = (uint32_t*)tbuf(ctx, T_TMP, 4 * ((size_t)(n + HD_CHUNK - 1) / HD_CHUNK + 2), &rc);
        uint32_t* cl = (uint32_t*)tbuf(ctx, T_D, 4 * (size_t)n, &rc);
        if (rc) return rc;
        const uint32_t nch = (n + HD_CHUNK - 1) / HD_CHUNK;
        k_tally_flag<<<std::min<uint32_t>(nblk(n), (uint32_t)ctx->n_cu * 8u), 256, 0, s>>>(b, d_verdict, d_bitmap, part,
                                                                                            at, d_dup);
        k_tally_chunk_counts<<<nch, 256, 0, s>>>(n, at, ccnt);
        k_tally_chunk_write<<<nch, 256, 0, s>>>(n, at, ccnt, cl, nullptr, ccnt + nch);
        TCHK(hipGetLastError(), "tally candidate kernels");
        if (!tw->scalar) TCHK(hipHostMalloc((void**)&tw->scalar, 64, hipHostMallocDefault), "tally scalar");
        TCHK(hipMemcpyAsync(tw->scalar, ccnt + nch, 4, hipMemcpyDeviceToHost, s), "candidate count");
        TCHK(hipStreamSynchronize(s), "candidate count sync");
        m = tw->scalar[0];
        cand = cl;
    }
    if (m == 0) {   // nothing to tally here (dup: every message 3)
        out->n_hr = out->n_counts = 0;
        if (out->dup) memset(out->dup, 3, n);
        return HD_OK;
    }
    TallyPlan p;
    if ((rc = tally_plan(ctx, m, false, s, p))) return rc;
    k_tally_rounds<<<p.grid, 256, 0, s>>>(b, cand, m, d_verdict, d_bitmap, part, p.G, p.mask, p.gslot, d_dup, p.ctr,
                                          p.Dd, 2 * p.S, p.nd);
    k_tally_logs<<<p.grid, 256, 0, s>>>(b, cand, m, p.gslot, p.G.gid, hd_adm_index(ctx), p.S, p.Dd, p.nd, p.d, p.mask,
                                        p.ref);
    k_tally_values<<<p.grid, 256, 0, s>>>(b, cand, m, p.Dd, p.S, p.d, p.G, p.C, p.mask, p.gslot, p.ref, p.cslot, d_dup);
    if (dup_global && gidx) k_dup_scatter<<<nblk(n), 256, 0, s>>>(n, d_dup, gidx, dup_global);
    TCHK(hipGetLastError(), "tally kernels");
    if (check && (rc = tally_check(ctx, b, cand, m, p, s))) return rc;
    // rows at capacity (H, Cg) in the stage, the rest in the overflow columns
    // (capacity m each: a batch has at most m groups of either kind)
    char* ovf = (char*)tbuf(ctx, T_NSEL, (kRoundRow + kValueRow) * m + 64, &rc);
    if (rc) return rc;
    const TallyCols sc = tally_cols(st + rows_off, H, Cg), oc = tally_cols(ovf, m, m);
    with_ipb(p.ipb, [&](auto ipb) {
        constexpr uint32_t IPB = decltype(ipb)::value;
        k_tally_firsts<IPB><<<p.nbo, 256, 0, s>>>(m, p.gslot, p.cslot, p.G.claim, p.C.claim, p.Bg, p.Bc, p.pre_g,
                                                  p.pre_c, p.blk);
        k_tally_emit<IPB><<<p.nbo, 256, 0, s>>>(b, cand, m, gidx, p.gslot, p.cslot, p.ref, p.G, p.C, p.d, p.Bg, p.Bc,
                                                p.pre_g, p.pre_c, p.blk, sc, H, Cg, oc, p.ctr, (uint32_t*)st);
    });
    TCHK(hipGetLastError(), "tally order kernels");
    tally_plan_done(ctx, p);
    if (check && (rc = tally_check_clean(ctx, p, s))) return rc;
    if (tk) {   // queued; hd_tally_collect waits for the signal (or tk->done), then reads the stage
        // the completion word restarts at 0 (the stage's previous ticket was collected)
        reinterpret_cast<volatile uint32_t*>(tk->stage)[2] = 0u;
        TCHK(hipMemcpyAsync(tk->stage, st, total, hipMemcpyDeviceToHost, s), "tally download");
        if (uint32_t* sig = ticket_signal(tk->stage)) k_tally_signal<<<1, 64, 0, s>>>(sig);
        if (!tk->done) TCHK(hipEventCreateWithFlags((hipEvent_t*)&tk->done, hipEventDisableTiming), "tally event");
        TCHK(hipEventRecord((hipEvent_t)tk->done, s), "tally event record");
        return hd_ctx_note_stream(ctx, s);
    }
    const char* hs = tally_download(ctx, st, total, s, &rc);
    if (!hs) return rc;
    const uint32_t n_hr = reinterpret_cast<const uint32_t*>(hs)[0];
    const uint32_t n_cnt = reinterpret_cast<const uint32_t*>(hs)[1];
    out->n_hr = n_hr;
    out->n_counts = n_cnt;
    tw->guess_hr = std::max<uint32_t>(1024u, n_hr + n_hr / 4);
    tw->guess_cnt = std::max<uint32_t>(1024u, n_cnt + n_cnt / 4);
    if (n_hr > out->cap_hr || n_cnt > out->cap_counts) return HD_ECAP;
    if (out->dup) memcpy(out->dup, hs + dup_off, (size_t)n);
    (void)tally_rows_copy(ctx, hs + rows_off, H, Cg, std::min(n_hr, H), std::min(n_cnt, Cg), 0, 0, out, copy_host);
    if (n_hr > H || n_cnt > Cg) {   // more groups than staged: the overflow columns, straight into out
        const uint32_t eh = n_hr > H ? n_hr - H : 0, ec = n_cnt > Cg ? n_cnt - Cg : 0;
        if ((rc = tally_rows_copy(ctx, ovf, m, m, eh, ec, H, Cg, out, copy_down(s)))) return rc;
        TCHK(hipStreamSynchronize(s), "tally overflow sync");
    }
    return HD_OK;
}

// hd_tally_routed_device with the classification scattered, on the device,
// to dup_global[global index] (n_global bytes the caller set to 3) instead of
// being downloaded (hd_multi.hip)
int hd_tally_routed_dup_device(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_gidx, hd_tally_out* out,
                               uint8_t* dup_global, hipStream_t s) {
    out->n_counts = out->n_hr = 0;
    if (dbatch->n == 0) return HD_OK;
    uint8_t* keep = out->dup;
    out->dup = nullptr;
    const int rc = tally_device(ctx, dbatch, nullptr, nullptr, Part{0, 1}, out, s, d_gidx, dup_global);
    out->dup = keep;
    return rc;
}

static bool tally_out_ok(const hd_tally_out* o) {
    return o && o->count_height && o->count_round && o->count_type && o->count_rep && o->count_n && o->hr_height &&
           o->hr_round && o->hr_prevotes && o->hr_precommits && o->hr_any;
}

extern "C" {

int hd_tally(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, hd_tally_out* out) {
    if (!ctx || !batch || !verdict || !tally_out_ok(out)) return HD_EINVAL;
    if (!batch->type || !batch->height || !batch->round || !batch->value32 || !batch->from32) return HD_EINVAL;
    out->n_counts = out->n_hr = 0;
    if (batch->n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    hd_batch hb = *batch;
    hb.sig65 = nullptr;  // not needed
    hb.valid_round = nullptr;
    hd_batch db;
    int rc = hd_upload_batch(ctx, &hb, &db);
    if (rc) return rc;
    rc = hd_dev_grow(ctx, &ctx->bufs[BUF_VERDICT].p, &ctx->bufs[BUF_VERDICT].cap, batch->n);
    if (rc) return rc;
    uint8_t* d_v = (uint8_t*)ctx->bufs[BUF_VERDICT].p;
    TCHK(hipMemcpyAsync(d_v, verdict, batch->n, hipMemcpyHostToDevice, ctx->stream), "verdict upload");
    return tally_device(ctx, &db, d_v, nullptr, Part{0, 1}, out, ctx->stream);
}

int hd_tally_device(hd_ctx* ctx, const hd_batch* dbatch, const uint8_t* d_verdict, hd_tally_out* out, void* stream) {
    if (!ctx || !dbatch || !tally_out_ok(out)) return HD_EINVAL;
    if (dbatch->n && !d_verdict) return HD_EINVAL;
    out->n_counts = out->n_hr = 0;
    if (dbatch->n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    return tally_device(ctx, dbatch, d_verdict, nullptr, Part{0, 1}, out, stream ? (hipStream_t)stream : ctx->stream);
}

int hd_tally_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap, hd_tally_out* out,
                           void* stream) {
    return hd_tally_device_bitmap_part(ctx, dbatch, d_valid_bitmap, 0, 1, out, stream);
}

int hd_tally_device_bitmap_async(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                 hd_tally_ticket* ticket, void* stream) {
    if (!ctx || !dbatch || !ticket) return HD_EINVAL;
    if (dbatch->n && !d_valid_bitmap) return HD_EINVAL;
    ticket->n = dbatch->n;
    ticket->H = ticket->Cg = 0;
    ticket->need = 0;
    if (dbatch->n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    hd_tally_out dummy{};
    return tally_device(ctx, dbatch, nullptr, d_valid_bitmap, Part{0, 1}, &dummy,
                        stream ? (hipStream_t)stream : ctx->stream, nullptr, nullptr, ticket);
}

int hd_tally_ticket_release(hd_tally_ticket* ticket) {
    if (!ticket) return HD_EINVAL;
    if (ticket->done) (void)hipEventDestroy((hipEvent_t)ticket->done);
    ticket->done = nullptr;
    return HD_OK;
}

size_t hd_tally_stage_bytes(hd_ctx* ctx, uint32_t n, int dup) {
    if (!ctx) return 0;
    const uint32_t h = ctx->tally ? ctx->tally->guess_hr.load() : 1024u, c = ctx->tally ? ctx->tally->guess_cnt.load() : 1024u;
    return tally_stage_bytes(n, dup != 0, h, c);
}

int hd_tally_collect(hd_ctx* ctx, const hd_tally_ticket* ticket, hd_tally_out* out) {
    if (!ctx || !ticket || !tally_out_ok(out)) return HD_EINVAL;
    out->n_counts = out->n_hr = 0;
    if (ticket->n == 0) return HD_OK;
    if (!ticket->stage || ticket->need == 0 || !ticket->done) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ticket_signal(ticket->stage)) {
        // poll the completion word without a HIP call per iteration; past
        // ~0.2 s, wait for the event (a fault surfaces there) and read it once more
        volatile const uint32_t* w = reinterpret_cast<volatile const uint32_t*>(ticket->stage) + 2;
        const auto t0 = std::chrono::steady_clock::now();
        while (*w != 1u) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
                TCHK(hipEventSynchronize((hipEvent_t)ticket->done), "tally collect wait");
                if (*w != 1u) return hd_ctx_fail(ctx, hipErrorUnknown, "tally collect signal");
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        TCHK(hipEventSynchronize((hipEvent_t)ticket->done), "tally collect wait");
    }
    const char* st = (const char*)ticket->stage;
    const uint32_t n_hr = reinterpret_cast<const uint32_t*>(st)[0];
    const uint32_t n_cnt = reinterpret_cast<const uint32_t*>(st)[1];
    out->n_hr = n_hr;
    out->n_counts = n_cnt;
    if (!ctx->tally) ctx->tally = new TallyWork();
    TallyWork* tw = ctx->tally;
    tw->guess_hr = std::max<uint32_t>(tw->guess_hr.load(), std::max<uint32_t>(1024u, n_hr + n_hr / 4));
    tw->guess_cnt = std::max<uint32_t>(tw->guess_cnt.load(), std::max<uint32_t>(1024u, n_cnt + n_cnt / 4));
    if (n_hr > out->cap_hr || n_cnt > out->cap_counts) return HD_ECAP;
    if (n_hr > ticket->H || n_cnt > ticket->Cg) return HD_EAGAIN;   // more groups than staged
    if (out->dup) {
        if (!ticket->dup) return HD_EINVAL;
        memcpy(out->dup, st + 64, (size_t)ticket->n);
    }
    return tally_rows_copy(ctx, st + tally_rows_off(ticket->n, ticket->dup != 0), ticket->H, ticket->Cg, n_hr, n_cnt, 0, 0,
                           out, copy_host);
}

int hd_tally_device_bitmap_part(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap, uint32_t part,
                                uint32_t nparts, hd_tally_out* out, void* stream) {
    if (!ctx || !dbatch || !tally_out_ok(out) || nparts == 0 || part >= nparts) return HD_EINVAL;
    if (dbatch->n && !d_valid_bitmap) return HD_EINVAL;
    out->n_counts = out->n_hr = 0;
    if (dbatch->n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    return tally_device(ctx, dbatch, nullptr, d_valid_bitmap, Part{part, nparts}, out,
                        stream ? (hipStream_t)stream : ctx->stream);
}

uint32_t hd_tally_partition_of(int64_t height, int64_t round, uint32_t nparts) {
    return part_of(hash_hr(height, round), nparts);
}

static int route_candidates(hd_ctx* ctx, const hd_batch* dshard, const uint32_t* d_valid_bitmap,
                            uint32_t base_index, uint32_t nparts, RoundList rl, uint8_t* d_rows, uint32_t cap_rows,
                            uint32_t* counts, void* stream);

int hd_route_candidates_device(hd_ctx* ctx, const hd_batch* dshard, const uint32_t* d_valid_bitmap,
                               uint32_t base_index, uint32_t nparts, uint8_t* d_rows, uint32_t cap_rows,
                               uint32_t* counts, void* stream) {
    return route_candidates(ctx, dshard, d_valid_bitmap, base_index, nparts, RoundList{nullptr, nullptr, 0}, d_rows,
                            cap_rows, counts, stream);
}

int hd_route_candidates_listed_device(hd_ctx* ctx, const hd_batch* dshard, const uint32_t* d_valid_bitmap,
                                      uint32_t base_index, uint32_t nparts, const int64_t* d_round_h,
                                      const int64_t* d_round_r, uint32_t n_rounds, uint8_t* d_rows,
                                      uint32_t cap_rows, uint32_t* counts, void* stream) {
    if (!ctx || !counts || nparts == 0 || nparts > HD_ROUTE_MAX_PARTS) return HD_EINVAL;
    if (n_rounds == 0) {   // nothing is shared: nothing to route
        for (uint32_t o = 0; o < nparts; o++) counts[o] = 0;
        return HD_OK;
    }
    if (!d_round_h || !d_round_r) return HD_EINVAL;
    return route_candidates(ctx, dshard, d_valid_bitmap, base_index, nparts, RoundList{d_round_h, d_round_r, n_rounds},
                            d_rows, cap_rows, counts, stream);
}

}  // extern "C"

static int route_candidates(hd_ctx* ctx, const hd_batch* dshard, const uint32_t* d_valid_bitmap,
                            uint32_t base_index, uint32_t nparts, RoundList rl, uint8_t* d_rows, uint32_t cap_rows,
                            uint32_t* counts, void* stream) {
    if (!ctx || !dshard || !counts || nparts == 0 || nparts > HD_ROUTE_MAX_PARTS) return HD_EINVAL;
    for (uint32_t o = 0; o < nparts; o++) counts[o] = 0;
    const uint32_t n = dshard->n;
    if (n == 0) return HD_OK;
    if (!d_valid_bitmap || !d_rows || !dshard->type || !dshard->height || !dshard->round || !dshard->value32 ||
        !dshard->from32 || ((uintptr_t)d_rows & 15) || ((uintptr_t)dshard->value32 & 15))
        return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (!ctx->tally) ctx->tally = new TallyWork();
    DevBatch b{n, dshard->type, dshard->height, dshard->round, nullptr, dshard->value32, dshard->from32, nullptr};
    const uint32_t nb = nblk(n);
    const size_t cells = (size_t)nparts * nb;
    int rc = 0;
    // starts[0 .. nparts] and, after them, the count of candidates outside the set
    uint32_t* cnt = (uint32_t*)tbuf(ctx, T_ROUTE, 4 * (2 * cells + nparts + 2) + 4096, &rc);
    if (rc) return rc;
    uint32_t* off = cnt + cells;
    uint32_t* starts = off + cells;
    void* tmp = (void*)(starts + nparts + 2);
    size_t tmp_bytes = 0;
    TCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt, off, (int)cells, s), "route scan size");
    // the scan's temporary storage after the counts (grown with them)
    cnt = (uint32_t*)tbuf(ctx, T_ROUTE, 4 * (2 * cells + nparts + 2) + 64 + tmp_bytes, &rc);
    if (rc) return rc;
    off = cnt + cells;
    starts = off + cells;
    tmp = (void*)(((uintptr_t)(starts + nparts + 2) + 63) & ~(uintptr_t)63);
    TCHK(hipMemsetAsync(starts + nparts + 1, 0, 4, s), "route outside count");
    k_route_count<<<nb, 256, 0, s>>>(b, d_valid_bitmap, nparts, hd_adm_index(ctx), ctx->n_adm, cnt,
                                     starts + nparts + 1, rl);
    TCHK(hipGetLastError(), "k_route_count");
    TCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, cnt, off, (int)cells, s), "route scan");
    k_route_starts<<<1, 64, 0, s>>>(off, cnt, nparts, nb, starts);
    std::vector<uint32_t> st(nparts + 2);
    TCHK(hipMemcpyAsync(st.data(), starts, 4 * (nparts + 2), hipMemcpyDeviceToHost, s), "route counts");
    TCHK(hipStreamSynchronize(s), "route counts");
    if (st[nparts + 1]) {
        // a VALID candidate whose From left the set since verification: its
        // row could not name it (the tally keys on the From), so refuse
        ctx->last_error = "hd_route_candidates_device: " + std::to_string(st[nparts + 1]) +
                          " candidates whose From is not in the current admitted set";
        return HD_EINVAL;
    }
    for (uint32_t o = 0; o < nparts; o++) counts[o] = st[o + 1] - st[o];
    if (st[nparts] > cap_rows) return HD_ECAP;
    k_route_write<<<nb, 256, 0, s>>>(b, d_valid_bitmap, nparts, base_index, off, hd_adm_index(ctx), ctx->n_adm,
                                     reinterpret_cast<RouteRow*>(d_rows), rl);
    TCHK(hipGetLastError(), "k_route_write");
    return hd_ctx_note_stream(ctx, s);
}

extern "C" {

int hd_unroute_device(hd_ctx* ctx, const uint8_t* d_rows, uint32_t n, const hd_batch_out* d_out, uint32_t* d_gidx,
                      void* stream) {
    if (!ctx || !d_out) return HD_EINVAL;
    if (n == 0) return HD_OK;
    if (!d_rows || !d_gidx || !d_out->type || !d_out->height || !d_out->round || !d_out->value32 || !d_out->from32 ||
        ((uintptr_t)d_rows & 15) || ((uintptr_t)d_out->value32 & 15) || ((uintptr_t)d_out->from32 & 15))
        return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    k_unroute<<<nblk(n), 256, 0, s>>>(reinterpret_cast<const RouteRow*>(d_rows), n, ctx->d_adm, ctx->n_adm, *d_out,
                                      d_gidx);
    TCHK(hipGetLastError(), "k_unroute");
    return hd_ctx_note_stream(ctx, s);
}

int hd_tally_routed_device(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_gidx, hd_tally_out* out,
                           void* stream) {
    if (!ctx || !dbatch || !tally_out_ok(out)) return HD_EINVAL;
    out->n_counts = out->n_hr = 0;
    if (dbatch->n == 0) return HD_OK;
    if (!d_gidx) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    return tally_device(ctx, dbatch, nullptr, nullptr, Part{0, 1}, out, stream ? (hipStream_t)stream : ctx->stream,
                        d_gidx);
}

int hd_process_batch(hd_ctx* ctx, const hd_batch* batch, uint8_t* verdict, uint8_t* recovered32,
                     uint32_t* valid_bitmap, hd_tally_out* tally) {
    if (!ctx || !batch || !verdict || !tally_out_ok(tally)) return HD_EINVAL;
    tally->n_counts = tally->n_hr = 0;
    if (batch->n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    hd_batch db;
    int rc = hd_upload_batch(ctx, batch, &db);
    if (rc) return rc;
    rc = hd_verify_uploaded(ctx, &db, verdict, recovered32, valid_bitmap);
    if (rc) return rc;
    return tally_device(ctx, &db, (const uint8_t*)ctx->bufs[BUF_VERDICT].p, nullptr, Part{0, 1}, tally, ctx->stream);
}

}  // extern "C"

// ------------------------------------------------------------------ decide
// hd_decide: the tally's tables plus the propose log of process.go:758-819,
// and one row per round with the counts and the eight predicate bits the
// 2f+1 / f+1 rules read (include/hd_verify.h).  The launch sequence is the
// tally's with two propose passes and a decide pass inside it, while the G /
// C / log tables are populated:
//
//   k_decide_claim   every eligible propose -> its round's slot of P, a claim
//                    table keyed (h, r): first-wins = the lowest batch index
//                    (CAS / atomicMin, wavefront-leader probing as pass 1);
//                    the other messages get their class (3, or 4 out of turn)
//   k_tally_rounds, k_tally_logs, k_tally_values      unchanged
//   k_decide_log     P's winners are the logged proposes: each takes (or
//                    creates -- a round no vote names) its round's G slot with
//                    its batch index, so a round's first item is its first
//                    vote candidate or logged propose; the other eligible
//                    proposes compare with the winner (Equal, message.go:83-89)
//   k_tally_firsts   unchanged: the first-item bitmap and its prefixes
//   k_decide_emit    each round's first item writes the round's row: counts
//                    from G, the propose from P, per-value counts by lookups
//                    in C (this round's and (h, valid_round)'s), "signer is
//                    new" from the round's dense log cells or D.  Read-only on
//                    the tables, so rows may read other rounds' slots
//   k_decide_clean   every first item / winner resets its slots of G, C, D
//                    and P: the tables are clean for the next call (tally or
//                    decide), as after k_tally_emit
struct DecideCols {
    int64_t *h, *r;
    uint32_t *rep, *propose, *prevotes, *precommits, *trace, *pv_value, *pc_value, *pv_nil, *pv_validround;
    uint8_t *flags, *bits;
};
#define HD_DCOL(f) HD_COL(DecideCols, f, hd_decide_out, f)
constexpr Col kDecideCols[] = {
    HD_COL(DecideCols, h, hd_decide_out, height), HD_COL(DecideCols, r, hd_decide_out, round),
    HD_DCOL(rep), HD_DCOL(propose), HD_DCOL(prevotes), HD_DCOL(precommits), HD_DCOL(trace), HD_DCOL(pv_value),
    HD_DCOL(pc_value), HD_DCOL(pv_nil), HD_DCOL(pv_validround), HD_DCOL(flags), HD_DCOL(bits),
};
constexpr size_t kDecideRow = row_bytes(kDecideCols);
static_assert(kDecideRow == 2 * 8 + 9 * 4 + 2, "decide row bytes");
static_assert(sizeof(kDecideCols) / sizeof(Col) == sizeof(DecideCols) / sizeof(void*), "every DecideCols pointer is a column");
// the ordered form's rows, after the decide rows at strides of their own
constexpr size_t kWhenRow = 8 * sizeof(uint32_t), kUntilRow = sizeof(uint32_t);

HD_HOSTONLY DecideCols decide_cols(char* base, uint32_t cap) {
    DecideCols x;
    cols_layout(kDecideCols, base, cap, &x);
    return x;
}

// DecideIn (f, the device schedule and value_ok): hd_internal.h

__device__ __forceinline__ bool msg_valid(const uint8_t* verdict, const uint32_t* bitmap, uint32_t i) {
    if (verdict && verdict[i] != V_VALID) return false;
    if (bitmap && !((bitmap[i >> 5] >> (i & 31)) & 1u)) return false;
    return true;
}

// class of message i before the log is known: 0 eligible, 3 not a propose
// candidate, 4 out of turn (process.go:759-781)
__device__ __forceinline__ uint8_t propose_class(const DevBatch& b, const uint8_t* verdict, const uint32_t* bitmap,
                                                 const DecideIn& in, uint32_t i) {
    if (b.type[i] != T_PROPOSE || !msg_valid(verdict, bitmap, i)) return 3;
    const int64_t h = b.height[i], r = b.round[i];
    if (r <= -1) return 3;                         // process.go:763
    if (!in.sched32) return 0;                     // p.scheduler == nil (770)
    if (h <= 0) return 3;
    const uint64_t turn = ((uint64_t)h + (uint64_t)r) % in.n_sched;   // scheduler.go:52
    uint32_t from[8], want[8];
    load_row32_be(from, b.from32, i);
    load_row32_be(want, in.sched32, turn);
    uint32_t diff = 0;
    HD_UNROLL for (int k = 0; k < 8; k++) diff |= from[k] ^ want[k];
    return diff ? 4 : 0;
}

__global__ void k_decide_claim(DevBatch b, const uint8_t* __restrict__ verdict, const uint32_t* __restrict__ bitmap,
                               DecideIn in, uint32_t* __restrict__ P, uint32_t mask, uint32_t* __restrict__ pslot,
                               uint8_t* __restrict__ pclass) {
    const uint32_t stride = gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * blockDim.x; base < b.n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool e = false;
        if (i < b.n) {
            const uint8_t cls = propose_class(b, verdict, bitmap, in, i);
            e = cls == 0;
            if (!e) {
                pslot[i] = kEmpty;
                if (pclass) pclass[i] = cls;
            }
        }
        const unsigned long long act = __ballot(e);
        if (!act) continue;
        const int lead = __ffsll((long long)act) - 1;
        const int64_t h = e ? b.height[i] : 0, r = e ? b.round[i] : 0;
        const int64_t hl = shfl64(h, lead), rl = shfl64(r, lead);   // every lane takes part in the shuffles
        const bool follower = e && lane != lead && hl == h && rl == r;
        uint32_t s = kEmpty;
        if (e && !follower) {
            bool created;
            s = probe(P, mask, hash_hr(h, r), i, [&](uint32_t o) { return b.height[o] == h && b.round[o] == r; },
                      created);
        }
        const uint32_t sl = (uint32_t)__shfl((int)s, lead, 64);
        if (e) pslot[i] = follower ? sl : s;
    }
}

__global__ void k_decide_log(DevBatch b, const uint32_t* __restrict__ P, const uint32_t* __restrict__ pslot, GTab G,
                             uint32_t mask, uint32_t* __restrict__ gslot, uint32_t* __restrict__ cslot,
                             uint32_t* __restrict__ ref, uint8_t* __restrict__ pclass) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < b.n; i += stride) {
        const uint32_t ps = pslot[i];
        if (ps == kEmpty) continue;
        const uint32_t w = P[ps];
        if (w == i) {   // logged (process.go:804, 811): the round's row may start here
            const int64_t h = b.height[i], r = b.round[i];
            bool created;
            gslot[i] = probe(G.claim, mask, hash_hr(h, r), i,
                             [&](uint32_t o) { return b.height[o] == h && b.round[o] == r; }, created);
            cslot[i] = kEmpty;   // no count group, no log cell
            ref[i] = 0;
            if (pclass) pclass[i] = 0;
        } else if (pclass) {     // process.go:788-795
            const bool same_vr = !b.valid_round || b.valid_round[w] == b.valid_round[i];
            const bool equal = same_vr && eq32(b.value32 + 32 * (size_t)w, b.value32 + 32 * (size_t)i) &&
                               eq32(b.from32 + 32 * (size_t)w, b.from32 + 32 * (size_t)i);
            pclass[i] = equal ? 1 : 2;
        }
    }
}

// first-wins votes of (G slot g, type t) for the value (v0, v1): C.n of the
// key's slot, 0 when no vote carries it (hash_count's hash, from registers)
__device__ __forceinline__ uint32_t count_of(const CTab& C, uint32_t mask, const DevBatch& b,
                                             const uint32_t* gslot, uint32_t g, uint8_t t, uint4 v0, uint4 v1) {
    const uint64_t hv = ((uint64_t)v0.y << 32 | v0.x) ^ ((uint64_t)v0.w << 32 | v0.z);
    const uint32_t c = find(C.claim, mask, mix64(hv ^ ((uint64_t)g << 1 | (t & 1u))), [&](uint32_t o) {
        if (gslot[o] != g || b.type[o] != t) return false;
        const uint4* p = reinterpret_cast<const uint4*>(b.value32 + 32 * (size_t)o);
        const uint4 a = p[0], d = p[1];
        return ((a.x ^ v0.x) | (a.y ^ v0.y) | (a.z ^ v0.z) | (a.w ^ v0.w) | (d.x ^ v1.x) | (d.y ^ v1.y) |
                (d.z ^ v1.z) | (d.w ^ v1.w)) == 0;
    });
    return c == kEmpty ? 0u : C.n[c];
}

template <uint32_t IPB>
__global__ __launch_bounds__(256) void k_decide_emit(DevBatch b, uint32_t m, DecideIn in,
                                                     const uint32_t* __restrict__ gslot, GTab G, CTab C,
                                                     const uint32_t* __restrict__ D, const uint32_t* __restrict__ P,
                                                     const uint32_t* __restrict__ Dd, AdmIndex ix, uint32_t S,
                                                     uint32_t nd, uint32_t mask, const uint32_t* __restrict__ Bg,
                                                     const uint32_t* __restrict__ pre_g,
                                                     const uint32_t* __restrict__ blk, DecideCols st, uint32_t H,
                                                     DecideCols ov, uint32_t* stage_hdr) {
    const uint32_t nb = gridDim.x;
    __shared__ uint32_t part[4];
    uint32_t sg = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256) sg += blk[k];
    for (int d = 32; d > 0; d >>= 1) sg += (uint32_t)__shfl_xor((int)sg, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sg;
    __syncthreads();
    const uint32_t og = part[0] + part[1] + part[2] + part[3];
    if (threadIdx.x == 0 && blockIdx.x == nb - 1) stage_hdr[0] = og + blk[nb - 1];   // rows
    const uint64_t q2 = 2ull * in.f + 1ull, q1 = (uint64_t)in.f + 1ull;
    const uint32_t lo = blockIdx.x * IPB;
    for (uint32_t k = 0; k < IPB / 256; k++) {
        const uint32_t q = lo + k * 256 + threadIdx.x;
        if (q >= m) break;
        const uint32_t g = gslot[q];
        if (g == kEmpty) continue;
        const uint32_t w = q >> 5, gw = Bg[w];
        if (!((gw >> (q & 31)) & 1u)) continue;
        const uint32_t pos = og + pre_g[w] + (uint32_t)__popc(gw & ((1u << (q & 31)) - 1u));
        const int64_t h = b.height[q], r = b.round[q];
        const uint32_t np = G.nprev[g], nc = G.nprec[g], any = np + nc - G.nboth[g];
        const uint4 zero = make_uint4(0, 0, 0, 0);
        const uint32_t ps = find(P, mask, hash_hr(h, r), [&](uint32_t o) { return b.height[o] == h && b.round[o] == r; });
        const uint32_t p = ps == kEmpty ? kEmpty : P[ps];
        uint32_t pv_value = 0, pc_value = 0, pv_vr = 0, flags = 0;
        bool valid = false, has_vr = false;
        if (p != kEmpty) {
            const uint4* vp = reinterpret_cast<const uint4*>(b.value32 + 32 * (size_t)p);
            const uint4 v0 = vp[0], v1 = vp[1];
            const bool nil = (v0.x | v0.y | v0.z | v0.w | v1.x | v1.y | v1.z | v1.w) == 0;
            valid = !nil && (!in.value_ok || in.value_ok[p] != 0);   // process.go:803
            pv_value = count_of(C, mask, b, gslot, g, T_PREVOTE, v0, v1);
            pc_value = count_of(C, mask, b, gslot, g, T_PRECOMMIT, v0, v1);
            const int64_t vr = b.valid_round ? b.valid_round[p] : -1;
            has_vr = vr > -1;
            if (has_vr) {   // process.go:486-491
                const uint32_t g2 = vr == r ? g : find(G.claim, mask, hash_hr(h, vr), [&](uint32_t o) {
                    return b.height[o] == h && b.round[o] == vr;
                });
                if (g2 != kEmpty) pv_vr = count_of(C, mask, b, gslot, g2, T_PREVOTE, v0, v1);
            }
            bool fresh = false;
            if (valid) {    // process.go:813-816: is From already in TraceLogs[r]?
                bool seen = false;
                if (np + nc) {
                    const uint32_t rid = G.gid[g];
                    int32_t signer = -1;
                    if (rid < nd) {
                        uint32_t from_be[8];
                        load_row32_be(from_be, b.from32, p);
                        signer = adm_index_find(ix, from_be);
                    }
                    if (signer >= 0) {   // the dense cells of (round, prevote | precommit, signer)
                        const uint32_t cell = rid * 2u * S + (uint32_t)signer;
                        seen = Dd[cell] != kEmpty || Dd[cell + S] != kEmpty;
                    } else {
                        const uint8_t* from = b.from32 + 32 * (size_t)p;
                        const uint64_t hhr = hash_hr(h, r);
                        for (uint32_t t = T_PREVOTE; t <= T_PRECOMMIT && !seen; t++)
                            seen = find(D, mask, hash_log(hhr, from, t), [&](uint32_t c) {
                                       return b.type[c] == t && b.height[c] == h && b.round[c] == r &&
                                              eq32(b.from32 + 32 * (size_t)c, from);
                                   }) != kEmpty;
                    }
                }
                fresh = !seen;
            }
            flags = 1u | (valid ? 2u : 0u) | (fresh ? 4u : 0u);
        }
        const uint32_t pv_nil = count_of(C, mask, b, gslot, g, T_PREVOTE, zero, zero);
        const uint32_t trace = any + ((flags >> 2) & 1u);
        uint32_t bits = 0;
        bits |= np >= q2 ? 1u : 0u;                        // timeout_prevote
        bits |= pv_nil >= q2 ? 2u : 0u;                    // precommit_nil
        bits |= nc >= q2 ? 4u : 0u;                        // timeout_precommit_reached
        bits |= nc == q2 ? 8u : 0u;                        // timeout_precommit_exact
        bits |= trace >= q1 ? 16u : 0u;                    // skip
        bits |= valid && pv_value >= q2 ? 32u : 0u;        // precommit_value
        bits |= valid && pc_value >= q2 ? 64u : 0u;        // commit
        bits |= has_vr && pv_vr >= q2 ? 128u : 0u;         // prevote_validround
        const DecideCols& x = pos < H ? st : ov;
        const uint32_t j = pos < H ? pos : pos - H;
        x.h[j] = h;
        x.r[j] = r;
        x.rep[j] = q;
        x.propose[j] = p;
        x.prevotes[j] = np;
        x.precommits[j] = nc;
        x.trace[j] = trace;
        x.pv_value[j] = pv_value;
        x.pc_value[j] = pc_value;
        x.pv_nil[j] = pv_nil;
        x.pv_validround[j] = pv_vr;
        x.flags[j] = (uint8_t)flags;
        x.bits[j] = (uint8_t)bits;
    }
}

// after k_decide_emit: every table slot back to empty / zero by the item that
// owns it (a round's first item, a count group's and a hashed log's winner,
// a logged propose), and the round numbering restarts
__global__ void k_decide_clean(uint32_t m, const uint32_t* __restrict__ gslot, const uint32_t* __restrict__ cslot,
                               const uint32_t* __restrict__ ref, const uint32_t* __restrict__ pslot, GTab G, CTab C,
                               uint32_t* __restrict__ D, uint32_t* __restrict__ P, const uint32_t* __restrict__ Bg,
                               TallyCtr* ctr) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr->n_rounds = 0;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += stride) {
        const uint32_t ps = pslot[q];
        if (ps != kEmpty && P[ps] == q) P[ps] = kEmpty;
        const uint32_t g = gslot[q];
        if (g == kEmpty) continue;
        if ((Bg[q >> 5] >> (q & 31)) & 1u) {
            G.claim[g] = kEmpty;
            G.nprev[g] = G.nprec[g] = G.nboth[g] = 0;
        }
        const uint32_t c = cslot[q];
        if (c != kEmpty && C.claim[c] == q) {
            C.claim[c] = kEmpty;
            C.n[c] = 0;
        }
        const uint32_t rf = ref[q];
        if ((rf & HD_REF_HASHED) && D[rf & ~HD_REF_HASHED] == q) D[rf & ~HD_REF_HASHED] = kEmpty;
    }
}

// ---------------------------------------------------------- decide, ordered
// hd_decide_ordered: per row and predicate the batch index at which the rule
// first holds when the batch is inserted one message at a time (when[8], and
// exact_until for the one rule that is not monotone; include/hd_verify.h).
// Every value is "the k-th smallest batch index among the logged votes of a
// round that have some property", so the passes run between k_decide_emit and
// k_decide_clean, while G / C / D / P and the dense cells are still populated:
//
//   k_decide_order_keys   every item's sort key: its round's number (G.gid),
//                         or the key mask for an item that is not a logged
//                         vote.  Bits 30 and 31, above the sorted bits, carry
//                         "precommit" and "this vote is its signer's trace
//                         entry" (the signer's logged vote of the other type
//                         is absent or later: the other dense cell, or D)
//   one stable radix sort of (key, batch index) over the key bits: each
//                         round's logged votes become one segment in arrival
//                         order, whichever log path they took
//   k_decide_when         one wavefront per emitted row: finds the round's
//                         segment (a 64-ary search by the wavefront), walks it
//                         64 items at a time with ballot / popcount prefixes
//                         of eight running counts, and records the index at
//                         which each count reaches its threshold.  Value
//                         classes compare C slots (an item's cslot against the
//                         slot of the propose's value), not value bytes.
#define HD_WKEY_PRECOMMIT 0x40000000u
#define HD_WKEY_TRACE 0x80000000u

// the D slot of the log (h, r, t, from), kEmpty when there is none
__device__ __forceinline__ uint32_t log_find(const DevBatch& b, const uint32_t* D, uint32_t mask, int64_t h, int64_t r,
                                             const uint8_t* from, uint32_t t) {
    return find(D, mask, hash_log(hash_hr(h, r), from, t), [&](uint32_t c) {
        return b.type[c] == t && b.height[c] == h && b.round[c] == r && eq32(b.from32 + 32 * (size_t)c, from);
    });
}

__global__ void k_decide_order_keys(DevBatch b, uint32_t m, const uint32_t* __restrict__ gslot,
                                    const uint32_t* __restrict__ cslot, const uint32_t* __restrict__ ref,
                                    const uint32_t* __restrict__ gid, const uint32_t* __restrict__ Dd, uint32_t S,
                                    const uint32_t* __restrict__ D, uint32_t mask, uint32_t kmask,
                                    uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < m; q += stride) {
        const uint32_t g = gslot[q];
        uint32_t k = kmask;
        if (g != kEmpty && cslot[q] != kEmpty) {   // a logged vote (a logged propose has no count slot)
            const bool pc = b.type[q] == T_PRECOMMIT;
            const uint32_t rf = ref[q];
            uint32_t other;   // the signer's logged vote of the other type in the round
            if (!(rf & HD_REF_HASHED)) {
                other = Dd[pc ? rf - S : rf + S];
            } else {
                const uint32_t o = log_find(b, D, mask, b.height[q], b.round[q], b.from32 + 32 * (size_t)q,
                                            pc ? T_PREVOTE : T_PRECOMMIT);
                other = o == kEmpty ? kEmpty : D[o];
            }
            k = gid[g] | (pc ? HD_WKEY_PRECOMMIT : 0u) | (other > q ? HD_WKEY_TRACE : 0u);
        }
        key[q] = k;
        val[q] = q;
    }
}

// the C slot of (G slot g, type t, value (v0, v1)), kEmpty when no vote carries it
__device__ __forceinline__ uint32_t cslot_of(const CTab& C, uint32_t mask, const DevBatch& b, const uint32_t* gslot,
                                             uint32_t g, uint8_t t, uint4 v0, uint4 v1) {
    const uint64_t hv = ((uint64_t)v0.y << 32 | v0.x) ^ ((uint64_t)v0.w << 32 | v0.z);
    return find(C.claim, mask, mix64(hv ^ ((uint64_t)g << 1 | (t & 1u))), [&](uint32_t o) {
        if (gslot[o] != g || b.type[o] != t) return false;
        const uint4* p = reinterpret_cast<const uint4*>(b.value32 + 32 * (size_t)o);
        const uint4 a = p[0], d = p[1];
        return ((a.x ^ v0.x) | (a.y ^ v0.y) | (a.z ^ v0.z) | (a.w ^ v0.w) | (d.x ^ v1.x) | (d.y ^ v1.y) |
                (d.z ^ v1.z) | (d.w ^ v1.w)) == 0;
    });
}

// first position of skey[0..n) whose sorted bits are >= target, by the whole
// wavefront: 64 probes per step narrow the range 64-fold
__device__ __forceinline__ uint32_t seg_start(const uint32_t* __restrict__ skey, uint32_t n, uint32_t kmask,
                                              uint32_t target) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t step = (hi - lo + 63u) / 64u;
        const uint64_t pos = (uint64_t)lo + (uint64_t)lane * step;
        const bool less = pos < hi && (skey[pos] & kmask) < target;
        const uint32_t c = (uint32_t)__popcll(__ballot(less));   // sorted: the lanes below the answer
        if (c == 0) return lo;
        const uint64_t nlo = (uint64_t)lo + (uint64_t)(c - 1) * step + 1u, nhi = (uint64_t)lo + (uint64_t)c * step;
        hi = nhi < hi ? (uint32_t)nhi : hi;
        lo = (uint32_t)nlo;
    }
    return lo;
}

// Walks a segment of the sorted items in arrival order.  flags_of(idx, key,
// cslot) gives an item's NC class bits; res[k] becomes, on the lane that holds
// it, the batch index of the item at which class k's running count equals
// target[k].  Four 64-item chunks are loaded before any is counted, so that a
// long segment pays the gather latency once per 256 items.
template <int NC, typename F>
__device__ __forceinline__ void seg_walk(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval,
                                         const uint32_t* __restrict__ cslot, uint32_t start, uint32_t len, F flags_of,
                                         const uint64_t (&target)[NC], uint32_t (&res)[NC]) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long le = (2ull << lane) - 1ull;   // this lane and the lanes below it
    uint32_t cnt[NC];
    HD_UNROLL for (int k = 0; k < NC; k++) cnt[k] = 0;
    for (uint32_t base = 0; base < len; base += 256u) {
        uint32_t key[4], idx[4], cs[4];
        HD_UNROLL for (int u = 0; u < 4; u++) {
            const uint32_t j = base + 64u * u + lane;
            key[u] = j < len ? skey[(size_t)start + j] : 0u;
            idx[u] = j < len ? sval[(size_t)start + j] : 0u;
        }
        HD_UNROLL for (int u = 0; u < 4; u++) {
            const uint32_t j = base + 64u * u + lane;
            cs[u] = j < len ? cslot[idx[u]] : kEmpty;
        }
        HD_UNROLL for (int u = 0; u < 4; u++) {
            const uint32_t j = base + 64u * u + lane;
            const uint32_t fl = j < len ? flags_of(idx[u], key[u], cs[u]) : 0u;
            HD_UNROLL for (int k = 0; k < NC; k++) {
                const bool f = (fl >> k) & 1u;
                const unsigned long long bal = __ballot(f);
                if (f && (uint64_t)(cnt[k] + (uint32_t)__popcll(bal & le)) == target[k]) res[k] = idx[u];
                cnt[k] += (uint32_t)__popcll(bal);
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
    for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_decide_when(DevBatch b, uint32_t m, DecideIn in,
                                                     const uint32_t* __restrict__ gslot,
                                                     const uint32_t* __restrict__ cslot, GTab G, CTab C,
                                                     const uint32_t* __restrict__ D, const uint32_t* __restrict__ Dd,
                                                     AdmIndex ix, uint32_t S, uint32_t nd, uint32_t mask,
                                                     const uint32_t* __restrict__ skey,
                                                     const uint32_t* __restrict__ sval, uint32_t kmask, DecideCols st,
                                                     uint32_t H, DecideCols ov, const uint32_t* stage_hdr,
                                                     uint32_t* __restrict__ st_when, uint32_t* __restrict__ st_until,
                                                     uint32_t* __restrict__ ov_when, uint32_t* __restrict__ ov_until) {
    const uint32_t rows = stage_hdr[0];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const uint64_t q2 = 2ull * in.f + 1ull, q1 = (uint64_t)in.f + 1ull;
    const uint32_t never = HD_WHEN_NEVER;
    for (uint32_t pos = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); pos < rows; pos += nwaves) {
        const DecideCols& x = pos < H ? st : ov;
        const uint32_t j = pos < H ? pos : pos - H;
        uint32_t* const o_when = (pos < H ? st_when : ov_when) + 8 * (size_t)j;
        uint32_t* const o_until = (pos < H ? st_until : ov_until) + j;
        const uint32_t bits = x.bits[j];
        uint32_t w[8] = {never, never, never, never, never, never, never, never}, until = never;
        if (bits) {   // no bit set: nothing ever held (bit 2 covers the exact rule's window)
            const uint32_t g = gslot[x.rep[j]], p = x.propose[j], flags = x.flags[j];
            const int64_t h = x.h[j], r = x.r[j];
            const uint32_t len = x.prevotes[j] + x.precommits[j];
            const bool valid = (flags & 2u) != 0;
            const uint4 zero = make_uint4(0, 0, 0, 0);
            uint4 v0 = zero, v1 = zero;
            if (p != kEmpty) {
                const uint4* vp = reinterpret_cast<const uint4*>(b.value32 + 32 * (size_t)p);
                v0 = vp[0];
                v1 = vp[1];
            }
            // the C slots an item's cslot is compared with (kEmpty matches no logged vote)
            const uint32_t c_nil = (bits & 2u) ? cslot_of(C, mask, b, gslot, g, T_PREVOTE, zero, zero) : kEmpty;
            const uint32_t c_pv = (bits & (32u | 128u)) ? cslot_of(C, mask, b, gslot, g, T_PREVOTE, v0, v1) : kEmpty;
            const uint32_t c_pc = (bits & 64u) ? cslot_of(C, mask, b, gslot, g, T_PRECOMMIT, v0, v1) : kEmpty;
            // the proposer's trace entry (process.go:813-816): the propose when it comes before the
            // proposer's first logged vote of the round, which then is no entry of its own
            bool addp = false;
            uint32_t fv = kEmpty;
            if ((bits & 16u) && valid) {
                if (!(flags & 4u)) {   // the proposer has logged votes in the round
                    const uint32_t rid = G.gid[g];
                    int32_t signer = -1;
                    if (rid < nd) {
                        uint32_t from_be[8];
                        load_row32_be(from_be, b.from32, p);
                        signer = adm_index_find(ix, from_be);
                    }
                    if (signer >= 0) {
                        const uint32_t cell = rid * 2u * S + (uint32_t)signer;
                        fv = min(Dd[cell], Dd[cell + S]);
                    } else {
                        const uint8_t* from = b.from32 + 32 * (size_t)p;
                        const uint32_t a = log_find(b, D, mask, h, r, from, T_PREVOTE),
                                       c = log_find(b, D, mask, h, r, from, T_PRECOMMIT);
                        fv = min(a == kEmpty ? kEmpty : D[a], c == kEmpty ? kEmpty : D[c]);
                    }
                }
                addp = p < fv;
            }
            uint32_t res[8] = {never, never, never, never, never, never, never, never};
            if (len) {
                const uint64_t target[8] = {q2, q2, q2, q2 + 1ull, q1 - 1ull, q1, q2, q2};
                const uint32_t start = seg_start(skey, m, kmask, G.gid[g]);
                seg_walk<8>(skey, sval, cslot, start, min(len, m - start),
                            [&](uint32_t idx, uint32_t key, uint32_t cs) {
                                const bool pc = (key & HD_WKEY_PRECOMMIT) != 0;
                                const bool tn = (key & HD_WKEY_TRACE) != 0 && !(addp && idx == fv);
                                return (pc ? 0u : 1u) | (cs == c_nil ? 2u : 0u) | (pc ? 4u | 8u : 0u) |
                                       (tn ? 16u | 32u : 0u) | (cs == c_pv ? 64u : 0u) | (cs == c_pc ? 128u : 0u);
                            },
                            target, res);
                HD_UNROLL for (int k = 0; k < 8; k++) res[k] = wave_min(res[k]);
            }
            w[0] = res[0];
            w[1] = res[1];
            w[2] = w[3] = res[2];
            until = res[3];
            // the q1-th smallest trace entry: the votes' entries with the propose merged in at p
            if (!addp) {
                w[4] = res[5];
            } else if (q1 == 1ull) {
                w[4] = min(p, res[5]);
            } else if (res[4] != never) {   // the (q1-1)-th vote entry exists
                w[4] = p < res[4] ? res[4] : min(p, res[5]);
            }
            if (valid && res[6] != never) w[5] = max(p, res[6]);
            if (valid && res[7] != never) w[6] = max(p, res[7]);
            if (bits & 128u) {   // the valid round's prevotes for the propose's value (process.go:486-491)
                const int64_t vr = b.valid_round[p];
                uint32_t k7 = res[6];
                if (vr != r) {
                    const uint32_t g2 = find(G.claim, mask, hash_hr(h, vr),
                                             [&](uint32_t o) { return b.height[o] == h && b.round[o] == vr; });
                    k7 = never;
                    if (g2 != kEmpty) {
                        const uint32_t c_vr = cslot_of(C, mask, b, gslot, g2, T_PREVOTE, v0, v1);
                        const uint64_t target1[1] = {q2};
                        uint32_t res1[1] = {never};
                        const uint32_t start2 = seg_start(skey, m, kmask, G.gid[g2]);
                        seg_walk<1>(skey, sval, cslot, start2, min(G.nprev[g2] + G.nprec[g2], m - start2),
                                    [&](uint32_t, uint32_t, uint32_t cs) { return cs == c_vr ? 1u : 0u; }, target1,
                                    res1);
                        k7 = wave_min(res1[0]);
                    }
                }
                if (k7 != never) w[7] = max(p, k7);
            }
        }
        if (lane == 0) {
            uint4* o = reinterpret_cast<uint4*>(o_when);
            o[0] = make_uint4(w[0], w[1], w[2], w[3]);
            o[1] = make_uint4(w[4], w[5], w[6], w[7]);
            *o_until = until;
        }
    }
}

// ------------------------------------------------------------ decide, catch
// hd_decide_catch: the offences of a batch, each with the logged message it
// contradicts -- the arguments of Catcher.CatchDoublePropose / CatchDoublePrevote
// / CatchDoublePrecommit / CatchOutOfTurnPropose (process.go:771-793, 838-841,
// 875-878).  A message has a record exactly when dup == 2 or pclass is 2 or 4,
// and the logged message is the winner the classifying kernel compared it
// with: the log cell its `ref` names (a dense cell, or a slot of D) for a vote,
// P[pslot] for a propose.  The passes run where the ordered passes run,
// between k_decide_emit and k_decide_clean, and read the winner again from
// the populated tables; k_tally_values and k_decide_log stay as they are (the
// tally runs the first beside every verification).  Records are in batch
// order by the firsts / emit idiom above -- ballot words, popcount prefixes,
// block totals summed by every emit block: no sort, no atomics.
//
//   k_catch_flags   "has a record" per item as whole bitmap words, their
//                   prefix within the block and the block's total.  The words
//                   go where k_tally_firsts put Bc / pre_c and the C half of
//                   the block totals: nothing reads those after the firsts
//                   pass of a decide (k_decide_clean reads Bg only)
//   k_catch_emit    each flagged item writes (index, against, kind) at its
//                   position, into the stage below the staged capacity and
//                   into the overflow columns past it; the last block writes
//                   the record count into word 1 of the stage header
struct CatchCols {
    uint32_t *index, *against;
    uint8_t* kind;
};
constexpr Col kCatchCols[] = {
    HD_COL(CatchCols, index, hd_catch_out, index), HD_COL(CatchCols, against, hd_catch_out, against),
    HD_COL(CatchCols, kind, hd_catch_out, kind),
};
constexpr size_t kCatchRow = row_bytes(kCatchCols);
static_assert(kCatchRow == 2 * 4 + 1, "catch record bytes");
static_assert(sizeof(kCatchCols) / sizeof(Col) == sizeof(CatchCols) / sizeof(void*), "every CatchCols pointer is a column");

HD_HOSTONLY CatchCols catch_cols(char* base, uint32_t cap) {
    CatchCols x;
    cols_layout(kCatchCols, base, cap, &x);
    return x;
}

__device__ __forceinline__ bool has_record(const uint8_t* dup, const uint8_t* pclass, uint32_t q) {
    const uint8_t pc = pclass[q];
    return dup[q] == 2 || pc == 2 || pc == 4;
}

template <uint32_t IPB>
__global__ __launch_bounds__(256) void k_catch_flags(uint32_t m, const uint8_t* __restrict__ dup,
                                                     const uint8_t* __restrict__ pclass, uint32_t* __restrict__ Bx,
                                                     uint32_t* __restrict__ pre_x, uint32_t* __restrict__ blk_x) {
    constexpr uint32_t W = IPB / 32;   // words per block (<= 64: one wavefront scans them)
    __shared__ uint32_t wx[W];
    const uint32_t lo = blockIdx.x * IPB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t k = 0; k < IPB / 256; k++) {
        const uint32_t q = lo + k * 256 + threadIdx.x;
        const unsigned long long bx = __ballot(q < m && has_record(dup, pclass, q));
        if (lane == 0) {
            const uint32_t w = k * 8 + wave * 2;
            wx[w] = (uint32_t)bx;
            wx[w + 1] = (uint32_t)(bx >> 32);
        }
    }
    __syncthreads();
    if (threadIdx.x < W) {   // one lane per word (wavefront 0)
        const uint32_t t = threadIdx.x, xw = wx[t];
        uint32_t ix = (uint32_t)__popc(xw);
        for (int d = 1; d < 64; d <<= 1) {   // inclusive scan across the wavefront
            const uint32_t yx = (uint32_t)__shfl_up((int)ix, d, 64);
            if ((int)t >= d) ix += yx;
        }
        const size_t wi = (size_t)blockIdx.x * W + t;
        Bx[wi] = xw;
        pre_x[wi] = ix - (uint32_t)__popc(xw);
        if (t == W - 1) blk_x[blockIdx.x] = ix;
    }
}

template <uint32_t IPB>
__global__ __launch_bounds__(256) void k_catch_emit(DevBatch b, uint32_t m, const uint8_t* __restrict__ dup,
                                                    const uint8_t* __restrict__ pclass,
                                                    const uint32_t* __restrict__ ref,
                                                    const uint32_t* __restrict__ pslot,
                                                    const uint32_t* __restrict__ Dd, const uint32_t* __restrict__ D,
                                                    const uint32_t* __restrict__ P, const uint32_t* __restrict__ Bx,
                                                    const uint32_t* __restrict__ pre_x,
                                                    const uint32_t* __restrict__ blk_x, CatchCols st, uint32_t H,
                                                    CatchCols ov, uint32_t* stage_hdr) {
    const uint32_t nb = gridDim.x;
    __shared__ uint32_t part[4];
    uint32_t sx = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256) sx += blk_x[k];
    for (int d = 32; d > 0; d >>= 1) sx += (uint32_t)__shfl_xor((int)sx, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sx;
    __syncthreads();
    const uint32_t ox = part[0] + part[1] + part[2] + part[3];
    if (threadIdx.x == 0 && blockIdx.x == nb - 1) stage_hdr[1] = ox + blk_x[nb - 1];   // records
    const uint32_t lo = blockIdx.x * IPB;
    for (uint32_t k = 0; k < IPB / 256; k++) {
        const uint32_t q = lo + k * 256 + threadIdx.x;
        if (q >= m) break;
        const uint32_t w = q >> 5, xw = Bx[w];
        if (!((xw >> (q & 31)) & 1u)) continue;
        const uint32_t pos = ox + pre_x[w] + (uint32_t)__popc(xw & ((1u << (q & 31)) - 1u));
        uint32_t against = HD_WHEN_NEVER;
        uint8_t kind = HD_CATCH_OUT_OF_TURN;
        if (dup[q] == 2) {   // a candidate vote: ref names its log cell, which holds the logged vote
            const uint32_t rf = ref[q];
            against = (rf & HD_REF_HASHED) ? D[rf & ~HD_REF_HASHED] : Dd[rf];
            kind = b.type[q] == T_PREVOTE ? HD_CATCH_DOUBLE_PREVOTE : HD_CATCH_DOUBLE_PRECOMMIT;
        } else if (pclass[q] == 2) {   // an eligible propose: its round's slot of P holds the logged propose
            against = P[pslot[q]];
            kind = HD_CATCH_DOUBLE_PROPOSE;
        }
        const CatchCols& x = pos < H ? st : ov;
        const uint32_t j = pos < H ? pos : pos - H;
        x.index[j] = q;
        x.against[j] = against;
        x.kind[j] = kind;
    }
}

static bool catch_out_ok(const hd_catch_out* c) { return c && (c->cap == 0 || (c->index && c->against && c->kind)); }

static bool decide_out_ok(const hd_decide_out* o) {
    return o && o->height && o->round && o->rep && o->propose && o->prevotes && o->precommits && o->trace &&
           o->pv_value && o->pc_value && o->pv_nil && o->pv_validround && o->flags && o->bits;
}

// the ordered form's second output: rows for every row of `out`; the sort keys keep bits 30 and 31
// for flags, so a batch has fewer than 2^30 messages
static bool decide_order_ok(const hd_decide_out* o, const hd_decide_order* w, uint32_t n) {
    return o && w && w->when && w->exact_until && w->cap >= o->cap && n < (1u << 30);
}

// Whole batch only (items = batch indices).  One download of the stage
// [rows | dup (n bytes, when asked) | pclass (n bytes, when asked) | rows at
// capacity H]; rows past H come from the overflow columns by a second round
// of copies.  With `ord` (hd_decide_ordered) the stage continues with
// [when (8 words per row) | exact_until] at capacity H, and the overflow
// buffer likewise after its rows.  With `ext` (hd_log.hip) the classes go to
// the caller's device arrays instead of the stage (hd_internal.h).  With
// `caught` (hd_decide_catch) the stage ends with the catch records at a staged
// capacity of their own, their count in word 1 of the header; records past
// that capacity come from T_CATCH with the overflow rows.  The catch passes
// read both classes, so a class the caller does not take stays in T_CATCH and
// is not downloaded.
int hd_decide_run(hd_ctx* ctx, const hd_batch* hb, const uint8_t* d_verdict, const uint32_t* d_bitmap, DecideIn in,
                  hd_decide_out* out, hipStream_t s, hd_decide_order* ord, const DecideExt* ext,
                  hd_catch_out* caught) {
    const uint32_t n = hb->n, m = n;
    if (!ctx->tally) ctx->tally = new TallyWork();
    TallyWork* tw = ctx->tally;
    DevBatch b{n, hb->type, hb->height, hb->round, hb->valid_round, hb->value32, hb->from32, nullptr};
    int rc = 0;
    const uint32_t H = tw->guess_dec;
    const bool st_dup = !ext && out->dup, st_pclass = !ext && out->pclass;   // staged and downloaded
    const size_t dup_off = 64, pc_off = dup_off + (st_dup ? pad64(n) : 0), rows_off = pc_off + (st_pclass ? pad64(n) : 0);
    const size_t when_off = rows_off + pad64(kDecideRow * H), until_off = when_off + kWhenRow * H;
    const size_t total0 = ord ? until_off + kUntilRow * H + 64 : rows_off + kDecideRow * H + 64;
    const uint32_t Hc = caught ? tw->guess_catch.load() : 0u;
    const size_t catch_off = pad64(total0), total = caught ? catch_off + kCatchRow * Hc + 64 : total0;
    char* st = (char*)tbuf(ctx, T_DSTAGE, total, &rc);
    if (rc) return rc;
    uint8_t* d_dup = ext ? ext->d_dup : st_dup ? (uint8_t*)(st + dup_off) : nullptr;
    uint8_t* d_pclass = ext ? ext->d_pclass : st_pclass ? (uint8_t*)(st + pc_off) : nullptr;
    // the catch list's overflow records (capacity m), then the classes nobody downloads
    char* covf = nullptr;
    if (caught) {
        const size_t cls_off = pad64(kCatchRow * m + 64);
        covf = (char*)tbuf(ctx, T_CATCH, cls_off + 2 * pad64(n), &rc);
        if (rc) return rc;
        if (!d_dup) d_dup = (uint8_t*)(covf + cls_off);
        if (!d_pclass) d_pclass = (uint8_t*)(covf + cls_off + pad64(n));
    }
    // the overflow rows (capacity m), the ordered form's after them
    const size_t ovw_off = pad64(kDecideRow * m + 64), ovu_off = ovw_off + kWhenRow * m;
    char* ovf = (char*)tbuf(ctx, T_DOVF, ord ? ovu_off + kUntilRow * m + 64 : kDecideRow * m + 64, &rc);
    // the ordered form's sort: keys over the bits that hold every round number and, above them, the
    // key of the items that are no logged vote
    uint32_t *wkey = nullptr, *wval = nullptr, kbits = 1;
    void* wtmp = nullptr;
    size_t wtmp_bytes = 0;
    if (ord) {
        while ((1ull << kbits) <= m) kbits++;
        wkey = (uint32_t*)tbuf(ctx, T_WKEY, 8 * (size_t)m, &rc);
        wval = (uint32_t*)tbuf(ctx, T_WVAL, 8 * (size_t)m, &rc);
        if (rc) return rc;
        TCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, wtmp_bytes, wkey, wkey + m, wval, wval + m, (int)m, 0,
                                                (int)kbits, s),
             "decide sort size");
        wtmp = tbuf(ctx, T_WTMP, wtmp_bytes + 64, &rc);
    }
    if (rc) return rc;
    TallyPlan p;
    if ((rc = tally_plan(ctx, m, true, s, p))) return rc;
    const AdmIndex ix = hd_adm_index(ctx);
    k_decide_claim<<<p.grid, 256, 0, s>>>(b, d_verdict, d_bitmap, in, p.P, p.mask, p.pslot, d_pclass);
    k_tally_rounds<<<p.grid, 256, 0, s>>>(b, nullptr, m, d_verdict, d_bitmap, Part{0, 1}, p.G, p.mask, p.gslot, d_dup,
                                          p.ctr, p.Dd, 2 * p.S, p.nd);
    k_tally_logs<<<p.grid, 256, 0, s>>>(b, nullptr, m, p.gslot, p.G.gid, ix, p.S, p.Dd, p.nd, p.d, p.mask, p.ref);
    k_tally_values<<<p.grid, 256, 0, s>>>(b, nullptr, m, p.Dd, p.S, p.d, p.G, p.C, p.mask, p.gslot, p.ref, p.cslot,
                                          d_dup);
    k_decide_log<<<p.grid, 256, 0, s>>>(b, p.P, p.pslot, p.G, p.mask, p.gslot, p.cslot, p.ref, d_pclass);
    TCHK(hipGetLastError(), "decide kernels");
    const DecideCols sc = decide_cols(st + rows_off, H), oc = decide_cols(ovf, m);
    with_ipb(p.ipb, [&](auto ipb) {
        constexpr uint32_t IPB = decltype(ipb)::value;
        k_tally_firsts<IPB><<<p.nbo, 256, 0, s>>>(m, p.gslot, p.cslot, p.G.claim, p.C.claim, p.Bg, p.Bc, p.pre_g,
                                                  p.pre_c, p.blk);
        k_decide_emit<IPB><<<p.nbo, 256, 0, s>>>(b, m, in, p.gslot, p.G, p.C, p.d, p.P, p.Dd, ix, p.S, p.nd, p.mask,
                                                 p.Bg, p.pre_g, p.blk, sc, H, oc, (uint32_t*)st);
    });
    if (ord) {   // between the emit and the clean: the tables are populated and read-only
        const uint32_t kmask = (uint32_t)((1ull << kbits) - 1ull);
        k_decide_order_keys<<<p.grid, 256, 0, s>>>(b, m, p.gslot, p.cslot, p.ref, p.G.gid, p.Dd, p.S, p.d, p.mask,
                                                   kmask, wkey, wval);
        TCHK(hipGetLastError(), "decide order keys");
        TCHK(hipcub::DeviceRadixSort::SortPairs(wtmp, wtmp_bytes, wkey, wkey + m, wval, wval + m, (int)m, 0,
                                                (int)kbits, s),
             "decide sort");
        const uint32_t wgrid = std::min<uint32_t>((m + 3) / 4, (uint32_t)ctx->n_cu * 8u);   // four rows per block
        k_decide_when<<<wgrid, 256, 0, s>>>(b, m, in, p.gslot, p.cslot, p.G, p.C, p.d, p.Dd, ix, p.S, p.nd, p.mask,
                                            wkey + m, wval + m, kmask, sc, H, oc, (const uint32_t*)st,
                                            (uint32_t*)(st + when_off), (uint32_t*)(st + until_off),
                                            (uint32_t*)(ovf + ovw_off), (uint32_t*)(ovf + ovu_off));
    }
    DecideRecs recs_dev{};
    if (caught) {   // likewise; Bc, pre_c and the C totals are free after the firsts pass
        const CatchCols cs = catch_cols(st + catch_off, Hc), co = catch_cols(covf, m);
        recs_dev = DecideRecs{(const uint32_t*)st, cs.index, cs.against, Hc, co.index, co.against};
        with_ipb(p.ipb, [&](auto ipb) {
            constexpr uint32_t IPB = decltype(ipb)::value;
            k_catch_flags<IPB><<<p.nbo, 256, 0, s>>>(m, d_dup, d_pclass, p.Bc, p.pre_c, p.blk + p.nbo);
            k_catch_emit<IPB><<<p.nbo, 256, 0, s>>>(b, m, d_dup, d_pclass, p.ref, p.pslot, p.Dd, p.d, p.P, p.Bc,
                                                    p.pre_c, p.blk + p.nbo, cs, Hc, co, (uint32_t*)st);
        });
    }
    k_decide_clean<<<p.grid, 256, 0, s>>>(m, p.gslot, p.cslot, p.ref, p.pslot, p.G, p.C, p.d, p.P, p.Bg, p.ctr);
    TCHK(hipGetLastError(), "decide order kernels");
    tally_plan_done(ctx, p);
    if (ext && ext->queued) {
        rc = ext->queued(ext->arg, s, caught ? &recs_dev : nullptr);
        if (rc) return rc;
    }
    const char* hs = tally_download(ctx, st, total, s, &rc);
    if (!hs) return rc;
    const uint32_t rows = reinterpret_cast<const uint32_t*>(hs)[0];
    out->n = rows;
    tw->guess_dec = std::max<uint32_t>(1024u, rows + rows / 4);
    const uint32_t recs = caught ? reinterpret_cast<const uint32_t*>(hs)[1] : 0u;
    if (caught) {
        caught->n = recs;
        tw->guess_catch = std::max<uint32_t>(1024u, recs + recs / 4);
    }
    if (rows > out->cap || (caught && recs > caught->cap)) return HD_ECAP;
    if (st_dup) memcpy(out->dup, hs + dup_off, n);
    if (st_pclass) memcpy(out->pclass, hs + pc_off, n);
    const uint32_t staged = std::min(rows, H);
    (void)cols_copy(ctx, kDecideCols, hs + rows_off, H, staged, 0, out, copy_host);
    if (ord) {
        memcpy(ord->when, hs + when_off, kWhenRow * staged);
        memcpy(ord->exact_until, hs + until_off, kUntilRow * staged);
    }
    if (caught) (void)cols_copy(ctx, kCatchCols, hs + catch_off, Hc, std::min(recs, Hc), 0, caught, copy_host);
    if (rows > H || recs > Hc) {   // more than staged: the overflow columns, straight into the caller's arrays
        const auto down = copy_down(s);
        if (rows > H) {
            const uint32_t e = rows - H;
            if ((rc = cols_copy(ctx, kDecideCols, ovf, m, e, H, out, down))) return rc;
            if (ord) {
                TCHK(down(ord->when + 8 * (size_t)H, ovf + ovw_off, kWhenRow * e), "decide overflow when");
                TCHK(down(ord->exact_until + H, ovf + ovu_off, kUntilRow * e), "decide overflow until");
            }
        }
        if (recs > Hc && (rc = cols_copy(ctx, kCatchCols, covf, m, recs - Hc, Hc, caught, down))) return rc;
        TCHK(hipStreamSynchronize(s), "decide overflow sync");
    }
    return HD_OK;
}

// hd_decide and hd_decide_ordered (ord non-NULL and checked by the caller)
static int decide_host(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in,
                       hd_decide_out* out, hd_decide_order* ord, hd_catch_out* caught = nullptr) {
    if (!ctx || !batch || !verdict || !in || !decide_out_ok(out)) return HD_EINVAL;
    if (caught) caught->n = 0;
    if (!batch->type || !batch->height || !batch->round || !batch->value32 || !batch->from32) return HD_EINVAL;
    if (in->sched32 && in->n_sched == 0) return HD_EINVAL;
    out->n = 0;
    const uint32_t n = batch->n;
    if (n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    if (!ctx->tally) ctx->tally = new TallyWork();
    hd_batch hb = *batch;
    hb.sig65 = nullptr;  // not needed
    hd_batch db;
    int rc = hd_upload_batch(ctx, &hb, &db);
    if (rc) return rc;
    rc = hd_dev_grow(ctx, &ctx->bufs[BUF_VERDICT].p, &ctx->bufs[BUF_VERDICT].cap, n);
    if (rc) return rc;
    uint8_t* d_v = (uint8_t*)ctx->bufs[BUF_VERDICT].p;
    TCHK(hipMemcpyAsync(d_v, verdict, n, hipMemcpyHostToDevice, ctx->stream), "verdict upload");
    DecideIn di{in->f, in->n_sched, nullptr, nullptr};
    if (in->sched32) {
        uint8_t* p = (uint8_t*)tbuf(ctx, T_SCHED, 32 * (size_t)in->n_sched, &rc);
        if (rc) return rc;
        TCHK(hipMemcpyAsync(p, in->sched32, 32 * (size_t)in->n_sched, hipMemcpyHostToDevice, ctx->stream),
             "schedule upload");
        di.sched32 = p;
    }
    if (in->value_ok) {
        uint8_t* p = (uint8_t*)tbuf(ctx, T_VOK, n, &rc);
        if (rc) return rc;
        TCHK(hipMemcpyAsync(p, in->value_ok, n, hipMemcpyHostToDevice, ctx->stream), "value_ok upload");
        di.value_ok = p;
    }
    return hd_decide_run(ctx, &db, d_v, nullptr, di, out, ctx->stream, ord, nullptr, caught);
}

static int decide_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap, const hd_decide_in* in,
                         hd_decide_out* out, void* stream, hd_decide_order* ord, hd_catch_out* caught = nullptr) {
    if (!ctx || !dbatch || !in || !decide_out_ok(out)) return HD_EINVAL;
    if (caught) caught->n = 0;
    if (dbatch->n && (!d_valid_bitmap || !dbatch->type || !dbatch->height || !dbatch->round || !dbatch->value32 ||
                      !dbatch->from32))
        return HD_EINVAL;
    if (in->sched32 && in->n_sched == 0) return HD_EINVAL;
    out->n = 0;
    if (dbatch->n == 0) return HD_OK;
    (void)hipSetDevice(ctx->device);
    return hd_decide_run(ctx, dbatch, nullptr, d_valid_bitmap, DecideIn{in->f, in->n_sched, in->sched32, in->value_ok},
                         out, stream ? (hipStream_t)stream : ctx->stream, ord, nullptr, caught);
}

extern "C" {

int hd_decide(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in, hd_decide_out* out) {
    return decide_host(ctx, batch, verdict, in, out, nullptr);
}

int hd_decide_ordered(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in,
                      hd_decide_out* out, hd_decide_order* order) {
    if (!decide_order_ok(out, order, batch ? batch->n : 0u)) return HD_EINVAL;
    return decide_host(ctx, batch, verdict, in, out, order);
}

int hd_decide_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                            const hd_decide_in* in, hd_decide_out* out, void* stream) {
    return decide_bitmap(ctx, dbatch, d_valid_bitmap, in, out, stream, nullptr);
}

int hd_decide_ordered_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                    const hd_decide_in* in, hd_decide_out* out, hd_decide_order* order,
                                    void* stream) {
    if (!decide_order_ok(out, order, dbatch ? dbatch->n : 0u)) return HD_EINVAL;
    return decide_bitmap(ctx, dbatch, d_valid_bitmap, in, out, stream, order);
}

int hd_decide_catch(hd_ctx* ctx, const hd_batch* batch, const uint8_t* verdict, const hd_decide_in* in,
                    hd_decide_out* out, hd_decide_order* order, hd_catch_out* caught) {
    if (!catch_out_ok(caught)) return HD_EINVAL;
    if (order && !decide_order_ok(out, order, batch ? batch->n : 0u)) return HD_EINVAL;
    return decide_host(ctx, batch, verdict, in, out, order, caught);
}

int hd_decide_catch_device_bitmap(hd_ctx* ctx, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                  const hd_decide_in* in, hd_decide_out* out, hd_decide_order* order,
                                  hd_catch_out* caught, void* stream) {
    if (!catch_out_ok(caught)) return HD_EINVAL;
    if (order && !decide_order_ok(out, order, dbatch ? dbatch->n : 0u)) return HD_EINVAL;
    return decide_bitmap(ctx, dbatch, d_valid_bitmap, in, out, stream, order, caught);
}

}  // extern "C"
