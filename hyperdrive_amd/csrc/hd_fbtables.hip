// hd_fbtables.hip -- the tables the known-key check (hd_fastverify.hip) runs
// on (hd_fixedbase.h), their slots, widths and foreign keys.
//   k_fb_list / k_fb_bases / k_fb_runs / k_fb_ready
//                   build the tables of newly learned keys (window bases,
//                   then the affine multiples by segments of consecutive
//                   entries, one addition per entry); with nothing learned
//                   each exits at once
// Table memory is capped by HD_FB_MAX_BYTES (default 64 GiB of the 288 GB):
// signatories beyond the cap always take the full recovery.
// G has one table with wider windows (HD_FB_WG bits), built once per device
// and process (fb_g_table).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hd_mathcheck.h"
#include "../../include/hd_verify.h"
#include "hd_fbwork.h"
#include "hd_keycarry.h"
#include "hd_modinv.h"

using namespace hd;

namespace {

__global__ void k_fb_list(uint32_t nslots, const uint32_t* __restrict__ state, uint32_t* __restrict__ list,
                          uint32_t* __restrict__ count) {
    __shared__ uint32_t c;
    if (threadIdx.x == 0) c = 0;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nslots; k += blockDim.x)
        if (state[k] == HD_FB_LEARNED) list[atomicAdd(&c, 1u)] = k;
    __syncthreads();
    if (threadIdx.x == 0) *count = c;
}

template <int W>
__global__ __launch_bounds__(256) void k_fb_bases(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                                                  const ge* __restrict__ pub, ge* __restrict__ base) {
    constexpr int NW = FbL<W>::NWIN;
    const uint32_t total = *count * NW;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const uint32_t slot = list[t / NW], j = t % NW;
        ge o;
        fb_window_base(o, pub[slot], W, (int)j);
        base[(size_t)slot * NW + j] = o;
    }
}

// Table entries by segments of HD_FB_SEG consecutive multiples of one window
// base B: a lane computes the segment's first point d0 B once (double-and-add)
// and walks the rest with one mixed addition each, in blocks of HD_FB_RUN:
// the forward walk keeps each step's z ratio (Z_{k+1} = Z_k zr_k) and parks
// the Jacobian X, Y canonically in the entry's own 64-B table slot; one
// inversion of the block's last Z, then the backward walk makes each entry
// affine (1/Z_k = 1/Z_{k+1} zr_k).  Per entry one addition and ~5 products
// plus a share of one inversion, instead of a double-and-add and an
// inversion per entry (fb_entry, the definition the host tests check).
// The walk never adds B to +-B: its first point is d0 B with d0 >= 2 (d = 1
// is B itself, written directly), so (d0 + k) B = +-B cannot occur.
#define HD_FB_RUN 32
#define HD_FB_SEG 512
#define HD_FB_CHUNK 8   // slots per table allocation (fb_grow_slots)
template <int W>
__global__ __launch_bounds__(256) void k_fb_runs(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                                                 const ge* __restrict__ base, gp* const* __restrict__ tabs,
                                                 uint32_t* __restrict__ zr_scratch) {
    constexpr uint32_t N = FbL<W>::N, NW = FbL<W>::NWIN;
    constexpr uint32_t SW = N / HD_FB_SEG;                                  // segments per full window
    constexpr uint32_t SB = (NW - 1) * SW + FbL<W>::NTOP / HD_FB_SEG;      // segments per base
    static_assert(N % HD_FB_SEG == 0 && FbL<W>::NTOP % HD_FB_SEG == 0 && HD_FB_SEG % HD_FB_RUN == 0, "segments");
    const uint32_t T = gridDim.x * blockDim.x;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t total = (uint64_t)*count * SB;
    for (uint64_t g = tid; g < total; g += T) {
        const uint32_t slot = list[g / SB];
        const uint32_t rem = (uint32_t)(g % SB);
        const uint32_t j = min(rem / SW, NW - 1);
        const uint32_t d0 = 1 + (rem - j * SW) * HD_FB_SEG;
        const ge B = base[(size_t)slot * NW + j];
        gp* out = tabs[slot] + (size_t)j * N + (d0 - 1);
        gej a;
        uint32_t k0 = 0;   // first entry of the segment the walk produces
        if (d0 == 1) {
            gp q;
            gp_pack(q, B);   // bases are canonical affine
            out[0] = q;
            gej b;
            gej_set_ge(b, B);
            gej_dbl(a, b);
            k0 = 1;
        } else {
            fb_mul_small(a, B, d0);
        }
        for (uint32_t blk = 0; blk < HD_FB_SEG; blk += HD_FB_RUN) {
            const uint32_t lo = blk + (blk == 0 ? k0 : 0), hi = blk + HD_FB_RUN;
            HD_NOUNROLL for (uint32_t k = lo; k < hi; k++) {
                if (k > lo) {
                    fe zr;
                    gej_add_ge_zr(a, a, B, zr);
                    HD_UNROLL for (int w = 0; w < 9; w++)
                        zr_scratch[((size_t)(k - 1 - blk) * 9 + w) * T + tid] = zr.n[w];
                }
                fe x = a.x, y = a.y;
                fe_normalize(x);
                fe_normalize(y);
                gp q;
                fe_to_le(q.x, x);
                fe_to_le(q.y, y);
                out[k] = q;
            }
            fe zinv;
            fe_inv_divsteps(zinv, a.z);
            HD_NOUNROLL for (uint32_t k = hi; k-- > lo;) {
                ge p;
                gp_unpack(p, out[k]);
                fe z2, ax, ay;
                fe_sqr(z2, zinv);
                fe_mul(ax, p.x, z2);
                fe_mul(z2, z2, zinv);
                fe_mul(ay, p.y, z2);
                fe_normalize(ax);
                fe_normalize(ay);
                gp q;
                fe_to_le(q.x, ax);
                fe_to_le(q.y, ay);
                out[k] = q;
                if (k > lo) {
                    fe zr;
                    HD_UNROLL for (int w = 0; w < 9; w++) zr.n[w] = zr_scratch[((size_t)(k - 1 - blk) * 9 + w) * T + tid];
                    fe_mul(zinv, zinv, zr);
                }
            }
            // the next block continues the walk from this block's last point
            if (hi < HD_FB_SEG) {
                fe zr;
                gej_add_ge_zr(a, a, B, zr);
            }
        }
    }
}

// One block.  not_ready counts admitted slots only: the foreign block
// [f0, f1) is left out, counted inside the parallel walk (one LDS atomic per
// thread), so a set change that builds 10^5-10^6 admitted tables pays no
// serial walk over the list.
__global__ void k_fb_ready(const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                           uint32_t* __restrict__ state, uint32_t* not_ready, uint32_t f0, uint32_t f1) {
    __shared__ uint32_t sh_admitted;
    const uint32_t c = *count;
    if (threadIdx.x == 0) sh_admitted = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t k = threadIdx.x; k < c; k += blockDim.x) {
        const uint32_t sl = list[k];
        state[sl] = HD_FB_READY;
        mine += (sl >= f0 && sl < f1) ? 0u : 1u;
    }
    if (mine) atomicAdd(&sh_admitted, mine);
    __syncthreads();
    if (threadIdx.x == 0 && c && not_ready) {
        const uint32_t ca = sh_admitted;
        const uint32_t v = *(volatile uint32_t*)not_ready;
        *(volatile uint32_t*)not_ready = v >= ca ? v - ca : 0u;
    }
}

// per-key table geometry of width wp (fb_nwin: hd_fbwork.h)
size_t fb_tab_entries(int wp) {
    return with_width(wp, [](auto w) { return (size_t)FbL<decltype(w)::value>::TAB; });
}
double fb_slot_bytes(int wp) {
    return (double)sizeof(gp) * (double)fb_tab_entries(wp) + (double)sizeof(ge) * (fb_nwin(wp) + 1) + 8;
}

// table bytes held by all contexts of a device (the budget is per device)
std::mutex g_fb_bytes_mutex;
std::map<int, size_t> g_fb_bytes;
void fb_account(hd_ctx* ctx, size_t add, size_t sub) {
    std::lock_guard<std::mutex> lock(g_fb_bytes_mutex);
    size_t& d = g_fb_bytes[ctx->device];
    d = d + add - std::min(d, sub);
    ctx->fb->bytes = ctx->fb->bytes + add - std::min(ctx->fb->bytes, sub);
}
size_t fb_device_bytes(int device) {
    std::lock_guard<std::mutex> lock(g_fb_bytes_mutex);
    return g_fb_bytes[device];
}

void fb_free_tables(hd_ctx* ctx) {
    FbWork* f = ctx->fb;
    for (gp* c : f->chunks) (void)hipFree(c);
    f->chunks.clear();
    void* ptrs[] = {f->tabs, f->base, f->pub, f->state, f->list};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    f->tabs = nullptr;
    f->base = f->pub = nullptr;
    f->state = f->list = nullptr;
    f->nslots = 0;
    fb_account(ctx, 0, f->bytes);
}

// The per-slot arrays for max_slots slots (small: bases, keys, states, table
// pointers), once per table width; no table memory yet.
int fb_alloc_slots(hd_ctx* ctx) {
    FbWork* f = ctx->fb;
    const size_t m = f->max_slots, NWIN = (size_t)fb_nwin(f->wp);
    FBCHK(hipMalloc(&f->tabs, sizeof(gp*) * m), "fb table pointers");
    FBCHK(hipMalloc(&f->base, sizeof(ge) * NWIN * m), "fb bases");
    FBCHK(hipMalloc(&f->pub, sizeof(ge) * m), "fb keys");
    FBCHK(hipMalloc(&f->state, 4 * m), "fb state");
    FBCHK(hipMalloc(&f->list, 4 * m), "fb list");
    FBCHK(hipMemsetAsync(f->state, 0, 4 * m, ctx->stream), "fb state clear");
    FBCHK(hipMemsetAsync(f->tabs, 0, sizeof(gp*) * m, ctx->stream), "fb table pointers clear");
    FBCHK(hipStreamSynchronize(ctx->stream), "fb slot arrays");
    fb_account(ctx, (sizeof(gp*) + sizeof(ge) * (NWIN + 1) + 8) * m, 0);
    return HD_OK;
}

// Table chunks until `want` slots have tables (chunks never move: the slots
// already built keep their tables).
int fb_grow_slots(hd_ctx* ctx, uint32_t want) {
    FbWork* f = ctx->fb;
    want = std::min(want, f->max_slots);
    const size_t TAB = fb_tab_entries(f->wp);
    // test hook: HD_FB_FAIL_WIDTH=w fails every table allocation at width w
    // as the device would when another process took the memory
    // (tests/test_fastpath.py: the narrower-width retry of hd_fb_map_signatories)
    if (const char* fw = getenv("HD_FB_FAIL_WIDTH"))
        if (atoi(fw) == f->wp && f->nslots < want) return hd_ctx_fail(ctx, hipErrorOutOfMemory, "fb table chunk (HD_FB_FAIL_WIDTH)");
    while (f->nslots < want) {
        const uint32_t k = std::min<uint32_t>(HD_FB_CHUNK, f->max_slots - f->nslots);
        gp* c = nullptr;
        FBCHK(hipMalloc(&c, sizeof(gp) * TAB * k), "fb table chunk");
        f->chunks.push_back(c);
        std::vector<gp*> ptr(k);
        for (uint32_t j = 0; j < k; j++) ptr[j] = c + TAB * j;
        FBCHK(hipMemcpyAsync(f->tabs + f->nslots, ptr.data(), sizeof(gp*) * k, hipMemcpyHostToDevice, ctx->stream),
              "fb table pointers");
        FBCHK(hipStreamSynchronize(ctx->stream), "fb table pointers");
        f->nslots += k;
        fb_account(ctx, sizeof(gp) * TAB * k, 0);
    }
    return HD_OK;
}

// k_fb_runs grid (4 blocks per CU) and its z-ratio scratch
uint32_t fb_run_blocks(const hd_ctx* ctx) { return (uint32_t)std::max(ctx->n_cu, 1) * 4u; }
size_t fb_run_scratch_bytes(const hd_ctx* ctx) { return (size_t)HD_FB_RUN * 9 * 4 * 256 * fb_run_blocks(ctx); }

}  // namespace

// a foreign key claimed since the last build (HD_VAR_FOREIGN_KEYS)
bool fb_foreign_pending(const FbWork* f) {
    return f->fcap && f->fpend_host && *(volatile uint32_t*)f->fpend_host != f->fseen;
}

// build the tables of every LEARNED slot, stream-ordered (nothing to launch
// once every mapped key is READY)
int fb_learn(hd_ctx* ctx, hipStream_t s) {
    FbWork* f = ctx->fb;
    const bool fnew = fb_foreign_pending(f);
    if (f->nr_host && *(volatile uint32_t*)f->nr_host == 0 && !fnew && !f->fforce) return HD_OK;
    if (fnew) f->fseen = *(volatile uint32_t*)f->fpend_host;
    f->fforce = false;
    const uint32_t g = (uint32_t)std::max(ctx->n_cu, 1) * 4u;
    k_fb_list<<<1, 256, 0, s>>>(f->nslots, f->state, f->list, f->counts);
    with_width(f->wp, [&](auto w) {
        constexpr int WP = decltype(w)::value;
        k_fb_bases<WP><<<g, 256, 0, s>>>(f->list, f->counts, f->pub, f->base);
        k_fb_runs<WP><<<fb_run_blocks(ctx), 256, 0, s>>>(f->list, f->counts, f->base, f->tabs, f->zr);
    });
    k_fb_ready<<<1, 256, 0, s>>>(f->list, f->counts, f->state, f->nr_dev, f->fbase, f->fbase + f->fres);
    FBCHK(hipGetLastError(), "fb table kernels");
    return HD_OK;
}

// empty the foreign dictionary, its counter and the hit counts (on s; a block whose allocation failed has
// none), and the foreign block's host-side state with them; the context is quiesced, so nothing in flight
// writes fpend_host and the host side need not wait for s
static int fb_foreign_forget(hd_ctx* ctx, hipStream_t s) {
    FbWork* f = ctx->fb;
    if (f->fdict) {
        FBCHK(hipMemsetAsync(f->fdict, 0, 4 * (size_t)HD_FD_WORDS, s), "fb foreign reset");
        FBCHK(hipMemsetAsync(f->fnext, 0, 4, s), "fb foreign reset");
        FBCHK(hipMemsetAsync(f->fhit, 0, 4 * (64 + (size_t)HD_FD_BUCKETS), s), "fb foreign reset");
    }
    ((volatile uint32_t*)f->fpend_host)[0] = 0;
    ((volatile uint32_t*)f->fpend_host)[1] = 0;
    f->fseen = 0;
    f->fwait = 1;
    f->fcalls = 0;
    f->fforce = false;
    return HD_OK;
}

// Foreign-slot eviction.  The fcap foreign slots go to the first Froms whose
// NOT_ADMITTED recovery claims them; later Froms stay in the dictionary
// without a slot (key kept, recoveries counted).  While such recoveries are
// flagged, every fwait-th call (fwait doubling up to HD_FD_EVICT_WAIT_MAX
// while checks change nothing) waits for the context's calls to finish --
// nothing may read a table about to be re-keyed -- and reads the counters:
// the slotless Froms by recoveries since the last check, hottest first, take
// the slots of the READY foreign keys with the fewest known-key checks while
// hot >= 2 cold + 4 (hysteresis: two senders of similar rates do not trade
// places every check).  A demoted From keeps its key and may come back;
// slotless entries without a recovery since the last check leave the
// dictionary (throwaway Froms cannot fill its 128 buckets either).  The
// dictionary is rebuilt on the host and uploaded, the counters restart, and
// the promoted slots (state LEARNED) are built at this call's end
// (fforce).  Verdicts never depend on it: a slot that is not READY sends its
// messages to the full recovery.
#define HD_FD_EVICT_WAIT_MAX 1024u
int fb_evict(hd_ctx* ctx, bool* changed) {
    FbWork* f = ctx->fb;
    *changed = false;
    if (!f->fcap || !f->fhit || !f->fkey || !f->fdict) return HD_OK;
    volatile uint32_t* miss = (volatile uint32_t*)f->fpend_host + 1;
    if (*miss == 0) return HD_OK;
    if (++f->fcalls < f->fwait) return HD_OK;
    f->fcalls = 0;
    int rq = hd_fb_quiesce(ctx);
    if (rq) return rq;
    *miss = 0;
    f->evict_checks++;
    hipStream_t s = ctx->stream;
    const uint32_t B = HD_FD_BUCKETS, R = f->fres;
    std::vector<uint32_t> fd(HD_FD_WORDS), hit(64 + B), st(R);
    std::vector<ge> key(B), pub(R);
    FBCHK(hipMemcpyAsync(fd.data(), f->fdict, 4 * (size_t)HD_FD_WORDS, hipMemcpyDeviceToHost, s), "evict read");
    FBCHK(hipMemcpyAsync(hit.data(), f->fhit, 4 * hit.size(), hipMemcpyDeviceToHost, s), "evict read");
    FBCHK(hipMemcpyAsync(key.data(), f->fkey, sizeof(ge) * B, hipMemcpyDeviceToHost, s), "evict read");
    FBCHK(hipMemcpyAsync(pub.data(), f->pub + f->fbase, sizeof(ge) * R, hipMemcpyDeviceToHost, s), "evict read");
    FBCHK(hipMemcpyAsync(st.data(), f->state + f->fbase, 4 * (size_t)R, hipMemcpyDeviceToHost, s), "evict read");
    FBCHK(hipStreamSynchronize(s), "evict read");
    struct Ent {
        uint32_t from[8];
        uint32_t slot, hits;
        ge key;
        bool moved;
    };
    std::vector<Ent> held, loose;
    for (uint32_t b = 0; b < B; b++) {
        if (fd[b] != 2u) continue;
        Ent e;
        memcpy(e.from, &fd[2 * B + 8 * b], 32);
        e.slot = fd[B + b];
        e.moved = false;
        if (e.slot != 0xFFFFFFFFu && e.slot >= f->fbase && e.slot < f->fbase + R) {
            e.hits = hit[e.slot - f->fbase];
            e.key = pub[e.slot - f->fbase];
            held.push_back(e);
        } else {
            e.slot = 0xFFFFFFFFu;
            e.hits = hit[64 + b];
            e.key = key[b];
            loose.push_back(e);
        }
    }
    std::stable_sort(loose.begin(), loose.end(), [](const Ent& a, const Ent& b) { return a.hits > b.hits; });
    std::vector<Ent*> cold;
    for (Ent& e : held)
        if (st[e.slot - f->fbase] == HD_FB_READY) cold.push_back(&e);   // built slots only: a new one had no chance
    std::stable_sort(cold.begin(), cold.end(), [](const Ent* a, const Ent* b) { return a->hits < b->hits; });
    std::vector<Ent> promoted;
    size_t swaps = 0;
    while (swaps < loose.size() && swaps < cold.size() && loose[swaps].hits >= 2 * cold[swaps]->hits + 4) {
        Ent& hot = loose[swaps];
        Ent* old = cold[swaps];
        hot.slot = old->slot;
        hot.moved = true;
        old->slot = 0xFFFFFFFFu;
        old->moved = true;
        promoted.push_back(hot);
        swaps++;
    }
    // the new dictionary: slot holders first (they always fit: at most 64 of
    // 128 buckets), then the slotless Froms worth keeping
    std::vector<Ent> keep;
    for (const Ent& e : held) keep.push_back(e);
    for (const Ent& e : loose)
        if (e.moved || e.hits > 0) keep.push_back(e);
    std::stable_partition(keep.begin(), keep.end(), [](const Ent& e) { return e.slot != 0xFFFFFFFFu; });
    const bool dropped = keep.size() < held.size() + loose.size();
    // nothing to change: the next check waits twice as long, the counters restart
    const auto unchanged = [&]() -> int {
        f->fwait = std::min(2 * f->fwait, HD_FD_EVICT_WAIT_MAX);
        FBCHK(hipMemsetAsync(f->fhit, 0, 4 * hit.size(), s), "evict counters");
        FBCHK(hipStreamSynchronize(s), "evict counters");
        return HD_OK;
    };
    if (swaps == 0 && !dropped) return unchanged();
    std::vector<uint32_t> nd(HD_FD_WORDS, 0u), efrom(8 * keep.size() + 8), eslot(keep.size() + 1);
    std::vector<int32_t> where(keep.size() + 1);
    for (size_t k = 0; k < keep.size(); k++) {
        memcpy(&efrom[8 * k], keep[k].from, 32);
        eslot[k] = keep[k].slot;
    }
    if (!fdict_rebuild(nd.data(), where.data(), efrom.data(), eslot.data(), (uint32_t)keep.size())) {
        // a slot holder would find no bucket: keep the old dictionary and
        // slots for this pass (fdict_rebuild)
        f->evict_aborts++;
        return unchanged();
    }
    std::vector<ge> nkey(B);
    for (size_t k = 0; k < keep.size(); k++)
        if (where[k] >= 0) nkey[where[k]] = keep[k].key;
    FBCHK(hipMemcpyAsync(f->fdict, nd.data(), 4 * (size_t)HD_FD_WORDS, hipMemcpyHostToDevice, s), "evict write");
    FBCHK(hipMemcpyAsync(f->fkey, nkey.data(), sizeof(ge) * B, hipMemcpyHostToDevice, s), "evict write");
    FBCHK(hipMemsetAsync(f->fhit, 0, 4 * hit.size(), s), "evict counters");
    const uint32_t learned = HD_FB_LEARNED;
    for (const Ent& e : promoted) {
        FBCHK(hipMemcpyAsync(f->pub + e.slot, &e.key, sizeof(ge), hipMemcpyHostToDevice, s), "evict key");
        FBCHK(hipMemcpyAsync(f->state + e.slot, &learned, 4, hipMemcpyHostToDevice, s), "evict state");
    }
    FBCHK(hipStreamSynchronize(s), "evict write");
    f->fwait = swaps ? 1u : std::min(2 * f->fwait, HD_FD_EVICT_WAIT_MAX);
    f->fforce = swaps > 0;
    f->evictions += (uint32_t)swaps;
    *changed = true;
    return HD_OK;
}

// The G table (W = HD_FB_WG) is built once per device and process and shared
// by every context on that device.
static std::mutex g_fb_g_mutex;
static std::map<int, gp*> g_fb_g_tables;

static int fb_g_table(hd_ctx* ctx, const gp** out) {
    std::lock_guard<std::mutex> lock(g_fb_g_mutex);
    auto it = g_fb_g_tables.find(ctx->device);
    if (it != g_fb_g_tables.end()) {
        *out = it->second;
        return HD_OK;
    }
    ge g;
    const uint32_t GX[8] = {0x79BE667Eu, 0xF9DCBBACu, 0x55A06295u, 0xCE870B07u,
                            0x029BFCDBu, 0x2DCE28D9u, 0x59F2815Bu, 0x16F81798u};
    const uint32_t GY[8] = {0x483ADA77u, 0x26A3C465u, 0x5DA4FBFCu, 0x0E1108A8u,
                            0xFD17B448u, 0xA6855419u, 0x9C47D08Fu, 0xFB10D4B8u};
    fe_from_be(g.x, GX);
    fe_from_be(g.y, GY);
    gp* tab = nullptr;
    gp** tp = nullptr;       // the builder's table pointer array: {tab}
    ge *base = nullptr, *pub = nullptr;
    uint32_t* cl = nullptr;  // [0] = list {0}, [1] = count 1
    FBCHK(hipMalloc(&tab, sizeof(gp) * (size_t)FbL<HD_FB_WG>::TAB), "G table");
    FBCHK(hipMalloc(&tp, sizeof(gp*)), "G table pointer");
    FBCHK(hipMalloc(&base, sizeof(ge) * FbL<HD_FB_WG>::NWIN), "G bases");
    FBCHK(hipMalloc(&pub, sizeof(ge)), "G point");
    FBCHK(hipMalloc(&cl, 8), "G list");
    const uint32_t hl[2] = {0u, 1u};
    hipStream_t s = ctx->stream;
    FBCHK(hipMemcpyAsync(pub, &g, sizeof(ge), hipMemcpyHostToDevice, s), "G point");
    FBCHK(hipMemcpyAsync(cl, hl, 8, hipMemcpyHostToDevice, s), "G list");
    FBCHK(hipMemcpyAsync(tp, &tab, sizeof(gp*), hipMemcpyHostToDevice, s), "G table pointer");
    k_fb_bases<HD_FB_WG><<<1, 64, 0, s>>>(cl, cl + 1, pub, base);
    k_fb_runs<HD_FB_WG><<<fb_run_blocks(ctx), 256, 0, s>>>(cl, cl + 1, base, tp, ctx->fb->zr);
    FBCHK(hipGetLastError(), "G table kernels");
    FBCHK(hipStreamSynchronize(s), "G table build");
    (void)hipFree(base);
    (void)hipFree(pub);
    (void)hipFree(cl);
    (void)hipFree(tp);
    g_fb_g_tables[ctx->device] = tab;
    *out = tab;
    return HD_OK;
}

int hd_fb_init(hd_ctx* ctx) {
    if (ctx->fb) return HD_OK;
    ctx->fb = new (std::nothrow) FbWork();
    if (!ctx->fb) return HD_ENOMEM;
    FbWork* f = ctx->fb;
    // the device's table budget: HD_FB_MAX_BYTES, else 64 GiB -- room for
    // the headline's 100 signatories at 20 bits beside the G table and
    // everything else the process keeps resident (its batches, torch's
    // cache, more contexts).  A budget of 3/4 of the device (216 GB: 22-bit
    // tables for 100 keys, one addition fewer) measured the same headline
    // within noise and starved the process's other allocations; a replica
    // that owns its GPU may still set it.
    f->budget = 64.0 * (1ull << 30);
    if (const char* m = getenv("HD_FB_MAX_BYTES")) f->budget = atof(m);
    if (const char* l = getenv("HD_INV_LEVELS")) f->inv_levels = atoi(l) == 1 ? 1 : 2;
    if (const char* k2 = getenv("HD_INV_K2")) f->inv_k2 = atoi(k2) == 8 ? 8 : 16;
    f->max_slots = (uint32_t)std::max(1.0, std::min(1e6, f->budget / fb_slot_bytes(f->wp)));
    FBCHK(hipMalloc(&f->counts, 8), "fb counts");
    FBCHK(hipMalloc(&f->zr, fb_run_scratch_bytes(ctx)), "fb builder scratch");
    FBCHK(hipHostMalloc((void**)&f->nr_host, 4, hipHostMallocMapped | hipHostMallocCoherent), "fb ready count");
    *f->nr_host = 0xFFFFFFFFu;
    FBCHK(hipHostGetDevicePointer((void**)&f->nr_dev, f->nr_host, 0), "fb ready count map");
    FBCHK(hipHostMalloc((void**)&f->est_host, 16, hipHostMallocMapped | hipHostMallocCoherent), "fb list estimate");
    f->est_host[0] = f->est_host[1] = f->est_host[2] = f->est_host[3] = 0xFFFFFFFFu;
    FBCHK(hipHostGetDevicePointer((void**)&f->est_dev, f->est_host, 0), "fb list estimate map");
    FBCHK(hipHostMalloc((void**)&f->fpend_host, 8, hipHostMallocMapped | hipHostMallocCoherent), "fb foreign claims");
    f->fpend_host[0] = f->fpend_host[1] = 0;
    FBCHK(hipHostGetDevicePointer((void**)&f->fpend_dev, f->fpend_host, 0), "fb foreign claims map");
    FBCHK(hipMalloc(&f->dstats, 16), "fb repeat counters");
    FBCHK(hipMemset(f->dstats, 0, 16), "fb repeat counters clear");   // (blocking: calls on any stream add to it)
    FBCHK(hipMalloc(&f->pstats, 16), "fb preimage counters");
    FBCHK(hipMemset(f->pstats, 0, 16), "fb preimage counters clear");
    int rc = fb_alloc_slots(ctx);
    if (rc) return rc;
    return fb_g_table(ctx, &f->gtab);
}

const gp* hd_fb_gtab(const hd_ctx* ctx) { return ctx && ctx->fb ? ctx->fb->gtab : nullptr; }

void hd_fb_release(hd_ctx* ctx) {
    if (!ctx || !ctx->fb) return;
    FbWork* f = ctx->fb;
    fb_free_tables(ctx);
    if (f->done) (void)hipEventDestroy(f->done);
    if (f->sums.done) (void)hipEventDestroy(f->sums.done);
    for (hipEvent_t e : f->ev_call) (void)hipEventDestroy(e);
    for (hipEvent_t e : f->ev_sums) (void)hipEventDestroy(e);
    for (auto& sc : f->sc) {
        if (sc.done) (void)hipEventDestroy(sc.done);
        void* sp[] = {sc.rows, sc.slow, sc.count, sc.slow2, sc.dtab, sc.pre, sc.roots};
        for (void* p : sp)
            if (p) (void)hipFree(p);
    }
    void* ptrs[] = {f->counts, f->adm_slot, f->zr, f->fdict, f->fnext, f->fhit, f->fkey, f->dstats, f->pstats};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (f->nr_host) (void)hipHostFree(f->nr_host);
    if (f->est_host) (void)hipHostFree(f->est_host);
    if (f->fpend_host) (void)hipHostFree(f->fpend_host);
    delete f;
    ctx->fb = nullptr;
}

// Per-key window width for an admitted set of m: the widest tables
// (HD_FB_WX, 12 windows of u2, 1.48 GB per key) when all m keys and the
// foreign-key block fit the device's table budget next to what other contexts
// hold; else the wide ones (HD_FB_WW, 13 windows, 407 MB) when the m keys do;
// else the 16-bit
// ones (16 windows, 36 MB) when all m keys fit the context's budget; else the
// narrow ones (HD_FB_WN, 20 windows, 5 MB), so that thousands of signatories
// still take the known-key check instead of the full recovery (a key
// without a slot costs ~10x per message).  HD_VAR_KEY_WIDTH forces one.
// The table bytes the device can still give this context: its free memory
// (other processes' allocations included) plus what this context holds.
static double fb_free_cap(hd_ctx* ctx) {
    size_t fr = 0, tot = 0;
    (void)hipSetDevice(ctx->device);
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 1e300;
    return 0.9 * (double)fr + (double)ctx->fb->bytes;
}

// (cap: the widest width allowed, 0 = any; hd_fb_map_signatories narrows it
// when an allocation fails)
static int fb_pick_width(hd_ctx* ctx, uint32_t m, int cap) {
    if (ctx->var[HD_VAR_KEY_WIDTH]) return ctx->var[HD_VAR_KEY_WIDTH];
    FbWork* f = ctx->fb;
    const double others = (double)(fb_device_bytes(ctx->device) - std::min(fb_device_bytes(ctx->device), f->bytes));
    const double free_cap = fb_free_cap(ctx);
    const double shared = std::min(f->budget - others, free_cap);
    // (+ the foreign-key block's slots)
    const double slots = (double)m + 1 + (ctx->var[HD_VAR_FOREIGN_KEYS] > 0 ? ctx->var[HD_VAR_FOREIGN_KEYS] : 0);
    const auto allowed = [cap](int w) { return cap == 0 || w <= cap; };
    if (allowed(HD_FB_WX) && fb_slot_bytes(HD_FB_WX) * slots <= shared) return HD_FB_WX;
    if (allowed(HD_FB_WW) && fb_slot_bytes(HD_FB_WW) * ((double)m + 1) <= shared) return HD_FB_WW;
    if (allowed(HD_FB_W) && fb_slot_bytes(HD_FB_W) * slots <= std::min(f->budget, free_cap)) return HD_FB_W;
    return HD_FB_WN;
}

// mapped slots whose state is not READY (device idle: called after a sync)
static int fb_count_not_ready(hd_ctx* ctx) {
    FbWork* f = ctx->fb;
    uint32_t nr = 0;
    if (!f->slot_of.empty()) {
        std::vector<uint32_t> st(f->nslots);
        FBCHK(hipMemcpyAsync(st.data(), f->state, 4 * (size_t)f->nslots, hipMemcpyDeviceToHost, ctx->stream),
              "fb state read");
        FBCHK(hipStreamSynchronize(ctx->stream), "fb state read");
        for (const auto& kv : f->slot_of) nr += st[kv.second] != HD_FB_READY ? 1u : 0u;
    }
    *(volatile uint32_t*)f->nr_host = nr;
    return HD_OK;
}

// What hd_fb_map_signatories knew at its entry, before its first attempt
// (hd_keycarry.h): the signatories with a slot, sorted, and every slot's
// state.  A failed attempt leaves slot_of with slots of departed signatories
// handed to new ones while their states still say READY, so this copy -- never
// slot_of -- is what a later attempt of the same call carries keys from.
struct FbSnapshot {
    std::vector<uint8_t> sig32;
    std::vector<uint32_t> slot, state;
    uint32_t f0 = 0, f1 = 0;
    uint32_t known = 0, staying = 0;   // its known keys, and those whose signatory is in the new set
    bool carry = false;     // the context picks its own width: known keys cross a re-tier
    bool gathered = false;   // stash holds the keys (the first attempt that frees the tables gathers)
    FbKeyStash stash;
    KeySnapshot view() const {
        return KeySnapshot{sig32.data(), slot.data(), (uint32_t)slot.size(), state.data(), (uint32_t)state.size(), f0, f1};
    }
};

static int fb_snapshot(hd_ctx* ctx, FbSnapshot& sn) {
    FbWork* f = ctx->fb;
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    sn.carry = ctx->var[HD_VAR_KEY_WIDTH] == 0;
    // (after a failed mapping nothing is known: it forgot the keys)
    if (!f->map_ok || !f->state || !f->pub || f->nslots < 2 || f->slot_of.empty()) return HD_OK;
    std::vector<std::pair<std::string, uint32_t>> rows(f->slot_of.begin(), f->slot_of.end());
    std::sort(rows.begin(), rows.end());
    sn.sig32.resize(32 * rows.size());
    sn.slot.resize(rows.size());
    for (size_t r = 0; r < rows.size(); r++) {
        memcpy(&sn.sig32[32 * r], rows[r].first.data(), 32);
        sn.slot[r] = rows[r].second;
    }
    sn.f0 = f->fbase;
    sn.f1 = f->fbase + f->fres;
    sn.state.resize(f->nslots);
    FBCHK(hipMemcpyAsync(sn.state.data(), f->state, 4 * (size_t)f->nslots, hipMemcpyDeviceToHost, ctx->stream),
          "fb state snapshot");
    FBCHK(hipStreamSynchronize(ctx->stream), "fb state snapshot");
    return HD_OK;
}

static int fb_map(hd_ctx* ctx, const uint8_t* sorted, uint32_t m, int cap, FbSnapshot& sn);

// HD_FB_TRACE=1: one stderr line per table-mapping attempt (debug aid)
static bool fb_trace() {
    static const bool on = getenv("HD_FB_TRACE") != nullptr;
    return on;
}

// One table mapping at a time per device: the width pick reads the bytes
// the device's other contexts hold and its free memory, so contexts mapping
// concurrently (hd_multi's per-device threads over one GPU) would each count
// the memory the others are about to take and oversubscribe the device.
static std::mutex g_fb_map_mutex[64];

// Map the admitted set to table slots.  A table allocation the device
// cannot serve (another process took the memory since the width was picked)
// retries at the next width below the one that failed, down to 13 bits,
// instead of failing the set change.  The keys known at entry (the snapshot)
// survive every attempt that ends in a successful mapping.
int hd_fb_map_signatories(hd_ctx* ctx, const uint8_t* sorted, uint32_t m) {
    std::lock_guard<std::mutex> lock(g_fb_map_mutex[(unsigned)ctx->device % 64u]);
    FbWork* f = ctx->fb;
    FbSnapshot sn;
    int rc = fb_snapshot(ctx, sn);
    if (!rc) key_snap_count(sn.view(), sorted, m, sn.known, sn.staying);
    // (until an attempt succeeds: every known key is lost)
    f->change = hd_set_change_info{f->wp, f->wp, 0, 0, sn.known};
    for (int cap = 0; rc == HD_OK || cap;) {   // (a failed snapshot: no attempt)
        if (fb_trace()) {
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            fprintf(stderr, "[fb] ctx %p m %u cap %d: wp %d nslots %u used %u max %u bytes %.2fG dev %.2fG free %.2fG\n",
                    (void*)ctx, m, cap, ctx->fb->wp, ctx->fb->nslots, ctx->fb->used, ctx->fb->max_slots,
                    ctx->fb->bytes / 1e9, fb_device_bytes(ctx->device) / 1e9, fr / 1e9);
        }
        rc = fb_map(ctx, sorted, m, cap, sn);
        if (fb_trace())
            fprintf(stderr, "[fb] ctx %p -> rc %d wp %d nslots %u used %u %s\n", (void*)ctx, rc, ctx->fb->wp,
                    ctx->fb->nslots, ctx->fb->used, rc ? ctx->last_error.c_str() : "");
        if (rc != HD_ENOMEM || ctx->var[HD_VAR_KEY_WIDTH]) break;
        (void)hipGetLastError();   // the failed allocation must not surface in a later launch check
        // the next width below the one that just failed: every retry is narrower
        const int failed = f->wp;
        cap = failed > HD_FB_WW ? HD_FB_WW : failed > HD_FB_W ? HD_FB_W : failed > HD_FB_WN ? HD_FB_WN : 0;
        if (!cap) break;
    }
    hd_key_stash_free(&sn.stash);
    // a set change that failed here leaves slots mapped without tables (and
    // the device's slot map of the previous set): until a mapping succeeds,
    // every message takes the full recovery against the new admitted set
    f->map_ok = rc == HD_OK;
    f->change.width_after = f->wp;
    if (!f->map_ok && f->state) {
        // and it forgets the keys: its attempts handed slots of departed
        // signatories to new ones without resetting their states
        (void)hipMemsetAsync(f->state, 0, 4 * (size_t)f->max_slots, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipGetLastError();
    }
    return rc;
}

static int fb_map(hd_ctx* ctx, const uint8_t* sorted, uint32_t m, int cap, FbSnapshot& sn) {
    FbWork* f = ctx->fb;
    // no verify call of this context may still learn into a slot reassigned
    // here (hd_set_signatories quiesced the context already)
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    *(volatile uint32_t*)f->nr_host = 0xFFFFFFFFu;
    const int wp = fb_pick_width(ctx, m, cap);
    const bool retier = wp != f->wp;
    std::vector<int32_t> adm_slot(std::max(m, 1u), -1);
    std::vector<uint32_t> fresh;
    KeyCarryPlan plan;
    if (retier) {
        // Another table width: the tables go, and the key and state arrays
        // with them.  When the context picks its own width the keys known at
        // the call's entry cross this step in a stash of their own, gathered
        // once, before the first free; with a forced width (HD_VAR_KEY_WIDTH)
        // every key is learned again (full recovery).
        if (sn.carry && !sn.gathered && !sn.slot.empty()) {
            const FbKeyView old{f->state, f->pub, nullptr, (uint32_t)sn.state.size()};
            int rg = hd_key_stash_gather(ctx, sn.slot.data(), (uint32_t)sn.slot.size(), old, sn.f0, sn.f1, &sn.stash);
            if (rg) return rg;
            sn.gathered = true;
        }
        fb_free_tables(ctx);
        f->slot_of.clear();
        f->free_slots.clear();
        f->used = 1;
        f->fcap = f->fres = 0;   // the foreign block goes with the tables
        f->wp = wp;
        f->max_slots =
            (uint32_t)std::max(1.0, std::min(1e6, std::min(f->budget, fb_free_cap(ctx)) / fb_slot_bytes(wp)));
        int ra = fb_alloc_slots(ctx);
        if (ra) return ra;
    }
    if (retier && sn.gathered) {
        // the carried signatories take slots first (hd_keycarry.h); every
        // state is EMPTY already (fb_alloc_slots)
        key_carry_plan(sn.view(), sorted, m, f->max_slots, plan);
        adm_slot = plan.adm_slot;
        for (uint32_t k = 0; k < m; k++)
            if (adm_slot[k] >= 0)
                f->slot_of.emplace(std::string(reinterpret_cast<const char*>(sorted + 32 * (size_t)k), 32),
                                   (uint32_t)adm_slot[k]);
        f->used = plan.used;
    } else {
        std::unordered_map<std::string, uint32_t> keep;
        for (uint32_t k = 0; k < m; k++) {
            std::string key(reinterpret_cast<const char*>(sorted + 32 * (size_t)k), 32);
            auto it = f->slot_of.find(key);
            if (it != f->slot_of.end()) {
                adm_slot[k] = (int32_t)it->second;
                keep.emplace(key, it->second);
                f->slot_of.erase(it);
            }
        }
        // signatories no longer admitted give their slots back
        for (auto& kv : f->slot_of) {
            f->free_slots.push_back(kv.second);
            fresh.push_back(kv.second);
        }
        f->slot_of.swap(keep);
        for (uint32_t k = 0; k < m; k++) {
            if (adm_slot[k] >= 0) continue;
            uint32_t slot;
            if (!f->free_slots.empty()) {
                slot = f->free_slots.back();
                f->free_slots.pop_back();
            } else if (f->used < f->max_slots) {
                slot = f->used++;
            } else {
                continue;  // over the slot cap: this signatory always takes the full recovery
            }
            adm_slot[k] = (int32_t)slot;
            f->slot_of.emplace(std::string(reinterpret_cast<const char*>(sorted + 32 * (size_t)k), 32), slot);
            fresh.push_back(slot);
        }
    }
    // foreign keys: a block of slots reserved once, after the admitted ones
    // of the first set that asks for it; emptied (dictionary and states) on
    // every set change -- a From that leaves or joins the set is learned again
    const uint32_t want = (uint32_t)std::max(0, ctx->var[HD_VAR_FOREIGN_KEYS]);
    if (want && !f->fres && f->used + want <= f->max_slots) {
        f->fbase = f->used;
        f->fres = want;
        f->used += want;
    }
    f->fcap = std::min(want, f->fres);   // 0: no foreign learning until a set change asks again
    int rc = fb_grow_slots(ctx, f->used);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    for (uint32_t slot : fresh) FBCHK(hipMemsetAsync(f->state + slot, 0, 4, s), "fb slot reset");
    if (f->fres) {
        if (!f->fdict) FBCHK(hipMalloc(&f->fdict, 4 * (size_t)HD_FD_WORDS), "fb foreign dictionary");
        if (!f->fnext) FBCHK(hipMalloc(&f->fnext, 4), "fb foreign count");
        if (!f->fhit) FBCHK(hipMalloc(&f->fhit, 4 * (64 + (size_t)HD_FD_BUCKETS)), "fb foreign hits");
        if (!f->fkey) FBCHK(hipMalloc(&f->fkey, sizeof(ge) * HD_FD_BUCKETS), "fb foreign keys");
        rc = fb_foreign_forget(ctx, s);
        if (rc) return rc;
        FBCHK(hipMemsetAsync(f->state + f->fbase, 0, 4 * (size_t)f->fres, s), "fb foreign reset");
    }
    rc = hd_dev_grow(ctx, (void**)&f->adm_slot, &f->cap_adm_slot, 4 * adm_slot.size());
    if (rc) return rc;
    FBCHK(hipMemcpyAsync(f->adm_slot, adm_slot.data(), 4 * adm_slot.size(), hipMemcpyHostToDevice, s), "fb adm_slot");
    FBCHK(hipStreamSynchronize(s), "fb map");
    if (!plan.carry.empty()) {
        // the carried keys into their new slots (after the resets above), and
        // their tables at the new width before the call returns: the next
        // verify call finds them READY and launches no builder kernel for them
        const FbKeyView now{f->state, f->pub, f->adm_slot, f->nslots};
        rc = hd_key_stash_carry(ctx, sn.stash, plan.carry.data(), (uint32_t)plan.carry.size(), now);
        if (!rc) rc = fb_learn(ctx, s);   // (nr_host is UINT32_MAX: the build runs)
        if (rc) return rc;
        FBCHK(hipStreamSynchronize(s), "fb key carry");
    }
    rc = fb_count_not_ready(ctx);
    if (rc) return rc;
    f->change.kept = retier ? 0 : sn.staying;
    f->change.carried = plan.carried;
    f->change.dropped = sn.known - f->change.kept - f->change.carried;
    return HD_OK;
}

int hd_fb_clear_keys(hd_ctx* ctx) {
    FbWork* f = ctx->fb;
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    if (f->nslots > 1) FBCHK(hipMemsetAsync(f->state + 1, 0, 4 * (size_t)(f->nslots - 1), ctx->stream), "fb clear");
    if (f->fres) {   // the foreign keys are learned again too
        int rf = fb_foreign_forget(ctx, ctx->stream);
        if (rf) return rf;
    }
    FBCHK(hipStreamSynchronize(ctx->stream), "fb clear");
    return fb_count_not_ready(ctx);
}

bool hd_fb_key_view(const hd_ctx* ctx, FbKeyView* v) {
    const FbWork* f = ctx->fb;
    if (!f || !ctx->n_adm || !f->adm_slot || !f->map_ok || !f->state || !f->pub) return false;
    *v = FbKeyView{f->state, f->pub, f->adm_slot, f->nslots};
    return true;
}

int hd_fb_learn_sync(hd_ctx* ctx) {
    int rc = fb_learn(ctx, ctx->stream);
    if (rc) return rc;
    FBCHK(hipStreamSynchronize(ctx->stream), "fb key import");
    return fb_count_not_ready(ctx);
}

extern "C" {

int hd_ctx_foreign_stats(hd_ctx* ctx, uint32_t* ready_slots, uint32_t* evictions, uint32_t* checks) {
    if (!ctx) return HD_EINVAL;
    if (ready_slots) *ready_slots = 0;
    if (evictions) *evictions = 0;
    if (checks) *checks = 0;
    if (!ctx->fb) return HD_OK;
    (void)hipSetDevice(ctx->device);
    FbWork* f = ctx->fb;
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    if (ready_slots && f->fres) {
        std::vector<uint32_t> st(f->fres);
        FBCHK(hipMemcpy(st.data(), f->state + f->fbase, 4 * (size_t)f->fres, hipMemcpyDeviceToHost), "state read");
        for (uint32_t v : st) *ready_slots += v == HD_FB_READY;
    }
    if (evictions) *evictions = f->evictions;
    if (checks) *checks = f->evict_checks;
    return HD_OK;
}

int hd_ctx_fastpath_stats(hd_ctx* ctx, uint32_t* known_keys, uint32_t* last_fallback) {
    if (!ctx) return HD_EINVAL;
    if (known_keys) *known_keys = 0;
    if (last_fallback) *last_fallback = 0;
    if (!ctx->fb) return HD_OK;
    (void)hipSetDevice(ctx->device);
    FbWork* f = ctx->fb;
    int rq = hd_ctx_quiesce(ctx);
    if (rq) return rq;
    if (known_keys && f->nslots > 1) {
        std::vector<uint32_t> st(f->nslots);
        FBCHK(hipMemcpy(st.data(), f->state, 4 * (size_t)f->nslots, hipMemcpyDeviceToHost), "state read");
        for (uint32_t k = 1; k < f->nslots; k++)   // admitted keys (not the foreign block)
            *known_keys += st[k] == HD_FB_READY && !(k >= f->fbase && k < f->fbase + f->fres);
    }
    if (last_fallback && f->last_set >= 0)
        FBCHK(hipMemcpy(last_fallback, f->sc[f->last_set].count, 4, hipMemcpyDeviceToHost), "fallback read");
    return HD_OK;
}

int hd_ctx_set_change_info(hd_ctx* ctx, hd_set_change_info* out) {
    if (!ctx || !out) return HD_EINVAL;
    *out = ctx->fb && ctx->fastpath ? ctx->fb->change : hd_set_change_info{0, 0, 0, 0, 0};
    return HD_OK;
}

// Test surface only (include/hd_mathcheck.h): table entries as the builder
// left them, copied to the host.  No kernel, nothing queued: the call waits
// for the context's work and reads.
int hd_fb_table_read(hd_ctx* ctx, int32_t which, uint64_t first, uint32_t count, uint8_t* out64, int* width,
                     uint32_t* state, uint8_t* key64) {
    if (!ctx || !ctx->fb || which < -1 || (count && !out64)) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    FbWork* f = ctx->fb;
    int rq = hd_fb_quiesce(ctx);
    if (rq) return rq;
    FBCHK(hipStreamSynchronize(ctx->stream), "table read sync");
    const gp* tab = nullptr;
    uint64_t entries = 0;
    uint32_t st = HD_FB_READY;
    int w = HD_FB_WG;
    gp key;
    if (which < 0) {
        ge g;
        const uint32_t GX[8] = {0x79BE667Eu, 0xF9DCBBACu, 0x55A06295u, 0xCE870B07u,
                                0x029BFCDBu, 0x2DCE28D9u, 0x59F2815Bu, 0x16F81798u};
        const uint32_t GY[8] = {0x483ADA77u, 0x26A3C465u, 0x5DA4FBFCu, 0x0E1108A8u,
                                0xFD17B448u, 0xA6855419u, 0x9C47D08Fu, 0xFB10D4B8u};
        fe_from_be(g.x, GX);
        fe_from_be(g.y, GY);
        gp_pack(key, g);
        tab = f->gtab;
        entries = FbL<HD_FB_WG>::TAB;
        if (!tab) return HD_EINVAL;
    } else {
        if ((uint32_t)which >= ctx->n_adm || !f->adm_slot || !f->map_ok) return HD_EINVAL;
        int32_t slot = -1;
        FBCHK(hipMemcpy(&slot, f->adm_slot + which, 4, hipMemcpyDeviceToHost), "slot read");
        if (slot < 1 || (uint32_t)slot >= f->nslots) return HD_EINVAL;   // over the slot cap: no table
        w = f->wp;
        entries = fb_tab_entries(w);
        FBCHK(hipMemcpy(&st, f->state + slot, 4, hipMemcpyDeviceToHost), "state read");
        gp* t = nullptr;
        FBCHK(hipMemcpy(&t, f->tabs + slot, sizeof(gp*), hipMemcpyDeviceToHost), "table pointer read");
        tab = t;
        memset(&key, 0, sizeof(key));
        if (st == HD_FB_LEARNED || st == HD_FB_READY) {
            ge p;
            FBCHK(hipMemcpy(&p, f->pub + slot, sizeof(ge), hipMemcpyDeviceToHost), "key read");
            fe_normalize(p.x);
            fe_normalize(p.y);
            gp_pack(key, p);
        }
    }
    if (width) *width = w;
    if (state) *state = st;
    if (key64) memcpy(key64, &key, 64);
    if (first > entries || count > entries - first) return HD_EINVAL;
    if (count && st == HD_FB_READY) {
        if (!tab) return HD_EINVAL;
        FBCHK(hipMemcpy(out64, tab + first, sizeof(gp) * (size_t)count, hipMemcpyDeviceToHost), "table read");
    }
    return HD_OK;
}

}  // extern "C"
