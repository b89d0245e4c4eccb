// hd_log.hip -- a height's vote and propose logs retained on the device
// across decide calls (include/hd_log.h).
//
// The log is a structure of arrays in HBM holding, in arrival order, the
// messages the reference keeps in ProposeLogs / PrevoteLogs / PrecommitLogs
// (every logged vote and logged propose of the height).  One insert of a batch
// of n messages behind L retained entries:
//
//   k_log_append   one lane per joined position: a new message's fields are
//                  copied behind the retained entries (positions L .. L+n-1)
//                  and every position gets its verdict byte -- a retained entry
//                  is VALID, a new message only when its verdict / bitmap bit
//                  says so and its height is the log's -- and value_ok byte
//   hd_decide_run  the ordered decide passes over the L + n items
//                  (hd_tally.hip), with dup / pclass left on the device; the
//                  catch list, when asked for, is in these joined coordinates
//                  as it leaves the decide
//   k_log_count    per block of 256 joined positions: how many retained
//                  entries came out logged again and how many new messages are
//                  kept (dup == 0 or pclass == 0); ballot / popcount per
//                  wavefront, the block's two totals through LDS
//   k_log_keep     a stable compaction of the kept new messages: a block's
//                  offset is the sum of the preceding blocks' totals (as
//                  k_tally_emit sums its offsets: no ticket, no device-scope
//                  release), a lane's the ballot prefix inside its wavefront
//                  plus the wavefronts before it.  Kept rows go to a second
//                  buffer -- compacting in place would let one block overwrite
//                  rows another has not read -- and k_log_commit copies them back
//                  behind the retained entries once the host has accepted the
//                  insert (stream-ordered before the next call).  The
//                  pass also fills logpos and gathers the batch's dup / pclass
//                  bytes next to it, so the insert downloads one small block.
//
// The host reads [kept, relogged | logpos | dup | pclass] from a pinned stage
// after the decide's one synchronisation (a class the caller passes NULL for
// is left out of the block: it is neither gathered nor downloaded); the log's length moves only after
// every check has passed, so any error leaves the log as it was.
//
// A log that keeps signatures (hd_log_keep_signatures) has an eighth column of
// 65 bytes per row.  k_log_append copies the batch's signatures into the joined
// rows with the other fields, so from there on a signature is one more column:
// k_log_keep compacts it, k_log_commit moves it, and every later reader finds
// the whole message of joined position q in row q, retained or new.
//
//   k_log_gather    hd_log_read: one lane per asked position packs that row's
//                   fields into one record of a device stage, which the host
//                   downloads in one copy and spreads over the caller's columns
//   k_log_evidence  hd_log_insert_evidence: the same packing for both messages
//                   of every catch record, queued behind the decide's passes
//                   (the records are read where k_catch_emit left them, their
//                   count from the stage header); record k fills records 2k
//                   and 2k + 1 of the evidence block, which follows the classes
//                   in the stage and comes down with them
//
// hd_log_select reads the retained entries by key (type, round range, value,
// From; hd_logselect.h holds the predicate and the rank arithmetic, which
// tests/native/hd_logselect_check.cpp replays on the host).  One lane per
// position of [pos_lo, min(pos_hi, L)), blocks of 256, two passes in the shape
// of k_log_count / k_log_keep:
//
//   k_log_sel_count  each block's number of matching entries
//   k_log_sel_emit   match number j, in ascending position, goes to slot j: a
//                    block's offset is the sum of the preceding blocks' counts
//                    (no ticket, no device-scope release), a lane's slot that
//                    plus the wavefronts before it plus its ballot prefix.  A
//                    lane stores only below min(limit or infinity, cap).  The
//                    host form packs one record per slot (pack_row's layout,
//                    the position in the record's last word); the device form
//                    scatters the row into the caller's columns.  The last
//                    block leaves [total, n] in the stage header.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "../../include/hd_log.h"
#include "hd_internal.h"
#include "hd_logselect.h"

using namespace hd;

#define HD_LOG_NOT_CANDIDATE 0xFFu   // verdict byte of a new message that is not VALID or not of the log's height

struct LogCols {
    uint8_t* type;
    int64_t* height;
    int64_t* round;
    int64_t* vround;
    uint8_t* value32;
    uint8_t* from32;
    uint8_t* vok;
    uint8_t* sig;   // 65 bytes per row; NULL on a log that keeps no signatures
};
static const size_t kLogWidth[8] = {1, 8, 8, 8, 32, 32, 1, 65};
static void** log_col(LogCols& c, int k) {
    void** p[8] = {(void**)&c.type, (void**)&c.height, (void**)&c.round, (void**)&c.vround,
                   (void**)&c.value32, (void**)&c.from32, (void**)&c.vok, (void**)&c.sig};
    return p[k];
}

// One message packed for the host (k_log_gather, k_log_evidence): 8-byte fields
// first, so a record at a multiple of 8 bytes is written with aligned stores.
enum : uint32_t {
    ROW_HEIGHT = 0, ROW_ROUND = 8, ROW_VROUND = 16, ROW_VALUE = 24, ROW_FROM = 56, ROW_TYPE = 88, ROW_VOK = 89,
    ROW_SIG = 90, ROW_BYTES = 96, ROW_BYTES_SIG = 160
};
static_assert(ROW_SIG + 65 <= ROW_BYTES_SIG && ROW_BYTES % 8 == 0 && ROW_BYTES_SIG % 8 == 0, "packed row");

struct hd_log {
    hd_ctx* ctx = nullptr;
    int device = 0;
    int64_t height = 0;
    uint32_t f = 0, n_sched = 0, max_entries = 0;
    uint32_t L = 0;               // retained entries
    uint8_t* d_sched = nullptr;
    size_t cap_sched = 0;
    LogCols lg{};                 // retained entries, then the call's batch: cap_items rows
    size_t cap_items = 0;
    DevBuf vd, dup, pclass;       // per joined position: verdict and the decide's classes
    LogCols tmp{};                // the kept rows of one insert: cap_new rows
    size_t cap_new = 0;
    DevBuf blk;                   // two totals per block of 256 joined positions
    DevBuf res;                   // [kept, relogged .. 64 B | logpos 4n | dup n | pclass n], the classes when taken
    DevBuf in_vok;                // the host form's uploaded value_ok
    char* host = nullptr;         // pinned image of res
    size_t host_cap = 0;
    bool keep_sig = false;        // hd_log_keep_signatures
    uint32_t guess_ev = 256;      // records of evidence staged with the classes; more take a second copy
    DevBuf pos;                   // hd_log_read: the asked positions
    hipStream_t commit_stream = nullptr;   // the caller's stream the last k_log_commit went on, if it was one
    DevBuf sel_blk;               // hd_log_select: one count per block of 256 looked-at positions
    uint32_t guess_sel = 256;     // records of a selection staged with its header; more take a second copy
    hipEvent_t sel_ev = nullptr;  // orders a selection on a caller's stream after the context's stream
};

__device__ __forceinline__ void copy_row(const LogCols& dst, size_t j, const uint8_t* type, const int64_t* height,
                                         const int64_t* round, const int64_t* vround, const uint8_t* value32,
                                         const uint8_t* from32, size_t i) {
    dst.type[j] = type[i];
    dst.height[j] = height[i];
    dst.round[j] = round[i];
    dst.vround[j] = vround ? vround[i] : -1;
    const uint4* v = reinterpret_cast<const uint4*>(value32 + 32 * i);
    const uint4* f = reinterpret_cast<const uint4*>(from32 + 32 * i);
    uint4* dv = reinterpret_cast<uint4*>(dst.value32 + 32 * j);
    uint4* df = reinterpret_cast<uint4*>(dst.from32 + 32 * j);
    const uint4 v0 = v[0], v1 = v[1], f0 = f[0], f1 = f[1];
    dv[0] = v0;
    dv[1] = v1;
    df[0] = f0;
    df[1] = f1;
}

// 65·i is no multiple of 4 and a device batch's base may be misaligned too, hence bytes.  All 65 loads are
// issued before the first store, so a row costs one trip to memory, not 65 in turn (round 14: a plain
// load-store loop cost an insert of 8,000 that keeps 5,000 some 40 µs).
__device__ __forceinline__ void load_sig(uint8_t (&r)[65], const uint8_t* __restrict__ src) {
#pragma unroll
    for (int t = 0; t < 65; t++) r[t] = src[t];
}
__device__ __forceinline__ void copy_sig(uint8_t* __restrict__ dst, size_t j, const uint8_t* __restrict__ src, size_t i) {
    uint8_t r[65];
    load_sig(r, src + 65 * i);
#pragma unroll
    for (int t = 0; t < 65; t++) dst[65 * j + t] = r[t];
}

__global__ __launch_bounds__(256) void k_log_append(DevBatch b, const uint8_t* __restrict__ verdict,
                                                    const uint32_t* __restrict__ bitmap,
                                                    const uint8_t* __restrict__ value_ok, int64_t height, uint32_t L,
                                                    LogCols lg, uint8_t* __restrict__ vd) {
    const uint32_t total = L + b.n, stride = gridDim.x * blockDim.x;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
        if (q < L) {   // retained: its row and value_ok byte are in place
            vd[q] = V_VALID;
            continue;
        }
        const uint32_t i = q - L;
        copy_row(lg, q, b.type, b.height, b.round, b.valid_round, b.value32, b.from32, i);
        lg.vok[q] = value_ok ? (value_ok[i] ? 1 : 0) : 1;
        if (lg.sig) copy_sig(lg.sig, q, b.sig65, i);
        bool ok = b.height[i] == height;
        if (verdict && verdict[i] != V_VALID) ok = false;
        if (bitmap && !((bitmap[i >> 5] >> (i & 31)) & 1u)) ok = false;
        vd[q] = ok ? V_VALID : HD_LOG_NOT_CANDIDATE;
    }
}

// one block per 256 joined positions, in both passes below
__global__ __launch_bounds__(256) void k_log_count(uint32_t total, uint32_t L, const uint8_t* __restrict__ dup,
                                                   const uint8_t* __restrict__ pclass, uint32_t* __restrict__ blk) {
    __shared__ uint32_t wo[4], wn[4];
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const bool logged = q < total && (dup[q] == 0 || pclass[q] == 0);
    const unsigned long long bo = __ballot(logged && q < L), bn = __ballot(logged && q >= L);
    if ((threadIdx.x & 63) == 0) {
        wo[threadIdx.x >> 6] = (uint32_t)__popcll(bo);
        wn[threadIdx.x >> 6] = (uint32_t)__popcll(bn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk[2 * blockIdx.x] = wo[0] + wo[1] + wo[2] + wo[3];
        blk[2 * blockIdx.x + 1] = wn[0] + wn[1] + wn[2] + wn[3];
    }
}

__global__ __launch_bounds__(256) void k_log_keep(uint32_t total, uint32_t L, const uint8_t* __restrict__ dup,
                                                  const uint8_t* __restrict__ pclass,
                                                  const uint32_t* __restrict__ blk, LogCols lg, LogCols tmp,
                                                  uint32_t* __restrict__ hdr, uint32_t* __restrict__ logpos,
                                                  uint8_t* __restrict__ o_dup, uint8_t* __restrict__ o_pclass) {
    __shared__ uint32_t part[4], old[4], wn[4];
    const uint32_t nb = gridDim.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool last = blockIdx.x == nb - 1;
    // kept messages of the blocks before this one; the last block also sums the retained entries
    // logged again, over every block, for the header
    uint32_t sn = 0, so = 0;
    for (uint32_t k = threadIdx.x; k < blockIdx.x; k += 256) sn += blk[2 * k + 1];
    if (last)
        for (uint32_t k = threadIdx.x; k < nb; k += 256) so += blk[2 * k];
    for (int d = 32; d > 0; d >>= 1) {
        sn += (uint32_t)__shfl_xor((int)sn, d, 64);
        so += (uint32_t)__shfl_xor((int)so, d, 64);
    }
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const bool fresh = q < total && q >= L;
    const uint8_t du = fresh ? dup[q] : 3, pc = fresh ? pclass[q] : 3;
    const bool keep = fresh && (du == 0 || pc == 0);
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) {
        part[w] = sn;
        old[w] = so;
        wn[w] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    uint32_t off = part[0] + part[1] + part[2] + part[3];
    if (last && threadIdx.x == 0) {
        hdr[0] = off + wn[0] + wn[1] + wn[2] + wn[3];   // kept
        hdr[1] = old[0] + old[1] + old[2] + old[3];     // relogged
    }
    if (!fresh) return;
    for (uint32_t k = 0; k < w; k++) off += wn[k];
    const uint32_t j = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    const uint32_t i = q - L;
    if (o_dup) o_dup[i] = du;         // a class the caller does not take is not gathered
    if (o_pclass) o_pclass[i] = pc;
    logpos[i] = keep ? L + j : HD_WHEN_NEVER;
    if (keep) {   // j < the batch's size: tmp has a row for every new message
        copy_row(tmp, j, lg.type, lg.height, lg.round, lg.vround, lg.value32, lg.from32, q);
        tmp.vok[j] = lg.vok[q];
        if (tmp.sig) copy_sig(tmp.sig, j, lg.sig, q);
    }
}

// the accepted insert's kept rows, from the second buffer to their place behind the retained entries
__global__ __launch_bounds__(256) void k_log_commit(uint32_t kept, uint32_t L, LogCols tmp, LogCols lg) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < kept; j += stride) {
        copy_row(lg, (size_t)L + j, tmp.type, tmp.height, tmp.round, tmp.vround, tmp.value32, tmp.from32, j);
        lg.vok[(size_t)L + j] = tmp.vok[j];
        if (lg.sig) copy_sig(lg.sig, (size_t)L + j, tmp.sig, j);
    }
}

// row q of the columns as one packed record at dst (8-byte aligned)
__device__ __forceinline__ void pack_row(uint8_t* dst, const LogCols& lg, size_t q, bool sig) {
    int64_t* d = reinterpret_cast<int64_t*>(dst);
    d[ROW_HEIGHT / 8] = lg.height[q];
    d[ROW_ROUND / 8] = lg.round[q];
    d[ROW_VROUND / 8] = lg.vround[q];
    const uint2* v = reinterpret_cast<const uint2*>(lg.value32 + 32 * q);
    const uint2* f = reinterpret_cast<const uint2*>(lg.from32 + 32 * q);
    uint2* dv = reinterpret_cast<uint2*>(dst + ROW_VALUE);
    uint2* df = reinterpret_cast<uint2*>(dst + ROW_FROM);
    for (int k = 0; k < 4; k++) {
        dv[k] = v[k];
        df[k] = f[k];
    }
    dst[ROW_TYPE] = lg.type[q];
    dst[ROW_VOK] = lg.vok[q];
    if (sig) copy_sig(dst + ROW_SIG, 0, lg.sig, q);
}

// hd_log_read: record k is entry pos[k], or first + k without a list (the host has checked every position)
__global__ __launch_bounds__(256) void k_log_gather(const uint32_t* __restrict__ pos, uint32_t first, uint32_t n,
                                                    LogCols lg, uint8_t* __restrict__ rows, uint32_t row_bytes) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride)
        pack_row(rows + (size_t)row_bytes * k, lg, pos ? pos[k] : first + k, row_bytes == ROW_BYTES_SIG);
}

// One lane per message of a catch record: lane 2k packs record k's offender, lane 2k + 1 the message it
// contradicts, both from the joined rows (a retained entry below L, this batch's messages from L on).  A
// position that is no joined row -- HD_WHEN_NEVER, the against of an out-of-turn propose -- gives zero bytes.
// `room` records fit in rows.
__global__ __launch_bounds__(256) void k_log_evidence(DecideRecs r, uint32_t room, uint32_t total, LogCols lg,
                                                      uint8_t* __restrict__ rows, uint32_t row_bytes) {
    const uint32_t recs = min(r.hdr[1], room), stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < 2 * recs; t += stride) {
        const uint32_t k = t >> 1;
        const uint32_t* col = (t & 1u) ? (k < r.H ? r.st_against : r.ov_against) : (k < r.H ? r.st_index : r.ov_index);
        const uint32_t q = col[k < r.H ? k : k - r.H];
        uint8_t* dst = rows + (size_t)row_bytes * t;
        if (q < total) {
            pack_row(dst, lg, q, row_bytes == ROW_BYTES_SIG);
        } else {
            uint2* z = reinterpret_cast<uint2*>(dst);
            for (uint32_t w = 0; w < row_bytes / 8; w++) z[w] = make_uint2(0u, 0u);
        }
    }
}

// ---------------------------------------------------------------- hd_log_select
// the device form's outputs: the caller's columns of cap rows (vround, sig, vok, pos: each may be NULL)
struct SelCols {
    uint8_t* type;
    int64_t* height;
    int64_t* round;
    int64_t* vround;
    uint8_t* value32;
    uint8_t* from32;
    uint8_t* sig;
    uint8_t* vok;
    uint32_t* pos;
};

// entry q against the filter; q < L, so the row is a retained entry's (16-byte aligned: row 32 q of a hipMalloc)
__device__ __forceinline__ bool sel_match(const hd_log_filter& f, const LogCols& lg, uint32_t q) {
    const uint8_t* v = static_cast<const uint8_t*>(__builtin_assume_aligned(lg.value32 + 32 * (size_t)q, 16));
    const uint8_t* s = static_cast<const uint8_t*>(__builtin_assume_aligned(lg.from32 + 32 * (size_t)q, 16));
    return log_match(f, lg.type[q], lg.round[q], v, s);
}

// one block per 256 positions of [lo, end), in both passes below; end <= L
__global__ __launch_bounds__(256) void k_log_sel_count(hd_log_filter f, uint32_t lo, uint32_t end, LogCols lg,
                                                       uint32_t* __restrict__ blk) {
    __shared__ uint32_t wn[LOG_SEL_WAVES];
    const uint32_t q = lo + blockIdx.x * LOG_SEL_BLOCK + threadIdx.x;
    const bool m = q < end && sel_match(f, lg, q);
    const unsigned long long bal = __ballot(m);
    if ((threadIdx.x & 63) == 0) wn[threadIdx.x >> 6] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = wn[0] + wn[1] + wn[2] + wn[3];
}

// HOST: slot j is record j of recs (rec_bytes each: a packed row with the position in its last word, or, with
// rows == false, the position alone).  Otherwise slot j is row j of the caller's columns.  room <= cap slots exist.
template <bool HOST>
__global__ __launch_bounds__(256) void k_log_sel_emit(hd_log_filter f, uint32_t lo, uint32_t end,
                                                      const uint32_t* __restrict__ blk, LogCols lg, uint32_t room,
                                                      uint8_t* __restrict__ recs, uint32_t rec_bytes, bool rows,
                                                      bool sig, SelCols o, uint32_t* __restrict__ hdr) {
    __shared__ uint32_t part[LOG_SEL_WAVES], wn[LOG_SEL_WAVES];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t sn = log_sel_partial(blk, blockIdx.x, threadIdx.x);
    for (int d = 32; d > 0; d >>= 1) sn += (uint32_t)__shfl_xor((int)sn, d, 64);
    const uint32_t q = lo + blockIdx.x * LOG_SEL_BLOCK + threadIdx.x;
    const bool m = q < end && sel_match(f, lg, q);
    const unsigned long long bal = __ballot(m);
    if (lane == 0) {
        part[w] = sn;
        wn[w] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    const uint32_t off = part[0] + part[1] + part[2] + part[3];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const uint32_t total = off + wn[0] + wn[1] + wn[2] + wn[3];
        hdr[0] = total;
        hdr[1] = log_sel_n(total, f.limit);
    }
    if (!m) return;
    const uint32_t j = log_sel_rank(off, wn, w, bal, lane);
    if (j >= room) return;   // past the limit, or no slot: nothing is stored at or beyond cap
    if (HOST) {
        uint8_t* dst = recs + (size_t)rec_bytes * j;
        if (rows) pack_row(dst, lg, q, sig);
        *reinterpret_cast<uint32_t*>(dst + rec_bytes - 4) = q;
    } else {
        o.type[j] = lg.type[q];
        o.height[j] = lg.height[q];
        o.round[j] = lg.round[q];
        if (o.vround) o.vround[j] = lg.vround[q];
        const uint4* v = reinterpret_cast<const uint4*>(lg.value32 + 32 * (size_t)q);
        const uint4* s = reinterpret_cast<const uint4*>(lg.from32 + 32 * (size_t)q);
        uint4* dv = reinterpret_cast<uint4*>(o.value32 + 32 * (size_t)j);
        uint4* ds = reinterpret_cast<uint4*>(o.from32 + 32 * (size_t)j);
        const uint4 v0 = v[0], v1 = v[1], s0 = s[0], s1 = s[1];
        dv[0] = v0;
        dv[1] = v1;
        ds[0] = s0;
        ds[1] = s1;
        if (o.sig) copy_sig(o.sig, j, lg.sig, q);
        if (o.vok) o.vok[j] = lg.vok[q];
        if (o.pos) o.pos[j] = q;
    }
}

// ---------------------------------------------------------------- host side
#define LCHK(expr, what)                                         \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) return hd_ctx_fail(ctx, _e, what); \
    } while (0)

static void cols_free(LogCols& c) {
    for (int k = 0; k < 8; k++) {
        void** p = log_col(c, k);
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

// rows for `need` items; the first `keep` rows survive a regrow (copied on s).  ncols: 8 on a log that keeps
// signatures, 7 otherwise (the setting changes only while the log holds no columns)
static int cols_grow(hd_ctx* ctx, LogCols& c, size_t& cap, size_t need, size_t keep, hipStream_t s, int ncols) {
    if (need <= cap) return HD_OK;
    const size_t want = std::max(need + need / 4, (size_t)4096);
    LogCols nw{};
    for (int k = 0; k < ncols; k++) {
        hipError_t e = hipMalloc(log_col(nw, k), kLogWidth[k] * want);
        if (e != hipSuccess) {
            cols_free(nw);
            return hd_ctx_fail(ctx, e, "log hipMalloc");
        }
    }
    if (keep) {
        hipError_t e = hipSuccess;
        for (int k = 0; k < ncols && e == hipSuccess; k++)
            e = hipMemcpyAsync(*log_col(nw, k), *log_col(c, k), kLogWidth[k] * keep, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            cols_free(nw);
            return hd_ctx_fail(ctx, e, "log regrow copy");
        }
    }
    cols_free(c);
    c = nw;
    cap = want;
    return HD_OK;
}

static int buf_grow(hd_ctx* ctx, DevBuf& b, size_t need) { return hd_dev_grow(ctx, &b.p, &b.cap, need); }

static size_t log_pad(size_t n) { return (n + 63) & ~(size_t)63; }

static int host_grow(hd_log* lg, size_t need) {
    hd_ctx* ctx = lg->ctx;
    if (lg->host_cap >= need) return HD_OK;
    if (lg->host) (void)hipHostFree(lg->host);
    lg->host = nullptr;
    lg->host_cap = 0;
    LCHK(hipHostMalloc((void**)&lg->host, need + (need >> 2), hipHostMallocDefault), "log host stage");
    lg->host_cap = need + (need >> 2);
    return HD_OK;
}

static bool rows_ok(const hd_log_rows* r) {
    return r && (r->cap == 0 || (r->type && r->height && r->round && r->valid_round && r->value32 && r->from32 &&
                                 r->value_ok));
}

// packed record -> row k of the caller's columns
static void unpack_row(const char* src, hd_log_rows* o, size_t k) {
    memcpy(o->height + k, src + ROW_HEIGHT, 8);
    memcpy(o->round + k, src + ROW_ROUND, 8);
    memcpy(o->valid_round + k, src + ROW_VROUND, 8);
    memcpy(o->value32 + 32 * k, src + ROW_VALUE, 32);
    memcpy(o->from32 + 32 * k, src + ROW_FROM, 32);
    o->type[k] = (uint8_t)src[ROW_TYPE];
    o->value_ok[k] = (uint8_t)src[ROW_VOK];
    if (o->sig65) memcpy(o->sig65 + 65 * k, src + ROW_SIG, 65);
}

struct KeepArgs {
    hd_log* lg;
    uint32_t n, total, nb;
    size_t dup_off, pc_off, res_bytes;   // dup_off / pc_off: 0 when the caller does not take the class
    // evidence: its block starts at ev_off of res with room for n records (two packed rows of ev_row bytes
    // each), of which the first ev_staged come down with the classes
    bool ev;
    size_t ev_off;
    uint32_t ev_row, ev_staged;
};

// hd_decide_run's hook: dup / pclass are complete on the stream
static int log_queue_keep(void* arg, hipStream_t s, const DecideRecs* recs) {
    const KeepArgs* a = static_cast<const KeepArgs*>(arg);
    hd_log* lg = a->lg;
    hd_ctx* ctx = lg->ctx;
    char* res = (char*)lg->res.p;
    const uint8_t *dup = (const uint8_t*)lg->dup.p, *pclass = (const uint8_t*)lg->pclass.p;
    uint32_t* blk = (uint32_t*)lg->blk.p;
    const size_t lp_off = 64;
    k_log_count<<<a->nb, 256, 0, s>>>(a->total, lg->L, dup, pclass, blk);
    k_log_keep<<<a->nb, 256, 0, s>>>(a->total, lg->L, dup, pclass, blk, lg->lg, lg->tmp, (uint32_t*)res,
                                     (uint32_t*)(res + lp_off), a->dup_off ? (uint8_t*)(res + a->dup_off) : nullptr,
                                     a->pc_off ? (uint8_t*)(res + a->pc_off) : nullptr);
    LCHK(hipGetLastError(), "log keep kernels");
    size_t down = a->res_bytes;
    if (a->ev && recs && a->n) {   // only a message of this batch is an offender: at most n records
        const uint32_t grid = std::min<uint32_t>((2u * a->n + 255u) / 256u, (uint32_t)ctx->n_cu * 16u);
        k_log_evidence<<<grid, 256, 0, s>>>(*recs, a->n, a->total, lg->lg, (uint8_t*)(res + a->ev_off), a->ev_row);
        LCHK(hipGetLastError(), "log evidence");
        down = a->ev_off + 2 * (size_t)a->ev_row * a->ev_staged;
    }
    LCHK(hipMemcpyAsync(lg->host, res, down, hipMemcpyDeviceToHost, s), "log download");
    return HD_OK;
}

static bool log_out_ok(const hd_decide_out* o, const hd_decide_order* w) {
    return o && o->height && o->round && o->rep && o->propose && o->prevotes && o->precommits && o->trace &&
           o->pv_value && o->pc_value && o->pv_nil && o->pv_validround && o->flags && o->bits && w && w->when &&
           w->exact_until && w->cap >= o->cap;
}

// db, d_verdict / d_bitmap (one of them) and d_vok are device pointers
static int log_insert(hd_log* lg, const hd_batch* db, const uint8_t* d_verdict, const uint32_t* d_bitmap,
                      const uint8_t* d_vok, hd_decide_out* out, hd_decide_order* order, hd_log_info* info,
                      hd_catch_out* caught, hd_evidence_out* ev, hipStream_t s) {
    hd_ctx* ctx = lg->ctx;
    const uint32_t n = db->n, L = lg->L, total = L + n;
    if (total == 0) return HD_OK;
    const uint32_t nb = (total + 255u) / 256u;
    const int ncols = lg->keep_sig ? 8 : 7;
    int rc = cols_grow(ctx, lg->lg, lg->cap_items, total, L, s, ncols);
    if (!rc) rc = cols_grow(ctx, lg->tmp, lg->cap_new, std::max(n, 1u), 0, s, ncols);
    if (!rc) rc = buf_grow(ctx, lg->vd, total);
    if (!rc) rc = buf_grow(ctx, lg->dup, total);
    if (!rc) rc = buf_grow(ctx, lg->pclass, total);
    if (!rc) rc = buf_grow(ctx, lg->blk, 8 * (size_t)nb);
    // [header | logpos | dup, when out->dup | pclass, when out->pclass]: a class the caller passes NULL for
    // stays in lg->dup / lg->pclass on the device and is neither gathered nor downloaded
    const size_t cls_off = 64 + log_pad(4 * (size_t)n);
    const size_t dup_off = out->dup ? cls_off : 0, pc_off = out->pclass ? cls_off + (out->dup ? log_pad(n) : 0) : 0;
    const size_t res_bytes = cls_off + (out->dup ? log_pad(n) : 0) + (out->pclass ? log_pad(n) : 0);
    // the evidence block behind them: room for n records on the device, the first ev_staged in the download
    const size_t ev_off = log_pad(res_bytes);
    const uint32_t ev_row = lg->keep_sig ? ROW_BYTES_SIG : ROW_BYTES, ev_staged = ev ? std::min(lg->guess_ev, n) : 0u;
    if (!rc) rc = buf_grow(ctx, lg->res, ev ? ev_off + 2 * (size_t)ev_row * n : res_bytes);
    if (!rc) rc = host_grow(lg, ev ? ev_off + 2 * (size_t)ev_row * ev_staged : res_bytes);
    if (rc) return rc;
    DevBatch b{n, db->type, db->height, db->round, db->valid_round, db->value32, db->from32,
               lg->keep_sig ? db->sig65 : nullptr};
    const uint32_t grid = std::min<uint32_t>(nb, (uint32_t)ctx->n_cu * 16u);
    k_log_append<<<grid, 256, 0, s>>>(b, d_verdict, d_bitmap, d_vok, lg->height, L, lg->lg, (uint8_t*)lg->vd.p);
    LCHK(hipGetLastError(), "log append");
    hd_batch jb;
    jb.n = total;
    jb.type = lg->lg.type;
    jb.height = lg->lg.height;
    jb.round = lg->lg.round;
    jb.valid_round = lg->lg.vround;
    jb.value32 = lg->lg.value32;
    jb.from32 = lg->lg.from32;
    jb.sig65 = nullptr;
    KeepArgs ka{lg, n, total, nb, dup_off, pc_off, res_bytes, ev != nullptr, ev_off, ev_row, ev_staged};
    const DecideExt ext{(uint8_t*)lg->dup.p, (uint8_t*)lg->pclass.p, log_queue_keep, &ka};
    rc = hd_decide_run(ctx, &jb, (const uint8_t*)lg->vd.p, nullptr,
                       DecideIn{lg->f, lg->n_sched, lg->n_sched ? lg->d_sched : nullptr, lg->lg.vok}, out, s, order,
                       &ext, caught);
    (void)hd_ctx_note_stream(ctx, s);
    if (ev) lg->guess_ev = std::max<uint32_t>(256u, caught->n + caught->n / 4);   // also after HD_ECAP: the retry is staged
    if (rc) return rc;
    // the items are the joined coordinates, so the records are final; they are in ascending index and a
    // retained entry, the only message of its key, is never an offender
    if (caught && caught->n && caught->index[0] < L) {
        ctx->last_error = "hd_log: the replay reported a retained entry as an offender";
        return HD_EDEVICE;
    }
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(lg->host);
    const uint32_t kept = hdr[0], relogged = hdr[1];
    info->kept = kept;
    info->relogged = relogged;
    if (relogged != L || kept > n) {
        ctx->last_error = "hd_log: the replay did not log every retained entry again";
        return HD_EDEVICE;
    }
    if (lg->max_entries && (uint64_t)L + kept > lg->max_entries) return HD_ECAP;
    const size_t lp_off = 64;
    if (info->logpos) memcpy(info->logpos, lg->host + lp_off, 4 * (size_t)n);
    if (out->dup) memcpy(out->dup, lg->host + dup_off, n);
    if (out->pclass) memcpy(out->pclass, lg->host + pc_off, n);
    if (ev) {   // caught->n <= caught->cap <= both row sets' cap, and <= n by the check above
        const uint32_t recs = caught->n, staged = std::min(recs, ev_staged);
        const auto spread = [&](const char* src, uint32_t k0, uint32_t cnt) {
            for (uint32_t k = 0; k < cnt; k++) {
                unpack_row(src + 2 * (size_t)ev_row * k, &ev->offender, k0 + k);
                unpack_row(src + 2 * (size_t)ev_row * k + ev_row, &ev->against, k0 + k);
            }
        };
        spread(lg->host + ev_off, 0, staged);
        if (recs > staged) {   // past the staged records: a second copy, as the catch list's own overflow
            const size_t more = 2 * (size_t)ev_row * (recs - staged);
            rc = host_grow(lg, more);   // everything the stage held has been copied out by now
            if (rc) return rc;
            char* dst = lg->host;
            LCHK(hipMemcpyAsync(dst, (char*)lg->res.p + ev_off + 2 * (size_t)ev_row * staged, more,
                                hipMemcpyDeviceToHost, s),
                 "log evidence overflow");
            LCHK(hipStreamSynchronize(s), "log evidence overflow sync");
            spread(dst, staged, recs - staged);
        }
        ev->offender.n = ev->against.n = recs;
    }
    if (kept) {   // the kept rows behind the retained ones; ordered before the next call by the stream
        k_log_commit<<<std::min<uint32_t>((kept + 255u) / 256u, (uint32_t)ctx->n_cu * 16u), 256, 0, s>>>(
            kept, L, lg->tmp, lg->lg);
        LCHK(hipGetLastError(), "log commit");
        (void)hd_ctx_note_stream(ctx, s);
        lg->commit_stream = s != ctx->stream ? s : nullptr;   // hd_log_read gathers on the context's stream
    }
    lg->L = L + kept;
    return HD_OK;
}

static bool log_args_ok(const hd_log* lg, const hd_batch* b, const hd_decide_out* out, const hd_decide_order* order,
                        hd_log_info* info, const hd_catch_out* caught, const hd_evidence_out* ev) {
    if (!lg || !lg->ctx || !b || !info || !log_out_ok(out, order)) return false;
    if (caught && caught->cap && (!caught->index || !caught->against || !caught->kind)) return false;
    if (b->n && (!b->type || !b->height || !b->round || !b->value32 || !b->from32)) return false;
    if (b->n && lg->keep_sig && !b->sig65) return false;
    if (ev) {   // rows for every record the list has room for, so the list's is the only capacity error
        if (!caught || !rows_ok(&ev->offender) || !rows_ok(&ev->against)) return false;
        if (ev->offender.cap < caught->cap || ev->against.cap < caught->cap) return false;
        if (!lg->keep_sig && (ev->offender.sig65 || ev->against.sig65)) return false;
    }
    return (uint64_t)lg->L + b->n < (1ull << 30);
}

// hd_log_insert and hd_log_insert_catch (caught non-NULL, checked by the caller)
static int insert_host(hd_log* lg, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                       hd_decide_out* out, hd_decide_order* order, hd_log_info* info, hd_catch_out* caught,
                       hd_evidence_out* ev) {
    if (!log_args_ok(lg, batch, out, order, info, caught, ev) || (batch->n && !verdict)) return HD_EINVAL;
    hd_ctx* ctx = lg->ctx;
    out->n = 0;
    if (caught) caught->n = 0;
    if (ev) ev->offender.n = ev->against.n = 0;
    info->base = lg->L;
    info->kept = info->relogged = 0;
    const uint32_t n = batch->n;
    (void)hipSetDevice(ctx->device);
    hd_batch db;
    memset(&db, 0, sizeof db);
    const uint8_t *d_v = nullptr, *d_vok = nullptr;
    if (n) {
        hd_batch hb = *batch;
        if (!lg->keep_sig) hb.sig65 = nullptr;   // not kept: Equal ignores it
        int rc = hd_upload_batch(ctx, &hb, &db);
        if (!rc) rc = hd_dev_grow(ctx, &ctx->bufs[BUF_VERDICT].p, &ctx->bufs[BUF_VERDICT].cap, n);
        if (!rc && value_ok) rc = buf_grow(ctx, lg->in_vok, n);
        if (rc) return rc;
        LCHK(hipMemcpyAsync(ctx->bufs[BUF_VERDICT].p, verdict, n, hipMemcpyHostToDevice, ctx->stream),
             "verdict upload");
        d_v = (const uint8_t*)ctx->bufs[BUF_VERDICT].p;
        if (value_ok) {
            LCHK(hipMemcpyAsync(lg->in_vok.p, value_ok, n, hipMemcpyHostToDevice, ctx->stream), "value_ok upload");
            d_vok = (const uint8_t*)lg->in_vok.p;
        }
    }
    return log_insert(lg, &db, d_v, nullptr, d_vok, out, order, info, caught, ev, ctx->stream);
}

static int insert_bitmap(hd_log* lg, const hd_batch* dbatch, const uint32_t* d_valid_bitmap, const uint8_t* d_value_ok,
                         hd_decide_out* out, hd_decide_order* order, hd_log_info* info, hd_catch_out* caught,
                         hd_evidence_out* ev, void* stream) {
    if (!log_args_ok(lg, dbatch, out, order, info, caught, ev) || (dbatch->n && !d_valid_bitmap)) return HD_EINVAL;
    hd_ctx* ctx = lg->ctx;
    out->n = 0;
    if (caught) caught->n = 0;
    if (ev) ev->offender.n = ev->against.n = 0;
    info->base = lg->L;
    info->kept = info->relogged = 0;
    (void)hipSetDevice(ctx->device);
    return log_insert(lg, dbatch, nullptr, dbatch->n ? d_valid_bitmap : nullptr, d_value_ok, out, order, info, caught,
                      ev, stream ? (hipStream_t)stream : ctx->stream);
}

extern "C" {

int hd_log_create(hd_ctx* ctx, hd_log** out) {
    if (!ctx || !out) return HD_EINVAL;
    hd_log* lg = new (std::nothrow) hd_log();
    if (!lg) return HD_ENOMEM;
    lg->ctx = ctx;
    lg->device = ctx->device;
    *out = lg;
    return HD_OK;
}

int hd_log_destroy(hd_log* lg) {
    if (!lg) return HD_EINVAL;
    (void)hipSetDevice(lg->device);
    (void)hipDeviceSynchronize();   // a commit's copies may still be queued on a caller's stream
    cols_free(lg->lg);
    cols_free(lg->tmp);
    DevBuf* bufs[] = {&lg->vd, &lg->dup, &lg->pclass, &lg->blk, &lg->res, &lg->in_vok, &lg->pos, &lg->sel_blk};
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (lg->sel_ev) (void)hipEventDestroy(lg->sel_ev);
    if (lg->d_sched) (void)hipFree(lg->d_sched);
    if (lg->host) (void)hipHostFree(lg->host);
    delete lg;
    return HD_OK;
}

int hd_log_reset(hd_log* lg, int64_t height, uint32_t f, const uint8_t* sched32, uint32_t n_sched,
                 uint32_t max_entries) {
    if (!lg || !lg->ctx || (sched32 && n_sched == 0)) return HD_EINVAL;
    hd_ctx* ctx = lg->ctx;
    (void)hipSetDevice(ctx->device);
    if (sched32) {
        // an earlier insert's kernels may still read the old schedule on the context's stream
        LCHK(hipStreamSynchronize(ctx->stream), "log reset sync");
        int rc = hd_dev_grow(ctx, (void**)&lg->d_sched, &lg->cap_sched, 32 * (size_t)n_sched);
        if (rc) return rc;
        LCHK(hipMemcpy(lg->d_sched, sched32, 32 * (size_t)n_sched, hipMemcpyHostToDevice), "log schedule upload");
    }
    lg->n_sched = sched32 ? n_sched : 0;
    lg->height = height;
    lg->f = f;
    lg->max_entries = max_entries;
    lg->L = 0;
    return HD_OK;
}

int hd_log_len(const hd_log* lg, int64_t* height, uint32_t* entries) {
    if (!lg) return HD_EINVAL;
    if (height) *height = lg->height;
    if (entries) *entries = lg->L;
    return HD_OK;
}

int hd_log_insert(hd_log* lg, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                  hd_decide_out* out, hd_decide_order* order, hd_log_info* info) {
    return insert_host(lg, batch, verdict, value_ok, out, order, info, nullptr, nullptr);
}

int hd_log_insert_device_bitmap(hd_log* lg, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                const uint8_t* d_value_ok, hd_decide_out* out, hd_decide_order* order,
                                hd_log_info* info, void* stream) {
    return insert_bitmap(lg, dbatch, d_valid_bitmap, d_value_ok, out, order, info, nullptr, nullptr, stream);
}

int hd_log_insert_catch(hd_log* lg, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                        hd_decide_out* out, hd_decide_order* order, hd_log_info* info, hd_catch_out* caught) {
    if (!caught) return HD_EINVAL;
    return insert_host(lg, batch, verdict, value_ok, out, order, info, caught, nullptr);
}

int hd_log_insert_catch_device_bitmap(hd_log* lg, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                      const uint8_t* d_value_ok, hd_decide_out* out, hd_decide_order* order,
                                      hd_log_info* info, hd_catch_out* caught, void* stream) {
    if (!caught) return HD_EINVAL;
    return insert_bitmap(lg, dbatch, d_valid_bitmap, d_value_ok, out, order, info, caught, nullptr, stream);
}

int hd_log_insert_evidence(hd_log* lg, const hd_batch* batch, const uint8_t* verdict, const uint8_t* value_ok,
                           hd_decide_out* out, hd_decide_order* order, hd_log_info* info, hd_catch_out* caught,
                           hd_evidence_out* evidence) {
    if (!caught || !evidence) return HD_EINVAL;
    return insert_host(lg, batch, verdict, value_ok, out, order, info, caught, evidence);
}

int hd_log_insert_evidence_device_bitmap(hd_log* lg, const hd_batch* dbatch, const uint32_t* d_valid_bitmap,
                                         const uint8_t* d_value_ok, hd_decide_out* out, hd_decide_order* order,
                                         hd_log_info* info, hd_catch_out* caught, hd_evidence_out* evidence,
                                         void* stream) {
    if (!caught || !evidence) return HD_EINVAL;
    return insert_bitmap(lg, dbatch, d_valid_bitmap, d_value_ok, out, order, info, caught, evidence, stream);
}

int hd_log_keep_signatures(hd_log* lg, int on) {
    if (!lg || lg->L != 0) return HD_EINVAL;
    if (lg->keep_sig == (on != 0)) return HD_OK;
    // the columns of an earlier height have the other shape: the next insert allocates them again
    (void)hipSetDevice(lg->device);
    (void)hipDeviceSynchronize();   // a commit may still be queued on a caller's stream
    cols_free(lg->lg);
    cols_free(lg->tmp);
    lg->cap_items = lg->cap_new = 0;
    lg->keep_sig = on != 0;
    return HD_OK;
}

int hd_log_read(hd_log* lg, const uint32_t* pos, uint32_t first, uint32_t n, hd_log_rows* out) {
    if (!lg || !lg->ctx || !rows_ok(out)) return HD_EINVAL;
    out->n = 0;
    if (out->cap < n || (out->sig65 && !lg->keep_sig)) return HD_EINVAL;
    if (pos) {
        for (uint32_t k = 0; k < n; k++)
            if (pos[k] >= lg->L) return HD_EINVAL;
    } else if ((uint64_t)first + n > lg->L) {
        return HD_EINVAL;
    }
    if (n == 0) return HD_OK;
    hd_ctx* ctx = lg->ctx;
    hipStream_t s = ctx->stream;
    (void)hipSetDevice(ctx->device);
    const uint32_t row = out->sig65 ? ROW_BYTES_SIG : ROW_BYTES;
    const size_t bytes = (size_t)row * n;
    int rc = buf_grow(ctx, lg->res, bytes);
    if (!rc) rc = host_grow(lg, bytes);
    if (!rc && pos) rc = buf_grow(ctx, lg->pos, 4 * (size_t)n);
    if (rc) return rc;
    if (lg->commit_stream) {
        // the last insert's commit ran on a caller's stream: wait for the event hd_ctx_note_stream recorded
        // behind it (a stream that is no longer listed has completed that work)
        for (const auto& se : ctx->caller_ev)
            if (se.first == lg->commit_stream) LCHK(hipStreamWaitEvent(s, se.second, 0), "log read wait");
        lg->commit_stream = nullptr;
    }
    if (pos) LCHK(hipMemcpyAsync(lg->pos.p, pos, 4 * (size_t)n, hipMemcpyHostToDevice, s), "log read positions");
    k_log_gather<<<std::min<uint32_t>((n + 255u) / 256u, (uint32_t)ctx->n_cu * 16u), 256, 0, s>>>(
        pos ? (const uint32_t*)lg->pos.p : nullptr, first, n, lg->lg, (uint8_t*)lg->res.p, row);
    LCHK(hipGetLastError(), "log gather");
    LCHK(hipMemcpyAsync(lg->host, lg->res.p, bytes, hipMemcpyDeviceToHost, s), "log read download");
    LCHK(hipStreamSynchronize(s), "log read sync");
    for (uint32_t k = 0; k < n; k++) unpack_row(lg->host + (size_t)row * k, out, k);
    out->n = n;
    return HD_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- hd_log_select
// The selection's kernels go on s behind the last insert's commit.  That commit went on the context's stream
// or on a caller's (commit_stream, with the event hd_ctx_note_stream recorded behind it, as hd_log_read waits
// for it); a selection on a caller's stream is ordered after the context's stream by an event of the log's own.
static int sel_order(hd_log* lg, hipStream_t s) {
    hd_ctx* ctx = lg->ctx;
    if (lg->commit_stream && lg->commit_stream != s) {
        for (const auto& se : ctx->caller_ev)
            if (se.first == lg->commit_stream) LCHK(hipStreamWaitEvent(s, se.second, 0), "log select wait");
    }
    if (s == ctx->stream) {
        lg->commit_stream = nullptr;   // the context's stream is behind it from here on
        return HD_OK;
    }
    if (!lg->sel_ev) LCHK(hipEventCreateWithFlags(&lg->sel_ev, hipEventDisableTiming), "log select event");
    LCHK(hipEventRecord(lg->sel_ev, ctx->stream), "log select record");
    LCHK(hipStreamWaitEvent(s, lg->sel_ev, 0), "log select wait");
    return HD_OK;
}

// rows / pos_out (host) or dev (device columns); want: an output was asked for
static int log_select(hd_log* lg, const hd_log_filter* flt, uint32_t* pos_out, hd_log_rows* rows, const SelCols* dev,
                      bool want, uint32_t cap, hd_log_selected* sel, hipStream_t s) {
    hd_ctx* ctx = lg->ctx;
    const hd_log_filter f = *flt;
    const uint32_t end = log_sel_end(f.pos_hi, lg->L), nb = log_sel_blocks(f.pos_lo, end);
    if (nb == 0 || f.round_lo > f.round_hi) return HD_OK;   // nothing to look at
    (void)hipSetDevice(ctx->device);
    const uint32_t room = want ? log_sel_room(f.limit, cap) : 0u;
    const bool sig = rows && rows->sig65;
    const uint32_t rec = dev ? 0u : rows ? (sig ? ROW_BYTES_SIG : ROW_BYTES) : 4u;
    const uint32_t staged = dev ? 0u : std::min(lg->guess_sel, room);
    const size_t hdr_bytes = 64;
    int rc = buf_grow(ctx, lg->sel_blk, 4 * (size_t)nb);
    if (!rc) rc = buf_grow(ctx, lg->res, hdr_bytes + (size_t)rec * room);
    if (!rc) rc = host_grow(lg, hdr_bytes + (size_t)rec * staged);
    if (!rc) rc = sel_order(lg, s);
    if (rc) return rc;
    uint32_t* blk = (uint32_t*)lg->sel_blk.p;
    char* res = (char*)lg->res.p;
    k_log_sel_count<<<nb, 256, 0, s>>>(f, f.pos_lo, end, lg->lg, blk);
    if (dev)
        k_log_sel_emit<false><<<nb, 256, 0, s>>>(f, f.pos_lo, end, blk, lg->lg, room, nullptr, 0u, false, false, *dev,
                                                (uint32_t*)res);
    else
        k_log_sel_emit<true><<<nb, 256, 0, s>>>(f, f.pos_lo, end, blk, lg->lg, room, (uint8_t*)(res + hdr_bytes), rec,
                                               rows != nullptr, sig, SelCols{}, (uint32_t*)res);
    LCHK(hipGetLastError(), "log select kernels");
    (void)hd_ctx_note_stream(ctx, s);
    LCHK(hipMemcpyAsync(lg->host, res, hdr_bytes + (size_t)rec * staged, hipMemcpyDeviceToHost, s),
         "log select download");
    LCHK(hipStreamSynchronize(s), "log select sync");
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(lg->host);
    const uint32_t n = hdr[1];
    sel->total = hdr[0];
    sel->n = n;
    if (!want) return HD_OK;
    if (!dev) lg->guess_sel = std::max<uint32_t>(256u, n + n / 4);   // also after HD_ECAP: the retry is staged
    if (n > cap) return HD_ECAP;
    if (dev) return HD_OK;
    // n <= room: every returned match has its record on the device, the first `staged` of them here too
    const auto spread = [&](const char* src, uint32_t k0, uint32_t cnt) {
        for (uint32_t k = 0; k < cnt; k++) {
            const char* r = src + (size_t)rec * k;
            if (rows) unpack_row(r, rows, k0 + k);
            if (pos_out) memcpy(pos_out + k0 + k, r + rec - 4, 4);
        }
    };
    const uint32_t first = std::min(n, staged);
    spread(lg->host + hdr_bytes, 0, first);
    if (n > first) {   // past the staged records: a second copy, as the evidence block's overflow
        const size_t more = (size_t)rec * (n - first);
        rc = host_grow(lg, more);   // everything the stage held has been copied out by now
        if (rc) return rc;
        LCHK(hipMemcpyAsync(lg->host, res + hdr_bytes + (size_t)rec * first, more, hipMemcpyDeviceToHost, s),
             "log select overflow");
        LCHK(hipStreamSynchronize(s), "log select overflow sync");
        spread(lg->host, first, n - first);
    }
    if (rows) rows->n = n;
    return HD_OK;
}

extern "C" {

int hd_log_select(hd_log* lg, const hd_log_filter* flt, uint32_t* pos_out, uint32_t cap, hd_log_rows* rows,
                  hd_log_selected* sel) {
    if (!lg || !lg->ctx || !flt || !sel || !log_filter_ok(*flt)) return HD_EINVAL;
    if (rows && (!rows_ok(rows) || rows->cap < cap || (rows->sig65 && !lg->keep_sig))) return HD_EINVAL;
    sel->total = sel->n = 0;
    if (rows) rows->n = 0;
    // rows of cap 0 hold nothing: with cap == 0 the call is the count-only form
    const bool want = cap != 0 && (pos_out || rows);
    return log_select(lg, flt, pos_out, cap ? rows : nullptr, nullptr, want, cap, sel, lg->ctx->stream);
}

int hd_log_select_device(hd_log* lg, const hd_log_filter* flt, const hd_batch_out* d_out, uint8_t* d_value_ok,
                         uint32_t* d_pos, uint32_t cap, hd_log_selected* sel, void* stream) {
    if (!lg || !lg->ctx || !flt || !sel || !log_filter_ok(*flt)) return HD_EINVAL;
    SelCols o{};
    if (d_out) {
        if (d_out->sig65 && !lg->keep_sig) return HD_EINVAL;
        if (cap && (!d_out->type || !d_out->height || !d_out->round || !d_out->value32 || !d_out->from32))
            return HD_EINVAL;
        if ((((uintptr_t)d_out->value32 | (uintptr_t)d_out->from32) & 15u) ||
            (((uintptr_t)d_out->height | (uintptr_t)d_out->round | (uintptr_t)d_out->valid_round) & 7u) ||
            ((uintptr_t)d_pos & 3u))
            return HD_EINVAL;
        o = SelCols{d_out->type,   d_out->height, d_out->round, d_out->valid_round, d_out->value32,
                    d_out->from32, d_out->sig65,  d_value_ok,   d_pos};
    } else if (cap) {
        return HD_EINVAL;
    }
    sel->total = sel->n = 0;
    const bool want = cap != 0;
    return log_select(lg, flt, nullptr, nullptr, want ? &o : nullptr, want, cap, sel,
                      stream ? (hipStream_t)stream : lg->ctx->stream);
}

}  // extern "C"
