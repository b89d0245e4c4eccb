// hd_keyimport.hip -- hd_import_keys / hd_export_keys (include/hd_verify.h):
// the caller-driven way into, and out of, the key slots of the known-key
// fast path (hd_fbtables.hip; DESIGN.md §4 "Where P comes from").
//
// Import, on the context's stream after the context is quiesced:
//   k_key_import   one key per lane (hd_keyimport.h key_classify): on the
//                  curve, hashed in the context's pubkey format, looked up in
//                  the admitted set, slot resolved.  IMPORTED or KNOWN is read
//                  from the slot's state, which nothing writes in this launch,
//                  so rows that repeat a key agree whatever the lane order.
//   k_key_publish  the IMPORTED rows publish as k_verify does: CAS EMPTY ->
//                  CLAIMED, the key, a fence, LEARNED.  Of rows that repeat a
//                  key one wins the CAS; the others carry the same key.
//   fb_learn       builds the tables of the LEARNED slots (hd_fb_learn_sync).
// Export is one gather kernel and one download.  Neither is a throughput
// kernel: a replica calls them once per restart or format change.
//
// The key carry (hd_keycarry.h) lives here too: k_key_gather and k_key_carry
// take the known keys over a set change that frees the tables (fb_map in
// hd_fbtables.hip calls hd_key_stash_*).  Those keys stay on the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/hd_verify.h"
#include "hd_internal.h"
#include "hd_keyimport.h"

using namespace hd;

#define KICHK(expr, what)                                        \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) return hd_ctx_fail(ctx, e_, what); \
    } while (0)

template <int PKFMT>
__global__ __launch_bounds__(256) void k_key_import(const uint8_t* __restrict__ keys64, uint32_t n, AdmIndex ix,
                                                    uint32_t n_adm, const int32_t* __restrict__ adm_perm,
                                                    const int32_t* __restrict__ adm_slot, uint32_t nslots,
                                                    const uint32_t* __restrict__ state, uint8_t* __restrict__ status,
                                                    int32_t* __restrict__ signer, int32_t* __restrict__ row_slot) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        ge q;
        int32_t idx, slot;
        uint8_t st = key_classify(PKFMT, keys64 + 64 * i, ix, n_adm, adm_slot, nslots, q, idx, slot);
        if (st == HD_KEY_IMPORTED && state[slot] != HD_FB_EMPTY) st = HD_KEY_KNOWN;
        status[i] = st;
        signer[i] = idx >= 0 ? adm_perm[idx] : -1;
        row_slot[i] = st == HD_KEY_IMPORTED ? slot : -1;
    }
}

// the rows k_key_import found IMPORTED; their keys passed key_parse there
__global__ __launch_bounds__(256) void k_key_publish(const uint8_t* __restrict__ keys64, uint32_t n,
                                                     const int32_t* __restrict__ row_slot, uint32_t* __restrict__ state,
                                                     ge* __restrict__ pub) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int32_t slot = row_slot[i];
        if (slot < 0) continue;
        if (atomicCAS(&state[slot], HD_FB_EMPTY, HD_FB_CLAIMED) != HD_FB_EMPTY) continue;
        uint32_t x_be[8], y_be[8];
        load_row32_be(x_be, keys64, 2 * i);
        load_row32_be(y_be, keys64, 2 * i + 1);
        ge q;
        fe_from_be(q.x, x_be);
        fe_from_be(q.y, y_be);
        pub[slot] = q;
        __threadfence();
        atomicExch(&state[slot], HD_FB_LEARNED);
    }
}

// Entry i of the caller's signatory array: its slot's key, canonical and
// big-endian, when the slot holds one.  view false: no slot map, nothing known.
__global__ __launch_bounds__(256) void k_key_export(const uint8_t* __restrict__ sig_caller, uint32_t n, AdmIndex ix,
                                                    uint32_t n_adm, bool view, const int32_t* __restrict__ adm_slot,
                                                    uint32_t nslots, const uint32_t* __restrict__ state,
                                                    const ge* __restrict__ pub, uint8_t* __restrict__ keys64,
                                                    uint8_t* __restrict__ known) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t sig[8], x_be[8], y_be[8];
        load_row32_be(sig, sig_caller, i);
        HD_UNROLL for (int w = 0; w < 8; w++) x_be[w] = y_be[w] = 0;
        const int32_t idx = n_adm ? adm_index_find(ix, sig) : -1;
        const int32_t slot = view && idx >= 0 ? adm_slot[idx] : -1;
        bool has = false;
        if (slot >= 1 && (uint32_t)slot < nslots) {
            const uint32_t st = state[slot];
            has = st == HD_FB_LEARNED || st == HD_FB_READY;
        }
        if (has) {
            ge q = pub[slot];
            fe_normalize(q.x);
            fe_normalize(q.y);
            fe_to_be(x_be, q.x);
            fe_to_be(y_be, q.y);
        }
        store_row32_be(keys64, 2 * i, x_be);
        store_row32_be(keys64, 2 * i + 1, y_be);
        known[i] = has ? 1 : 0;
    }
}

// The key carry of a set change that re-tiers the tables (hd_keycarry.h):
// row r of the snapshot keeps the key of its old slot in a stash of its own
// -- the key and state arrays are freed with the tables -- when that slot's
// state says the key is there.  Launched before the tables are freed.
__global__ __launch_bounds__(256) void k_key_gather(const uint32_t* __restrict__ snap_slot, uint32_t n,
                                                    const uint32_t* __restrict__ state, const ge* __restrict__ pub,
                                                    uint32_t n_state, uint32_t f0, uint32_t f1,
                                                    ge* __restrict__ stash_key, uint32_t* __restrict__ stash_flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint32_t slot = snap_slot[r];
        bool has = false;
        if (slot >= 1 && slot < n_state && !(slot >= f0 && slot < f1)) {
            const uint32_t st = state[slot];
            has = st == HD_FB_LEARNED || st == HD_FB_READY;
        }
        if (has) stash_key[r] = pub[slot];
        stash_flag[r] = has ? 1u : 0u;
    }
}

// Pair i = (snapshot row, new slot): the row's key into the new slot, state
// LEARNED, for the table builder.  After the new slot arrays exist and their
// states are reset; the context is quiesced and every slot appears in one
// pair at most, so plain stores do.
__global__ __launch_bounds__(256) void k_key_carry(const uint32_t* __restrict__ pairs, uint32_t n, uint32_t n_rows,
                                                   const ge* __restrict__ stash_key,
                                                   const uint32_t* __restrict__ stash_flag, uint32_t nslots,
                                                   ge* __restrict__ pub, uint32_t* __restrict__ state) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t row = pairs[2 * i], slot = pairs[2 * i + 1];
        if (row >= n_rows || slot < 1 || slot >= nslots || !stash_flag[row]) continue;
        pub[slot] = stash_key[row];
        state[slot] = HD_FB_LEARNED;
    }
}

namespace {
uint32_t key_grid(const hd_ctx* ctx, uint32_t n) {
    return (uint32_t)std::min<uint64_t>(((uint64_t)n + 255u) / 256u, (uint64_t)std::max(ctx->n_cu, 1) * 8u);
}
}  // namespace

int hd_key_stash_gather(hd_ctx* ctx, const uint32_t* snap_slot, uint32_t n, const FbKeyView& old, uint32_t f0,
                        uint32_t f1, FbKeyStash* st) {
    if (n == 0 || !old.state || !old.pub) return HD_OK;
    // flag (n words), then the index words both kernels read: the n snapshot
    // slots here, the (row, slot) pairs of a carry later (2 n at most)
    KICHK(hipMalloc(&st->key, sizeof(ge) * (size_t)n), "key stash");
    KICHK(hipMalloc(&st->words, 4 * 3 * (size_t)n), "key stash index");
    st->n = n;
    hipStream_t s = ctx->stream;
    uint32_t* d_slot = st->words + n;
    KICHK(hipMemcpyAsync(d_slot, snap_slot, 4 * (size_t)n, hipMemcpyHostToDevice, s), "key stash upload");
    (void)hipGetLastError();
    k_key_gather<<<key_grid(ctx, n), 256, 0, s>>>(d_slot, n, old.state, old.pub, old.nslots, f0, f1, st->key, st->words);
    KICHK(hipGetLastError(), "k_key_gather launch");
    KICHK(hipStreamSynchronize(s), "key stash gather");
    return HD_OK;
}

int hd_key_stash_carry(hd_ctx* ctx, const FbKeyStash& st, const std::pair<uint32_t, uint32_t>* carry, uint32_t n,
                       const FbKeyView& now) {
    if (n == 0) return HD_OK;
    if (!st.key || !st.words || n > st.n || !now.state || !now.pub) return HD_EINVAL;
    std::vector<uint32_t> pairs(2 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        pairs[2 * i] = carry[i].first;
        pairs[2 * i + 1] = carry[i].second;
    }
    hipStream_t s = ctx->stream;
    uint32_t* d_pairs = st.words + st.n;
    KICHK(hipMemcpyAsync(d_pairs, pairs.data(), 4 * pairs.size(), hipMemcpyHostToDevice, s), "key carry upload");
    (void)hipGetLastError();
    k_key_carry<<<key_grid(ctx, n), 256, 0, s>>>(d_pairs, n, st.n, st.key, st.words, now.nslots, now.pub, now.state);
    KICHK(hipGetLastError(), "k_key_carry launch");
    KICHK(hipStreamSynchronize(s), "key carry");   // (pairs is read until then)
    return HD_OK;
}

void hd_key_stash_free(FbKeyStash* st) {
    if (st->key) (void)hipFree(st->key);
    if (st->words) (void)hipFree(st->words);
    *st = FbKeyStash{};
}

extern "C" {

int hd_import_keys(hd_ctx* ctx, const uint8_t* keys64, uint32_t n, uint8_t* status, int32_t* signer) {
    if (!ctx) return HD_EINVAL;
    if (n == 0) return HD_OK;
    if (!keys64 || !status) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    int rc = hd_ctx_quiesce(ctx);
    if (rc) return rc;
    // the context's host-batch buffers are idle after the quiesce: the keys
    // go where a batch's signatures go, the outputs where its signatories go
    // (signer and slot per row, 4-byte aligned, then the status bytes)
    DevBuf& in = ctx->bufs[BUF_SIG];
    DevBuf& out = ctx->bufs[BUF_REC];
    rc = hd_dev_grow(ctx, &in.p, &in.cap, 64 * (size_t)n);
    if (!rc) rc = hd_dev_grow(ctx, &out.p, &out.cap, 9 * (size_t)n);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint8_t* d_keys = (const uint8_t*)in.p;
    int32_t* d_signer = (int32_t*)out.p;
    int32_t* d_slot = d_signer + n;
    uint8_t* d_status = (uint8_t*)(d_slot + n);
    KICHK(hipMemcpyAsync(in.p, keys64, 64 * (size_t)n, hipMemcpyHostToDevice, s), "key upload");
    // no slot map with the fast path off: an admitted key is NO_SLOT
    FbKeyView v{nullptr, nullptr, nullptr, 0};
    const bool view = ctx->fastpath && hd_fb_key_view(ctx, &v);
    const uint32_t g = key_grid(ctx, n);
    (void)hipGetLastError();   // an error some earlier call left in this thread is not this launch's
#define HD_LAUNCH_IMPORT(C)                                                                                       \
    k_key_import<C><<<g, 256, 0, s>>>(d_keys, n, hd_adm_index(ctx), ctx->n_adm, ctx->d_adm_perm, v.adm_slot,     \
                                      v.nslots, v.state, d_status, d_signer, d_slot)
    if (ctx->pkfmt == HD_PUBKEY_COMPRESSED) HD_LAUNCH_IMPORT(1);
    else if (ctx->pkfmt == HD_PUBKEY_RAW64) HD_LAUNCH_IMPORT(2);
    else if (ctx->pkfmt == HD_PUBKEY_XY_STRIPPED) HD_LAUNCH_IMPORT(3);
    else HD_LAUNCH_IMPORT(0);
#undef HD_LAUNCH_IMPORT
    KICHK(hipGetLastError(), "k_key_import launch");
    if (view) {
        k_key_publish<<<g, 256, 0, s>>>(d_keys, n, d_slot, v.state, v.pub);
        KICHK(hipGetLastError(), "k_key_publish launch");
    }
    KICHK(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, s), "key status download");
    if (signer) KICHK(hipMemcpyAsync(signer, d_signer, 4 * (size_t)n, hipMemcpyDeviceToHost, s), "key signer download");
    if (view) return hd_fb_learn_sync(ctx);
    KICHK(hipStreamSynchronize(s), "key import");
    return HD_OK;
}

int hd_export_keys(hd_ctx* ctx, uint8_t* keys64, uint8_t* known, uint32_t cap, uint32_t* n_out) {
    if (!ctx || !n_out) return HD_EINVAL;
    const uint32_t n = ctx->n_sig_caller;
    *n_out = n;
    if (cap < n) return HD_ECAP;
    if (n == 0) return HD_OK;
    if (!keys64 || !known) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    int rc = hd_ctx_quiesce(ctx);
    if (rc) return rc;
    DevBuf& out = ctx->bufs[BUF_REC];
    rc = hd_dev_grow(ctx, &out.p, &out.cap, 65 * (size_t)n);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* d_keys = (uint8_t*)out.p;
    uint8_t* d_known = d_keys + 64 * (size_t)n;
    FbKeyView v{nullptr, nullptr, nullptr, 0};
    const bool view = hd_fb_key_view(ctx, &v);
    (void)hipGetLastError();   // an error some earlier call left in this thread is not this launch's
    k_key_export<<<key_grid(ctx, n), 256, 0, s>>>(ctx->d_sig_caller, n, hd_adm_index(ctx), ctx->n_adm, view, v.adm_slot,
                                                  v.nslots, v.state, v.pub, d_keys, d_known);
    KICHK(hipGetLastError(), "k_key_export launch");
    std::vector<uint8_t> host(65 * (size_t)n);
    KICHK(hipMemcpyAsync(host.data(), out.p, host.size(), hipMemcpyDeviceToHost, s), "key download");
    KICHK(hipStreamSynchronize(s), "key export");
    memcpy(keys64, host.data(), 64 * (size_t)n);
    memcpy(known, host.data() + 64 * (size_t)n, n);
    return HD_OK;
}

}  // extern "C"
