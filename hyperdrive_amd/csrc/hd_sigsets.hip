// hd_sigsets.hip -- hd_sigsets (include/hd_sigsets.h): signatory sets kept on
// the device apart from the context's admitted set.  The builder and the
// placement are hd_sigsets.h, which the host tests run as plain C++; this file
// is the allocations and the ABI.  The check that reads the sets is
// hd_certcheck.hip k_cert_check_sets.
#include <new>

#include "hd_internal.h"
#include "hd_sigsets.h"

using namespace hd;

namespace {

// One device array that grows by copy: `want` bytes in a new allocation, or
// nothing when the array is large enough.
struct Grow {
    void* fresh = nullptr;
    size_t cap = 0;
};
bool grow_alloc(size_t have, size_t need, Grow* g) {
    if (need <= have) return true;
    const size_t want = std::max(need + need / 2, (size_t)4096);
    if (hipMalloc(&g->fresh, want) != hipSuccess) {
        (void)hipGetLastError();
        g->fresh = nullptr;
        return false;
    }
    g->cap = want;
    return true;
}
// the old contents into the new allocation, which replaces the old one
template <typename T>
bool grow_commit(Grow* g, T** p, size_t* cap, size_t used_bytes) {
    if (!g->fresh) return true;
    if (*p && used_bytes && hipMemcpy(g->fresh, *p, used_bytes, hipMemcpyDeviceToDevice) != hipSuccess) return false;
    if (*p) (void)hipFree(*p);
    *p = (T*)g->fresh;
    *cap = g->cap;
    g->fresh = nullptr;
    return true;
}

}  // namespace

extern "C" {

int hd_sigsets_create(hd_ctx* ctx, hd_sigsets** out) {
    if (!ctx || !out) return HD_EINVAL;
    hd_sigsets* s = new (std::nothrow) hd_sigsets();
    if (!s) return HD_ENOMEM;
    s->ctx = ctx;
    s->device = ctx->device;
    *out = s;
    return HD_OK;
}

int hd_sigsets_destroy(hd_sigsets* s) {
    if (!s) return HD_EINVAL;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();   // a check may still be queued on a caller's stream; the context is not asked
    if (s->d_words) (void)hipFree(s->d_words);
    if (s->d_slots) (void)hipFree(s->d_slots);
    if (s->d_desc) (void)hipFree(s->d_desc);
    delete s;
    return HD_OK;
}

int hd_sigsets_add(hd_sigsets* s, const uint8_t* sigs32, uint32_t n, uint32_t* set_id) {
    if (!s || !set_id || (n && !sigs32)) return HD_EINVAL;
    SigSetBuild b;
    SigSetDesc d;
    try {
        if (!sigset_build(sigs32, n, &b)) return HD_EINVAL;
        if (!sigset_place(s->rows_used, s->slots_used, s->desc.size(), b.n_distinct, (uint32_t)b.slot.size(), &d))
            return HD_EINVAL;
        s->desc.reserve(s->desc.size() + 1);
        s->n_rows.reserve(s->n_rows.size() + 1);
    } catch (const std::bad_alloc&) {
        return HD_ENOMEM;
    }
    (void)hipSetDevice(s->device);
    const size_t used_w = 32 * (size_t)s->rows_used, used_s = 4 * (size_t)s->slots_used,
                 used_d = sizeof(SigSetDesc) * s->desc.size();
    const size_t add_w = 32 * (size_t)b.n_distinct, add_s = 4 * b.slot.size();
    // every allocation before anything changes: HD_ENOMEM leaves the object as it was
    Grow gw, gs, gd;
    if (!grow_alloc(s->cap_words, used_w + add_w, &gw) || !grow_alloc(s->cap_slots, used_s + add_s, &gs) ||
        !grow_alloc(s->cap_desc, used_d + sizeof(SigSetDesc), &gd)) {
        if (gw.fresh) (void)hipFree(gw.fresh);
        if (gs.fresh) (void)hipFree(gs.fresh);
        return HD_ENOMEM;   // gd is the last one tried: it holds nothing when it failed
    }
    // No check is in flight (they return synchronised), so the copies below order against nothing; the
    // sets already there keep their offsets and their contents.
    bool ok = grow_commit(&gw, &s->d_words, &s->cap_words, used_w) && grow_commit(&gs, &s->d_slots, &s->cap_slots, used_s) &&
              grow_commit(&gd, &s->d_desc, &s->cap_desc, used_d);
    if (ok && add_w)
        ok = hipMemcpy((char*)s->d_words + used_w, b.words.data(), add_w, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = hipMemcpy((char*)s->d_slots + used_s, b.slot.data(), add_s, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = hipMemcpy((char*)s->d_desc + used_d, &d, sizeof d, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        void* left[] = {gw.fresh, gs.fresh, gd.fresh};
        for (void* p : left)
            if (p) (void)hipFree(p);
        return HD_EDEVICE;   // the sets already there are untouched; what was written lies behind them
    }
    *set_id = (uint32_t)s->desc.size();
    s->desc.push_back(d);
    s->n_rows.push_back(n);
    s->rows_used += b.n_distinct;
    s->slots_used += b.slot.size();
    return HD_OK;
}

int hd_sigsets_clear(hd_sigsets* s) {
    if (!s) return HD_EINVAL;
    s->desc.clear();
    s->n_rows.clear();
    s->rows_used = s->slots_used = 0;
    return HD_OK;
}

int hd_sigsets_info(const hd_sigsets* s, uint32_t set_id, uint32_t* n_rows, uint32_t* n_distinct) {
    if (!s || set_id >= s->desc.size()) return HD_EINVAL;
    if (n_rows) *n_rows = s->n_rows[set_id];
    if (n_distinct) *n_distinct = s->desc[set_id].n;
    return HD_OK;
}

}  // extern "C"
