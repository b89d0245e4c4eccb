// hd_certcheck.hip -- hd_check_certificates (include/hd_cert.h): K quorum
// certificates, each a segment of one verified batch, decided in one launch.
// The arithmetic and the plan are hd_certcheck.h, which the host tests run as
// plain C++; this file is the kernel around it and the ABI.  Second half:
// hd_check_certificates_sets, the same check with every certificate under the
// signatory set it names (an hd_sigsets; the lookup is hd_sigsets.h).
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "hd_certcheck.h"
#include "hd_internal.h"
#include "hd_sigsets.h"

using namespace hd;

// the context's buffers of the check (hd_ctx::cert)
struct CertWork {
    DevBuf rows;      // K certificate rows (the sets form: then K set ids), then K result rows
    DevBuf scratch;   // the tables of the scratch placement: CERT_EMPTY between calls
    uint32_t lds_limit = 0;
    std::vector<char> stage;   // the sets form's one upload: K rows, then K set ids
};

namespace {

#define CCHK(expr, what)                                       \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hd_ctx_fail(ctx, e_, what); \
    } while (0)

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    for (int d = CERT_WAVE / 2; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
    for (int d = CERT_WAVE / 2; d > 0; d >>= 1) x = cert_min(x, __shfl_xor(x, d));
    return x;
}

// LDS: the table is the dynamic LDS of the block (plan.lds_bytes), set to
// CERT_EMPTY when the block starts; otherwise slice blockIdx of `scratch`
// (slice_words each), which is CERT_EMPTY between launches.  Either way the
// block itself leaves the table as it found it after every certificate.
template <bool LDS>
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_check(const uint8_t* __restrict__ type,
                                                           const int64_t* __restrict__ height,
                                                           const int64_t* __restrict__ round,
                                                           const uint8_t* __restrict__ value32,
                                                           const uint32_t* __restrict__ bitmap,
                                                           const int32_t* __restrict__ signer, uint32_t n_signers,
                                                           const hd_cert* __restrict__ certs, uint32_t K,
                                                           hd_cert_result* __restrict__ res, uint32_t* scratch,
                                                           uint64_t slice_words) {
    extern __shared__ uint32_t lds_tab[];
    __shared__ hd_cert s_cert;
    __shared__ uint32_t s_good, s_bad;
    const uint32_t tid = threadIdx.x;
    uint32_t* tab = LDS ? lds_tab : scratch + (uint64_t)blockIdx.x * slice_words;
    if (LDS)
        for (uint32_t e = tid; e < n_signers; e += CERT_BLOCK) tab[e] = CERT_EMPTY;
    for (uint32_t k = blockIdx.x; k < K; k += gridDim.x) {
        // the certificate's 64-byte row: 16 lanes, one dword each, once per block
        if (tid < sizeof(hd_cert) / 4) reinterpret_cast<uint32_t*>(&s_cert)[tid] = reinterpret_cast<const uint32_t*>(certs + k)[tid];
        if (tid == 0) {
            s_good = 0;
            s_bad = CERT_EMPTY;
        }
        __syncthreads();   // the row and the accumulators; on the first certificate also the table
        const CertKey key = cert_key(s_cert);
        const uint32_t first = s_cert.first, count = s_cert.count;   // first + count <= n: cert_row_ok
        uint32_t good = 0, bad = HD_WHEN_NEVER;
        for (uint64_t j = tid; j < count; j += CERT_BLOCK) {   // 64 bits: j + 256 may pass 2^32
            const uint32_t i = first + (uint32_t)j;
            uint32_t s;
            if (cert_class(key, type, height, round, value32, bitmap, signer, n_signers, i, &s) == CERT_CLEAN)
                cert_first(atomicMin(&tab[s], i), i, &good, &bad);   // s < n_signers: cert_valid
            else
                bad = cert_min(bad, i);
        }
        good = wave_sum(good);
        bad = wave_min(bad);
        if ((tid & (CERT_WAVE - 1)) == 0) {
            if (good) atomicAdd(&s_good, good);
            if (bad != HD_WHEN_NEVER) atomicMin(&s_bad, bad);
        }
        __syncthreads();   // every atomicMin on the table is done; the accumulators are final
        // the restore: only the message whose index an entry holds writes it
        for (uint64_t j = tid; j < count; j += CERT_BLOCK) {
            const uint32_t i = first + (uint32_t)j;
            uint32_t s;
            if (cert_valid(bitmap, signer, i, n_signers, &s)) (void)atomicCAS(&tab[s], i, (uint32_t)CERT_EMPTY);
        }
        if (tid == 0) {
            const uint32_t b = s_bad;
            uint32_t s, cls = CERT_CLEAN;
            if (b != HD_WHEN_NEVER) cls = cert_class(key, type, height, round, value32, bitmap, signer, n_signers, b, &s);
            hd_cert_result r;
            r.status = cert_status(count, s_cert.quorum, b, cls);
            r.good = s_good;
            r.first_bad = b;
            r.reserved = 0;
            res[k] = r;
        }
        __syncthreads();   // the table is restored and the row read before the next certificate replaces it
    }
}

// hd_check_certificates_sets: the same sweeps, with the table index of a message
// looked up in the set its certificate names (hd_sigsets.h certset_class).  The
// table has n_max words, the largest distinct count among the sets the call
// names; a certificate of a smaller set uses the head of it.  A lane keeps the
// indices of its first CERTSET_KEEP messages in registers for the restore;
// which lane holds an index changes nothing the table or the accumulators see.
template <bool LDS>
__global__ __launch_bounds__(CERT_BLOCK) void k_cert_check_sets(
    const uint8_t* __restrict__ type, const int64_t* __restrict__ height, const int64_t* __restrict__ round,
    const uint8_t* __restrict__ value32, const uint8_t* __restrict__ from32, const uint8_t* __restrict__ verdict,
    const uint32_t* __restrict__ words, const uint32_t* __restrict__ slots, const SigSetDesc* __restrict__ desc,
    uint32_t n_max, const hd_cert* __restrict__ certs, const uint32_t* __restrict__ set_of, uint32_t K,
    hd_cert_result* __restrict__ res, uint32_t* scratch, uint64_t slice_words) {
    extern __shared__ uint32_t lds_tab[];
    __shared__ hd_cert s_cert;
    __shared__ SigSetDesc s_desc;
    __shared__ uint32_t s_good, s_bad;
    const uint32_t tid = threadIdx.x;
    uint32_t* tab = LDS ? lds_tab : scratch + (uint64_t)blockIdx.x * slice_words;
    if (LDS)
        for (uint32_t e = tid; e < n_max; e += CERT_BLOCK) tab[e] = CERT_EMPTY;
    for (uint32_t k = blockIdx.x; k < K; k += gridDim.x) {
        if (tid < sizeof(hd_cert) / 4) reinterpret_cast<uint32_t*>(&s_cert)[tid] = reinterpret_cast<const uint32_t*>(certs + k)[tid];
        if (tid == 0) {
            s_desc = desc[set_of[k]];   // set_of[k] names a set of the object: checked before the launch
            s_good = 0;
            s_bad = CERT_EMPTY;
        }
        __syncthreads();   // the row, the set and the accumulators; on the first certificate also the table
        const CertKey key = cert_key(s_cert);
        const CertSet st = certset_of(words, slots, s_desc);
        const uint32_t first = s_cert.first, count = s_cert.count;   // first + count <= n: cert_row_ok
        uint32_t good = 0, bad = HD_WHEN_NEVER;
        uint32_t keep[CERTSET_KEEP];   // the table index of a clean message, CERT_EMPTY otherwise
#pragma unroll
        for (uint32_t r = 0; r < CERTSET_KEEP; r++) {
            const uint32_t j = tid + r * CERT_BLOCK;
            keep[r] = CERT_EMPTY;
            if (j < count) {
                const uint32_t i = first + j;
                uint32_t s;
                if (certset_class(key, type, height, round, value32, st, verdict, from32, i, &s) == CERT_CLEAN) {
                    cert_first(atomicMin(&tab[s], i), i, &good, &bad);   // s < s_desc.n <= n_max
                    keep[r] = s;
                } else {
                    bad = cert_min(bad, i);
                }
            }
        }
        for (uint64_t j = tid + (uint64_t)CERTSET_KEEP * CERT_BLOCK; j < count; j += CERT_BLOCK) {
            const uint32_t i = first + (uint32_t)j;
            uint32_t s;
            if (certset_class(key, type, height, round, value32, st, verdict, from32, i, &s) == CERT_CLEAN)
                cert_first(atomicMin(&tab[s], i), i, &good, &bad);
            else
                bad = cert_min(bad, i);
        }
        good = wave_sum(good);
        bad = wave_min(bad);
        if ((tid & (CERT_WAVE - 1)) == 0) {
            if (good) atomicAdd(&s_good, good);
            if (bad != HD_WHEN_NEVER) atomicMin(&s_bad, bad);
        }
        __syncthreads();   // every atomicMin on the table is done; the accumulators are final
        // the restore: only the message whose index an entry holds writes it
#pragma unroll
        for (uint32_t r = 0; r < CERTSET_KEEP; r++)
            if (keep[r] != CERT_EMPTY) (void)atomicCAS(&tab[keep[r]], first + tid + r * CERT_BLOCK, (uint32_t)CERT_EMPTY);
        for (uint64_t j = tid + (uint64_t)CERTSET_KEEP * CERT_BLOCK; j < count; j += CERT_BLOCK) {
            const uint32_t i = first + (uint32_t)j;
            uint32_t s;
            if (certset_member(st, verdict, from32, i, &s) == CERT_CLEAN) (void)atomicCAS(&tab[s], i, (uint32_t)CERT_EMPTY);
        }
        if (tid == 0) {
            const uint32_t b = s_bad;
            uint32_t s, cls = CERT_CLEAN;
            if (b != HD_WHEN_NEVER) cls = certset_class(key, type, height, round, value32, st, verdict, from32, b, &s);
            hd_cert_result r;
            r.status = certset_status(count, s_cert.quorum, b, cls);
            r.good = s_good;
            r.first_bad = b;
            r.reserved = 0;
            res[k] = r;
        }
        __syncthreads();   // the table is restored and the row read before the next certificate replaces it
    }
}

int cert_work(hd_ctx* ctx, CertWork** out) {
    if (!ctx->cert) {
        CertWork* w = new (std::nothrow) CertWork();
        if (!w) return HD_ENOMEM;
        // what one workgroup may allocate: CDNA4's figure, or less where the device reports less
        hipDeviceProp_t prop;
        w->lds_limit = CERT_LDS_CDNA4;
        if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess)
            w->lds_limit = (uint32_t)std::min<size_t>(prop.sharedMemPerBlock, CERT_LDS_CDNA4);
        ctx->cert = w;
    }
    *out = ctx->cert;
    return HD_OK;
}

bool rows_ok(const hd_cert* certs, uint32_t K, uint32_t n) {
    for (uint32_t k = 0; k < K; k++)
        if (!cert_row_ok(certs[k], n)) return false;
    return true;
}

// everything after the argument checks: upload, one launch, download; no synchronisation
int cert_queue(hd_ctx* ctx, const hd_batch* db, const uint32_t* d_bitmap, const int32_t* d_signer, uint32_t n_signers,
               const hd_cert* certs, uint32_t K, hd_cert_result* results, hipStream_t s) {
    CertWork* w;
    int rc = cert_work(ctx, &w);
    if (rc) return rc;
    const hd_cert_plan p = cert_plan(n_signers, K, w->lds_limit);
    const size_t in_bytes = sizeof(hd_cert) * (size_t)K, out_bytes = sizeof(hd_cert_result) * (size_t)K;
    rc = hd_dev_grow(ctx, &w->rows.p, &w->rows.cap, in_bytes + out_bytes);
    if (rc) return rc;
    if (p.scratch_bytes > w->scratch.cap) {
        rc = hd_dev_grow(ctx, &w->scratch.p, &w->scratch.cap, (size_t)p.scratch_bytes);
        if (rc) return rc;
        // a new allocation starts EMPTY; from here on the blocks keep it so
        CCHK(hipMemsetAsync(w->scratch.p, 0xFF, w->scratch.cap, s), "certificate scratch");
    }
    hd_cert* d_certs = (hd_cert*)w->rows.p;
    hd_cert_result* d_res = (hd_cert_result*)((char*)w->rows.p + in_bytes);
    CCHK(hipMemcpyAsync(d_certs, certs, in_bytes, hipMemcpyHostToDevice, s), "certificate upload");
    if (p.in_lds) {
        if (p.lds_bytes > 48u * 1024u)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cert_check<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        k_cert_check<true><<<p.blocks, CERT_BLOCK, p.lds_bytes, s>>>(db->type, db->height, db->round, db->value32, d_bitmap,
                                                                   d_signer, n_signers, d_certs, K, d_res, nullptr, 0);
    } else {
        k_cert_check<false><<<p.blocks, CERT_BLOCK, 0, s>>>(db->type, db->height, db->round, db->value32, d_bitmap,
                                                           d_signer, n_signers, d_certs, K, d_res,
                                                           (uint32_t*)w->scratch.p, p.slice_bytes / 4);
    }
    CCHK(hipGetLastError(), "k_cert_check");
    CCHK(hipMemcpyAsync(results, d_res, out_bytes, hipMemcpyDeviceToHost, s), "certificate download");
    return HD_OK;
}

// What the sets form refuses beside the rows: a set id the object does not hold.  *n_max: the largest
// distinct count among the sets named, which sizes the table.
bool sets_ok(const hd_sigsets* sets, const uint32_t* set_of, uint32_t K, uint32_t* n_max) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < K; k++) {
        if (set_of[k] >= sets->desc.size()) return false;
        m = std::max(m, sets->desc[set_of[k]].n);
    }
    *n_max = m;
    return true;
}

// the sets form after the argument checks: one upload, one launch, one download; no synchronisation
int cert_queue_sets(hd_ctx* ctx, const hd_sigsets* sets, const hd_batch* db, const uint8_t* d_verdict,
                    const hd_cert* certs, const uint32_t* set_of, uint32_t K, uint32_t n_max, hd_cert_result* results,
                    hipStream_t s) {
    CertWork* w;
    int rc = cert_work(ctx, &w);
    if (rc) return rc;
    const hd_cert_plan p = cert_plan(n_max, K, w->lds_limit);
    const size_t row_bytes = sizeof(hd_cert) * (size_t)K, id_bytes = (4 * (size_t)K + 15) & ~(size_t)15,
                 out_bytes = sizeof(hd_cert_result) * (size_t)K;
    try {
        w->stage.resize(row_bytes + id_bytes);
    } catch (const std::bad_alloc&) {
        return HD_ENOMEM;
    }
    memcpy(w->stage.data(), certs, row_bytes);
    memcpy(w->stage.data() + row_bytes, set_of, 4 * (size_t)K);
    rc = hd_dev_grow(ctx, &w->rows.p, &w->rows.cap, row_bytes + id_bytes + out_bytes);
    if (rc) return rc;
    if (p.scratch_bytes > w->scratch.cap) {
        rc = hd_dev_grow(ctx, &w->scratch.p, &w->scratch.cap, (size_t)p.scratch_bytes);
        if (rc) return rc;
        CCHK(hipMemsetAsync(w->scratch.p, 0xFF, w->scratch.cap, s), "certificate scratch");
    }
    hd_cert* d_certs = (hd_cert*)w->rows.p;
    const uint32_t* d_ids = (const uint32_t*)((char*)w->rows.p + row_bytes);
    hd_cert_result* d_res = (hd_cert_result*)((char*)w->rows.p + row_bytes + id_bytes);
    // the staging copy stays as it is until the caller's synchronisation: one call at a time per context
    CCHK(hipMemcpyAsync(d_certs, w->stage.data(), row_bytes + id_bytes, hipMemcpyHostToDevice, s), "certificate upload");
    if (p.in_lds) {
        if (p.lds_bytes > 48u * 1024u)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cert_check_sets<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        k_cert_check_sets<true><<<p.blocks, CERT_BLOCK, p.lds_bytes, s>>>(
            db->type, db->height, db->round, db->value32, db->from32, d_verdict, sets->d_words, sets->d_slots,
            sets->d_desc, n_max, d_certs, d_ids, K, d_res, nullptr, 0);
    } else {
        k_cert_check_sets<false><<<p.blocks, CERT_BLOCK, 0, s>>>(
            db->type, db->height, db->round, db->value32, db->from32, d_verdict, sets->d_words, sets->d_slots,
            sets->d_desc, n_max, d_certs, d_ids, K, d_res, (uint32_t*)w->scratch.p, p.slice_bytes / 4);
    }
    CCHK(hipGetLastError(), "k_cert_check_sets");
    CCHK(hipMemcpyAsync(results, d_res, out_bytes, hipMemcpyDeviceToHost, s), "certificate download");
    return HD_OK;
}

}  // namespace

void hd_cert_release(hd_ctx* ctx) {
    CertWork* w = ctx->cert;
    if (!w) return;
    if (w->rows.p) (void)hipFree(w->rows.p);
    if (w->scratch.p) (void)hipFree(w->scratch.p);
    delete w;
    ctx->cert = nullptr;
}

extern "C" {

int hd_check_certificates_device(hd_ctx* ctx, const hd_batch* db, const uint32_t* d_valid_bitmap,
                                 const int32_t* d_signer, uint32_t n_signers, const hd_cert* certs, uint32_t K,
                                 hd_cert_result* results, void* stream) {
    if (!ctx || !db) return HD_EINVAL;
    if (K == 0) return HD_OK;
    if (!certs || !results) return HD_EINVAL;
    if (db->n && (!db->type || !db->height || !db->round || !db->value32 || !d_valid_bitmap || !d_signer))
        return HD_EINVAL;
    if ((((uintptr_t)db->height | (uintptr_t)db->round) & 7u) || (((uintptr_t)d_valid_bitmap | (uintptr_t)d_signer) & 3u))
        return HD_EINVAL;
    if (!rows_ok(certs, K, db->n)) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int rc = cert_queue(ctx, db, d_valid_bitmap, d_signer, n_signers, certs, K, results, s);
    if (rc) return rc;
    CCHK(hipStreamSynchronize(s), "certificate check");
    return hd_ctx_note_stream(ctx, s);
}

int hd_check_certificates(hd_ctx* ctx, const hd_batch* batch, const hd_cert* certs, uint32_t K,
                          hd_cert_result* results, uint8_t* verdict) {
    if (!ctx || !batch) return HD_EINVAL;
    const uint32_t n = batch->n;
    if (n && (!batch->type || !batch->height || !batch->round || !batch->value32 || !batch->from32 || !batch->sig65))
        return HD_EINVAL;
    if (K && (!certs || !results || !rows_ok(certs, K, n))) return HD_EINVAL;
    if (K == 0 && (!verdict || n == 0)) return HD_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    hd_batch db = {};
    uint8_t* d_v = nullptr;
    int32_t* d_s = nullptr;
    uint32_t* d_b = nullptr;
    if (n) {
        int rc = hd_upload_batch(ctx, batch, &db);
        if (!rc) rc = hd_dev_grow(ctx, &ctx->bufs[BUF_VERDICT].p, &ctx->bufs[BUF_VERDICT].cap, n);
        if (!rc) rc = hd_dev_grow(ctx, &ctx->bufs[BUF_SIGNER].p, &ctx->bufs[BUF_SIGNER].cap, 4 * (size_t)n);
        if (!rc) rc = hd_dev_grow(ctx, &ctx->bufs[BUF_BITMAP].p, &ctx->bufs[BUF_BITMAP].cap, 4 * (((size_t)n + 31) / 32));
        if (rc) return rc;
        d_v = (uint8_t*)ctx->bufs[BUF_VERDICT].p;
        d_s = (int32_t*)ctx->bufs[BUF_SIGNER].p;
        d_b = (uint32_t*)ctx->bufs[BUF_BITMAP].p;
        rc = hd_verify_batch_device(ctx, &db, d_v, nullptr, d_s, d_b, s);
        if (rc) return rc;
    }
    if (K) {
        // the signer index names a row of the array given to hd_set_signatories
        const int rc = cert_queue(ctx, &db, d_b, d_s, ctx->n_sig_caller, certs, K, results, s);
        if (rc) return rc;
    }
    if (verdict && n) CCHK(hipMemcpyAsync(verdict, d_v, n, hipMemcpyDeviceToHost, s), "certificate verdicts");
    CCHK(hipStreamSynchronize(s), "certificate check");
    return HD_OK;
}

int hd_check_certificates_sets_device(hd_ctx* ctx, const hd_sigsets* sets, const hd_batch* db, const uint8_t* d_verdict,
                                      const hd_cert* certs, const uint32_t* set_of, uint32_t K,
                                      hd_cert_result* results, void* stream) {
    if (!ctx || !sets || !db || sets->ctx != ctx) return HD_EINVAL;
    if (K == 0) return HD_OK;
    if (!certs || !set_of || !results) return HD_EINVAL;
    if (db->n && (!db->type || !db->height || !db->round || !db->value32 || !db->from32 || !d_verdict)) return HD_EINVAL;
    if ((((uintptr_t)db->height | (uintptr_t)db->round) & 7u) || (((uintptr_t)db->value32 | (uintptr_t)db->from32) & 15u))
        return HD_EINVAL;
    uint32_t n_max = 0;
    if (!rows_ok(certs, K, db->n) || !sets_ok(sets, set_of, K, &n_max)) return HD_EINVAL;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    int rc = cert_queue_sets(ctx, sets, db, d_verdict, certs, set_of, K, n_max, results, s);
    if (rc) return rc;
    CCHK(hipStreamSynchronize(s), "certificate check");
    return hd_ctx_note_stream(ctx, s);
}

int hd_check_certificates_sets(hd_ctx* ctx, const hd_sigsets* sets, const hd_batch* batch, const hd_cert* certs,
                               const uint32_t* set_of, uint32_t K, hd_cert_result* results, uint8_t* verdict) {
    if (!ctx || !sets || !batch || sets->ctx != ctx) return HD_EINVAL;
    const uint32_t n = batch->n;
    if (n && (!batch->type || !batch->height || !batch->round || !batch->value32 || !batch->from32 || !batch->sig65))
        return HD_EINVAL;
    uint32_t n_max = 0;
    if (K && (!certs || !set_of || !results || !rows_ok(certs, K, n) || !sets_ok(sets, set_of, K, &n_max))) return HD_EINVAL;
    if (K == 0 && (!verdict || n == 0)) return HD_OK;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    hd_batch db = {};
    uint8_t* d_v = nullptr;
    if (n) {
        int rc = hd_upload_batch(ctx, batch, &db);   // the context's buffers: 16-byte aligned
        if (!rc) rc = hd_dev_grow(ctx, &ctx->bufs[BUF_VERDICT].p, &ctx->bufs[BUF_VERDICT].cap, n);
        if (rc) return rc;
        d_v = (uint8_t*)ctx->bufs[BUF_VERDICT].p;
        // the verdicts only: membership is the sets', not the context's
        rc = hd_verify_batch_device(ctx, &db, d_v, nullptr, nullptr, nullptr, s);
        if (rc) return rc;
    }
    if (K) {
        const int rc = cert_queue_sets(ctx, sets, &db, d_v, certs, set_of, K, n_max, results, s);
        if (rc) return rc;
    }
    if (verdict && n) CCHK(hipMemcpyAsync(verdict, d_v, n, hipMemcpyDeviceToHost, s), "certificate verdicts");
    CCHK(hipStreamSynchronize(s), "certificate check");
    return HD_OK;
}

int hd_cert_plan_info(uint32_t n_signers, uint32_t K, hd_cert_plan* plan) {
    if (!plan) return HD_EINVAL;
    uint32_t limit = CERT_LDS_CDNA4;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        limit = (uint32_t)std::min<size_t>(prop.sharedMemPerBlock, CERT_LDS_CDNA4);
    *plan = cert_plan(n_signers, K, limit);
    return HD_OK;
}

}  // extern "C"
