// hd_fastsums.hip -- k_fast_sums, the known-key check's u1 G + u2 P (the split check's kernels and their
// order: hd_fastverify.hip), and the launch of the form a call's plan names.
#include <hip/hip_runtime.h>

#include "hd_fbwork.h"
#include "hd_inv2.h"
#include "hd_scmont.h"

using namespace hd;

namespace {

// u1 G + u2 P from the digit rows: the first G window's point starts the
// sum (no addition), then one mixed addition per further window, the next
// point loaded one addition ahead.  A zero digit contributes nothing; while
// no digit has been non-zero the sum is the point at infinity.  Zero digits
// are rare (~2^-W per window), so the selects they need run only in a
// wavefront that has one (a uniform branch); every other step is the bare
// addition.  (Sending such messages to the full recovery instead costs a
// whole recovery's latency per verify call: measured 1.95 -> 3.0 ms per 1M.)
// The sums are XYZZ (gxz, hd_fixedbase.h: 8M + 2S per addition).
// One window step (gxz_sum_step, hd_fixedbase.h): dst = src + the window's
// point; the repair branch runs in a wavefront with a zero digit or a
// not-yet-started sum.
template <bool FIRST>
HD void sum_add(gxz& dst, const gxz& src, bool& started, const ge& p0, const ge& g, uint32_t ec) {
    const bool nz = !(ec & HD_REF_ZERO);
    const bool rare = __ballot(!(started && nz)) != 0ull;
    gxz_sum_step<FIRST>(dst, src, started, p0, g, (ec & HD_REF_NEG) != 0, nz, rare);
}

// the window digits of u1 = m / s and u2 = r / s (Montgomery products with
// s^-1 R come out plain) as table references: G windows, then P windows;
// dst[w * stride] for window w
template <int WP>
HD void fast_digit_refs(uint32_t* dst, size_t stride, const SplitRows& rows, uint32_t n, uint32_t i) {
    sm sinv, x;
    soa_load(sinv.n, rows.pre, n, i);
    sc u;
    soa_load(u.v, rows.u1, n, i);
    sm_from_sc(x, u);
    sm_mul(x, x, sinv);
    sm_to_sc(u, x);
    HD_UNROLL for (int w = 0; w < FbL<HD_FB_WG>::NWIN; w++)
        dst[(size_t)w * stride] = fb_ref<HD_FB_WG>(fb_digit<HD_FB_WG>(u, w), w);
    soa_load(u.v, rows.u2, n, i);
    sm_from_sc(x, u);
    sm_mul(x, x, sinv);
    sm_to_sc(u, x);
    HD_UNROLL for (int w = 0; w < FbL<WP>::NWIN; w++)
        dst[(size_t)(FbL<HD_FB_WG>::NWIN + w) * stride] = fb_ref<WP>(fb_digit<WP>(u, w), w);
}

// a table point read through a global (address space 1) pointer (k_fast_sums)
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(1))) const gp gp_global;
#else
typedef const gp gp_global;
#endif

// The digits are computed here, into this lane's column of an LDS array (no
// digit pass, no digit rows in HBM).
template <int WAVES, int WP>
__global__ __launch_bounds__(256, WAVES) void k_fast_sums(uint32_t n, const gp* __restrict__ gtab,
                                                          const gp* const* __restrict__ tabs, SplitRows rows) {
    constexpr int NG = FbL<HD_FB_WG>::NWIN, NT = NG + FbL<WP>::NWIN;
    // prefetch depth: one addition ahead; the 4-wave form loads the point when it is used
    // (two ahead spilt and lost, 0.97-0.99 of this: DESIGN.md §5 round 12)
    constexpr int PF = WAVES == 4 ? 0 : 1;
    __shared__ uint32_t sdig[NT * 256];
    // lane i takes compact slot i; the grid is sized for n, and the waves past
    // the slots in use exit here
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows.cnt[2]) return;
    const uint32_t a = rows.aux[i];
    if ((a & 0xFFu) != HD_FAST_LIVE) return;
    // The table pointers as global (address space 1) pointers: the loads
    // are then global_load (counted in vmcnt only).  A flat load -- what a
    // pointer read from memory (tabs[]) compiles to -- also counts in
    // lgkmcnt, so the wait for the next digit's LDS read would wait for the
    // point prefetched one addition ahead as well, exposing its latency.
    const gp_global* gt = (const gp_global*)gtab;
    const gp_global* pt = (const gp_global*)tabs[a >> 8];
    // a lane reads back only its own column: no barrier
    const size_t dstride = 256;
    const uint32_t* dp = sdig + threadIdx.x;
    fast_digit_refs<WP>(sdig + threadIdx.x, 256, rows, n, i);
    uint32_t e = dp[0];
    gxz acc;
    ge p0;
    gp_unpack(p0, gt[e & HD_REF_IDX]);
    if (e & HD_REF_NEG) fe_neg(p0.y, p0.y);
    fe_norm_weak(p0.y);
    gxz_set_ge(acc, p0);
    bool started = !(e & HD_REF_ZERO);   // (while not started, acc is never read)
    // The next window's point, packed (16 words) until used; the digit of
    // the window after it is read one addition earlier still, so no load
    // waits on another load inside an addition.  Window indices past the
    // last are clamped to it (a wasted but valid load), so every load is
    // unconditional and lands straight in the registers that carry it.
    auto tab = [&](int w) { return w < NG ? gt : pt; };
    auto dig = [&](int w) { return dp[(size_t)(w < NT - 1 ? w : NT - 1) * dstride]; };
    uint32_t c1 = dig(1), dn = 0;
    gp q1;
    if (PF > 0) q1 = gt[c1 & HD_REF_IDX];
    if (PF > 0) dn = dig(PF + 1);
    // window j's point and digit reference, advancing the prefetch queue
    // (PF = 0: loaded when used; the other waves of the SIMD cover the wait)
    auto advance = [&](int j, gp& cur, uint32_t& ec) {
        if (PF == 0) {
            ec = j == 1 ? c1 : dig(j);
            cur = tab(j)[ec & HD_REF_IDX];
            return;
        }
        cur = q1;
        ec = c1;
        c1 = dn;
        q1 = tab(j + 1 < NT ? j + 1 : NT - 1)[c1 & HD_REF_IDX];
        dn = dig(j + PF + 1);
    };
    // two accumulators in turn (gxz_sum_step): window 1 into b, then a, b, ...
    gxz b;
    auto step = [&](int j, gxz& dst, const gxz& src) {
        gp cur;
        uint32_t ec;
        advance(j, cur, ec);
        ge g;
        gp_unpack(g, cur);
        if (j == 1) sum_add<true>(dst, src, started, p0, g, ec);
        else sum_add<false>(dst, src, started, p0, g, ec);
    };
    step(1, b, acc);
    HD_NOUNROLL for (int j = 2; j + 1 < NT; j += 2) {
        step(j, acc, b);
        step(j + 1, b, acc);
    }
    if constexpr ((NT - 2) % 2 == 1) step(NT - 1, acc, b);   // an odd number of windows after the first two
    else acc = b;
    // infinity, or a degenerate addition on the way (ZZ = 0): full recovery
    if (!started || gxz_is_inf(acc)) {
        rows.aux[i] = (a & ~0xFFu) | HD_NEEDS_SLOW;
        return;
    }
    // (X ZZZ, Y ZZ, ZZ ZZZ): k_fast_zinv inverts the third like a Jacobian Z
    fe xn, yn, t;
    gxz_finish(xn, yn, t, acc);
    soa_store(rows.xyz, n, i, xn.n);
    soa_store(rows.xyz + 9 * (size_t)n, n, i, yn.n);
    soa_store(rows.xyz + 18 * (size_t)n, n, i, t.n);
}

// HD_VAR_SUM_CAP: the dynamic LDS that holds the 3-wave k_fast_sums at two
// 256-lane blocks per CU (two waves per SIMD, 2 x 168 of its 512 VGPRs; 176
// stay free for other kernels' waves).  A block reserves HD_SUMS_CAP_LDS in
// all, `stat` bytes of it the kernel's own digit array: two such blocks fit
// the CU's 160 KiB (MI355X: HD_CU_LDS) and a third does not, whatever the
// allocation granule up to 4 KiB, and 40 KiB stay for the other kernels'
// blocks (under 1 KiB each).  The kernel never addresses the reservation.
#define HD_CU_LDS (160u * 1024u)
#define HD_SUMS_CAP_LDS (60u * 1024u)
static_assert(2 * HD_SUMS_CAP_LDS <= HD_CU_LDS && 3 * HD_SUMS_CAP_LDS > HD_CU_LDS + 2 * 4096, "two blocks per CU");
static_assert(HD_SUMS_CAP_LDS <= 64u * 1024u, "the LDS limit of one block");
template <int WP>
static constexpr size_t sums_cap_lds() {
    constexpr size_t stat = 4 * 256 * (size_t)(FbL<HD_FB_WG>::NWIN + FbL<WP>::NWIN);   // k_fast_sums' sdig
    static_assert(stat < HD_SUMS_CAP_LDS, "k_fast_sums' digit array exceeds the capped block's LDS");
    return HD_SUMS_CAP_LDS - stat;
}

}  // namespace

// the plan's k_fast_sums form (waves per SIMD), the 3-wave form with the
// residency cap where the plan says so
void fb_launch_sums(const FbCallPlan& p, int wp, uint32_t blocks, hipStream_t s, uint32_t n, const gp* gtab,
                    const gp* const* tabs, const SplitRows& rows) {
    with_width(wp, [&](auto w) {
        constexpr int WP = decltype(w)::value;
        const size_t cap = p.capped ? sums_cap_lds<WP>() : 0;
        if (p.sums_waves == 2) k_fast_sums<2, WP><<<blocks, 256, 0, s>>>(n, gtab, tabs, rows);
        else if (p.sums_waves == 4) k_fast_sums<4, WP><<<blocks, 256, 0, s>>>(n, gtab, tabs, rows);
        else k_fast_sums<3, WP><<<blocks, 256, cap, s>>>(n, gtab, tabs, rows);
    });
}
