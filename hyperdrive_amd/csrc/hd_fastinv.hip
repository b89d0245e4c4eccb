// hd_fastinv.hip -- the two inversions of the known-key check, K messages per lane (of s mod n before
// k_fast_sums, of Z mod p after it; the split check's kernels and their order: hd_fastverify.hip), in three
// forms each -- in registers, lean, lean in two levels (hd_inv2.h) -- and the launch of the form a call takes.
#include <hip/hip_runtime.h>

#include "hd_fbwork.h"
#include "hd_inv2.h"
#include "hd_modinv.h"
#include "hd_scmont.h"

using namespace hd;

namespace {

// K per lane: prefix products of s over the lane's live messages, one
// inversion mod n, then s^-1 of each.  The products are Montgomery products in
// radix 2^29 (hd_scmont.h, R = 2^261): with P_l = prod_{i<=l} s_i R^-l the l-th
// live prefix, inv = P_last^-1 R gives, walking back, s_l^-1 R =
// M(inv_l, P_{l-1}) and inv_{l-1} = M(inv_l, s_l).  s^-1 R leaves in the pre
// row.  The lane's K scalars and prefixes stay in registers (both walks are
// unrolled), and the loads of all K messages issue together up front: with
// n / K lanes there are too few waves to hide a load per step.
//
// The slots in use come from k_fast_prep's counter; T, the lanes of the
// K-per-lane kernels (a multiple of 64), follows from it in the kernel, so a
// batch of repeats does not spread its few slots over lanes sized for n.
// (split_lanes<K>: hd_inv2.h)

// est / stats: the first lane of a call's s inversion, whichever form, stores the call's slot count for
// the host's next launches and adds the call to the context's cumulative counters
__device__ __forceinline__ void sinv_note_call(uint32_t n, uint32_t nc, const SplitRows& rows,
                                               uint32_t* __restrict__ est, unsigned long long* __restrict__ stats) {
    const uint32_t reps = rows.cnt[3];
    if (est) {   // the call's slots, then its n (read in this order by fb_verify_impl's snapshot)
        est[1] = n;
        est[0] = nc;
    }
    if (nc + reps) atomicAdd(&stats[0], (unsigned long long)nc + reps);
    if (reps) atomicAdd(&stats[1], (unsigned long long)reps);
}

template <int K>
__global__ __launch_bounds__(256) void k_fast_sinv(uint32_t n, SplitRows rows, uint32_t* __restrict__ est,
                                                   unsigned long long* __restrict__ stats) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t == 0) sinv_note_call(n, nc, rows, est, stats);
    if (t >= T) return;
    sc sv[K];
    uint32_t live = 0;   // bit j: message j of this lane goes on
    static_for<K>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const uint32_t i = (uint32_t)j * T + t;
        const uint32_t ic = i < nc ? i : nc - 1;   // slots in use end at nc - 1 (T > 0: nc >= 1)
        const uint32_t a = rows.aux[ic];
        soa_load(sv[j].v, rows.s, n, ic);
        live |= (i < nc && (a & 0xFFu) == HD_FAST_LIVE) ? 1u << j : 0u;
    });
    if (!live) return;
    sm pre[K], acc;
    HD_UNROLL for (int k = 0; k < 9; k++) acc.n[k] = 0;
    static_for<K>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if ((live >> j) & 1u) {
            sm ss;
            sm_from_sc(ss, sv[j]);
            if (live & ((1u << j) - 1u)) sm_mul(acc, acc, ss);
            else acc = ss;
        }
        pre[j] = acc;   // the product of the live messages up to j
    });
    sm inv;
    {
        sc p, pinv;
        sm_to_sc(p, acc);
        sc_inv_divsteps(pinv, p);   // a product of scalars in [1, n) times R^-k: never 0
        sm_from_sc(inv, pinv);
        sm r2;
        sm_r2(r2);
        sm_mul(inv, inv, r2);
    }
    static_for<K>([&](auto jc) {
        constexpr int j = K - 1 - decltype(jc)::value;
        if (!((live >> j) & 1u)) return;
        const uint32_t i = (uint32_t)j * T + t;
        if (j > 0 && (live & ((1u << j) - 1u))) {   // a live message before this one
            sm sinv, ss;
            sm_mul(sinv, inv, pre[j > 0 ? j - 1 : 0]);
            sm_from_sc(ss, sv[j]);
            sm_mul(inv, inv, ss);
            soa_store(rows.pre, n, i, sinv.n);
        } else {
            soa_store(rows.pre, n, i, inv.n);
        }
    });
}

// Batch inversion over the K messages of a lane as a product tree (K a power
// of two), node[i] = node[2i] node[2i+1] with the leaves at K .. 2K-1: K - 1
// products up, one inversion of the root, 2 (K - 1) products down
// (node[2i] <- node[i] node[2i+1], node[2i+1] <- node[i] node[2i]) -- the
// product count of Montgomery's trick, but at most log2 K products on any
// dependency chain instead of 3 (K - 1): the inversion kernels run one wave
// per SIMD, where a single chain leaves the SIMD waiting on each product.
// Every index is a compile-time constant (static_for), so node[] lives in
// registers.  A message that is not live takes the leaf 1.
//
// k_fast_zinv: K per lane, Z^-1 of the lane's live sums by that product
// tree (plain field products), into the pre row.  (k_fast_sinv keeps the
// linear walk: its Montgomery-form tree needs more registers than a wave has
// and spills -- measured 90 -> 100-129 us, while the tree takes zinv 76 -> 73.)
template <int K>
__global__ __launch_bounds__(256) void k_fast_zinv(uint32_t n, SplitRows rows) {
    static_assert(K >= 2 && (K & (K - 1)) == 0, "K: a power of two");
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t >= T) return;
    const uint32_t* zrow = rows.xyz + 18 * (size_t)n;
    fe node[2 * K];
    uint32_t live = 0;
    static_for<K>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const uint32_t i = (uint32_t)j * T + t;
        const uint32_t ic = i < nc ? i : nc - 1;
        const uint32_t a = rows.aux[ic];
        fe z;
        soa_load(z.n, zrow, n, ic);
        const bool on = i < nc && (a & 0xFFu) == HD_FAST_LIVE;
        live |= on ? 1u << j : 0u;
        HD_UNROLL for (int k = 1; k < 9; k++) z.n[k] = on ? z.n[k] : 0u;
        z.n[0] = on ? z.n[0] : 1u;
        node[K + j] = z;
    });
    if (!live) return;
    static_for<K - 1>([&](auto ic) {
        constexpr int i = K - 1 - decltype(ic)::value;
        fe_mul(node[i], node[2 * i], node[2 * i + 1]);
    });
    fe_inv_divsteps(node[1], node[1]);   // a product of non-zero Z (and ones): never 0
    static_for<K - 1>([&](auto ic) {
        constexpr int i = 1 + decltype(ic)::value;
        fe a, b;
        fe_mul(a, node[i], node[2 * i + 1]);
        fe_mul(b, node[i], node[2 * i]);
        node[2 * i] = a;
        node[2 * i + 1] = b;
    });
    static_for<K>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if ((live >> j) & 1u) soa_store(rows.pre, n, (uint32_t)j * T + t, node[K + j].n);
    });
}

// Lean forms of the two inversion kernels (HD_VAR_LEAN_INV): the same
// inverses from one inversion per lane over the same lanes and slots, but a
// linear walk whose prefix products go through the pre row of each message
// (which receives that message's inverse on the way back) instead of K
// inputs and K prefixes, or a product tree, in registers.  The launch bound
// holds them to 168 VGPRs where k_fast_sinv / k_fast_zinv take 368 / 397, so
// a wave of either fits beside two waves per SIMD of a running k_fast_sums
// (HD_VAR_SUM_CAP) and one call's inversions run beside another call's sums.
// A lane reads back only what it stored itself.  (The walk: inv2_lean, hd_inv2.h.)
template <int K>
__global__ __launch_bounds__(256, 3) void k_fast_sinv_lean(uint32_t n, SplitRows rows, uint32_t* __restrict__ est,
                                                           unsigned long long* __restrict__ stats) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t == 0) sinv_note_call(n, nc, rows, est, stats);
    if (t >= T) return;
    inv2_lean<sm, K>(t, T, nc, n, rows.aux, rows.s, rows.pre);
}

template <int K>
__global__ __launch_bounds__(256, 3) void k_fast_zinv_lean(uint32_t n, SplitRows rows) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t >= T) return;
    inv2_lean<fe, K>(t, T, nc, n, rows.aux, rows.xyz + 18 * (size_t)n, rows.pre);
}

// The lean inversions in two levels (hd_ctx_inv_levels 2; hd_inv2.h): each
// lean kernel as three kernels on the call's stream.  up is the lean walk's
// first loop and leaves each lane's product in the roots row, mid runs the
// lean walk over those T roots (K2 per lane, split_lanes<K2>(T) lanes: the
// only lanes that invert), down is the walk's second loop from the root's
// inverse.  A wave's divstep inversion costs the same whether 64 lanes need
// it or one, so a call pays for 1 / K2 of the lean forms' inversions and for
// about three more products per lane.  T and T2 follow from the slot counter
// as T does above; the mid grids are sized from n like the others.  The same
// slots come out of the same rows as in the lean forms.

template <int K>
__global__ __launch_bounds__(256, 3) void k_fast_sinv_up(uint32_t n, SplitRows rows, RootRows rr,
                                                         uint32_t* __restrict__ est,
                                                         unsigned long long* __restrict__ stats) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t == 0) sinv_note_call(n, nc, rows, est, stats);
    if (t >= T) return;
    inv2_up<sm, K>(t, T, nc, n, rows.aux, rows.s, rows.pre, rr.roots);
}

template <int K2, int K>
__global__ __launch_bounds__(256, 3) void k_fast_sinv_mid(SplitRows rows, RootRows rr) {
    wave_prio(rows.prio);
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t T = split_lanes<K>(rows.cnt[2]), T2 = split_lanes<K2>(T);
    if (u >= T2) return;
    inv2_mid<sm, K2>(u, T2, T, rr.roots, rr.rpre);
}

template <int K>
__global__ __launch_bounds__(256, 3) void k_fast_sinv_down(uint32_t n, SplitRows rows, RootRows rr) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t >= T) return;
    inv2_down<sm, K>(t, T, nc, n, rows.aux, rows.s, rows.pre, rr.roots);
}

template <int K>
__global__ __launch_bounds__(256, 3) void k_fast_zinv_up(uint32_t n, SplitRows rows, RootRows rr) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t >= T) return;
    inv2_up<fe, K>(t, T, nc, n, rows.aux, rows.xyz + 18 * (size_t)n, rows.pre, rr.roots);
}

template <int K2, int K>
__global__ __launch_bounds__(256, 3) void k_fast_zinv_mid(SplitRows rows, RootRows rr) {
    wave_prio(rows.prio);
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t T = split_lanes<K>(rows.cnt[2]), T2 = split_lanes<K2>(T);
    if (u >= T2) return;
    inv2_mid<fe, K2>(u, T2, T, rr.roots, rr.rpre);
}

template <int K>
__global__ __launch_bounds__(256, 3) void k_fast_zinv_down(uint32_t n, SplitRows rows, RootRows rr) {
    wave_prio(rows.prio);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nc = rows.cnt[2], T = split_lanes<K>(nc);
    if (t >= T) return;
    inv2_down<fe, K>(t, T, nc, n, rows.aux, rows.xyz + 18 * (size_t)n, rows.pre, rr.roots);
}

uint32_t blocks(uint32_t lanes) { return (lanes + 255) / 256; }

}  // namespace

// HD_VAR_LEAN_INV: the inversion kernels that fit beside a capped sums; a
// call that takes the 4-wave sums (a small batch) keeps the register forms.
// hd_ctx_inv_levels 2: each lean kernel as up, mid, down (hd_inv2.h).  The
// grids cover n slots; the waves past the slots in use exit at once.
void fb_launch_sinv(const FbCallPlan& p, int inv_levels, int inv_k2, hipStream_t s, uint32_t n, const SplitRows& rows,
                    const RootRows& rr, uint32_t* est, unsigned long long* stats) {
    with_k(p.k, [&](auto k) {
        constexpr int K = decltype(k)::value;
        const uint32_t T = split_lanes<K>(n), tb = blocks(T);   // (the mid kernels: K2 roots per lane)
        if (p.lean && inv_levels == 2) {
            k_fast_sinv_up<K><<<tb, 256, 0, s>>>(n, rows, rr, est, stats);
            if (inv_k2 == 8) k_fast_sinv_mid<8, K><<<blocks(split_lanes<8>(T)), 256, 0, s>>>(rows, rr);
            else k_fast_sinv_mid<16, K><<<blocks(split_lanes<16>(T)), 256, 0, s>>>(rows, rr);
            k_fast_sinv_down<K><<<tb, 256, 0, s>>>(n, rows, rr);
        } else if (p.lean) k_fast_sinv_lean<K><<<tb, 256, 0, s>>>(n, rows, est, stats);
        else k_fast_sinv<K><<<tb, 256, 0, s>>>(n, rows, est, stats);
    });
}

void fb_launch_zinv(const FbCallPlan& p, int inv_levels, int inv_k2, hipStream_t s, uint32_t n, const SplitRows& rows,
                    const RootRows& rr) {
    with_k(p.k, [&](auto k) {
        constexpr int K = decltype(k)::value;
        const uint32_t T = split_lanes<K>(n), tb = blocks(T);   // (the mid kernels: K2 roots per lane)
        if (p.lean && inv_levels == 2) {
            k_fast_zinv_up<K><<<tb, 256, 0, s>>>(n, rows, rr);
            if (inv_k2 == 8) k_fast_zinv_mid<8, K><<<blocks(split_lanes<8>(T)), 256, 0, s>>>(rows, rr);
            else k_fast_zinv_mid<16, K><<<blocks(split_lanes<16>(T)), 256, 0, s>>>(rows, rr);
            k_fast_zinv_down<K><<<tb, 256, 0, s>>>(n, rows, rr);
        } else if (p.lean) k_fast_zinv_lean<K><<<tb, 256, 0, s>>>(n, rows);
        else k_fast_zinv<K><<<tb, 256, 0, s>>>(n, rows);
    });
}
