// hd_inv2.h -- the lean inversions of the known-key check (hd_fastinv.hip,
// DESIGN.md §4).  In one level (inv2_lean: k_fast_sinv_lean /
// k_fast_zinv_lean) a lane walks up its K slots, inverts its product and
// walks back down.  In two levels the same walk is cut at its inversion into
// three passes, and applied a second time to the lanes' own products, so that
// one divstep inversion serves K * K2 slots instead of K.
//
//   up    lane t < T: prefix products of its K slots j T + t into the pre
//         row (inv2_walk_up), then the lane's product as root t; a lane
//         without a live slot stores the domain's identity
//   mid   lane u < T2 = split_lanes<K2>(T): the same walk over the roots
//         j T2 + u < T, prefixes through the roots-prefix row, ONE
//         inversion, and on the way back each root's inverse in its place
//   down  lane t < T: inv2_walk_down, inv loaded from root t
//
// Every root below T is a value of the domain (a product or the identity), so
// the middle level needs no marker: its live roots are exactly those below
// T, and a dead lane's identity changes no product.  Both root rows are
// word-major with stride T.  No lane reads what another lane of its own pass
// stored.  Plain HD code: tests/native/hd_inv2_check.cpp runs these same
// bodies on the host, lane by lane.
#pragma once
#include "hd_modinv.h"
#include "hd_scmont.h"

namespace hd {

#define HD_FAST_LIVE 0xFDu   // aux code: keep going (the rest are final verdicts or HD_NEEDS_SLOW)

template <int NW>
HD void soa_load(uint32_t (&w)[NW], const uint32_t* __restrict__ p, uint32_t n, uint32_t i) {
    HD_UNROLL for (int k = 0; k < NW; k++) w[k] = p[(size_t)k * n + i];
}
template <int NW>
HD void soa_store(uint32_t* __restrict__ p, uint32_t n, uint32_t i, const uint32_t (&w)[NW]) {
    HD_UNROLL for (int k = 0; k < NW; k++) p[(size_t)k * n + i] = w[k];
}

// lanes of a K-per-lane pass over nc entries: a multiple of 64
template <int K>
HD uint32_t split_lanes(uint32_t nc) {
    return ((nc + (uint32_t)K - 1) / (uint32_t)K + 63u) & ~63u;
}

// The two domains, by element type.  sm, the scalars mod n: Montgomery
// factors in radix 2^29 (hd_scmont.h), a slot's input 8 plain words;
// inv2_inv(a) = a^-1 R, the form in which M(inv, prefix) is s^-1 R; identity
// R mod n.  fe, the field mod p: plain products of 9-limb elements.
HD void inv2_leaf(sm& x, const uint32_t* __restrict__ row, uint32_t n, uint32_t i) {
    sc s;
    soa_load(s.v, row, n, i);
    sm_from_sc(x, s);
}
HD void inv2_mul(sm& r, const sm& a, const sm& b) { sm_mul(r, a, b); }
HD void inv2_inv(sm& r, const sm& a) {
    sc p, pinv;
    sm_to_sc(p, a);
    sc_inv_divsteps(pinv, p);   // a product of scalars in [1, n) times a power of R: never 0
    sm_from_sc(r, pinv);
    sm r2;
    sm_r2(r2);
    sm_mul(r, r, r2);
}
HD void inv2_one(sm& r) {
    sm u, r2;
    HD_UNROLL for (int k = 0; k < 9; k++) u.n[k] = k == 0 ? 1u : 0u;
    sm_r2(r2);
    sm_mul(r, r2, u);
}

HD void inv2_leaf(fe& x, const uint32_t* __restrict__ row, uint32_t n, uint32_t i) { soa_load(x.n, row, n, i); }
HD void inv2_mul(fe& r, const fe& a, const fe& b) { fe_mul(r, a, b); }
HD void inv2_inv(fe& r, const fe& a) { fe_inv_divsteps(r, a); }   // a product of non-zero Z: never 0
HD void inv2_one(fe& r) {
    HD_UNROLL for (int k = 0; k < 9; k++) r.n[k] = k == 0 ? 1u : 0u;
}

HD bool inv2_live(const uint32_t* __restrict__ aux, uint32_t nc, uint32_t i) {
    return i < nc && (aux[i] & 0xFFu) == HD_FAST_LIVE;
}

// The walk up, lane t < T over slots j T + t (rows of stride n): the prefix
// products of the live slots into pre.  Returns the mask of the live slots
// (bit j) and leaves the lane's product in acc (0 when no slot is live).
template <class E, int K>
HD uint32_t inv2_walk_up(E& acc, uint32_t t, uint32_t T, uint32_t nc, uint32_t n, const uint32_t* __restrict__ aux,
                         const uint32_t* __restrict__ in, uint32_t* __restrict__ pre) {
    uint32_t live = 0;
    HD_UNROLL for (int k = 0; k < 9; k++) acc.n[k] = 0;
    HD_NOUNROLL for (int j = 0; j < K; j++) {
        const uint32_t i = (uint32_t)j * T + t;
        if (!inv2_live(aux, nc, i)) continue;
        E x;
        inv2_leaf(x, in, n, i);
        if (live) inv2_mul(acc, acc, x);
        else acc = x;
        live |= 1u << j;
        soa_store(pre, n, i, acc.n);   // the product of the live slots up to j
    }
    return live;
}

// The walk back, from inv = the inverse (as inv2_inv gives it) of the product
// of the slots in `live`: each live slot's inverse into pre.
template <class E, int K>
HD void inv2_walk_down(E inv, uint32_t live, uint32_t t, uint32_t T, uint32_t n, const uint32_t* __restrict__ in,
                       uint32_t* __restrict__ pre) {
    HD_NOUNROLL for (int j = K - 1; j >= 0; j--) {
        if (!((live >> j) & 1u)) continue;
        const uint32_t i = (uint32_t)j * T + t;
        const uint32_t below = live & ((1u << j) - 1u);
        if (below) {   // a live slot before this one: the highest such holds the prefix
            const uint32_t ip = (uint32_t)(31 - __builtin_clz(below)) * T + t;
            E pp, x, xi;
            soa_load(pp.n, pre, n, ip);
            inv2_leaf(x, in, n, i);
            inv2_mul(xi, inv, pp);
            inv2_mul(inv, inv, x);
            soa_store(pre, n, i, xi.n);
        } else {
            soa_store(pre, n, i, inv.n);
        }
    }
}

// The lean inversion in one level (k_fast_sinv_lean / k_fast_zinv_lean), lane
// t < T: up, one inversion per lane, back down with the mask the walk up
// returned.  A lane without a live slot stores nothing.
template <class E, int K>
HD void inv2_lean(uint32_t t, uint32_t T, uint32_t nc, uint32_t n, const uint32_t* __restrict__ aux,
                  const uint32_t* __restrict__ in, uint32_t* __restrict__ pre) {
    E acc, inv;
    const uint32_t live = inv2_walk_up<E, K>(acc, t, T, nc, n, aux, in, pre);
    if (!live) return;
    inv2_inv(inv, acc);
    inv2_walk_down<E, K>(inv, live, t, T, n, in, pre);
}

// up, lane t < T: the walk up, then the lane's product (or the identity) to root t
template <class E, int K>
HD void inv2_up(uint32_t t, uint32_t T, uint32_t nc, uint32_t n, const uint32_t* __restrict__ aux,
                const uint32_t* __restrict__ in, uint32_t* __restrict__ pre, uint32_t* __restrict__ roots) {
    E acc;
    if (!inv2_walk_up<E, K>(acc, t, T, nc, n, aux, in, pre)) inv2_one(acc);
    soa_store(roots, T, t, acc.n);
}

// mid, lane u < T2 over roots j T2 + u < T (rows of stride T): each root's
// inverse, in the form inv2_inv gives, in the root's place
template <class E, int K2>
HD void inv2_mid(uint32_t u, uint32_t T2, uint32_t T, uint32_t* __restrict__ roots, uint32_t* __restrict__ rpre) {
    int m = 0;   // roots of this lane: j T2 + u < T holds for a prefix of j
    E acc;
    HD_UNROLL for (int k = 0; k < 9; k++) acc.n[k] = 0;
    HD_NOUNROLL for (int j = 0; j < K2; j++) {
        const uint32_t r = (uint32_t)j * T2 + u;
        if (r >= T) break;
        E x;
        soa_load(x.n, roots, T, r);
        if (j) inv2_mul(acc, acc, x);
        else acc = x;
        m = j + 1;
        soa_store(rpre, T, r, acc.n);
    }
    if (!m) return;
    E inv;
    inv2_inv(inv, acc);
    HD_NOUNROLL for (int j = m - 1; j >= 0; j--) {
        const uint32_t r = (uint32_t)j * T2 + u;
        if (j) {
            E pp, x, xi;
            soa_load(pp.n, rpre, T, r - T2);
            soa_load(x.n, roots, T, r);
            inv2_mul(xi, inv, pp);
            inv2_mul(inv, inv, x);
            soa_store(roots, T, r, xi.n);
        } else {
            soa_store(roots, T, r, inv.n);
        }
    }
}

// down, lane t < T: each live slot's inverse into pre, from the inverse of
// the lane's product that mid left in root t
template <class E, int K>
HD void inv2_down(uint32_t t, uint32_t T, uint32_t nc, uint32_t n, const uint32_t* __restrict__ aux,
                  const uint32_t* __restrict__ in, uint32_t* __restrict__ pre, const uint32_t* __restrict__ roots) {
    uint32_t live = 0;
    HD_NOUNROLL for (int j = 0; j < K; j++) live |= inv2_live(aux, nc, (uint32_t)j * T + t) ? 1u << j : 0u;
    if (!live) return;
    E inv;
    soa_load(inv.n, roots, T, t);
    inv2_walk_down<E, K>(inv, live, t, T, n, in, pre);
}

}  // namespace hd
