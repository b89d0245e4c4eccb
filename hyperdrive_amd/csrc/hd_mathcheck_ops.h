// hd_mathcheck_ops.h -- one row of each single-operation check
// (include/hd_mathcheck.h), written once for both builds: the gfx950 kernels
// of hd_mathcheck.hip and the host harness (tests/native/hd_host_check.cpp)
// run this same text over the same rows, so a word that differs between them
// is code generation.
#pragma once
#include "../../include/hd_mathcheck.h"
#include "hd_fixedbase.h"
#include "hd_scmont.h"

namespace hd {

// words per input / output row; 0 for an unknown op
HD constexpr uint32_t mc_in_words(int op) {
    switch (op) {
        case HD_MC_FE_MUL: case HD_MC_FE_ADD: case HD_MC_FE_SUB2: case HD_MC_FE_FLAGS: case HD_MC_FE_SQR_MUL_B:
        case HD_MC_FE_MUL_ALIAS: return 18;
        case HD_MC_FE_SQR: case HD_MC_FE_NORM_WEAK: case HD_MC_FE_NORMALIZE: case HD_MC_FE_NEG: case HD_MC_FE_INV:
        case HD_MC_FE_INV_DIVSTEPS: case HD_MC_FE_SQRT: case HD_MC_FE_SQR_SQR: case HD_MC_FE_SQR_MUL_A:
        case HD_MC_FE_SQR_N88: return 9;
        case HD_MC_FE_MUL_INT: return 10;
        case HD_MC_SC_MUL: case HD_MC_SC_ADD: case HD_MC_SC_REDUCE512: case HD_MC_SM_MUL: return 16;
        case HD_MC_SC_SQR: case HD_MC_SC_NEG: case HD_MC_SC_INV: case HD_MC_SC_INV_DIVSTEPS:
        case HD_MC_SC_FROM_BE_REDUCE: case HD_MC_SC_SPLIT_LAMBDA: case HD_MC_BOOTH: case HD_MC_BOOTH160:
        case HD_MC_FB_DIGITS: return 8;
        case HD_MC_SM_CHAIN: return 8 + 8 * HD_MC_SM_CHAIN_LEN;
        case HD_MC_GEJ_DBL: return 27;
        case HD_MC_GEJ_ADD_GE: case HD_MC_GEJ_ADD_GE_NX: return 45;
        case HD_MC_GEJ_ADD: case HD_MC_GXZ_ADD_GE_NX: return 54;
        case HD_MC_GEJ_ADD_GE_Z1: case HD_MC_GXZ_ADD_GE_Z1: return 36;
        case HD_MC_GXZ_CHAIN: return 20 * HD_MC_CHAIN_LEN;
        default: return 0;
    }
}
HD constexpr uint32_t mc_out_words(int op) {
    switch (op) {
        case HD_MC_FE_SQRT: return 10;
        case HD_MC_FE_FLAGS: return 3;
        case HD_MC_SC_SPLIT_LAMBDA: return 16;
        case HD_MC_SM_MUL: return 17;
        case HD_MC_BOOTH: return 98;
        case HD_MC_BOOTH160: return 50;
        case HD_MC_FB_DIGITS: return 84;
        case HD_MC_GXZ_ADD_GE_NX: case HD_MC_GXZ_ADD_GE_Z1: return 36;
        case HD_MC_GXZ_CHAIN: return 29;
        default: break;
    }
    if (op >= HD_MC_FE_MUL && op <= HD_MC_FE_SQR_N88) return 9;
    if (op >= HD_MC_SC_MUL && op <= HD_MC_SM_CHAIN) return 8;
    if (op >= HD_MC_GEJ_DBL && op <= HD_MC_GEJ_ADD_GE_Z1) return 27;
    return 0;
}

HD void mc_fe_in(fe& r, const uint32_t* w) {
    HD_UNROLL for (int i = 0; i < 9; i++) r.n[i] = w[i];
    HD_B(fe_bound_exact(r);)
}
HD void mc_fe_out(uint32_t* w, const fe& a) {
    HD_UNROLL for (int i = 0; i < 9; i++) w[i] = a.n[i];
}
HD void mc_sc_in(sc& r, const uint32_t* w) {
    HD_UNROLL for (int i = 0; i < 8; i++) r.v[i] = w[i];
}
HD void mc_sc_out(uint32_t* w, const sc& a) {
    HD_UNROLL for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
HD void mc_ge_in(ge& r, const uint32_t* w) { mc_fe_in(r.x, w); mc_fe_in(r.y, w + 9); }
HD void mc_gej_in(gej& r, const uint32_t* w) { mc_fe_in(r.x, w); mc_fe_in(r.y, w + 9); mc_fe_in(r.z, w + 18); }
HD void mc_gej_out(uint32_t* w, const gej& a) { mc_fe_out(w, a.x); mc_fe_out(w + 9, a.y); mc_fe_out(w + 18, a.z); }
HD void mc_gxz_out(uint32_t* w, const gxz& a) {
    mc_fe_out(w, a.x); mc_fe_out(w + 9, a.y); mc_fe_out(w + 18, a.zz); mc_fe_out(w + 27, a.zzz);
}

// `rare` of one window step as k_fast_sums' sum_add takes it: on the device a
// vote of the wavefront's active lanes, on the host this row alone
HD bool mc_rare(bool started, bool nz) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(!(started && nz)) != 0ull;
#else
    return !(started && nz);
#endif
}

template <int W, int OFF>
HD void mc_fb_digits(uint32_t* out, const sc& k) {
    HD_UNROLL for (int j = 0; j < FbL<W>::NWIN; j++) out[OFF + j] = (uint32_t)fb_digit<W>(k, j);
}

// one row of op OP: `in` and `out` point at the row's words
template <int OP>
HD void mc_row(const uint32_t* in, uint32_t* out) {
    if constexpr (OP >= HD_MC_FE_MUL && OP <= HD_MC_FE_SQR_N88) {
        fe a, b, r;
        mc_fe_in(a, in);
        if constexpr (mc_in_words(OP) == 18) mc_fe_in(b, in + 9);
        if constexpr (OP == HD_MC_FE_MUL) fe_mul(r, a, b);
        if constexpr (OP == HD_MC_FE_SQR) fe_sqr(r, a);
        if constexpr (OP == HD_MC_FE_NORM_WEAK) { r = a; fe_norm_weak(r); }
        if constexpr (OP == HD_MC_FE_NORMALIZE) { r = a; fe_normalize(r); }
        if constexpr (OP == HD_MC_FE_ADD) fe_add(r, a, b);
        if constexpr (OP == HD_MC_FE_SUB2) fe_sub_k<2>(r, a, b);
        if constexpr (OP == HD_MC_FE_NEG) fe_neg(r, a);
        if constexpr (OP == HD_MC_FE_MUL_INT) fe_mul_int(r, a, in[9]);
        if constexpr (OP == HD_MC_FE_INV) fe_inv(r, a);
        if constexpr (OP == HD_MC_FE_INV_DIVSTEPS) fe_inv_divsteps(r, a);
        if constexpr (OP == HD_MC_FE_SQRT) out[9] = fe_sqrt(r, a) ? 1u : 0u;
        if constexpr (OP == HD_MC_FE_SQR_SQR) { fe t; fe_sqr(t, a); fe_sqr(r, t); }
        if constexpr (OP == HD_MC_FE_SQR_MUL_A) { fe t; fe_sqr(t, a); fe_mul(r, t, a); }
        if constexpr (OP == HD_MC_FE_SQR_MUL_B) { fe t; fe_sqr(t, a); fe_mul(r, t, b); }
        if constexpr (OP == HD_MC_FE_MUL_ALIAS) { fe t = a; fe_mul(t, t, b); r = t; }
        if constexpr (OP == HD_MC_FE_SQR_N88) fe_sqr_n(r, a, 88);
        if constexpr (OP == HD_MC_FE_FLAGS) {
            out[0] = fe_is_zero(a) ? 1u : 0u;
            out[1] = fe_is_odd(a) ? 1u : 0u;
            out[2] = fe_eq(a, b) ? 1u : 0u;
        } else {
            mc_fe_out(out, r);
        }
    } else if constexpr (OP == HD_MC_SC_REDUCE512) {
        uint32_t t[16];
        HD_UNROLL for (int i = 0; i < 16; i++) t[i] = in[i];
        sc r;
        sc_reduce(r, t);
        mc_sc_out(out, r);
    } else if constexpr (OP == HD_MC_SC_FROM_BE_REDUCE) {
        uint32_t be[8];
        HD_UNROLL for (int i = 0; i < 8; i++) be[i] = in[7 - i];
        sc r;
        sc_from_be_reduce(r, be);
        mc_sc_out(out, r);
    } else if constexpr (OP == HD_MC_SC_SPLIT_LAMBDA) {
        sc k, k1, k2;
        mc_sc_in(k, in);
        sc_split_lambda(k1, k2, k);
        mc_sc_out(out, k1);
        mc_sc_out(out + 8, k2);
    } else if constexpr (OP == HD_MC_SM_MUL) {
        sc a, b, o;
        mc_sc_in(a, in);
        mc_sc_in(b, in + 8);
        sm x, y, r;
        sm_from_sc(x, a);
        sm_from_sc(y, b);
        sm_mul(r, x, y);
        HD_UNROLL for (int i = 0; i < 9; i++) out[8 + i] = r.n[i];
        sm_to_sc(o, r);
        mc_sc_out(out, o);
    } else if constexpr (OP == HD_MC_SM_CHAIN) {
        sc a, o;
        mc_sc_in(a, in);
        sm x;
        sm_from_sc(x, a);
        HD_UNROLL for (int t = 0; t < HD_MC_SM_CHAIN_LEN; t++) {
            sc b;
            mc_sc_in(b, in + 8 + 8 * t);
            sm y;
            sm_from_sc(y, b);
            sm_mul(x, x, y);
        }
        sm_to_sc(o, x);
        mc_sc_out(out, o);
    } else if constexpr (OP == HD_MC_BOOTH) {
        sc k;
        mc_sc_in(k, in);
        HD_UNROLL for (int j = 0; j < HD_NWIN_R; j++) out[j] = (uint32_t)booth_digit<HD_WR>(k, j);
        HD_UNROLL for (int j = 0; j < HD_NWIN_G; j++) out[HD_NWIN_R + j] = (uint32_t)booth_digit<HD_WG>(k, j);
    } else if constexpr (OP == HD_MC_BOOTH160) {
        sc k;
        mc_sc_in(k, in);
        uint32_t a[5];
        const bool neg = sc_signed_abs(a, k);
        out[0] = neg ? 1u : 0u;
        HD_UNROLL for (int i = 0; i < 5; i++) out[1 + i] = a[i];
        HD_UNROLL for (int j = 0; j < HD_GLV_NWIN_R; j++) out[6 + j] = (uint32_t)booth_digit160<HD_WR>(a, j, neg);
        HD_UNROLL for (int j = 0; j < HD_GLV_NWIN_G; j++)
            out[6 + HD_GLV_NWIN_R + j] = (uint32_t)booth_digit160<HD_WG_GLV>(a, j, neg);
    } else if constexpr (OP == HD_MC_FB_DIGITS) {
        static_assert(FbL<HD_FB_WG>::NWIN <= 84 - 62, "HD_MC_FB_DIGITS row too short for this G window width");
        sc k;
        mc_sc_in(k, in);
        HD_UNROLL for (int j = 0; j < 84; j++) out[j] = 0;
        out[0] = HD_FB_WG;
        mc_fb_digits<13, 1>(out, k);
        mc_fb_digits<16, 21>(out, k);
        mc_fb_digits<20, 37>(out, k);
        mc_fb_digits<22, 50>(out, k);
        mc_fb_digits<HD_FB_WG, 62>(out, k);
    } else if constexpr (OP >= HD_MC_SC_MUL && OP <= HD_MC_SC_INV_DIVSTEPS) {
        sc a, b, r;
        mc_sc_in(a, in);
        if constexpr (mc_in_words(OP) == 16) mc_sc_in(b, in + 8);
        if constexpr (OP == HD_MC_SC_MUL) sc_mul(r, a, b);
        if constexpr (OP == HD_MC_SC_SQR) sc_sqr(r, a);
        if constexpr (OP == HD_MC_SC_NEG) sc_neg(r, a);
        if constexpr (OP == HD_MC_SC_ADD) sc_add(r, a, b);
        if constexpr (OP == HD_MC_SC_INV) sc_inv(r, a);
        if constexpr (OP == HD_MC_SC_INV_DIVSTEPS) sc_inv_divsteps(r, a);
        mc_sc_out(out, r);
    } else if constexpr (OP == HD_MC_GEJ_DBL) {
        gej a, r;
        mc_gej_in(a, in);
        gej_dbl(r, a);
        mc_gej_out(out, r);
    } else if constexpr (OP == HD_MC_GEJ_ADD_GE || OP == HD_MC_GEJ_ADD_GE_NX) {
        gej a, r;
        ge b;
        mc_gej_in(a, in);
        mc_ge_in(b, in + 27);
        if constexpr (OP == HD_MC_GEJ_ADD_GE) gej_add_ge(r, a, b);
        else gej_add_ge_nx(r, a, b);
        mc_gej_out(out, r);
    } else if constexpr (OP == HD_MC_GEJ_ADD) {
        gej a, b, r;
        mc_gej_in(a, in);
        mc_gej_in(b, in + 27);
        gej_add(r, a, b);
        mc_gej_out(out, r);
    } else if constexpr (OP == HD_MC_GEJ_ADD_GE_Z1) {
        ge a, b;
        gej r;
        mc_ge_in(a, in);
        mc_ge_in(b, in + 18);
        gej_add_ge_z1(r, a, b);
        mc_gej_out(out, r);
    } else if constexpr (OP == HD_MC_GXZ_ADD_GE_NX) {
        gxz a, r;
        ge b;
        mc_fe_in(a.x, in); mc_fe_in(a.y, in + 9); mc_fe_in(a.zz, in + 18); mc_fe_in(a.zzz, in + 27);
        mc_ge_in(b, in + 36);
        gxz_add_ge_nx(r, a, b);
        mc_gxz_out(out, r);
    } else if constexpr (OP == HD_MC_GXZ_ADD_GE_Z1) {
        ge a, b;
        gxz r;
        mc_ge_in(a, in);
        mc_ge_in(b, in + 18);
        gxz_add_ge_z1(r, a, b);
        mc_gxz_out(out, r);
    } else if constexpr (OP == HD_MC_GXZ_CHAIN) {
        // the window loop of k_fast_sums (hdh_xyzz_sum is its host form)
        gxz acc, next;
        ge p0;
        bool started;
        {
            ge g;
            mc_ge_in(g, in);
            p0 = g;
            if (in[18]) fe_neg(p0.y, p0.y);
            fe_norm_weak(p0.y);
            gxz_set_ge(acc, p0);
            started = in[19] == 0;
        }
        static_for<HD_MC_CHAIN_LEN - 1>([&](auto kk) {
            constexpr int k = decltype(kk)::value + 1;
            ge g;
            mc_ge_in(g, in + 20 * k);
            const bool neg = in[20 * k + 18] != 0, nz = in[20 * k + 19] == 0;
            const bool rare = mc_rare(started, nz);
            gxz_sum_step<k == 1>(next, acc, started, p0, g, neg, nz, rare);
            acc = next;
        });
        fe xn, yn, t;
        gxz_finish(xn, yn, t, acc);
        mc_fe_out(out, xn);
        mc_fe_out(out + 9, yn);
        mc_fe_out(out + 18, t);
        out[27] = started ? 1u : 0u;
        out[28] = gxz_is_inf(acc) ? 1u : 0u;
    }
}

}  // namespace hd
