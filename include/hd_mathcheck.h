/* hd_mathcheck.h -- single operations of the device arithmetic (hd_field.h,
 * hd_modinv.h, hd_scmont.h, hd_group.h, hd_fixedbase.h) run on the GPU, one
 * row per lane, for the operation-by-operation tests
 * (tests/test_gpu_devmath.py).  Test surface only: nothing in the product
 * calls it.
 *
 * Rows are 32-bit words.  A field element is its 9 raw radix-2^29 limbs
 * (loose limb classes can be fed and are returned as produced); a scalar is 8
 * little-endian words; a Jacobian point is X, Y, Z (27 words), an XYZZ point
 * X, Y, ZZ, ZZZ (36), an affine point x, y (18); flags and digits are one
 * word each (digits as two's complement).  Row layouts per op are listed
 * with the op codes below: "in -> out" in words.
 *
 * The entry points are stateless: they allocate, copy in, launch one kernel,
 * synchronise, copy back and free, and return the library's error codes
 * (HD_OK 0, HD_EINVAL -1, HD_ENOMEM -2, HD_EDEVICE -3). */
#ifndef HD_MATHCHECK_H
#define HD_MATHCHECK_H
#include <stdint.h>

#define HD_MC_MAX_ROWS 65536u
#define HD_MC_CHAIN_LEN 6  /* table points per row of HD_MC_GXZ_CHAIN */
#define HD_MC_SM_CHAIN_LEN 4

enum hd_mc_op {
    /* field */
    HD_MC_FE_MUL = 0,          /* a b -> a*b                      18 -> 9 */
    HD_MC_FE_SQR = 1,          /* a -> a^2                         9 -> 9 */
    HD_MC_FE_NORM_WEAK = 2,    /*                                  9 -> 9 */
    HD_MC_FE_NORMALIZE = 3,    /*                                  9 -> 9 */
    HD_MC_FE_ADD = 4,          /*                                 18 -> 9 */
    HD_MC_FE_SUB2 = 5,         /* a + 2p - b                      18 -> 9 */
    HD_MC_FE_NEG = 6,          /* 2p - a                           9 -> 9 */
    HD_MC_FE_MUL_INT = 7,      /* a k -> a * k (limb-wise)        10 -> 9 */
    HD_MC_FE_INV = 8,          /*                                  9 -> 9 */
    HD_MC_FE_INV_DIVSTEPS = 9, /*                                  9 -> 9 */
    HD_MC_FE_SQRT = 10,        /* a -> root, flag                  9 -> 10 */
    HD_MC_FE_FLAGS = 11,       /* a b -> is_zero(a) is_odd(a) eq(a,b)  18 -> 3 */
    HD_MC_FE_SQR_SQR = 12,     /* (a^2)^2                          9 -> 9 */
    HD_MC_FE_SQR_MUL_A = 13,   /* a^2 * a                          9 -> 9 */
    HD_MC_FE_SQR_MUL_B = 14,   /* a^2 * b                         18 -> 9 */
    HD_MC_FE_MUL_ALIAS = 15,   /* t = a; t = t * b                18 -> 9 */
    HD_MC_FE_SQR_N88 = 16,     /* a^(2^88)                         9 -> 9 */
    /* scalar */
    HD_MC_SC_MUL = 20,         /*                                 16 -> 8 */
    HD_MC_SC_SQR = 21,         /*                                  8 -> 8 */
    HD_MC_SC_NEG = 22,         /*                                  8 -> 8 */
    HD_MC_SC_ADD = 23,         /*                                 16 -> 8 */
    HD_MC_SC_INV = 24,         /*                                  8 -> 8 */
    HD_MC_SC_INV_DIVSTEPS = 25,/*                                  8 -> 8 */
    HD_MC_SC_FROM_BE_REDUCE = 26, /* 256-bit value (LE words) mod n 8 -> 8 */
    HD_MC_SC_REDUCE512 = 27,   /* 512-bit value mod n             16 -> 8 */
    HD_MC_SC_SPLIT_LAMBDA = 28,/* k -> k1 k2                       8 -> 16 */
    HD_MC_SM_MUL = 29,         /* a b -> a b R^-1 mod n (R = 2^261) canonical, then the 9 raw limbs of
                                  sm_mul before sm_to_sc          16 -> 17 */
    HD_MC_SM_CHAIN = 30,       /* x y0..y3 -> x y0 y1 y2 y3 R^-4  40 -> 8 */
    HD_MC_BOOTH = 31,          /* k -> booth_digit<4> x 65, booth_digit<8> x 33        8 -> 98 */
    HD_MC_BOOTH160 = 32,       /* k -> sign, |k| (5 words), booth_digit160<4> x 33, <12> x 11   8 -> 50 */
    HD_MC_FB_DIGITS = 33,      /* k -> WG, fb_digit<13> x 20, <16> x 16, <20> x 13, <22> x 12, <WG> x NWIN(WG)
                                  (WG: the library's G window width; the rest of the row is 0)   8 -> 84 */
    /* points */
    HD_MC_GEJ_DBL = 40,        /* a                               27 -> 27 */
    HD_MC_GEJ_ADD_GE = 41,     /* a (Jacobian) b (affine)         45 -> 27 */
    HD_MC_GEJ_ADD = 42,        /* a b (Jacobian)                  54 -> 27 */
    HD_MC_GEJ_ADD_GE_NX = 43,  /*                                 45 -> 27 */
    HD_MC_GEJ_ADD_GE_Z1 = 44,  /* a b (affine)                    36 -> 27 */
    HD_MC_GXZ_ADD_GE_NX = 45,  /* a (XYZZ) b (affine)             54 -> 36 */
    HD_MC_GXZ_ADD_GE_Z1 = 46,  /* a b (affine)                    36 -> 36 */
    HD_MC_GXZ_CHAIN = 47       /* HD_MC_CHAIN_LEN x (x y neg skip) -> gxz_finish's X ZZZ, Y ZZ, ZZ ZZZ, then
                                  started, ZZ == 0; the window steps are gxz_sum_step with `rare` from a
                                  wavefront vote, as k_fast_sums takes it     120 -> 29 */
};

#ifdef __cplusplus
extern "C" {
#endif
/* words per input and output row of op; HD_EINVAL for an unknown op */
int hd_mathcheck_words(int op, uint32_t* in_words, uint32_t* out_words);
/* runs op over n rows (1 <= n <= HD_MC_MAX_ROWS) in blocks of `block` threads
 * (64 or 256); in and out are host arrays of n rows */
int hd_mathcheck(int device, int op, uint32_t n, int block, const uint32_t* in, uint32_t* out);

/* The fixed-base tables as the device built them (tests/test_gpu_fb_tables.py).
 * Test surface only, read-only: no kernel, nothing queued, nothing in the
 * product calls it.
 * which = -1: the device's G table; which >= 0: the table of the admitted
 * signatory with that index in the sorted admitted set.  Waits for the
 * context's verify calls and table builds, then copies entries
 * [first, first + count) to out64, 64 bytes each (x, y as 8 little-endian
 * words).  *width = window bits, *state = the slot's state (0 empty, 1 claimed,
 * 2 key learned, 3 table ready; 3 for G), key64 = the slot's key in the same
 * 64-byte layout (G for which = -1; zeros while no key is known).  A slot that
 * is not ready copies nothing.  count == 0 returns width / state / key only.
 * Any of width, state, key64 may be NULL.  HD_EINVAL for a range outside the
 * table or an index without a slot. */
struct hd_ctx;
int hd_fb_table_read(struct hd_ctx* ctx, int32_t which, uint64_t first, uint32_t count, uint8_t* out64,
                     int* width, uint32_t* state, uint8_t* key64);
#ifdef __cplusplus
}
#endif
#endif
