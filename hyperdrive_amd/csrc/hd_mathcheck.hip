// hd_mathcheck.hip -- single operations of the device arithmetic on the GPU,
// one row per lane (include/hd_mathcheck.h).  One kernel instantiation per
// op, everything inlined (no device function call), so each op is compiled
// on its own as the product kernels compile it: with the inline-asm carry
// chain of macc96, the wavefront vote of modinv30's early exit, and the
// backend's choices for back-to-back field products.  The rows themselves
// are in hd_mathcheck_ops.h, shared with the host harness.
#include <hip/hip_runtime.h>

#include "hd_mathcheck_ops.h"

using namespace hd;

template <int OP>
__global__ __launch_bounds__(256) void k_mathcheck(uint32_t n, const uint32_t* __restrict__ in,
                                                   uint32_t* __restrict__ out) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;   // the lanes past n leave: a wavefront vote counts the rows that are there
    mc_row<OP>(in + (size_t)row * mc_in_words(OP), out + (size_t)row * mc_out_words(OP));
}

#define HD_MC_OPS(X)                                                                                              \
    X(HD_MC_FE_MUL) X(HD_MC_FE_SQR) X(HD_MC_FE_NORM_WEAK) X(HD_MC_FE_NORMALIZE) X(HD_MC_FE_ADD) X(HD_MC_FE_SUB2)  \
    X(HD_MC_FE_NEG) X(HD_MC_FE_MUL_INT) X(HD_MC_FE_INV) X(HD_MC_FE_INV_DIVSTEPS) X(HD_MC_FE_SQRT)                 \
    X(HD_MC_FE_FLAGS) X(HD_MC_FE_SQR_SQR) X(HD_MC_FE_SQR_MUL_A) X(HD_MC_FE_SQR_MUL_B) X(HD_MC_FE_MUL_ALIAS)       \
    X(HD_MC_FE_SQR_N88) X(HD_MC_SC_MUL) X(HD_MC_SC_SQR) X(HD_MC_SC_NEG) X(HD_MC_SC_ADD) X(HD_MC_SC_INV)           \
    X(HD_MC_SC_INV_DIVSTEPS) X(HD_MC_SC_FROM_BE_REDUCE) X(HD_MC_SC_REDUCE512) X(HD_MC_SC_SPLIT_LAMBDA)            \
    X(HD_MC_SM_MUL) X(HD_MC_SM_CHAIN) X(HD_MC_BOOTH) X(HD_MC_BOOTH160) X(HD_MC_FB_DIGITS) X(HD_MC_GEJ_DBL)        \
    X(HD_MC_GEJ_ADD_GE) X(HD_MC_GEJ_ADD) X(HD_MC_GEJ_ADD_GE_NX) X(HD_MC_GEJ_ADD_GE_Z1) X(HD_MC_GXZ_ADD_GE_NX)     \
    X(HD_MC_GXZ_ADD_GE_Z1) X(HD_MC_GXZ_CHAIN)

extern "C" int hd_mathcheck_words(int op, uint32_t* in_words, uint32_t* out_words) {
    const uint32_t iw = mc_in_words(op), ow = mc_out_words(op);
    if (!iw || !ow) return -1;
    if (in_words) *in_words = iw;
    if (out_words) *out_words = ow;
    return 0;
}

extern "C" int hd_mathcheck(int device, int op, uint32_t n, int block, const uint32_t* in, uint32_t* out) {
    const uint32_t iw = mc_in_words(op), ow = mc_out_words(op);
    if (!in || !out || !iw || !ow || n == 0 || n > HD_MC_MAX_ROWS || (block != 64 && block != 256)) return -1;
    if (hipSetDevice(device) != hipSuccess) return -3;
    const size_t ib = (size_t)n * iw * sizeof(uint32_t), ob = (size_t)n * ow * sizeof(uint32_t);
    uint32_t *din = nullptr, *dout = nullptr;
    if (hipMalloc(&din, ib) != hipSuccess) return -2;
    if (hipMalloc(&dout, ob) != hipSuccess) {
        (void)hipFree(din);
        return -2;
    }
    int rc = 0;
    if (hipMemcpy(din, in, ib, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dout, 0, ob) != hipSuccess) rc = -3;
    if (rc == 0) {
        const uint32_t blocks = (n + (uint32_t)block - 1) / (uint32_t)block;
        switch (op) {
#define HD_MC_CASE(OP) \
    case OP: k_mathcheck<OP><<<blocks, block>>>(n, din, dout); break;
            HD_MC_OPS(HD_MC_CASE)
#undef HD_MC_CASE
            default: rc = -1;
        }
        if (rc == 0 && (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)) rc = -3;
    }
    if (rc == 0 && hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost) != hipSuccess) rc = -3;
    (void)hipFree(din);
    (void)hipFree(dout);
    return rc;
}
