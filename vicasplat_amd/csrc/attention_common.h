// What attention.hip and attention_bwd.hip share on the device (head dim 64): the argument block's key addressing, the 16-bit MFMA and
// convert wrappers, the LDS-DMA instruction and the transpose-read type.  The launch routes of both files are in routes.h.
#pragma once
#include "common.h"
#include "routes.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
// operand type of the LDS transpose read ds_read_b64_tr_b16 (semantics probed in tools/probe/tr_read.hip): lane t of a 16-lane group supplies
// the address of 4 consecutive halfs of row (row0 + (t >> 2)) at column col0 + (t & 3) * 4 and receives tile[row0 .. row0 + 3][col0 + t]
typedef short tr4_t __attribute__((ext_vector_type(4)));
typedef void __attribute__((address_space(3))) *lds_ptr_t;

constexpr int HD = 64;       // head dim

// The forward's arguments, T = the element type of q | k | v and out (unsigned short: f16 / bf16 bits; float: the f32 and split classes).
template <class T>
struct AttnArgs {
    const T *q, *k, *v;
    T *out;
    const int32_t *kv_seg;   // [nbatch,4] base0,len0,base1,len1 (rows) or null
    const int32_t *q_kvlen;  // [nbatch*Lq] or null
    int nbatch, H, Lq, Lk;
    long long q_batch_rows, k_batch_rows;
    int ldq, ldk, ldv, ldo;
    float scale_log2e;
    float *lse;  // optional [rows, H] f32: log2-domain logsumexp of the scaled scores (saved for the backward pass)
    int out_packed;   // split class: write O in the packed (hi, lo) form (the A operand of the projection GEMM: vs_gemm_split_packed); the 16-bit and f32 kernels ignore it
};

// The key list of batch item b: the two segments of kv_seg[b] concatenated, or rows b * k_batch_rows + [0, Lk).  Positions past the end
// read the last key (the callers mask them).
struct KeyList {
    int base0, len0, base1, len1, Lk;
    __device__ __forceinline__ long long row(int j) const {
        j = min(j, Lk - 1);
        return j < len0 ? (long long)base0 + j : (long long)base1 + (j - len0);
    }
};
template <class Args>
__device__ __forceinline__ KeyList key_list(const Args &a, int b) {
    KeyList kl;
    if (a.kv_seg) {
        kl.base0 = a.kv_seg[4 * b + 0]; kl.len0 = a.kv_seg[4 * b + 1]; kl.base1 = a.kv_seg[4 * b + 2]; kl.len1 = a.kv_seg[4 * b + 3];
    } else {
        kl.base0 = (int)(b * a.k_batch_rows); kl.len0 = a.Lk; kl.base1 = 0; kl.len1 = 0;
    }
    kl.Lk = kl.len0 + kl.len1;
    return kl;
}
// keys that query qi of item b sees: its prefix of the list (all of it without q_kvlen), none for a query slot past Lq.  (qvalid by
// reference: with a by-value flag the compiler swaps source operands in the kernels' softmax loops -- the same instructions, but no longer the
// code the open-coded form compiled to.  The backward kernels were written in another order of the same three steps and keep it: profiles/attention_refactor.md.)
template <class Args>
__device__ __forceinline__ int query_len(const Args &a, const KeyList &kl, int b, int qi, const bool &qvalid) {
    int ml = kl.Lk;
    if (a.q_kvlen && qvalid) ml = min(kl.Lk, a.q_kvlen[(long long)b * a.Lq + qi]);
    if (!qvalid) ml = 0;
    return ml;
}

template <bool BF16>
__device__ __forceinline__ f4 mfma(const uint4 &a, const uint4 &b, f4 c) {
    if constexpr (BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf8 *>(&a), *reinterpret_cast<const bf8 *>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const half8 *>(&a), *reinterpret_cast<const half8 *>(&b), c, 0, 0, 0);
}

template <bool BF16>
__device__ __forceinline__ unsigned pack2(float a, float b) {
    // one packed convert (round to nearest even) instead of two converts + an OR: the softmax / dS path is VALU-bound
    unsigned r;
    if constexpr (BF16) asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    else asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The same convert for a value that goes STRAIGHT INTO AN MFMA: compiler-visible instructions, so that the hazard recogniser inserts the
// VALU-write -> MFMA-read wait states (it does not look inside inline asm).  Round 4: attention_sp_kernel's third query group came out
// 5e-5 off with the asm form whenever the scheduler placed a P V MFMA right behind the convert; the older kernels used the asm form for
// their P fragments too and were only protected by what happened to be scheduled in between.
template <bool BF16>
__device__ __forceinline__ unsigned pack2v(float a, float b) {
    typedef float f2p_ __attribute__((ext_vector_type(2)));
    if constexpr (BF16) {
        typedef __bf16 b2p_ __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(unsigned, __builtin_convertvector(f2p_{a, b}, b2p_));
    } else {
        typedef _Float16 h2p_ __attribute__((ext_vector_type(2)));
        return __builtin_bit_cast(unsigned, __builtin_convertvector(f2p_{a, b}, h2p_));
    }
}

// LDS-DMA: 64 lanes x 16 bytes from gp (per lane) to 1 KiB of LDS at lds_off (wave-uniform).  Inline asm: the compiler adds no waits of
// its own around it, so every user places its s_waitcnt vmcnt itself before the barrier that publishes the tile.
__device__ __forceinline__ void glds16(const void *gp, unsigned lds_off) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_off), "v"(gp) : "memory");
}

}  // namespace
