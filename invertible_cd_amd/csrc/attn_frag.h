// attn_frag.h - the MFMA fragment layout every attention kernel of the library shares (attention.hip: fused, cross, probabilities;
// attention_masked.hip; the cross-attention epilogues of gemm.hip and gemm_big.hip), written once, and the helpers that could be shared
// without changing a kernel's instruction stream (gemm_big.hip follows the layout but keeps its own code: any helper moved its schedule).
//
//   * S^T = K.Q^T on v_mfma_f32_32x32x16_f16, K as the A operand, Q as the B operand: lane (lr = l & 31, lh = l >> 5) holds for
//     k-step ks the head dims 16 ks + 8 lh .. + 7 of query row lr, and owns ONE query column of the result.  The
//     softmax row reductions are therefore in-lane plus one exchange with lane l ^ 32 (half_max / half_sum).
//   * K rows enter the MFMA bit-swapped: MFMA row r of a 32-key tile is key attn_key_row(r), bits 2 and 3 of the index exchanged.
//     Accumulator element e of tile kt is then key 32 kt + 16 (e >> 3) + 8 lh + (e & 7) (attn_key): two runs of 8 CONSECUTIVE keys
//     per lane, which is the B-operand layout of the second MFMA.
//   * O^T += V^T.P^T takes P straight from those accumulators (elements 8 j .. 8 j + 7 of tile kt -> k-step 2 kt + j), no lane
//     movement, and a V^T fragment is 16 contiguous bytes: head-dim row 32 i + lr, keys 16 st + 8 lh .. + 7.
//   * Element e of O^T tile i is head-dim column 32 i + 8 (e >> 2) + 4 lh + (e & 3) of query row lr: a lane owns runs of 4
//     consecutive columns.  They leave either directly as f16x4 (attn_store_direct) or through a per-wave 32 x 72 LDS patch as
//     128-byte row segments (the cross-attention epilogues of the GEMMs).
#pragma once
#include "common.h"

constexpr float ATTN_LOG2E = 1.4426950408889634f;      // scores are scaled by scale * log2(e): the exponential is v_exp_f32 (base 2)

// MFMA row lr of a 32-key tile <- key attn_key_row(lr) of it (bits 2 and 3 exchanged; an involution)
__device__ __forceinline__ int attn_key_row(int lr) { return (lr & 0x13) | ((lr & 4) << 1) | ((lr & 8) >> 1); }

// Key of accumulator element e of 32-key tile kt in half-wave lh = attn_key_slot(kt, e) + 8 lh.  A mask is `attn_key(kt, e, lh) vs
// limit`; the kernels whose limit is loop-invariant compare the compile-time slot with ONE per-lane value (limit - 8 lh) instead,
// which keeps the predicates out of the scalar registers.
__device__ __forceinline__ constexpr int attn_key_slot(int kt, int e) { return 32 * kt + 16 * (e >> 3) + (e & 7); }
__device__ __forceinline__ int attn_key(int kt, int e, int lh) { return kt * 32 + (e >> 3) * 16 + lh * 8 + (e & 7); }

// max / sum over lanes l and l ^ 32 on the VALU (v_permlane32_swap; a ds_bpermute would drain the LDS queue)
__device__ __forceinline__ float half_max(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// DT O^T tiles x inv -> out row op (head h of the lane's query row), columns < d
template <int DT>
__device__ __forceinline__ void attn_store_direct(half_t* op, const f32x16 (&o)[DT], float inv, int d, int lh) {
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int dc = i * 32 + 8 * g + 4 * lh;
            if (dc < d) {
                const f16x4 v = {(half_t)(o[i][4 * g] * inv), (half_t)(o[i][4 * g + 1] * inv), (half_t)(o[i][4 * g + 2] * inv),
                                 (half_t)(o[i][4 * g + 3] * inv)};
                *reinterpret_cast<f16x4*>(op + dc) = v;
            }
        }
}
