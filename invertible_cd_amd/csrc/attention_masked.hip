// attention_masked.hip - attention under a per-sample key count (BERT's padding mask; the self-attention of the BLIP text tower).
//
// Sample b attends to its first min(key_counts[b], Nk) keys; every other key has probability exactly zero.  Nk <= 128, so the whole
// key row of a query tile lives in registers and the softmax is one pass: no running maximum, no rescaling.
//
//   * one wave = 32 query rows of one (sample, head); a block is one wave, nothing is shared, there is no LDS and no barrier.  (The
//     sequences this serves are 35 tokens: two waves per head.  K and V^T fragments come straight from global memory, 16 B per lane.)
//   * S^T = K.Q^T and O^T += V^T.P^T in the fragment layout of attn_frag.h: P goes from the accumulators to the second MFMA with no
//     lane movement.
//   * the mask is a per-element compare of the key index against the wave-uniform count, applied to the scores (-> -inf, so the
//     probability is exp2(-inf) = 0 exactly; the row maximum is clamped to a finite value so that a count <= 0, where every score is
//     -inf, gives zeros and not exp2(-inf - -inf) = NaN) and to the V^T fragment (-> 0: pad columns of V^T may hold anything, and
//     0 * NaN is NaN).  No branch depends on the count.
//   * the denominator sums the fp16-rounded probabilities the numerator uses; a count <= 0 has denominator 0 and writes zeros.
#include "attn_frag.h"
#include "attn_host.h"

namespace {

struct MaskedK {
    const half_t* q; const half_t* k; const half_t* vt; half_t* out; const int32_t* counts;
    int H, Nq, Nk, d, ldq, ldk, ldvt, ldo;
    long long vt_bs;
    float scale_log2;
};

// NT = 32-key tiles (Nk <= 32 NT), DT = 32-row tiles of the head dim (d <= 32 DT)
template <int NT, int DT>
__global__ __launch_bounds__(64) void attn_masked_kernel(MaskedK p) {
    const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 32;
    int kc = p.counts[b];
    kc = kc < p.Nk ? (kc > 0 ? kc : 0) : p.Nk;                        // (0: nothing is attended to)
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- S^T[key, query] = sum_c K[key, c] Q[query, c]
    f32x16 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[t][i] = 0.f;
    const int qrow = q0 + r;
    const half_t* qp = p.q + ((long long)b * p.Nq + (qrow < p.Nq ? qrow : 0)) * p.ldq + h * p.d;
    const int kswz = attn_key_row(r);
    const int ksteps = (p.d + 15) >> 4;
    for (int ks = 0; ks < ksteps; ++ks) {
        const int c = ks * 16 + hf * 8;                               // d % 8 == 0: a chunk of 8 is inside the head dim or outside it
        const bool cin = c < p.d;
        // (written out: a shared Q-fragment loader changed the schedule of every instantiation, profiles/r17_attn_isa.txt)
        const f16x8 qf = (cin && qrow < p.Nq) ? *(const f16x8*)(qp + c) : zero8;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int key = t * 32 + kswz;
            const f16x8 kf = (cin && key < p.Nk) ? *(const f16x8*)(p.k + ((long long)b * p.Nk + key) * p.ldk + h * p.d + c) : zero8;
            s[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf, s[t], 0, 0, 0);
        }
    }

    // ---- one-pass softmax over the keys of this lane's query
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            // (attn_key(t, i, hf) written out: as a call the NT = 1 kernels take 4 more SGPRs, profiles/r17_attn_isa.txt)
            const int key = t * 32 + (i >> 3) * 16 + hf * 8 + (i & 7);
            s[t][i] = key < kc ? s[t][i] * p.scale_log2 : -INFINITY;
            m = fmaxf(m, s[t][i]);
        }
    m = fmaxf(half_max(m), -3.0e38f);                                 // count <= 0: every score is -inf; a finite m keeps -inf - m = -inf
    f16x8 pf[NT][2];
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const half_t ph = (half_t)__builtin_amdgcn_exp2f(s[t][i] - m);      // a masked score is -inf: exactly 0
            pf[t][i >> 3][i & 7] = ph;
            l += (float)ph;
        }
    l = half_sum(l);
    const float inv = l > 0.f ? 1.0f / l : 0.f;

    // ---- O^T[c, query] = sum_key V^T[c, key] P[query, key]
    f32x16 o[DT];
#pragma unroll
    for (int u = 0; u < DT; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[u][i] = 0.f;
    const half_t* vp = p.vt + (long long)b * p.vt_bs + (long long)h * p.d * p.ldvt;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const int key0 = t * 32 + st * 16 + hf * 8;               // ldvt % 8 == 0 and ldvt >= Nk: a chunk that starts below Nk is inside the row
#pragma unroll
            for (int u = 0; u < DT; ++u) {
                const int c = u * 32 + r;
                const f16x8 vf = (c < p.d && key0 < p.Nk) ? *(const f16x8*)(vp + (long long)c * p.ldvt + key0) : zero8;
                u32x4 vw = __builtin_bit_cast(u32x4, vf);              // keys >= count -> 0, as sign-bit masks (no condition registers)
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned lo = (unsigned)((key0 + 2 * w - kc) >> 31), hi = (unsigned)((key0 + 2 * w + 1 - kc) >> 31);
                    vw[w] &= (lo & 0xffffu) | (hi & 0xffff0000u);
                }
                o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, vw), pf[t][st], o[u], 0, 0, 0);
            }
        }

    // ---- out[query, h d + c]
    if (qrow < p.Nq) {
        half_t* op = p.out + ((long long)b * p.Nq + qrow) * p.ldo + h * p.d;
        attn_store_direct(op, o, inv, p.d, hf);
    }
}

struct MaskedRow { int NT, DT; };
constexpr MaskedRow MASKED[16] = {{1, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 1}, {2, 2}, {2, 3}, {2, 4},       // row = 4 (NT - 1) + DT - 1
                                  {3, 1}, {3, 2}, {3, 3}, {3, 4}, {4, 1}, {4, 2}, {4, 3}, {4, 4}};

int masked_validate(const AttnArgs& a, const int32_t* key_counts) {
    ICD_CHECK_ARG(key_counts, "icd_attention_masked: key_counts is null");
    ICD_CHECK_ARG(a.B <= 65535 && a.H <= 65535, "icd_attention_masked: B and H must be <= 65535");
    if (a.d <= 0 || a.d % 8 != 0 || a.d > 128) {
        icd_set_error("icd_attention_masked: head dim must be a multiple of 8, <= 128 (got %d)", a.d);
        return ICD_ERR_UNSUPPORTED;
    }
    if (a.Nk > 128) {
        icd_set_error("icd_attention_masked: at most 128 keys (got %d); longer rows go through icd_attention_fused", a.Nk);
        return ICD_ERR_UNSUPPORTED;
    }
    ICD_CHECK_ARG((uintptr_t)key_counts % 4 == 0, "icd_attention_masked: q, k and vt must be 16-byte aligned, out 8-byte");
    return attn_check_common("icd_attention_masked", a);
}

void masked_plan(int B, int H, int Nq, int Nk, int d, AttnPlan* p) {
    *p = AttnPlan{};
    p->family = ATTN_MASKED; p->variants = 16;
    p->variant = 4 * (Nk <= 32 ? 0 : Nk <= 64 ? 1 : Nk <= 96 ? 2 : 3) + (d <= 32 ? 0 : d <= 64 ? 1 : d <= 96 ? 2 : 3);
    p->NT = MASKED[p->variant].NT; p->DT = MASKED[p->variant].DT;
    p->grid_x = (Nq + 31) / 32; p->grid_y = H; p->grid_z = B;
}

template <int ROW>
int masked_launch_row(const AttnPlan& p, const MaskedK& k, hipStream_t st) {
    hipLaunchKernelGGL((attn_masked_kernel<MASKED[ROW].NT, MASKED[ROW].DT>), dim3(p.grid_x, p.grid_y, p.grid_z), dim3(64), 0, st, k);
    ICD_CHECK_LAUNCH("icd_attention_masked");
    return ICD_OK;
}

}  // namespace

int attn_masked_decide(const AttnArgs& a, const int32_t* key_counts, AttnPlan* p) {
    const int rc = masked_validate(a, key_counts);
    if (rc == ICD_OK) masked_plan(a.B, a.H, a.Nq, a.Nk, a.d, p);
    return rc;
}

extern "C" int icd_attention_masked(const void* q, const void* k, const void* vt, void* out, const int32_t* key_counts, int32_t B,
                                    int32_t H, int32_t Nq, int32_t Nk, int32_t d, int32_t ldq, int32_t ldk, int32_t ldvt, int32_t ldo,
                                    int64_t vt_batch_stride, float scale, void* stream) {
    AttnPlan p;
    const int rc = attn_masked_decide(AttnArgs{q, k, vt, out, B, H, Nq, Nk, d, ldq, ldk, ldvt, ldo, vt_batch_stride, scale}, key_counts, &p);
    if (rc != ICD_OK) return rc;
    const MaskedK kk{(const half_t*)q, (const half_t*)k, (const half_t*)vt, (half_t*)out, key_counts, H, Nq, Nk, d, ldq, ldk, ldvt, ldo,
                     vt_batch_stride > 0 ? vt_batch_stride : (long long)H * d * ldvt, scale * ATTN_LOG2E};
    return attn_launch_row(p.variant, [&](auto row) { return masked_launch_row<decltype(row)::value>(p, kk, (hipStream_t)stream); },
                           std::make_index_sequence<16>{});
}
