// ffn_fused.hip - the GEGLU feed-forward of a transformer block as ONE launch (icd_ffn_geglu):
//     out = resid + (value * gelu(gate)) @ W2^T + b2,   [value | gate] = LN(x) @ W1^T + b1
// The 4C-wide hidden tensor of the two-launch form (icd_gemm with ICD_GEMM_GEGLU, then the output projection) never reaches memory.
//
// The feed-forward is flash attention with another row function, on the fragment layout of attn_frag.h:
//     keys    = the 4C hidden units, 32 per chunk          K   = W1 (value rows and gate rows of the chunk)
//     softmax = value * gelu(gate): elementwise, no running maximum and no rescaling
//     V^T     = W2 (row n holds the hidden units contiguously: already "transposed")       head dim = C = 320
// A wave owns 32 activation rows.  Their MFMA B fragments (K = 320: 20 k-steps, 80 registers) come straight from global memory
// once, as attn_cross_kernel loads K / V.  H^T = W1.x^T leaves the accumulators with ONE activation row per lane, so the LayerNorm
// fold rstd (acc - mu s) + b is two per-lane scalars (gemm_epilogue.h, GEGLU patches: the same FMAs in the same order), and the
// fp16-rounded H^T is directly the B operand of out^T += W2.H^T - as P feeds P.V.  Only weights go through LDS: per 32 hidden units
// 64 rows of W1 (40 KiB) and a 320 x 32 slice of W2 (20 KiB), double-buffered by LDS-DMA; the chunk after the current one is
// in flight under its 60 MFMAs.  One workgroup of 4 waves (128 rows) per CU, one wave per SIMD: 160 accumulators + 80 operand
// registers per lane.  Every ds_read_b128 feeds one MFMA (half the LDS read rate a CU has, MI355X: 256 B / clock).
// The epilogue is the GEMMs' own (gemm_epilogue.h wave_epilogue on a 1 x 10 wave tile): bias, residual, error carry, fp32 twin.
#include "attn_frag.h"
#include "gemm_epilogue.h"

using namespace icd_gemm_detail;

namespace {

constexpr int FFN_C = 320;                            // model width the kernel is specialised on
constexpr int FFN_HID = 4 * FFN_C;
constexpr int FFN_KS = FFN_C / 16;                    // k-steps of H^T = W1.x^T
constexpr int FFN_NT = FFN_C / 32;                    // 32-column tiles of out^T
constexpr int FFN_CHUNKS = FFN_HID / 32;
constexpr int FFN_W1_BYTES = 64 * FFN_C * 2;          // LDS image of one chunk: 64 rows of W1 ...
constexpr int FFN_W2_BYTES = FFN_C * 32 * 2;          // ... and 320 rows x 32 hidden units of W2
constexpr int FFN_STAGE = FFN_W1_BYTES + FFN_W2_BYTES;
constexpr int FFN_TAB = 2 * FFN_HID * 4;              // b1 or the LayerNorm column sums of W1: 2560 floats
constexpr int FFN_LDS = 2 * FFN_STAGE + 2 * FFN_TAB;  // 140 KiB
constexpr int FFN_ROWS = 128;                         // activation rows per workgroup

struct FfnK {
    const half_t* x; const half_t* w1; const half_t* w2;
    const float* b1; const float* ln_s; const float* b2;
    const float* ln_stats; float* ln_stats_w;         // LN: statistics read, or (ln_stats_w) computed from the fragments and stored
    const void* resid; const unsigned char* resid_c;
    half_t* out; unsigned char* out_c; float* out32;
    int M, ldx, ldw1, ldw2, ldo, ldr, flags;
    float ln_eps;
};

// LDS images (16-byte slots), both free of bank conflicts for the fragment reads (ds_read_b128 is served in groups of 16 lanes):
//   W1: row r (0..31 value, 32..63 gate; rows enter the MFMA through attn_key_row), 40 slots per row, slot c at c ^ ((r >> 1) & 7)
//   W2: row n (0..319), 4 slots per row, slot c at c ^ ((n >> 2) & 3)
// LDS-DMA fills an image in slot order, 64 slots per wave instruction: the lane computes which (row, slot) its slot holds.
template <bool LN, bool CARRY>
__global__ __launch_bounds__(256, 1) void ffn_fused_kernel(FfnK a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const int tid = threadIdx.x, l = tid & 63, lr = l & 31, lh = l >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * FFN_ROWS;
    float* tab_b = reinterpret_cast<float*>(smem + 2 * FFN_STAGE);
    float* tab_s = tab_b + 2 * FFN_HID;

    // ---- weight stream: per-lane source offsets of the 10 + 5 DMA instructions a wave issues per chunk
    const auto rs1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.w1), 0,
                                                       (unsigned)(((long long)(2 * FFN_HID - 1) * a.ldw1 + FFN_C) * 2), 0x00020000);
    const auto rs2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<half_t*>(a.w2), 0,
                                                       (unsigned)(((long long)(FFN_C - 1) * a.ldw2 + FFN_HID) * 2), 0x00020000);
    int voff1[10], voff2[5];
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const int s = (wv * 10 + i) * 64 + l, r = s / 40, c = (s - r * 40) ^ ((r >> 1) & 7);
        voff1[i] = (r * a.ldw1 + c * 8) * 2;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int s = (wv * 5 + i) * 64 + l, n = s >> 2, c = (s & 3) ^ ((n >> 2) & 3);
        voff2[i] = (n * a.ldw2 + c * 8) * 2;
    }
    auto issue = [&](int j, int stage) {
        unsigned char* d1 = smem + stage * FFN_STAGE + wv * 10 * 1024;
        unsigned char* d2 = smem + stage * FFN_STAGE + FFN_W1_BYTES + wv * 5 * 1024;
        const int so1 = j * 64 * a.ldw1 * 2, so2 = j * 64;
#pragma unroll
        for (int i = 0; i < 10; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (__attribute__((address_space(3))) void*)(d1 + i * 1024), 16, voff1[i], so1, 0, 0);
#pragma unroll
        for (int i = 0; i < 5; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs2, (__attribute__((address_space(3))) void*)(d2 + i * 1024), 16, voff2[i], so2, 0, 0);
    };
    issue(0, 0);

    // ---- the wave's 32 activation rows as B fragments: lane (lr, lh) holds columns 16 ks + 8 lh .. + 7 of row lr
    const int row = m0 + wv * 32 + lr;
    const bool row_ok = row < a.M;
    f16x8 z8;
#pragma unroll
    for (int e = 0; e < 8; ++e) z8[e] = (half_t)0.f;
    f16x8 xf[FFN_KS];
    {
        const half_t* xp = a.x + (long long)(row_ok ? row : 0) * a.ldx + lh * 8;
#pragma unroll
        for (int ks = 0; ks < FFN_KS; ++ks) xf[ks] = *reinterpret_cast<const f16x8*>(xp + ks * 16);
        if (!row_ok)
#pragma unroll
            for (int ks = 0; ks < FFN_KS; ++ks) xf[ks] = z8;
    }
    // b1 and the LayerNorm column sums, once, for every chunk
    for (int i = tid; i < 2 * FFN_HID / 4; i += 256) {
        reinterpret_cast<f32x4*>(tab_b)[i] = a.b1 ? reinterpret_cast<const f32x4*>(a.b1)[i] : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (LN) reinterpret_cast<f32x4*>(tab_s)[i] = reinterpret_cast<const f32x4*>(a.ln_s)[i];
    }
    // LayerNorm of the row as two scalars: value = acc * ra + (s * rm + b)
    float ra = 1.f, rm = 0.f;
    if (LN) {
        float mean, rstd;
        if (a.ln_stats_w) {                           // statistics from the fragments: the lane and lane ^ 32 hold the whole row
            float s = 0.f;
#pragma unroll
            for (int ks = 0; ks < FFN_KS; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) s += (float)xf[ks][e];
            mean = half_sum(s) * (1.f / FFN_C);
            float q = 0.f;
#pragma unroll
            for (int ks = 0; ks < FFN_KS; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float dlt = (float)xf[ks][e] - mean; q = __builtin_fmaf(dlt, dlt, q); }
            rstd = rsqrtf(half_sum(q) * (1.f / FFN_C) + a.ln_eps);
            if (row_ok && lh == 0) *reinterpret_cast<f32x2*>(a.ln_stats_w + 2 * (long long)row) = (f32x2){mean, rstd};
        } else {
            const f32x2 st = row_ok ? *reinterpret_cast<const f32x2*>(a.ln_stats + 2 * (long long)row) : (f32x2){0.f, 1.f};
            mean = st[0]; rstd = st[1];
        }
        ra = rstd; rm = -rstd * mean;
    }
    const f32x2 ra2 = {ra, ra}, rm2 = {rm, rm};

    // ---- fragment addresses inside a stage
    const int prow = attn_key_row(lr);
    int t1[4];                                        // W1: slot (2 ks | lh) ^ f of row prow, for the 4 values of (2 ks) & 7
#pragma unroll
    for (int q = 0; q < 4; ++q) t1[q] = prow * (FFN_C * 2) + (((2 * q) | lh) ^ ((prow >> 1) & 7)) * 16;
    int t2[2];                                        // W2: slot (2 st + lh) ^ f of row lr
#pragma unroll
    for (int st = 0; st < 2; ++st) t2[st] = FFN_W1_BYTES + lr * 64 + (((2 * st) | lh) ^ ((lr >> 2) & 3)) * 16;

    f32x16 o[1][FFN_NT];
#pragma unroll
    for (int i = 0; i < FFN_NT; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[0][i][e] = 0.f;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    auto chunk = [&](int j, int stage) {
        const unsigned char* sb = smem + stage * FFN_STAGE;
        // H^T tiles of the chunk: gate first, so that its GELU can run beside the value tile's MFMAs
        f32x16 sg = zero16, sv = zero16;
#pragma unroll
        for (int ks = 0; ks < FFN_KS; ++ks) {
            const f16x8 wg = *reinterpret_cast<const f16x8*>(sb + 32 * FFN_C * 2 + t1[ks & 3] + (ks >> 2) * 128);
            sg = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg, xf[ks], sg, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < FFN_KS; ++ks) {
            const f16x8 wvf = *reinterpret_cast<const f16x8*>(sb + t1[ks & 3] + (ks >> 2) * 128);
            sv = __builtin_amdgcn_mfma_f32_32x32x16_f16(wvf, xf[ks], sv, 0, 0, 0);
        }
        // accumulator element e is hidden unit 32 j + 16 (e >> 3) + 8 lh + (e & 7) (attn_key) of the lane's row
        const float* bp = tab_b + 64 * j + 8 * lh;
        const float* sp = tab_s + 64 * j + 8 * lh;
        f16x8 hf[2];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + 16 * st + 4 * q), bg = *reinterpret_cast<const f32x4*>(bp + 32 + 16 * st + 4 * q);
                f32x4 cv = bv, cg = bg;
                if (LN) {
                    const f32x4 s_v = *reinterpret_cast<const f32x4*>(sp + 16 * st + 4 * q), s_g = *reinterpret_cast<const f32x4*>(sp + 32 + 16 * st + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { cv[e] = __builtin_fmaf(s_v[e], rm, bv[e]); cg[e] = __builtin_fmaf(s_g[e], rm, bg[e]); }
                }
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const int ae = 8 * st + 4 * q + e;
                    const f32x2 v2 = __builtin_elementwise_fma((f32x2){sv[ae], sv[ae + 1]}, ra2, (f32x2){cv[e], cv[e + 1]});
                    const f32x2 g2 = __builtin_elementwise_fma((f32x2){sg[ae], sg[ae + 1]}, ra2, (f32x2){cg[e], cg[e + 1]});
                    const f32x2 h2 = v2 * gelu_fast2(g2);
                    hf[st][4 * q + e] = (half_t)h2[0]; hf[st][4 * q + e + 1] = (half_t)h2[1];
                }
            }
        // out^T += W2.H^T: the fp16-rounded hidden values are the B operand as they stand
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int i = 0; i < FFN_NT; ++i) {
                const f16x8 w2f = *reinterpret_cast<const f16x8*>(sb + t2[st] + i * 2048);
                o[0][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2f, hf[st], o[0][i], 0, 0, 0);
            }
    };

    // chunk j + 1 lands in the other stage while chunk j is consumed.  The barrier at the top says both "every wave's part of chunk j
    // has landed" (each waited for its own DMA) and "every wave is done with the stage chunk j + 1 goes to" (read by chunk j - 1).
    for (int j = 0; j < FFN_CHUNKS; j += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        issue(j + 1, 1);
        chunk(j, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (j + 2 < FFN_CHUNKS) issue(j + 2, 0);
        chunk(j + 1, 1);
    }

    // ---- epilogue: the GEMMs' own, on a 1 x 10 wave tile (first thing it does is the barrier that frees the stages)
    GemmK p = {};
    p.bias = a.b2; p.resid = reinterpret_cast<const half_t*>(a.resid); p.out = a.out;
    p.M = a.M; p.N = FFN_C; p.K = FFN_HID; p.Nw = FFN_C; p.ldo = a.ldo; p.ldr = a.ldr;
    p.alpha = 1.f; p.flags = a.flags; p.ksplit = 1;
    p.out32 = a.out32; p.resid_c = a.resid_c; p.out_c = a.out_c;
    p.orm_pack = 1u; p.orm_magic = 0u;
    wave_epilogue<1, FFN_NT, true, CARRY>(p, o, smem, wv, wv, 0, l, m0, 0, 0, nullptr);
}

template <bool LN, bool CARRY>
int launch(const FfnK& k, hipStream_t st) {
    static std::atomic<unsigned long long> armed{0};
    return icd_launch_lds(armed, "icd_ffn_geglu", ffn_fused_kernel<LN, CARRY>, dim3((k.M + FFN_ROWS - 1) / FFN_ROWS), dim3(256), FFN_LDS, st, k);
}

}  // namespace

extern "C" int icd_ffn_geglu(const icd_ffn_desc* d, void* stream) {
    ICD_CHECK_ARG(d != nullptr, "icd_ffn_geglu: descriptor must be non-null");
    ICD_CHECK_ARG(d->x && d->w1 && d->w2 && d->out, "icd_ffn_geglu: x, w1, w2 and out must be non-null");
    ICD_CHECK_ARG(d->C == FFN_C && d->hidden == FFN_HID, "icd_ffn_geglu: C = %d, hidden = %d: the kernel is built for C = 320, hidden = 1280", d->C,
                  d->hidden);
    ICD_CHECK_ARG(d->M > 0, "icd_ffn_geglu: M = %d must be positive", d->M);
    ICD_CHECK_ARG((d->flags & ~(ICD_GEMM_LN_COMPUTE | ICD_GEMM_RESID_F32)) == 0, "icd_ffn_geglu: flags 0x%x: only ICD_GEMM_LN_COMPUTE and ICD_GEMM_RESID_F32", d->flags);
    ICD_CHECK_ARG(d->ldx >= FFN_C && d->ldx % 8 == 0 && d->ldo >= FFN_C && d->ldo % 8 == 0, "icd_ffn_geglu: ldx = %d, ldo = %d must be multiples of 8, >= C",
                  d->ldx, d->ldo);
    ICD_CHECK_ARG(d->ldw1 >= FFN_C && d->ldw1 % 8 == 0 && d->ldw2 >= FFN_HID && d->ldw2 % 8 == 0,
                  "icd_ffn_geglu: ldw1 = %d (>= C) and ldw2 = %d (>= hidden) must be multiples of 8", d->ldw1, d->ldw2);
    ICD_CHECK_ARG((long long)(2 * FFN_HID) * d->ldw1 * 2 < (1ll << 31) && (long long)FFN_C * d->ldw2 * 2 < (1ll << 31),
                  "icd_ffn_geglu: weight leading dimensions beyond 31-bit byte offsets");
    const bool ln = d->ln_stats != nullptr || (d->flags & ICD_GEMM_LN_COMPUTE);
    ICD_CHECK_ARG(!(d->flags & ICD_GEMM_LN_COMPUTE) || d->ln_stats, "icd_ffn_geglu: ICD_GEMM_LN_COMPUTE stores the statistics: ln_stats must be non-null");
    ICD_CHECK_ARG(!ln || d->ln_colsum, "icd_ffn_geglu: the LayerNorm fold needs ln_colsum (row sums of the gamma-scaled W1)");
    ICD_CHECK_ARG(ln || !d->ln_colsum, "icd_ffn_geglu: ln_colsum without ln_stats: give both for the LayerNorm fold, or neither");
    ICD_CHECK_ARG(!d->resid || d->ldr >= FFN_C, "icd_ffn_geglu: ldr = %d must be >= C", d->ldr);
    ICD_CHECK_ARG(!(d->flags & ICD_GEMM_RESID_F32) || d->resid, "icd_ffn_geglu: ICD_GEMM_RESID_F32 without resid");
    ICD_CHECK_ARG(!d->resid_carry || (d->resid && !(d->flags & ICD_GEMM_RESID_F32)), "icd_ffn_geglu: resid_carry goes with an fp16 resid");
    ICD_CHECK_ARG(!((d->resid_carry || d->out_carry) && d->out_f32), "icd_ffn_geglu: the error carry and the fp32 twin are alternatives");
    ICD_CHECK_ARG(!d->resid || d->ldr % 8 == 0, "icd_ffn_geglu: ldr = %d must be a multiple of 8", d->ldr);
    const uintptr_t al16 = (uintptr_t)d->x | (uintptr_t)d->w1 | (uintptr_t)d->w2 | (uintptr_t)d->out | (uintptr_t)d->resid | (uintptr_t)d->b1 |
                           (uintptr_t)d->b2 | (uintptr_t)d->ln_colsum | (uintptr_t)d->out_f32;
    ICD_CHECK_ARG((al16 & 15) == 0, "icd_ffn_geglu: x, w1, w2, out, resid, b1, b2, ln_colsum and out_f32 must be 16-byte aligned");
    ICD_CHECK_ARG((((uintptr_t)d->ln_stats | (uintptr_t)d->resid_carry | (uintptr_t)d->out_carry) & 7) == 0,
                  "icd_ffn_geglu: ln_stats, resid_carry and out_carry must be 8-byte aligned");
    FfnK k = {};
    k.x = (const half_t*)d->x; k.w1 = (const half_t*)d->w1; k.w2 = (const half_t*)d->w2;
    k.b1 = d->b1; k.ln_s = d->ln_colsum; k.b2 = d->b2;
    k.ln_stats = d->ln_stats; k.ln_stats_w = (d->flags & ICD_GEMM_LN_COMPUTE) ? const_cast<float*>(d->ln_stats) : nullptr;
    k.resid = d->resid; k.resid_c = (const unsigned char*)d->resid_carry;
    k.out = (half_t*)d->out; k.out_c = (unsigned char*)d->out_carry; k.out32 = d->out_f32;
    k.M = d->M; k.ldx = d->ldx; k.ldw1 = d->ldw1; k.ldw2 = d->ldw2; k.ldo = d->ldo; k.ldr = d->ldr;
    k.flags = d->flags & ICD_GEMM_RESID_F32;
    k.ln_eps = d->ln_eps > 0.f ? d->ln_eps : 1e-5f;
    hipStream_t st = (hipStream_t)stream;
    const bool carry = k.resid_c || k.out_c;
    if (ln) return carry ? launch<true, true>(k, st) : launch<true, false>(k, st);
    return carry ? launch<false, true>(k, st) : launch<false, false>(k, st);
}
