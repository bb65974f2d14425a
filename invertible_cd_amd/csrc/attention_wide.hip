// attention_wide.hip - flash attention at head dims 168 .. 512 (the mid-block attention of AutoencoderKL: one head as wide as the block,
// 512 channels at the SD / SDXL width).  out = softmax(scale q k^T) v with no N^2 buffer; not causal, no prescaled form.
//
//   * the head dim is split over the waves of a block: a block owns one 32-query tile of one (sample, head) and runs NW = ceil(d / 128)
//     waves; wave w owns head-dim columns [128 w, 128 w + 128) (the last slice may be ragged: fragments outside d are zero).  Per wave:
//     8 Q fragments, 4 O^T accumulator tiles and the partial S^T of a 64-key tile - the register budget of a head dim of 128.
//   * per 64-key tile, in the fragment layout of attn_frag.h: every wave computes its PARTIAL S^T = K_w Q_w^T over its slice and writes
//     it to an LDS exchange buffer (NW x 8 KiB, two of them: tile t + 1 writes the other one, so ONE barrier per tile orders both the
//     read-after-write of this tile and the write-after-read of the tile before).  After the barrier every wave sums the NW partials in
//     the fixed order 0, 1, ..: all waves hold the same bits, whatever the timing, and run the same online softmax redundantly
//     (running maximum, moved only when a row maximum outgrows it by more than 2^8, as in the tiled kernel).  P goes from the
//     accumulators to the second MFMA with no lane movement; each wave accumulates O_w^T += V^T_w P^T for its own 128 columns.
//   * K and V^T fragments are consumed by exactly one wave of the block, so they come straight from global memory, 16 B per lane, with
//     no LDS staging: V^T of a tile is requested at its top, K of the next tile as soon as this tile's S^T MFMAs have read the registers.
//     Every such load is unconditional, at a clamped address; what a clamp reads is masked, meets a zero operand or is never stored.
//   * the ragged last key tile masks its scores to -inf and its V^T fragment to 0 (pad columns of V^T may hold anything, NaN included).
//   * the denominator sums the fp16-rounded probabilities the numerator uses.
#include "attn_frag.h"
#include "attn_host.h"

namespace {

struct WideK {
    const half_t* q; const half_t* k; const half_t* vt; half_t* out;
    int H, Nq, Nk, d, ldq, ldk, ldvt, ldo, nqt;
    long long vt_bs;
    float scale_log2;
};

constexpr float WIDE_LAZY = 8.f;          // the running offset moves when a row maximum exceeds it by more than this (P <= 2^8 in fp16)

// K fragments of 64-key tile `tile` for this wave's slice: kb = k + sample + head + slice + 8 hf, dw = columns of the slice inside d.
// Every load is unconditional, at a clamped address (a conditional load is a branch of its own, and the waits around 32 of them drain
// the whole queue): a key >= Nk reads key Nk - 1, and its score is masked; a chunk outside d reads chunk 0, and meets a zero Q fragment.
__device__ __forceinline__ void wide_load_k(f16x8 (&kf)[2][8], const half_t* kb, int tile, int kswz, int hf, int dw, int Nk, int ldk) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int key = tile * 64 + t * 32 + kswz;
        const half_t* kr = kb + (long long)(key < Nk ? key : Nk - 1) * ldk;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) kf[t][ks] = *(const f16x8*)(kr + (ks * 16 + hf * 8 < dw ? ks * 16 : -hf * 8));      // (kb holds + 8 hf)
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_wide_kernel(WideK p) {
    __shared__ f32x4 xch[2][NW][8][64];                               // [buffer][wave][4 accumulator elements][lane]
    const int lane = threadIdx.x & 63, r = lane & 31, hf = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x / p.nqt, q0 = (blockIdx.x - bh * p.nqt) * 32;
    const int b = bh / p.H, h = bh - b * p.H;
    const int c0 = 128 * w;                                           // this wave's slice of the head dim
    const int dw = p.d - c0 < 128 ? p.d - c0 : 128;                   // columns of it inside the head dim (d % 8 == 0: whole chunks of 8)
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    const int qrow = q0 + r;
    f16x8 qf[8];
    {
        const half_t* qp = p.q + ((long long)b * p.Nq + (qrow < p.Nq ? qrow : 0)) * p.ldq + h * p.d + c0 + hf * 8;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) qf[ks] = (ks * 16 + hf * 8 < dw && qrow < p.Nq) ? *(const f16x8*)(qp + ks * 16) : zero8;
    }
    const int kswz = attn_key_row(r);
    const half_t* kb = p.k + (long long)b * p.Nk * p.ldk + h * p.d + c0 + hf * 8;
    const half_t* vb = p.vt + (long long)b * p.vt_bs + (long long)(h * p.d + c0) * p.ldvt;

    f32x16 o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[u][i] = 0.f;
    float m = -INFINITY, l = 0.f;

    f16x8 kf[2][8];
    wide_load_k(kf, kb, 0, kswz, hf, dw, p.Nk, p.ldk);
    const int ntiles = (p.Nk + 63) >> 6, kclamp = (p.Nk - 1) & ~7;
    for (int tile = 0; tile < ntiles; ++tile) {
        const bool ragged = tile * 64 + 64 > p.Nk;                    // (block-uniform)
        // ---- V^T fragments of this tile: head-dim row 32 u + r of the slice, keys 64 tile + 16 j + 8 hf .. + 7.  Unconditional loads
        // again: a row outside d reads row 0 of the slice into accumulator rows that are never stored; a chunk at or beyond Nk reads the
        // chunk that holds key Nk - 1 (ldvt % 8 == 0 and ldvt >= Nk: inside the row) and is zeroed below, as every key >= Nk is.
        f16x8 vf[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = u * 32 + r;
            const half_t* vr = vb + (long long)(c < dw ? c : 0) * p.ldvt;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int key0 = tile * 64 + j * 16 + hf * 8;
                vf[u][j] = *(const f16x8*)(vr + (key0 < p.Nk ? key0 : kclamp));
            }
        }

        // ---- partial S^T[key, query] over this wave's slice of the head dim
        f32x16 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) s[t][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[t][ks], qf[ks], s[t], 0, 0, 0);
        f32x4 (&xb)[NW][8][64] = xch[tile & 1];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) xb[w][t * 4 + g][lane] = f32x4{s[t][4 * g], s[t][4 * g + 1], s[t][4 * g + 2], s[t][4 * g + 3]};
        if (tile + 1 < ntiles) wide_load_k(kf, kb, tile + 1, kswz, hf, dw, p.Nk, p.ldk);      // (in flight under the softmax and P.V)
        __syncthreads();

        // ---- S^T = partial 0 + partial 1 + .. (the same order, so the same bits, in every wave)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 a = xb[0][t * 4 + g][lane];
#pragma unroll
                for (int ww = 1; ww < NW; ++ww) a += xb[ww][t * 4 + g][lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) s[t][4 * g + e] = a[e];
            }

        // ---- the ragged last tile, in ONE block-uniform branch: scores of keys >= Nk -> -inf (scale > 0 keeps them there), their V^T
        // elements -> 0 as sign-bit masks
        if (ragged) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) s[t][i] = tile * 64 + attn_key(t, i, hf) < p.Nk ? s[t][i] : -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int key0 = tile * 64 + j * 16 + hf * 8;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    u32x4 vw = __builtin_bit_cast(u32x4, vf[u][j]);
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const unsigned lo = (unsigned)((key0 + 2 * x - p.Nk) >> 31), hi = (unsigned)((key0 + 2 * x + 1 - p.Nk) >> 31);
                        vw[x] &= (lo & 0xffffu) | (hi & 0xffff0000u);
                    }
                    vf[u][j] = __builtin_bit_cast(f16x8, vw);
                }
            }
        }

        // ---- online softmax over the keys of this lane's query
        float mt = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                s[t][i] *= p.scale_log2;
                mt = fmaxf(mt, s[t][i]);
            }
        mt = half_max(mt);                                            // finite: key 64 tile is below Nk
        if (__builtin_amdgcn_ballot_w64(mt > m + WIDE_LAZY) != 0) {   // (first tile: m = -inf, every row moves)
            const float mn = fmaxf(m, mt);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);       // m = -inf: 0, and o = l = 0
            m = mn;
            l *= alpha;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[u][i] *= alpha;
        }
        f16x8 pf[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const half_t ph = (half_t)__builtin_amdgcn_exp2f(s[t][i] - m);      // a masked score is -inf: exactly 0
                pf[t][i >> 3][i & 7] = ph;
                l += (float)ph;
            }

        // ---- O^T[c, query] += sum_key V^T[c, key] P[query, key]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u) o[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[u][j], pf[j >> 1][j & 1], o[u], 0, 0, 0);
    }

    // ---- out[query, h d + 128 w + c]
    l = half_sum(l);
    if (qrow < p.Nq) {
        half_t* op = p.out + ((long long)b * p.Nq + qrow) * p.ldo + h * p.d + c0;
        attn_store_direct(op, o, 1.0f / l, dw, hf);
    }
}

struct WideRow { int NW; };
constexpr WideRow WIDE[3] = {{2}, {3}, {4}};                          // row = ceil(d / 128) - 2
constexpr int wide_lds(const WideRow& r) { return 2 * r.NW * 8192; }

int wide_validate(const AttnArgs& a) {
    if (a.d < 168 || a.d > 512 || a.d % 8 != 0) {
        icd_set_error("icd_attention_wide: head dim must be a multiple of 8 in 168 ... 512 (got %d); up to 160 goes through icd_attention_fused", a.d);
        return ICD_ERR_UNSUPPORTED;
    }
    const int rc = attn_check_common("icd_attention_wide", a);
    if (rc != ICD_OK) return rc;
    // (a launch holds fewer than 2^32 threads: 2^24 blocks of up to 256)
    ICD_CHECK_ARG(((long long)a.Nq + 31) / 32 * a.B * a.H < (1LL << 24), "icd_attention_wide: ceil(Nq / 32) * B * H exceeds the grid limit");
    return ICD_OK;
}

void wide_plan(int B, int H, int Nq, int d, AttnPlan* p) {
    *p = AttnPlan{};
    p->family = ATTN_WIDE; p->variants = 3;
    p->variant = (d + 127) / 128 - 2;
    const WideRow& r = WIDE[p->variant];
    p->NW = r.NW; p->KS = 8; p->DT = 4; p->NT = 2;                     // per wave: 8 k-steps, 4 O^T tiles, 2 32-key tiles per step of the loop
    p->grid_x = (Nq + 31) / 32 * B * H; p->grid_y = p->grid_z = 1;
    p->lds_bytes = wide_lds(r);
}

template <int ROW>
int wide_launch_row(const AttnPlan& p, const WideK& k, hipStream_t st) {
    constexpr WideRow R = WIDE[ROW];
    static_assert(wide_lds(R) <= 64 * 1024, "the exchange buffers are static LDS");
    hipLaunchKernelGGL((attn_wide_kernel<R.NW>), dim3(p.grid_x), dim3(64 * R.NW), 0, st, k);
    ICD_CHECK_LAUNCH("icd_attention_wide");
    return ICD_OK;
}

}  // namespace

int attn_wide_decide(const AttnArgs& a, AttnPlan* p) {
    const int rc = wide_validate(a);
    if (rc == ICD_OK) wide_plan(a.B, a.H, a.Nq, a.d, p);
    return rc;
}

extern "C" int icd_attention_wide(const void* q, const void* k, const void* vt, void* out, int32_t B, int32_t H, int32_t Nq, int32_t Nk,
                                  int32_t d, int32_t ldq, int32_t ldk, int32_t ldvt, int32_t ldo, int64_t vt_batch_stride, float scale,
                                  void* stream) {
    AttnPlan p;
    const int rc = attn_wide_decide(AttnArgs{q, k, vt, out, B, H, Nq, Nk, d, ldq, ldk, ldvt, ldo, vt_batch_stride, scale}, &p);
    if (rc != ICD_OK) return rc;
    const WideK kk{(const half_t*)q, (const half_t*)k, (const half_t*)vt, (half_t*)out, H, Nq, Nk, d, ldq, ldk, ldvt, ldo, (Nq + 31) / 32,
                   vt_batch_stride > 0 ? vt_batch_stride : (long long)H * d * ldvt, scale * ATTN_LOG2E};
    return attn_launch_row(p.variant, [&](auto row) { return wide_launch_row<decltype(row)::value>(p, kk, (hipStream_t)stream); },
                           std::make_index_sequence<3>{});
}
