// p2p.hip - the prompt-to-prompt cross-attention edit, fused and in place.
//
// Reference: AttentionControlEdit.forward, utils/p2p.py:190-207 with replace_cross_attention of AttentionReplace
// (:227, einsum('hpw,bwn->bhpn', base, mapper)), AttentionRefine (:238-241, gather by mapper * alphas + cur * (1 - alphas))
// and AttentionReweight (:254-258, per-token equalizer chained on a previous controller), followed by the time-dependent
// blend  P[1:] = a_t * edit(P[0], P[1:]) + (1 - a_t) * P[1:].  For every controller the result is, per probability row,
//     new_row[b] = base_row . A_b + D_b (*) cur_row[b]
// with a (n_tokens x n_tokens) matrix A_b and a diagonal D_b that depend only on the step (built on the host by
// invertible_cd_amd/p2p.py from the mapper / alphas / equalizer / cross_replace_alpha tensors).  One kernel applies it to
// the conditional rows of the materialised probabilities, in place, where the reference issues a reshape, an einsum or
// gather, two multiplies, an add and a strided copy per layer.
#include <algorithm>
#include <cstdint>
#include "common.h"

namespace {

// One wave = 32 probability rows.  out^T[n][row] = sum_w A^T[n][w] . base^T[w][row] on the matrix cores:
//   B operand: the base rows themselves, 16 B per lane straight from global (lane = row, k = 16ks + 8lh ..),
//   A operand: fragments of the pre-transposed fp16 operator At[e][n][w] (96 x 80 per edit, zero padded),
//   accumulator: lane = row, 4 consecutive tokens per (n-tile, g) -> 8-byte read-modify-write of the edited prompt's row.
constexpr int P2P_KS = 5;          // 16-token k-steps  (80 token slots)
constexpr int P2P_NT = 3;          // 32-token n-tiles  (96 output slots)

// blockIdx.y = prompt group (one image's [base | edits] rows; the groups are contiguous, nedit + 1 prompts each).
__global__ __launch_bounds__(256) void p2p_cross_edit_kernel(half_t* __restrict__ probs, long long rows, long long group_stride,
                                                              int ld, int nedit, const half_t* __restrict__ At,
                                                              const float* __restrict__ D) {
    const int tid = threadIdx.x, l = tid & 63, lr = l & 31, lh = l >> 5, wv = tid >> 6;
    const int grp = blockIdx.y;
    probs += (long long)grp * (nedit + 1) * group_stride;
    At += (long long)grp * nedit * (P2P_NT * 32) * (P2P_KS * 16);
    D += (long long)grp * nedit * (P2P_NT * 32);
    const long long row = ((long long)blockIdx.x * 4 + wv) * 32 + lr;
    const bool ok = row < rows;
    f16x8 z8;
#pragma unroll
    for (int e = 0; e < 8; ++e) z8[e] = (half_t)0.f;
    f16x8 bf[P2P_KS];
#pragma unroll
    for (int ks = 0; ks < P2P_KS; ++ks)
        bf[ks] = ok ? *reinterpret_cast<const f16x8*>(probs + row * ld + ks * 16 + lh * 8) : z8;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < nedit; ++e) {
        const half_t* Ae = At + (long long)e * (P2P_NT * 32) * (P2P_KS * 16);
        f32x16 acc[P2P_NT];
#pragma unroll
        for (int nt = 0; nt < P2P_NT; ++nt)
#pragma unroll
            for (int ks = 0; ks < P2P_KS; ++ks) {
                const f16x8 af = *reinterpret_cast<const f16x8*>(Ae + (nt * 32 + lr) * (P2P_KS * 16) + ks * 16 + lh * 8);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf[ks], ks == 0 ? zero16 : acc[nt], 0, 0, 0);
            }
        if (!ok) continue;
        half_t* cp = probs + (long long)(e + 1) * group_stride + row * ld;
        const float* De = D + (long long)e * (P2P_NT * 32);
#pragma unroll
        for (int nt = 0; nt < P2P_NT; ++nt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = nt * 32 + 8 * g + 4 * lh;
                if (n + 4 > ld) continue;                           // token slots past the row (pad columns stay zero)
                const f16x4 cur = *reinterpret_cast<const f16x4*>(cp + n);
                const f32x4 d = *reinterpret_cast<const f32x4*>(De + n);
                f16x4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (half_t)fmaf(d[i], (float)cur[i], acc[nt][4 * g + i]);
                *reinterpret_cast<f16x4*>(cp + n) = o;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// LocalBlend (utils/p2p.py:18-44).  The heat of a prompt,
//   heat_q[pix] = mean over (layer, head) of sum_w maps[l][(q*H_l + h), pix, w] * alpha[q][w]          (fp32)
// is summed in ONE order everywhere: words ascending inside a (layer, head), then (layer, head) ascending - the order of the
// one-launch kernel this file started with, so results do not depend on how the work is split.  Two ways to get it:
//   * local_blend_heat_kernel (the reduce launch, callers that bring a workspace): every heat map is built once, [prompt][main | sub]
//     [pix] fp32; lanes spread over (layer, head) x pixel, the (layer, head) terms of a pixel meet in LDS and one lane adds them in
//     order.  SDXL's 50 layers x 20 heads x 1024 pixels are read once, by 64 .. 128 blocks.
//   * in the blend kernel itself (no workspace): block p rebuilds the base prompt's heat next to its own - a few hundred KB at SD1.5's
//     five 16 x 16 layers.
// The blend kernel, block p = prompt p:
//   on_q = (maxpool3x3(heat_q) / max(maxpool3x3(heat_q))) > th_pool        (pad = -inf, stride 1; max over the pixels the resize reads)
//   mask_p = on_0 | on_p ;  with substruct words: mask_p &= ~(sub_0 | sub_p), sub_q = (heat'_q / max heat'_q) > th_sub, no pooling
//   out[p] = x[0] + float(mask_p, nearest-resized to H x W) * (x[p] - x[0])     (difference in x's dtype, the rest fp32: torch's
//                                                                               promotion of `base + mask.float() * (x_t - base)`)
// Prompt groups (batched editing): blockIdx.y = group of P contiguous prompts, every index above relative to the group's first
// prompt, with the group's own thresholds; an inactive group (flags bit 0 clear) is copied.  Up to BLEND_MAX_GROUPS per launch.
constexpr int BLEND_MAX_GROUPS = 32;
constexpr int BLEND_MAX_LAYERS = 64;
struct BlendArgs {
    const half_t* maps[BLEND_MAX_LAYERS];
    int heads[BLEND_MAX_LAYERS];
    int n_layers, P, res, n_words, ld;
    const float* alpha;          // [P][n_words]
    const float* alpha_sub;      // [P][n_words] or null
    const float* heat;           // [P][2][res*res] from local_blend_heat_kernel, or null: the blocks build it themselves
    const void* x;               // [P][C][H][W] fp16 or fp32
    int x_f32, C, H, W;
    float* out;                  // [P][C][H][W] fp32
    float th_pool[BLEND_MAX_GROUPS], th_sub[BLEND_MAX_GROUPS];
    int flags[BLEND_MAX_GROUPS]; // bit 0 active, bit 1 substruct words
};

// one (layer, head) term of one pixel: words ascending, words the mask leaves out skipped
__device__ __forceinline__ float blend_word_sum(const half_t* __restrict__ row, const float* __restrict__ al, int n_words) {
    float s = 0.f;
    for (int w = 0; w < n_words; ++w) {
        const float aw = al[w];
        if (aw != 0.f) s += (float)row[w] * aw;
    }
    return s;
}

struct HeatArgs {
    const half_t* maps[BLEND_MAX_LAYERS];
    int heads[BLEND_MAX_LAYERS];
    int n_layers, res2, n_words, ld, total_heads;
    const float* alpha;          // [prompts][n_words]
    const float* alpha_sub;      // [prompts][n_words] or null (then gridDim.z == 1)
    float* heat;                 // [prompts][2][res2]
};

// grid (pixel tiles of HEAT_PIX, prompts, 1 | 2: main / substruct words), 256 threads = HEAT_PIX pixels x HEAT_LANES (layer, head) lanes
constexpr int HEAT_PIX = 16, HEAT_LANES = 16, HEAT_CHUNK = 64;
__global__ __launch_bounds__(256) void local_blend_heat_kernel(HeatArgs a) {
    __shared__ float part[HEAT_CHUNK][HEAT_PIX + 1];
    const int tid = threadIdx.x, px = tid & (HEAT_PIX - 1), lane = tid / HEAT_PIX;
    const int pix = blockIdx.x * HEAT_PIX + px, q = blockIdx.y, sel = blockIdx.z;
    const bool live = pix < a.res2;
    const float* al = (sel ? a.alpha_sub : a.alpha) + (long long)q * a.n_words;
    float tot = 0.f;
    int l = 0, l_first = 0;                                            // layer of this lane's next (layer, head) term, its first term
    for (int c0 = 0; c0 < a.total_heads; c0 += HEAT_CHUNK) {
        const int cn = min(HEAT_CHUNK, a.total_heads - c0);
        for (int i = lane; i < cn; i += HEAT_LANES) {
            const int lh = c0 + i;
            while (lh >= l_first + a.heads[l]) {                                 // lh < total_heads: l stays below n_layers
                l_first += a.heads[l];
                ++l;
            }
            const int h = lh - l_first;
            part[i][px] = live ? blend_word_sum(a.maps[l] + (((long long)q * a.heads[l] + h) * a.res2 + pix) * a.ld, al, a.n_words) : 0.f;
        }
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < cn; ++i) tot += part[i][px];
        __syncthreads();
    }
    if (lane == 0 && live) a.heat[((long long)q * 2 + sel) * a.res2 + pix] = tot / (float)a.total_heads;
}

__global__ __launch_bounds__(256) void local_blend_kernel(BlendArgs a) {
    __shared__ float heat[1024], pooled[1024], red[4];
    __shared__ unsigned char mask[1024], on_tmp[1024], hit_y[32], hit_x[32];
    const int p = blockIdx.x, gl = blockIdx.y, tid = threadIdx.x, res2 = a.res * a.res;
    const long long per = (long long)a.C * a.H * a.W;
    const long long q0 = (long long)gl * a.P;                 // the group's base prompt
    if (!(a.flags[gl] & 1)) {                                  // start_blend not reached / no LocalBlend: x_t unchanged
        for (long long i = tid; i < per; i += 256) {
            const long long o = (q0 + p) * per + i;
            a.out[o] = a.x_f32 ? reinterpret_cast<const float*>(a.x)[o] : (float)reinterpret_cast<const half_t*>(a.x)[o];
        }
        return;
    }
    int total_heads = 0;
    for (int l = 0; l < a.n_layers; ++l) total_heads += a.heads[l];
    for (int i = tid; i < res2; i += 256) mask[i] = 0;
    // The reference normalises AFTER its nearest resize: the maximum is over the map pixels the resize reads - all of them when
    // H, W >= res, every other one of a 16 x 16 map under an 8 x 8 latent.
    const float sy = (float)a.res / (float)a.H, sx = (float)a.res / (float)a.W;
    if (tid < 32) hit_y[tid] = hit_x[tid] = 0;
    __syncthreads();
    for (int i = tid; i < a.H; i += 256) hit_y[min((int)floorf(i * sy), a.res - 1)] = 1;
    for (int i = tid; i < a.W; i += 256) hit_x[min((int)floorf(i * sx), a.res - 1)] = 1;
    __syncthreads();
    // pass 0 / 1: main words of prompt 0 / p (pooled, OR-ed into mask); pass 2 / 3: substruct words (cleared from mask)
    const int npass = (a.alpha_sub && (a.flags[gl] & 2)) ? 4 : 2;
    unsigned char sub_any = 0;
    for (int pass = 0; pass < npass; ++pass) {
        const int q = (pass & 1) ? p : 0;
        const bool sub = pass >= 2;
        if ((pass & 1) && p == 0) continue;                        // the base prompt's own pass is pass 0 / 2
        if (a.heat) {
            const float* hq = a.heat + ((q0 + q) * 2 + (sub ? 1 : 0)) * res2;
            for (int pix = tid; pix < res2; pix += 256) heat[pix] = hq[pix];
        } else {
            const float* al = (sub ? a.alpha_sub : a.alpha) + (q0 + q) * a.n_words;
            for (int pix = tid; pix < res2; pix += 256) {
                float tot = 0.f;
                for (int l = 0; l < a.n_layers; ++l)
                    for (int h = 0; h < a.heads[l]; ++h)
                        tot += blend_word_sum(a.maps[l] + (((q0 + q) * a.heads[l] + h) * res2 + pix) * a.ld, al, a.n_words);
                heat[pix] = tot / (float)total_heads;
            }
        }
        __syncthreads();
        float mx = -INFINITY;
        for (int pix = tid; pix < res2; pix += 256) {
            float v = heat[pix];
            const int y = pix / a.res, x = pix - y * a.res;
            if (!sub) {                                             // 3x3 max pool, stride 1, padding 1 (out-of-range taps ignored)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int yy = y + dy, xx = x + dx;
                        if (yy >= 0 && yy < a.res && xx >= 0 && xx < a.res) v = fmaxf(v, heat[yy * a.res + xx]);
                    }
            }
            pooled[pix] = v;
            if (hit_y[y] && hit_x[x]) mx = fmaxf(mx, v);
        }
        mx = wave_max(mx);                                          // (a maximum does not depend on the order it is taken in)
        if ((tid & 63) == 0) red[tid >> 6] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const float th = sub ? a.th_sub[gl] : a.th_pool[gl];
        for (int pix = tid; pix < res2; pix += 256) {
            const bool on = (pooled[pix] / mx) > th;
            if (!sub) mask[pix] |= on ? 1 : 0;
            else on_tmp[pix] = (pass == 2 ? 0 : on_tmp[pix]) | (on ? 1 : 0);
        }
        __syncthreads();
        if (sub) sub_any = 1;
    }
    if (sub_any) {
        for (int pix = tid; pix < res2; pix += 256) mask[pix] = mask[pix] & (on_tmp[pix] ? 0 : 1);
        __syncthreads();
    }
    // blend
    for (long long i = tid; i < per; i += 256) {
        const int xw = (int)(i % a.W), yh = (int)((i / a.W) % a.H);
        const int my = min((int)floorf(yh * sy), a.res - 1), mxi = min((int)floorf(xw * sx), a.res - 1);
        const float m = mask[my * a.res + mxi] ? 1.f : 0.f;
        float base, diff;
        if (a.x_f32) {
            const float* xf = reinterpret_cast<const float*>(a.x);
            base = xf[q0 * per + i];
            diff = xf[(q0 + p) * per + i] - base;
        } else {
            const half_t* xh = reinterpret_cast<const half_t*>(a.x);
            const half_t b = xh[q0 * per + i];
            base = (float)b;
            diff = (float)(half_t)((float)xh[(q0 + p) * per + i] - base);      // the subtraction happens in fp16 in torch
        }
        a.out[(q0 + p) * per + i] = base + m * diff;
    }
}

// dst[i] += src[i] for many fp16 tensors in ONE launch (AttentionStore.between_steps, utils/p2p.py:164-170: 32 stored maps at SD1.5,
// 130 at SDXL).  blockIdx.y = tensor; its pointers and count come from the kernel arguments (up to 32 tensors, host arrays) or from a
// table in device memory: int64 [3][n] = dst pointers | src pointers | counts.
__device__ __forceinline__ void accumulate_one(half_t* __restrict__ d, const half_t* __restrict__ s, long long n) {
    const long long n8 = n >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        f16x8 x = *reinterpret_cast<const f16x8*>(d + i * 8), y = *reinterpret_cast<const f16x8*>(s + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = (half_t)((float)x[e] + (float)y[e]);
        *reinterpret_cast<f16x8*>(d + i * 8) = x;
    }
    if (blockIdx.x == 0)
        for (long long i = (n8 << 3) + threadIdx.x; i < n; i += 256) d[i] = (half_t)((float)d[i] + (float)s[i]);
}
struct AccumArgs { half_t* dst[32]; const half_t* src[32]; long long n[32]; };
__global__ __launch_bounds__(256) void accumulate_multi_kernel(AccumArgs a) {
    const int t = blockIdx.y;
    accumulate_one(a.dst[t], a.src[t], a.n[t]);
}
__global__ __launch_bounds__(256) void accumulate_table_kernel(const long long* __restrict__ table, int n_tensors) {
    const int t = blockIdx.y;
    accumulate_one(reinterpret_cast<half_t*>(table[t]), reinterpret_cast<const half_t*>(table[n_tensors + t]), table[2 * n_tensors + t]);
}

}  // namespace

extern "C" int icd_p2p_cross_edit_groups(void* probs, int32_t n_groups, int32_t n_prompts, int32_t heads, int64_t nq, int32_t nk,
                                         int32_t ld, const void* At, const float* D, void* stream) {
    ICD_CHECK_ARG(probs && At && D, "icd_p2p_cross_edit: null pointer");
    ICD_CHECK_ARG(n_groups >= 1 && n_groups <= 65535, "icd_p2p_cross_edit_groups: 1 .. 65535 groups (got %d)", n_groups);
    ICD_CHECK_ARG(n_prompts >= 2 && heads > 0 && nq > 0, "icd_p2p_cross_edit: need a base prompt and at least one edit");
    ICD_CHECK_ARG(nk > 0 && nk <= 80 && ld >= 80 && ld % 8 == 0,
                  "icd_p2p_cross_edit: tokens <= 80, row stride >= 80 and a multiple of 8 (got %d, %d)", nk, ld);
    const long long rows = (long long)heads * nq;
    hipLaunchKernelGGL(p2p_cross_edit_kernel, dim3((unsigned)((rows + 127) / 128), (unsigned)n_groups), dim3(256), 0, (hipStream_t)stream,
                       (half_t*)probs, rows, rows * ld, ld, n_prompts - 1, (const half_t*)At, D);
    ICD_CHECK_LAUNCH("icd_p2p_cross_edit");
    return ICD_OK;
}

extern "C" int icd_p2p_cross_edit(void* probs, int32_t n_prompts, int32_t heads, int64_t nq, int32_t nk, int32_t ld,
                                  const void* At, const float* D, void* stream) {
    return icd_p2p_cross_edit_groups(probs, 1, n_prompts, heads, nq, nk, ld, At, D, stream);
}

extern "C" int64_t icd_local_blend_workspace_bytes(int32_t n_groups, int32_t n_prompts, int32_t res) {
    if (n_groups <= 0 || n_prompts <= 0 || res <= 0) return 0;
    return (int64_t)n_groups * n_prompts * 2 * res * res * (int64_t)sizeof(float);
}

extern "C" int icd_local_blend_groups_ws(const void* const* maps, const int32_t* heads, int32_t n_layers, int32_t n_groups, int32_t n_prompts,
                                         int32_t res, int32_t n_words, int32_t ld, const float* alpha, const float* alpha_sub,
                                         const float* th_pool, const float* th_sub, const int32_t* flags, const void* x, int32_t x_is_f32,
                                         int32_t C, int32_t H, int32_t W, float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    ICD_CHECK_ARG(maps && heads && alpha && x && out && th_pool && th_sub && flags, "icd_local_blend: null pointer");
    ICD_CHECK_ARG(n_layers > 0 && n_layers <= BLEND_MAX_LAYERS && n_groups > 0 && n_prompts > 0 && res > 0 && res * res <= 1024 && n_words > 0 &&
                      ld >= n_words,
                  "icd_local_blend: 1..64 layers, res*res <= 1024, ld >= n_words");
    ICD_CHECK_ARG(C > 0 && H > 0 && W > 0, "icd_local_blend: empty latent");
    long long total_heads = 0;
    for (int l = 0; l < n_layers; ++l) {
        ICD_CHECK_ARG(maps[l] && heads[l] > 0, "icd_local_blend: layer %d has no maps", l);
        total_heads += heads[l];
    }
    ICD_CHECK_ARG(total_heads <= 0x7fffffff, "icd_local_blend: too many heads");
    bool any_sub = false, any_active = false;
    for (int g = 0; g < n_groups; ++g) {
        ICD_CHECK_ARG(!(flags[g] & 2) || alpha_sub, "icd_local_blend_groups: group %d has substruct words but alpha_sub is NULL", g);
        any_active |= (flags[g] & 1) != 0;
        any_sub |= (flags[g] & 3) == 3;
    }
    const int res2 = res * res;
    float* heat = nullptr;
    if (workspace) {                                               // the reduce launch: every prompt's heat maps, once
        ICD_CHECK_ARG(workspace_bytes >= icd_local_blend_workspace_bytes(n_groups, n_prompts, res) && (uintptr_t)workspace % 4 == 0,
                      "icd_local_blend: workspace of %lld bytes, icd_local_blend_workspace_bytes asks for %lld", (long long)workspace_bytes,
                      (long long)icd_local_blend_workspace_bytes(n_groups, n_prompts, res));
        ICD_CHECK_ARG((long long)n_groups * n_prompts <= 65535, "icd_local_blend: at most 65535 prompts with a workspace");
        heat = (float*)workspace;
        if (any_active) {
            HeatArgs h{};
            for (int l = 0; l < n_layers; ++l) { h.maps[l] = (const half_t*)maps[l]; h.heads[l] = heads[l]; }
            h.n_layers = n_layers; h.res2 = res2; h.n_words = n_words; h.ld = ld; h.total_heads = (int)total_heads;
            h.alpha = alpha; h.alpha_sub = alpha_sub; h.heat = heat;
            hipLaunchKernelGGL(local_blend_heat_kernel, dim3((res2 + HEAT_PIX - 1) / HEAT_PIX, n_groups * n_prompts, any_sub ? 2 : 1), dim3(256), 0,
                               (hipStream_t)stream, h);
            ICD_CHECK_LAUNCH("icd_local_blend(heat)");
        }
    }
    const long long per = (long long)C * H * W;
    for (int g0 = 0; g0 < n_groups; g0 += BLEND_MAX_GROUPS) {      // (launches in chunks of the groups the argument block holds)
        const int ng = std::min(n_groups - g0, BLEND_MAX_GROUPS);
        const long long s0 = (long long)g0 * n_prompts;            // first prompt of the chunk
        BlendArgs a{};
        for (int l = 0; l < n_layers; ++l) {
            a.maps[l] = (const half_t*)maps[l] + s0 * heads[l] * res2 * ld; a.heads[l] = heads[l];
        }
        a.n_layers = n_layers; a.P = n_prompts; a.res = res; a.n_words = n_words; a.ld = ld;
        a.alpha = alpha + s0 * n_words; a.alpha_sub = alpha_sub ? alpha_sub + s0 * n_words : nullptr;
        a.heat = heat ? heat + s0 * 2 * res2 : nullptr;
        a.x = x_is_f32 ? (const void*)((const float*)x + s0 * per) : (const void*)((const half_t*)x + s0 * per);
        a.x_f32 = x_is_f32; a.C = C; a.H = H; a.W = W; a.out = out + s0 * per;
        for (int g = 0; g < ng; ++g) { a.th_pool[g] = th_pool[g0 + g]; a.th_sub[g] = th_sub[g0 + g]; a.flags[g] = flags[g0 + g]; }
        hipLaunchKernelGGL(local_blend_kernel, dim3(n_prompts, ng), dim3(256), 0, (hipStream_t)stream, a);
        ICD_CHECK_LAUNCH("icd_local_blend");
    }
    return ICD_OK;
}

extern "C" int icd_local_blend_groups(const void* const* maps, const int32_t* heads, int32_t n_layers, int32_t n_groups, int32_t n_prompts,
                                      int32_t res, int32_t n_words, int32_t ld, const float* alpha, const float* alpha_sub, const float* th_pool,
                                      const float* th_sub, const int32_t* flags, const void* x, int32_t x_is_f32, int32_t C, int32_t H, int32_t W,
                                      float* out, void* stream) {
    return icd_local_blend_groups_ws(maps, heads, n_layers, n_groups, n_prompts, res, n_words, ld, alpha, alpha_sub, th_pool, th_sub, flags, x,
                                     x_is_f32, C, H, W, out, nullptr, 0, stream);
}

extern "C" int icd_local_blend(const void* const* maps, const int32_t* heads, int32_t n_layers, int32_t n_prompts, int32_t res,
                               int32_t n_words, int32_t ld, const float* alpha, const float* alpha_sub, float th_pool, float th_sub,
                               const void* x, int32_t x_is_f32, int32_t C, int32_t H, int32_t W, float* out, void* stream) {
    const int32_t flags = 1 | (alpha_sub ? 2 : 0);
    return icd_local_blend_groups(maps, heads, n_layers, 1, n_prompts, res, n_words, ld, alpha, alpha_sub, &th_pool, &th_sub, &flags, x,
                                  x_is_f32, C, H, W, out, stream);
}

static unsigned accumulate_grid_x(long long nmax) {
    return (unsigned)std::min<long long>(std::max<long long>((nmax / 8 + 255) / 256, 1), 512);
}

extern "C" int icd_accumulate_multi(void* const* dst, const void* const* src, const int64_t* counts, int32_t n_tensors, void* stream) {
    ICD_CHECK_ARG(dst && src && counts && n_tensors > 0 && n_tensors <= 32, "icd_accumulate_multi: 1..32 tensors");
    AccumArgs a{};
    long long nmax = 0;
    for (int t = 0; t < n_tensors; ++t) {
        ICD_CHECK_ARG(dst[t] && src[t] && counts[t] >= 0, "icd_accumulate_multi: tensor %d", t);
        ICD_CHECK_ARG(((uintptr_t)dst[t] % 16 == 0) && ((uintptr_t)src[t] % 16 == 0), "icd_accumulate_multi: tensor %d is not 16-byte aligned", t);
        a.dst[t] = (half_t*)dst[t]; a.src[t] = (const half_t*)src[t]; a.n[t] = counts[t];
        nmax = counts[t] > nmax ? counts[t] : nmax;
    }
    hipLaunchKernelGGL(accumulate_multi_kernel, dim3(accumulate_grid_x(nmax), n_tensors), dim3(256), 0, (hipStream_t)stream, a);
    ICD_CHECK_LAUNCH("icd_accumulate_multi");
    return ICD_OK;
}

extern "C" int icd_accumulate_multi_n(const int64_t* table, int32_t n_tensors, int64_t max_count, void* stream) {
    ICD_CHECK_ARG(table && n_tensors > 0 && n_tensors <= 65535 && max_count >= 0, "icd_accumulate_multi_n: 1..65535 tensors and a device table");
    ICD_CHECK_ARG((uintptr_t)table % 8 == 0, "icd_accumulate_multi_n: the table is not 8-byte aligned");
    hipLaunchKernelGGL(accumulate_table_kernel, dim3(accumulate_grid_x(max_count), n_tensors), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)table, (int)n_tensors);
    ICD_CHECK_LAUNCH("icd_accumulate_multi_n");
    return ICD_OK;
}
