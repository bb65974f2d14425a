// LPIPS on the device (invertible_cd_amd/lpips.py): the ReLU and 2 x 2 max-pool between the 3 x 3 convolutions of the VGG16 stack (which
// are icd_gemm's), and the distance head: channel normalisation, squared difference, per-channel weights, spatial mean.  All are
// bandwidth kernels with 16-byte accesses and 64-bit row offsets; no float atomics, every sum has a fixed order.  (The ingest of the
// uint8 images, icd_image_resize_norm, is ingest.hip's.)
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ ReLU, max-pool
__device__ __forceinline__ f16x8 relu8(f16x8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] > (half_t)0 ? v[j] : (half_t)0;
    return v;
}

__global__ __launch_bounds__(256) void relu_kernel(const half_t* x, long long nvec, half_t* out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    *reinterpret_cast<f16x8*>(out + i * 8) = relu8(*reinterpret_cast<const f16x8*>(x + i * 8));
}

// One thread owns 8 channels of one output pixel: four 16-byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const half_t* x, long long total, int H, int W, int Ho, int Wo, int vpr, int relu,
                                                         half_t* out) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= total) return;
    const long long pix = it / vpr;                             // (b * Ho + yo) * Wo + xo
    const int c8 = (int)(it - pix * vpr) * 8;
    const long long by = pix / Wo;
    const int xo = (int)(pix - by * Wo);
    const long long b = by / Ho;
    const int yo = (int)(by - b * Ho);
    const long long C = (long long)vpr * 8;
    const half_t* src = x + ((b * H + 2 * yo) * W + 2 * xo) * C + c8;
    const f16x8 a = *reinterpret_cast<const f16x8*>(src), bq = *reinterpret_cast<const f16x8*>(src + C);
    const f16x8 c = *reinterpret_cast<const f16x8*>(src + (long long)W * C), d = *reinterpret_cast<const f16x8*>(src + (long long)W * C + C);
    f16x8 m;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const half_t t = a[j] > bq[j] ? a[j] : bq[j], u = c[j] > d[j] ? c[j] : d[j];
        m[j] = t > u ? t : u;
    }
    if (relu) m = relu8(m);
    *reinterpret_cast<f16x8*>(out + pix * C + c8) = m;
}

// --------------------------------------------------------------------------------------------------------------- the distance head
constexpr int LP_THREADS = 256;
constexpr int LP_PASSES = 8;                   // pixels per lane group of one block

inline int lp_group(int C) {                   // lanes that own one pixel: C / 8 rounded up to a power of two, at most 64
    int g = 1;
    while (g < 64 && g * 8 < C) g <<= 1;
    return g;
}
inline int lp_blocks(int HW, int C) {          // blocks per sample
    const int ppb = LP_THREADS / lp_group(C) * LP_PASSES;
    return (HW + ppb - 1) / ppb;
}

__device__ __forceinline__ float group_sum_n(float v, int G) {                // G a power of two <= 64, wave-uniform; every lane gets the sum
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct Vec8 { float v[8]; };
__device__ __forceinline__ Vec8 load8(const half_t* p, int relu) {
    const f16x8 h = *reinterpret_cast<const f16x8*>(p);
    Vec8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float f = (float)h[j]; r.v[j] = relu ? fmaxf(f, 0.f) : f; }
    return r;
}
__device__ __forceinline__ float sumsq8(const Vec8& a) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += a.v[j] * a.v[j];
    return s;
}
// sum_j w_j (a_j r1 - b_j r2)^2: the two products are rounded on their own (no contraction into the subtraction), so that identical
// inputs give exactly zero
__device__ __forceinline__ float wdiff8(const Vec8& a, const Vec8& b, float r1, float r2, const float* w) {
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w), w1 = *reinterpret_cast<const f32x4*>(w + 4);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float d;
        {
#pragma clang fp contract(off)
            const float na = a.v[j] * r1, nb = b.v[j] * r2;
            d = na - nb;
        }
        s += (j < 4 ? w0[j] : w1[j - 4]) * d * d;
    }
    return s;
}

// grid (blocks per sample, B).  A group of G lanes owns a pixel of both halves; the groups of a block walk LP_PASSES pixels each in a
// fixed order, then one thread adds the groups' sums in group order: partial[b][block] depends on nothing but the sample's own data.
__global__ __launch_bounds__(LP_THREADS) void lpips_layer_kernel(const half_t* f, int ldf, int B, int HW, int C, const float* w, int relu,
                                                                 int G, float* partial) {
    __shared__ float gsum[LP_THREADS];
    const int b = blockIdx.y, ngroups = LP_THREADS / G;
    const int g = threadIdx.x / G, l = threadIdx.x - g * G;
    const int p0 = blockIdx.x * ngroups * LP_PASSES;
    const half_t* f1 = f + (long long)b * HW * ldf;
    const half_t* f2 = f + ((long long)B + b) * HW * ldf;
    const int c0 = l * 8, step = G * 8;
    float acc = 0.f;
    for (int it = 0; it < LP_PASSES; ++it) {
        const int p = p0 + it * ngroups + g;                    // wave-uniform per group; G <= 64 divides the wave
        if (p >= HW) break;
        const half_t* pa = f1 + (long long)p * ldf;
        const half_t* pb = f2 + (long long)p * ldf;
        const bool own = c0 < C;
        Vec8 a0 = {}, b0 = {};
        if (own) { a0 = load8(pa + c0, relu); b0 = load8(pb + c0, relu); }
        float s1 = sumsq8(a0), s2 = sumsq8(b0);
        for (int c = c0 + step; c < C; c += step) {             // C > 512 only
            s1 += sumsq8(load8(pa + c, relu));
            s2 += sumsq8(load8(pb + c, relu));
        }
        s1 = group_sum_n(s1, G); s2 = group_sum_n(s2, G);
        const float r1 = 1.0f / (sqrtf(s1) + 1e-10f), r2 = 1.0f / (sqrtf(s2) + 1e-10f);
        float d = own ? wdiff8(a0, b0, r1, r2, w + c0) : 0.f;
        for (int c = c0 + step; c < C; c += step) d += wdiff8(load8(pa + c, relu), load8(pb + c, relu), r1, r2, w + c);
        acc += group_sum_n(d, G);
    }
    if (l == 0) gsum[g] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < ngroups; ++i) s += gsum[i];
        partial[(long long)b * gridDim.x + blockIdx.x] = s;
    }
}

// One wave per sample: lane l adds partials l, l + 64, ... in order, the lanes are added by a fixed butterfly.
__global__ __launch_bounds__(64) void lpips_finish_kernel(const float* partial, int nblk, float inv_hw, int accumulate, float* out) {
    const int b = blockIdx.x;
    const float* p = partial + (long long)b * nblk;
    float s = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 64) s += p[i];
    s = group_sum_n(s, 64);
    if (threadIdx.x == 0) {
        const float v = s * inv_hw;
        out[b] = accumulate ? out[b] + v : v;
    }
}

}  // namespace

extern "C" int icd_relu(const void* x, int64_t n, void* out, void* stream) {
    ICD_CHECK_ARG(x && out, "icd_relu: null pointer");
    ICD_CHECK_ARG(n > 0 && n % 8 == 0, "icd_relu: n must be a positive multiple of 8 (got %lld)", (long long)n);
    ICD_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "icd_relu: pointers must be 16-byte aligned");
    const long long nvec = n / 8, blocks = (nvec + 255) / 256;
    ICD_CHECK_ARG(blocks <= 0x7fffffffLL, "icd_relu: %lld blocks exceed the grid limit", blocks);
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, nvec, (half_t*)out);
    ICD_CHECK_LAUNCH("icd_relu");
    return ICD_OK;
}

extern "C" int icd_maxpool2x2(const void* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t relu, void* out, void* stream) {
    ICD_CHECK_ARG(x && out, "icd_maxpool2x2: null pointer");
    ICD_CHECK_ARG(B > 0, "icd_maxpool2x2: B must be positive (got %d)", B);
    ICD_CHECK_ARG(H >= 2 && W >= 2, "icd_maxpool2x2: H and W must be at least 2 (got %d x %d)", H, W);
    ICD_CHECK_ARG(C > 0 && C % 8 == 0, "icd_maxpool2x2: C must be a positive multiple of 8 (got %d)", C);
    ICD_CHECK_ARG(relu == 0 || relu == 1, "icd_maxpool2x2: relu must be 0 or 1");
    ICD_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "icd_maxpool2x2: pointers must be 16-byte aligned");
    ICD_CHECK_ARG(x != out, "icd_maxpool2x2: in-place pooling is not supported");
    const int Ho = H / 2, Wo = W / 2, vpr = C / 8;
    const long long total = (long long)B * Ho * Wo * vpr, blocks = (total + 255) / 256;
    ICD_CHECK_ARG(blocks <= 0x7fffffffLL, "icd_maxpool2x2: %lld blocks exceed the grid limit", blocks);
    hipLaunchKernelGGL(maxpool2x2_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, total, H, W, Ho, Wo,
                       vpr, relu, (half_t*)out);
    ICD_CHECK_LAUNCH("icd_maxpool2x2");
    return ICD_OK;
}

extern "C" int64_t icd_lpips_layer_workspace_bytes(int32_t B, int32_t HW, int32_t C) {
    if (B <= 0 || HW <= 0 || C <= 0) return 0;
    return (int64_t)B * lp_blocks(HW, C) * (int64_t)sizeof(float);
}

extern "C" int icd_lpips_layer(const void* f, int32_t ldf, int32_t B, int32_t HW, int32_t C, const float* w, int32_t relu,
                               int32_t accumulate, void* workspace, int64_t workspace_bytes, float* out, void* stream) {
    ICD_CHECK_ARG(f && w && workspace && out, "icd_lpips_layer: null pointer");
    ICD_CHECK_ARG(B > 0 && B <= 65535, "icd_lpips_layer: B must be positive, at most 65535 (got %d)", B);
    ICD_CHECK_ARG(HW > 0, "icd_lpips_layer: HW must be positive (got %d)", HW);
    ICD_CHECK_ARG(C > 0 && C % 8 == 0, "icd_lpips_layer: C must be a positive multiple of 8 (got %d)", C);
    ICD_CHECK_ARG(ldf >= C && ldf % 8 == 0, "icd_lpips_layer: ldf must be a multiple of 8, >= C (got %d, C %d)", ldf, C);
    ICD_CHECK_ARG(relu == 0 || relu == 1, "icd_lpips_layer: relu must be 0 or 1");
    ICD_CHECK_ARG(accumulate == 0 || accumulate == 1, "icd_lpips_layer: accumulate must be 0 or 1");
    ICD_CHECK_ARG((((uintptr_t)f | (uintptr_t)w) & 15) == 0 && (((uintptr_t)workspace | (uintptr_t)out) & 3) == 0,
                  "icd_lpips_layer: f and w must be 16-byte aligned, workspace and out 4-byte aligned");
    const int64_t need = icd_lpips_layer_workspace_bytes(B, HW, C);
    ICD_CHECK_ARG(workspace_bytes >= need, "icd_lpips_layer: workspace of %lld bytes is too small (need %lld)", (long long)workspace_bytes,
                  (long long)need);
    const int G = lp_group(C), nblk = lp_blocks(HW, C);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lpips_layer_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(LP_THREADS), 0, st, (const half_t*)f, ldf, B, HW, C, w, relu,
                       G, (float*)workspace);
    ICD_CHECK_LAUNCH("icd_lpips_layer");
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)workspace, nblk, 1.0f / (float)HW, accumulate, out);
    ICD_CHECK_LAUNCH("icd_lpips_layer (finish)");
    return ICD_OK;
}
