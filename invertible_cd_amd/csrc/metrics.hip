// Edit-quality metrics on the device: CLIP / DINOv2 image preprocessing (Pillow's BICUBIC resample, bit for bit), the token assembly of
// a ViT's embeddings, row-wise cosine, and the exact integer sum of squared differences behind PSNR.  All are bandwidth kernels; the
// resample arithmetic is restated from Pillow's documented behaviour (invertible_cd_amd/resample.py builds the coefficient tables).
#include "common.h"
#include "resample_pass.h"

namespace {

// Vertical pass + crop + normalise + patch scatter.  One block owns one row of patches (P output rows): the resampled bytes go to LDS,
// then the G patch-matrix rows leave as 16-byte stores in column order (c * P + py) * P + px, pad columns zero.
__global__ __launch_bounds__(256) void clip_resample_v_kernel(PreK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // [P, S * 3]
    const int b = blockIdx.x / p.G, pr = blockIdx.x - b * p.G;
    const int rowb = p.S * 3, wpr = rowb / 4;
    const unsigned char* src = p.tmp + (long long)b * p.H * rowb;
    for (int it = threadIdx.x; it < p.P * wpr; it += blockDim.x) {
        const int yy = it / wpr, wd = it - yy * wpr;
        const int y = pr * p.P + yy;
        const int f = max(p.vfirst[y], 0);
        const int n = min(p.vcount[y], min(p.vk, p.H - f));
        const int* kk = p.vcoef + (long long)y * p.vk;
        const unsigned char* col = src + (long long)f * rowb + wd * 4;
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                          // four neighbouring bytes of each tap row: one 4-byte segment per lane
            int acc = 0;
            for (int k = 0; k < n; ++k) acc += kk[k] * (int)col[(long long)k * rowb + j];
            packed |= clip8(acc) << (8 * j);
        }
        *reinterpret_cast<unsigned*>(lds + yy * rowb + wd * 4) = packed;
    }
    __syncthreads();
    const int PP = p.P * p.P, cols = 3 * PP, vpr = p.ldo / 8;
    half_t* out = p.out + ((long long)b * p.G + pr) * p.G * p.ldo;
    for (int it = threadIdx.x; it < p.G * vpr; it += blockDim.x) {
        const int px_blk = it / vpr, c8 = (it - px_blk * vpr) * 8;
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int col = c8 + j;
            float f = 0.f;
            if (col < cols) {
                const int c = col / PP, rem = col - c * PP, py = rem / p.P, px = rem - py * p.P;
                const float u = (float)lds[py * rowb + (px_blk * p.P + px) * 3 + c];
                f = (u / 255.0f - p.mean[c]) / p.stdv[c];
            }
            v[j] = (half_t)f;
        }
        *reinterpret_cast<f16x8*>(out + (long long)px_blk * p.ldo + c8) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------- ViT token assembly
// One thread owns 8 consecutive columns of one output row: two 16-byte loads from the token table (and from the patch GEMM's fp32
// accumulator for a patch row), one fp32 add, two 16-byte fp32 stores and one 16-byte fp16 store.  Row offsets are 64-bit.
__global__ __launch_bounds__(256) void vit_tokens_kernel(const float* acc, int lda, const float* tok, long long total, int T, int vpr,
                                                         half_t* out16, float* out32) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= total) return;
    const long long row = it / vpr;                            // b * T + t
    const int c8 = (int)(it - row * vpr) * 8;
    const long long b = row / T;
    const int t = (int)(row - b * T);
    const int C = vpr * 8;
    const float* pt = tok + (long long)t * C + c8;
    f32x4 lo = *reinterpret_cast<const f32x4*>(pt), hi = *reinterpret_cast<const f32x4*>(pt + 4);
    if (t > 0) {                                               // patch p = t - 1 of image b: row b * n + p of the accumulator
        const float* pa = acc + (b * (T - 1) + (t - 1)) * (long long)lda + c8;
        lo = *reinterpret_cast<const f32x4*>(pa) + lo;
        hi = *reinterpret_cast<const f32x4*>(pa + 4) + hi;
    }
    float* po = out32 + row * C + c8;
    *reinterpret_cast<f32x4*>(po) = lo;
    *reinterpret_cast<f32x4*>(po + 4) = hi;
    f16x8 h;
#pragma unroll
    for (int j = 0; j < 4; ++j) { h[j] = (half_t)lo[j]; h[4 + j] = (half_t)hi[j]; }
    *reinterpret_cast<f16x8*>(out16 + row * C + c8) = h;
}

// ---------------------------------------------------------------------------------------------------------------- cosine of rows
template <typename T>
__global__ __launch_bounds__(256) void cosine_rows_kernel(const T* a, const T* b, long long rows, int D, int lda, int ldb, float* out) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);     // one wave per row
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const T* pa = a + r * lda;
    const T* pb = b + r * ldb;
    constexpr int V = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(V)));
    float dot = 0.f, na = 0.f, nb = 0.f;
    const bool vec = ((lda | ldb) % V) == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
    const int dv = vec ? D / V : 0;
    for (int i = lane; i < dv; i += 64) {
        const vec_t x = *reinterpret_cast<const vec_t*>(pa + i * V), y = *reinterpret_cast<const vec_t*>(pb + i * V);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float fx = (float)x[j], fy = (float)y[j];
            dot += fx * fy; na += fx * fx; nb += fy * fy;
        }
    }
    for (int i = dv * V + lane; i < D; i += 64) {
        const float fx = (float)pa[i], fy = (float)pb[i];
        dot += fx * fy; na += fx * fx; nb += fy * fy;
    }
    dot = wave_sum(dot); na = wave_sum(na); nb = wave_sum(nb);
    if (lane == 0) out[r] = dot / (sqrtf(na) * sqrtf(nb));     // x / |x| . y / |y| as the reference forms it: a zero row gives NaN there too
}

// ------------------------------------------------------------------------------------------- exact sum of squared byte differences
constexpr int SQ_CHUNK = 256 * 16 * 8;         // bytes of one row per block: 8 x 16-byte loads per thread

__global__ __launch_bounds__(256) void sq_diff_sum_u8_kernel(const unsigned char* a, const unsigned char* b, long long n, unsigned long long* out) {
    const long long row = blockIdx.y;
    const unsigned char* pa = a + row * n;
    const unsigned char* pb = b + row * n;
    const long long c0 = (long long)blockIdx.x * SQ_CHUNK, c1 = min(c0 + SQ_CHUNK, n);
    unsigned acc = 0;                          // <= 128 bytes per thread * 65025 fits 32 bits
    if (((((uintptr_t)pa) | ((uintptr_t)pb)) & 15) == 0) {
        for (long long i = c0 + threadIdx.x * 16; i + 16 <= c1; i += 256 * 16) {
            const uint4 x = *reinterpret_cast<const uint4*>(pa + i), y = *reinterpret_cast<const uint4*>(pb + i);
            const unsigned xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int s = 0; s < 32; s += 8) {
                    const int d = (int)((xs[w] >> s) & 255u) - (int)((ys[w] >> s) & 255u);
                    acc += (unsigned)(d * d);
                }
        }
        const long long tail = c0 + ((c1 - c0) & ~15LL);       // SQ_CHUNK is a multiple of 16: only the row's last chunk has a tail
        for (long long i = tail + threadIdx.x; i < c1; i += 256) {
            const int d = (int)pa[i] - (int)pb[i];
            acc += (unsigned)(d * d);
        }
    } else {
        for (long long i = c0 + threadIdx.x; i < c1; i += 256) {      // 128 bytes per thread
            const int d = (int)pa[i] - (int)pb[i];
            acc += (unsigned)(d * d);
        }
    }
    // 64 lanes * 128 * 65025 overflows 32 bits: widen before the reduction
    unsigned long long s = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out + row, part[0] + part[1] + part[2] + part[3]);
}

}  // namespace

extern "C" int icd_clip_preprocess(const void* images, int32_t B, int32_t H, int32_t W, int32_t resized_h, int32_t resized_w, int32_t crop,
                                   int32_t patch, const int32_t* h_first, const int32_t* h_count, const int32_t* h_coef, int32_t h_taps,
                                   const int32_t* v_first, const int32_t* v_count, const int32_t* v_coef, int32_t v_taps,
                                   const float* mean, const float* stdv, void* tmp, void* out, int32_t ldo, void* stream) {
    ICD_CHECK_ARG(images && tmp && out && mean && stdv, "icd_clip_preprocess: null pointer");
    ICD_CHECK_ARG(h_first && h_count && h_coef && v_first && v_count && v_coef, "icd_clip_preprocess: null coefficient table");
    ICD_CHECK_ARG(B > 0, "icd_clip_preprocess: B must be positive (got %d)", B);
    ICD_CHECK_ARG(H > 0 && W > 0 && resized_h > 0 && resized_w > 0, "icd_clip_preprocess: sizes must be positive");
    ICD_CHECK_ARG(patch > 0 && crop > 0 && crop % patch == 0 && crop % 4 == 0 && crop <= 1024 && patch <= 64,
                  "icd_clip_preprocess: crop must be a multiple of the patch size and of 4, <= 1024");
    ICD_CHECK_ARG(resized_h >= crop && resized_w >= crop, "icd_clip_preprocess: the resized image (%d x %d) is smaller than the crop %d",
                  resized_h, resized_w, crop);
    ICD_CHECK_ARG(ldo % 8 == 0 && ldo >= 3 * patch * patch, "icd_clip_preprocess: ldo must be a multiple of 8, >= 3 * patch^2");
    ICD_CHECK_ARG(W <= 4096, "icd_clip_preprocess: image width %d exceeds 4096", W);
    ICD_CHECK_ARG(((uintptr_t)tmp & 3) == 0 && ((uintptr_t)out & 15) == 0,
                  "icd_clip_preprocess: tmp must be 4-byte aligned, out 16-byte aligned");
    ICD_CHECK_ARG((long long)patch * crop * 3 <= 65536, "icd_clip_preprocess: patch * crop * 3 = %lld bytes of LDS exceed 64 KiB",
                  (long long)patch * crop * 3);
    // the tables' row length follows from the sizes (Pillow: 2 * ceil(2 * max(in / out, 1)) + 1): a table built for other sizes is refused
    auto taps = [](int in, int o) { const double s = (double)in / o; return (int)ceil(2.0 * (s > 1.0 ? s : 1.0)) * 2 + 1; };
    ICD_CHECK_ARG(h_taps == taps(W, resized_w) && v_taps == taps(H, resized_h),
                  "icd_clip_preprocess: tables do not match the sizes (taps %d / %d, expected %d / %d)", h_taps, v_taps, taps(W, resized_w),
                  taps(H, resized_h));
    for (int c = 0; c < 3; ++c) ICD_CHECK_ARG(stdv[c] > 0.f, "icd_clip_preprocess: std must be positive");
    PreK p;
    p.img = (const unsigned char*)images; p.tmp = (unsigned char*)tmp; p.out = (half_t*)out;
    const int left = (resized_w - crop) / 2, top = (resized_h - crop) / 2;
    p.hfirst = h_first + left; p.hcount = h_count + left; p.hcoef = h_coef + (long long)left * h_taps;
    p.vfirst = v_first + top; p.vcount = v_count + top; p.vcoef = v_coef + (long long)top * v_taps;
    p.B = B; p.H = H; p.W = W; p.S = crop; p.P = patch; p.G = crop / patch; p.ldo = ldo; p.hk = h_taps; p.vk = v_taps;
    p.rows = (long long)B * H;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    hipStream_t st = (hipStream_t)stream;
    const size_t lds_h = (size_t)HROWS * W * 3 + 32;
    hipLaunchKernelGGL(clip_resample_h_kernel, dim3((unsigned)((p.rows + HROWS - 1) / HROWS)), dim3(256), lds_h, st, p);
    ICD_CHECK_LAUNCH("icd_clip_preprocess (horizontal)");
    hipLaunchKernelGGL(clip_resample_v_kernel, dim3((unsigned)(B * p.G)), dim3(256), (size_t)patch * crop * 3, st, p);
    ICD_CHECK_LAUNCH("icd_clip_preprocess (vertical)");
    return ICD_OK;
}

extern "C" int icd_vit_tokens(const float* acc, int32_t lda, const float* tok, int32_t B, int32_t n, int32_t C, void* out16, float* out32,
                              void* stream) {
    ICD_CHECK_ARG(acc && tok && out16 && out32, "icd_vit_tokens: null pointer");
    ICD_CHECK_ARG(B >= 1 && n >= 1, "icd_vit_tokens: B and n must be positive (got %d, %d)", B, n);
    ICD_CHECK_ARG(C > 0 && C % 8 == 0, "icd_vit_tokens: C must be a positive multiple of 8 (got %d)", C);
    ICD_CHECK_ARG(lda >= C && lda % 4 == 0, "icd_vit_tokens: lda must be a multiple of 4, >= C (got %d, C %d)", lda, C);
    ICD_CHECK_ARG((((uintptr_t)acc | (uintptr_t)tok | (uintptr_t)out16 | (uintptr_t)out32) & 15) == 0,
                  "icd_vit_tokens: pointers must be 16-byte aligned");
    const int vpr = C / 8;
    const long long total = (long long)B * ((long long)n + 1) * vpr;
    const long long blocks = (total + 255) / 256;
    ICD_CHECK_ARG(blocks <= 0x7fffffffLL, "icd_vit_tokens: %lld blocks exceed the grid limit", blocks);
    hipLaunchKernelGGL(vit_tokens_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, lda, tok, total, n + 1, vpr,
                       (half_t*)out16, out32);
    ICD_CHECK_LAUNCH("icd_vit_tokens");
    return ICD_OK;
}

extern "C" int icd_cosine_rows(const void* a, const void* b, int64_t rows, int32_t D, int32_t lda, int32_t ldb, int32_t is_f32, float* out,
                               void* stream) {
    ICD_CHECK_ARG(a && b && out, "icd_cosine_rows: null pointer");
    ICD_CHECK_ARG(rows > 0 && D > 0 && lda >= D && ldb >= D, "icd_cosine_rows: bad shape (rows %lld, D %d, lda %d, ldb %d)", (long long)rows, D,
                  lda, ldb);
    ICD_CHECK_ARG(is_f32 == 0 || is_f32 == 1, "icd_cosine_rows: is_f32 must be 0 or 1");
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (is_f32)
        hipLaunchKernelGGL(cosine_rows_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)a, (const float*)b, (long long)rows,
                           D, lda, ldb, out);
    else
        hipLaunchKernelGGL(cosine_rows_kernel<half_t>, grid, dim3(256), 0, (hipStream_t)stream, (const half_t*)a, (const half_t*)b,
                           (long long)rows, D, lda, ldb, out);
    ICD_CHECK_LAUNCH("icd_cosine_rows");
    return ICD_OK;
}

extern "C" int icd_sq_diff_sum_u8(const void* a, const void* b, int64_t rows, int64_t n, uint64_t* out, void* stream) {
    ICD_CHECK_ARG(a && b && out, "icd_sq_diff_sum_u8: null pointer");
    ICD_CHECK_ARG(rows > 0 && rows <= 65535 && n > 0, "icd_sq_diff_sum_u8: rows must be in 1 .. 65535 and n positive");
    ICD_CHECK_ARG(n <= (1LL << 40), "icd_sq_diff_sum_u8: n too large");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, (size_t)rows * sizeof(uint64_t), st) != hipSuccess) {
        icd_set_error("icd_sq_diff_sum_u8: hipMemsetAsync failed");
        return ICD_ERR_HIP;
    }
    hipLaunchKernelGGL(sq_diff_sum_u8_kernel, dim3((unsigned)((n + SQ_CHUNK - 1) / SQ_CHUNK), (unsigned)rows), dim3(256), 0, st,
                       (const unsigned char*)a, (const unsigned char*)b, (long long)n, (unsigned long long*)out);
    ICD_CHECK_LAUNCH("icd_sq_diff_sum_u8");
    return ICD_OK;
}
