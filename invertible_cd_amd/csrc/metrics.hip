// Edit-quality metrics on the device: the token assembly of a ViT's embeddings, row-wise cosine, and the exact integer sum of squared
// differences behind PSNR.  All are bandwidth kernels.  (The image preprocessing of CLIP / DINOv2 is ingest.hip's.)
#include "common.h"

namespace {

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
