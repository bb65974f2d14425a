// layernorm_f32.hip - LayerNorm of an fp32 stream (the post-LayerNorm blocks of the BLIP text tower: x <- LN(x + f(x))).
//
// The sum x + f(x) arrives in fp32 from the GEMM epilogue (icd_gemm_desc.out_f32) and is normalised here with no fp16 rounding in
// between; the result leaves twice, as fp16 for the next GEMM and as fp32 for the next residual add.
//
// One wave per row, four rows per block; a row (<= 16 KiB) is read three times, the second and third time from cache:
//   1. the mean, summed in double (a row of mean 100 and deviation 0.1 loses its deviation's low bits in an fp32 sum),
//   2. the variance as the mean of (x - mean)^2 - the exact two-pass form, the differences taken in double and squared in fp32,
//   3. the normalised, affine row.
#include "common.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, long long rows, int C, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, half_t* __restrict__ out16,
                                                            float* __restrict__ out32) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                           // wave-uniform
    const float* xr = x + row * C;
    double sum = 0.0;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        sum += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
    }
    const double mean = wave_sum_f64(sum) / C;
    float sq = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dlt = (float)((double)v[j] - mean);
            sq += dlt * dlt;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / C + eps);
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *(const f32x4*)(xr + c);
        const f32x4 g = *(const f32x4*)(gamma + c), bt = *(const f32x4*)(beta + c);
        f32x4 y;
        f16x4 yh;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            y[j] = (float)((double)v[j] - mean) * rstd * g[j] + bt[j];
            yh[j] = (half_t)y[j];
        }
        if (out32) *(f32x4*)(out32 + row * C + c) = y;
        if (out16) *(f16x4*)(out16 + row * C + c) = yh;
    }
}

}  // namespace

extern "C" int icd_layernorm_f32(const float* x, int64_t rows, int32_t C, const float* gamma, const float* beta, float eps, void* out16,
                                 float* out32, void* stream) {
    ICD_CHECK_ARG(x && gamma && beta, "icd_layernorm_f32: null pointer");
    ICD_CHECK_ARG(out16 || out32, "icd_layernorm_f32: both outputs are null");
    ICD_CHECK_ARG(rows > 0 && rows <= 4ll * 0x7fffffff, "icd_layernorm_f32: rows must be positive");
    if (C <= 0 || C % 8 != 0 || C > 4096) {
        icd_set_error("icd_layernorm_f32: C must be a multiple of 8, <= 4096 (got %d)", C);
        return ICD_ERR_UNSUPPORTED;
    }
    ICD_CHECK_ARG(eps >= 0.f, "icd_layernorm_f32: eps must not be negative");
    ICD_CHECK_ARG(((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out32) % 16 == 0 && (uintptr_t)out16 % 8 == 0,
                  "icd_layernorm_f32: x, gamma, beta and out32 must be 16-byte aligned, out16 8-byte");
    hipLaunchKernelGGL(layernorm_f32_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (long long)rows, C, gamma,
                       beta, eps, (half_t*)out16, out32);
    ICD_CHECK_LAUNCH("icd_layernorm_f32");
    return ICD_OK;
}
