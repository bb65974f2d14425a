// Pillow's BICUBIC resample on the device, the part every image ingest shares: the fixed-point constants, the tables' descriptor and the
// horizontal pass (invertible_cd_amd/resample.py builds the coefficient tables).  Included by metrics.hip (icd_clip_preprocess) and
// lpips.hip (icd_image_resize_norm); each translation unit gets its own copy of the kernel.
#pragma once
#include "common.h"

namespace {

constexpr int PREC_BITS = 32 - 8 - 2;          // Pillow's fixed-point fraction
constexpr int HROWS = 4;                       // image rows per block of the horizontal pass

__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = (acc + (1 << (PREC_BITS - 1))) >> PREC_BITS;
    return (unsigned)min(max(v, 0), 255);
}

struct PreK {
    const unsigned char* img;                  // [B, H, W, 3]
    unsigned char* tmp;                        // [B * H, S, 3]: the horizontal pass, cropped to the S columns that survive
    half_t* out;                               // [B * G * G, ldo]
    const int *hfirst, *hcount, *hcoef, *vfirst, *vcount, *vcoef;     // tables, already offset to the crop's first column / row
    int B, H, W, S, P, G, ldo, hk, vk;
    long long rows;                            // B * H
    float mean[3], stdv[3];
};

// Horizontal pass.  One block owns HROWS consecutive image rows (they are contiguous in memory): 16-byte loads stage them in LDS, every
// thread then produces 4 consecutive output bytes of one row (taps from LDS) and stores them as one dword.
__global__ __launch_bounds__(256) void clip_resample_h_kernel(PreK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const long long r0 = (long long)blockIdx.x * HROWS;
    const int nrows = (int)min((long long)HROWS, p.rows - r0);
    const long long rowb = (long long)p.W * 3;
    const long long total = p.rows * rowb;
    const long long start = r0 * rowb, end = start + nrows * rowb;
    // 16-byte chunks are taken at aligned ADDRESSES: the batch may start anywhere (a slice of a larger tensor), and so may its rows
    const int mis = (int)((uintptr_t)p.img & 15);
    const long long a0 = (start + mis) & ~15LL;                // offsets from the aligned address below the base
    const int shift = (int)(start + mis - a0);
    const int nchunk = (int)((end + mis - a0 + 15) >> 4);
    const unsigned char* abase = p.img - mis;
    for (int c = threadIdx.x; c < nchunk; c += blockDim.x) {
        const long long off = a0 + (long long)c * 16;
        if (off >= mis && off + 16 <= total + mis) {
            *reinterpret_cast<uint4*>(lds + c * 16) = *reinterpret_cast<const uint4*>(abase + off);
        } else {                                               // the first / last bytes of the batch: nothing outside the buffer is read
            for (int j = 0; j < 16; ++j) lds[c * 16 + j] = (off + j >= mis && off + j < total + mis) ? abase[off + j] : 0;
        }
    }
    __syncthreads();
    const int wpr = p.S * 3 / 4;                               // output dwords per row
    for (int it = threadIdx.x; it < nrows * wpr; it += blockDim.x) {
        const int row = it / wpr, wd = it - row * wpr;
        const unsigned char* src = lds + shift + (long long)row * rowb;
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = wd * 4 + j, x = e / 3, c = e - x * 3;
            const int f = max(p.hfirst[x], 0);
            const int n = min(p.hcount[x], min(p.hk, p.W - f));     // clamped: a wrong table cannot read outside the row
            const int* kk = p.hcoef + (long long)x * p.hk;
            int acc = 0;
            for (int k = 0; k < n; ++k) acc += kk[k] * (int)src[(f + k) * 3 + c];
            packed |= clip8(acc) << (8 * j);
        }
        *reinterpret_cast<unsigned*>(p.tmp + (r0 + row) * (long long)(p.S * 3) + wd * 4) = packed;
    }
}

}  // namespace
