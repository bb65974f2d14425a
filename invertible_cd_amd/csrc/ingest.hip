// Image ingest on the device: uint8 NHWC images through Pillow's two-pass resample (BICUBIC or LANCZOS, bit for bit), cropped, into what
// each metric's network reads.  invertible_cd_amd/resample.py builds the coefficient tables; the arithmetic is restated from Pillow's
// documented behaviour.
//   icd_clip_preprocess    CLIP / DINOv2: shortest-edge resize, centre crop, normalise, scatter into the ViT's patch matrix
//   icd_image_resize_norm  LPIPS: both axes stretched to S x S, normalise, NHWC fp16 padded to 8 channels
//   icd_fid_ingest         FID: resize + crop to uint8 (the bytes ToTensor sees), then bilinear to R x R and 2 u / 255 - 1, fp16 x 8
//   icd_vae_ingest         VAE encoder: both axes stretched to S x S, u / 127.5 - 1, NHWC fp16 padded to 8 channels (+ the resized bytes)
//   icd_vae_ingest_f32     fp32-fidelity VAE encoder (SDXL): the same resize, 2 (u / 255) - 1 in fp32, split3 [hi | lo | hi] of 8 channels
// All five share resample_h (the argument checks, the tables' descriptor, the horizontal pass); the vertical passes differ in what they
// store.  icd_image_to_u8 (truncating, SD1.5) and icd_image_to_u8_round (half to even, SDXL) are the way back: a decoded NCHW sample
// to uint8 NHWC.  Bandwidth kernels, 64-bit row offsets.
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

// The taps of output index i along one axis: the first input index, how many, their coefficients (table rows are k wide).  Clamped to
// the row of the table and to the n_in inputs there are: a wrong table cannot read outside the image.
struct Taps {
    int first, count;
    const int* coef;
};
__device__ __forceinline__ Taps taps_of(const int* first, const int* count, const int* coef, int k, int i, int n_in) {
    const int f = max(first[i], 0);
    return {f, min(count[i], min(k, n_in - f)), coef + (long long)i * k};
}

__device__ __forceinline__ float normalised(const PreK& p, int c, float u) { return (u / 255.0f - p.mean[c]) / p.stdv[c]; }

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
            const Taps t = taps_of(p.hfirst, p.hcount, p.hcoef, p.hk, x, p.W);
            int acc = 0;
            for (int k = 0; k < t.count; ++k) acc += t.coef[k] * (int)src[(t.first + k) * 3 + c];
            packed |= clip8(acc) << (8 * j);
        }
        *reinterpret_cast<unsigned*>(p.tmp + (r0 + row) * (long long)(p.S * 3) + wd * 4) = packed;
    }
}

// Vertical pass + crop + normalise + patch scatter.  One block owns one row of patches (P output rows): the resampled bytes go to LDS,
// then the G patch-matrix rows leave as 16-byte stores in column order (c * P + py) * P + px, pad columns zero.
__global__ __launch_bounds__(256) void clip_resample_v_kernel(PreK p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];      // [P, S * 3]
    const int b = blockIdx.x / p.G, pr = blockIdx.x - b * p.G;
    const int rowb = p.S * 3, wpr = rowb / 4;
    const unsigned char* src = p.tmp + (long long)b * p.H * rowb;
    for (int it = threadIdx.x; it < p.P * wpr; it += blockDim.x) {
        const int yy = it / wpr, wd = it - yy * wpr;
        const Taps t = taps_of(p.vfirst, p.vcount, p.vcoef, p.vk, pr * p.P + yy, p.H);
        const unsigned char* col = src + (long long)t.first * rowb + wd * 4;
        unsigned packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                          // four neighbouring bytes of each tap row: one 4-byte segment per lane
            int acc = 0;
            for (int k = 0; k < t.count; ++k) acc += t.coef[k] * (int)col[(long long)k * rowb + j];
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
                f = normalised(p, c, (float)lds[py * rowb + (px_blk * p.P + px) * 3 + c]);
            }
            v[j] = (half_t)f;
        }
        *reinterpret_cast<f16x8*>(out + (long long)px_blk * p.ldo + c8) = v;
    }
}

// What the per-pixel vertical pass does with the three resampled bytes of pixel `it`.
struct StoreNormalised {                       // one 16-byte store: channels 0 .. 2 normalised, 3 .. 7 zero (a first convolution's Cin = 8)
    __device__ void operator()(const PreK& p, long long it, const unsigned (&u)[3]) const {
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (half_t)normalised(p, c, (float)u[c]);
        *reinterpret_cast<f16x8*>(p.out + it * 8) = v;
    }
};
struct StoreBytes {                            // the uint8 [B, S, S, 3] intermediate: the bytes ToTensor would see
    unsigned char* mid;
    __device__ void operator()(const PreK&, long long it, const unsigned (&u)[3]) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) mid[it * 3 + c] = (unsigned char)u[c];
    }
};
struct StoreVae {                              // the VAE encoder's input: fp16(fp32(u) / 127.5f - 1.0f) as torch evaluates `arr.float() / 127.5 - 1`
    unsigned char* bytes;                      // and .to(float16): a division, a subtraction, one rounding to fp16; channels 3 .. 7 zero.
    __device__ void operator()(const PreK& p, long long it, const unsigned (&u)[3]) const {      // bytes (or null): the resized image itself
#pragma clang fp contract(off)
        f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float q = (float)u[c] / 127.5f;
            v[c] = (half_t)(q - 1.0f);
        }
        *reinterpret_cast<f16x8*>(p.out + it * 8) = v;
        if (bytes) StoreBytes{bytes}(p, it, u);
    }
};

struct StoreVaeF32 {                           // the fp32-fidelity encoder's first operand: v = 2.0f * (fp32(u) / 255.0f) - 1.0f as diffusers'
    unsigned char* bytes;                      // VaeImageProcessor.preprocess evaluates it (a division, a doubling, a subtraction), then the
    __device__ void operator()(const PreK& p, long long it, const unsigned (&u)[3]) const {      // split of split_cast_kernel at scale 1:
#pragma clang fp contract(off)
        f16x8 hi = {0, 0, 0, 0, 0, 0, 0, 0}, lo = {0, 0, 0, 0, 0, 0, 0, 0};                       // hi = fp16(v), lo = fp16(v - hi); three
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                                            // 16-byte stores [hi | lo | hi], pads zero
            const float q = (float)u[c] / 255.0f;
            const float v = 2.0f * q - 1.0f;
            hi[c] = (half_t)v;
            lo[c] = (half_t)(v - (float)hi[c]);
        }
        f16x8* o = reinterpret_cast<f16x8*>(p.out + it * 24);
        o[0] = hi; o[1] = lo; o[2] = hi;
        if (bytes) StoreBytes{bytes}(p, it, u);
    }
};

// Vertical pass, no patches: one thread owns one output pixel, three byte columns of the horizontal pass's rows.
template <typename Store>
__global__ __launch_bounds__(256) void resample_v_pixel_kernel(PreK p, Store store) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long SS = (long long)p.S * p.S;
    if (it >= p.B * SS) return;
    const long long b = it / SS;
    const int rem = (int)(it - b * SS), y = rem / p.S, x = rem - y * p.S;
    const int rowb = p.S * 3;
    const Taps t = taps_of(p.vfirst, p.vcount, p.vcoef, p.vk, y, p.H);
    const unsigned char* col = p.tmp + (b * p.H + t.first) * (long long)rowb + x * 3;
    int acc[3] = {0, 0, 0};
    for (int k = 0; k < t.count; ++k) {
        const int w = t.coef[k];
        const unsigned char* s = col + (long long)k * rowb;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += w * (int)s[c];
    }
    const unsigned u[3] = {clip8(acc[0]), clip8(acc[1]), clip8(acc[2])};
    store(p, it, u);
}

// F.interpolate(u / 255, (R, R), mode='bilinear', align_corners=False), then 2 v - 1: one thread owns one output pixel, one 16-byte
// store (channels 3 .. 7 zero: the Cin = 8 layout of the first convolution).  The roundings are spelled out (no contraction but the
// fmaf written here): source index fma(scale, i + 0.5, -0.5), rows fma(1 - lx, p0, lx p1), columns likewise - what torch's CPU kernel
// evaluates, so the fp32 value is the same; near 2 v - 1 = 0 one fp32 ulp of v is worth several fp16 ulps of the result.
__global__ __launch_bounds__(256) void fid_bilinear_kernel(const unsigned char* mid, long long B, int S, int R, half_t* out) {
#pragma clang fp contract(off)
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long RR = (long long)R * R;
    if (it >= B * RR) return;
    const long long b = it / RR;
    const int rem = (int)(it - b * RR), y = rem / R, x = rem - y * R;
    const float scale = (float)S / (float)R;
    const float sy = fmaxf(fmaf(scale, (float)y + 0.5f, -0.5f), 0.f), sx = fmaxf(fmaf(scale, (float)x + 0.5f, -0.5f), 0.f);
    const int y0 = min((int)sy, S - 1), x0 = min((int)sx, S - 1);
    const int y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const unsigned char* img = mid + b * S * S * 3;
    const unsigned char *p00 = img + ((long long)y0 * S + x0) * 3, *p01 = img + ((long long)y0 * S + x1) * 3;
    const unsigned char *p10 = img + ((long long)y1 * S + x0) * 3, *p11 = img + ((long long)y1 * S + x1) * 3;
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (float)p00[c] / 255.0f, bq = (float)p01[c] / 255.0f, cq = (float)p10[c] / 255.0f, d = (float)p11[c] / 255.0f;
        const float top = fmaf(1.f - lx, a, lx * bq), bot = fmaf(1.f - lx, cq, lx * d);
        const float u = fmaf(1.f - ly, top, ly * bot);
        v[c] = (half_t)(2.0f * u - 1.0f);
    }
    *reinterpret_cast<f16x8*>(out + it * 8) = v;
}

// `(image / 2 + 0.5).clamp(0, 1) * 255` and the cast to uint8 as torch evaluates them on a tensor of type T: every step in fp32, rounded to
// T before the next one (for T = float the roundings are the fp32 ones).  +-inf clamp; NaN is outside the contract.
template <typename T>
__device__ __forceinline__ unsigned sample_to_u8(T x) {
#pragma clang fp contract(off)
    T v = (T)((float)x * 0.5f);
    v = (T)((float)v + 0.5f);
    v = v < (T)0.f ? (T)0.f : (v > (T)1.f ? (T)1.f : v);
    v = (T)((float)v * 255.0f);
    return (unsigned)(int)(float)v;            // [0, 255]: truncation towards zero
}

// diffusers' VaeImageProcessor.postprocess: `(image / 2 + 0.5).clamp(0, 1)` in T as above, then `.float().numpy() * 255` - ONE fp32
// product, not rounded to T - and `.round().astype("uint8")`: to nearest, ties to even.
template <typename T>
__device__ __forceinline__ unsigned sample_to_u8_round(T x) {
#pragma clang fp contract(off)
    T v = (T)((float)x * 0.5f);
    v = (T)((float)v + 0.5f);
    v = v < (T)0.f ? (T)0.f : (v > (T)1.f ? (T)1.f : v);
    return (unsigned)(int)rintf((float)v * 255.0f);
}

// Decoded sample NCHW [B, 3, HW] -> uint8 NHWC [B, HW, 3].  One thread owns four consecutive pixels of the flattened batch (they may
// straddle two samples when HW % 4 != 0) and stores their 12 bytes as three dwords; the last thread of an odd batch stores bytes.
template <typename T, bool ROUND>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const T* x, long long npix, long long HW, unsigned char* out) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= npix) return;
    const int n = (int)min(4LL, npix - p0);
    unsigned char u[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long px = min(p0 + j, npix - 1), b = px / HW;
        const T* s = x + b * 2 * HW + px;                      // b * 3 HW + (px - b HW)
#pragma unroll
        for (int c = 0; c < 3; ++c) u[j * 3 + c] = (unsigned char)(ROUND ? sample_to_u8_round(s[c * HW]) : sample_to_u8(s[c * HW]));
    }
    if (n == 4) {
        unsigned* o = reinterpret_cast<unsigned*>(out + p0 * 3);
#pragma unroll
        for (int w = 0; w < 3; ++w) o[w] = u[4 * w] | (u[4 * w + 1] << 8) | (u[4 * w + 2] << 16) | ((unsigned)u[4 * w + 3] << 24);
    } else {
        for (int i = 0; i < n * 3; ++i) out[p0 * 3 + i] = u[i];
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host side
// One axis of a resample: its tables (rows `taps` wide), the image's extent, the extent it is resized to, where the crop starts in that.
struct Axis {
    const int32_t *first, *count, *coef;
    int taps, in, resized, off;
};

// The row length of Pillow's tables follows from the sizes: a table built for other sizes, or for another filter, is refused.
inline int pillow_taps(double support, int in, int out) {
    const double s = (double)in / out;
    return 2 * (int)ceil(support * (s > 1.0 ? s : 1.0)) + 1;
}

// What the three entry points share, for the exported function `fn` and a filter of `support` (2.0 BICUBIC, 3.0 LANCZOS): the checks
// that are not the caller's own, in the order the callers had them; the descriptor `p` (tables offset to the crop, which the rectangle
// check keeps inside them); the horizontal pass.  P * S * 3 bytes are the LDS of a patch row in clip_resample_v_kernel (P = 1 without
// patches), vblocks the grid of the caller's vertical pass.
int resample_h(const char* fn, double support, const void* images, int B, const Axis& h, const Axis& v, int S, int P, int ldo,
               const float* mean, const float* stdv, void* tmp, void* out, long long vblocks, hipStream_t st, PreK& p) {
    const int W = h.in, H = v.in;
    ICD_CHECK_ARG(W <= 4096, "%s: image width %d exceeds 4096", fn, W);
    ICD_CHECK_ARG(v.off >= 0 && h.off >= 0 && v.off + S <= v.resized && h.off + S <= h.resized,
                  "%s: the crop of %d at (%d, %d) does not lie inside the resized image (%d x %d)", fn, S, v.off, h.off, v.resized, h.resized);
    ICD_CHECK_ARG(((uintptr_t)tmp & 3) == 0 && ((uintptr_t)out & 15) == 0, "%s: tmp must be 4-byte aligned, out 16-byte aligned", fn);
    ICD_CHECK_ARG((long long)P * S * 3 <= 65536, "%s: patch * crop * 3 = %lld bytes of LDS exceed 64 KiB", fn, (long long)P * S * 3);
    const int ht = pillow_taps(support, W, h.resized), vt = pillow_taps(support, H, v.resized);
    ICD_CHECK_ARG(h.taps == ht && v.taps == vt, "%s: tables do not match the sizes (taps %d / %d, expected %d / %d)", fn, h.taps, v.taps, ht, vt);
    for (int c = 0; c < 3; ++c) ICD_CHECK_ARG(stdv[c] > 0.f, "%s: std must be positive", fn);
    p.rows = (long long)B * H;
    const long long hblocks = (p.rows + HROWS - 1) / HROWS;
    ICD_CHECK_ARG(vblocks <= 0x7fffffffLL && hblocks <= 0x7fffffffLL, "%s: the batch exceeds the grid limit", fn);
    p.img = (const unsigned char*)images; p.tmp = (unsigned char*)tmp; p.out = (half_t*)out;
    p.hfirst = h.first + h.off; p.hcount = h.count + h.off; p.hcoef = h.coef + (long long)h.off * h.taps;
    p.vfirst = v.first + v.off; p.vcount = v.count + v.off; p.vcoef = v.coef + (long long)v.off * v.taps;
    p.B = B; p.H = H; p.W = W; p.S = S; p.P = P; p.G = S / P; p.ldo = ldo; p.hk = h.taps; p.vk = v.taps;
    for (int c = 0; c < 3; ++c) { p.mean[c] = mean[c]; p.stdv[c] = stdv[c]; }
    hipLaunchKernelGGL(clip_resample_h_kernel, dim3((unsigned)hblocks), dim3(256), (size_t)HROWS * W * 3 + 32, st, p);
    char what[96];
    snprintf(what, sizeof(what), "%s (horizontal)", fn);
    ICD_CHECK_LAUNCH(what);
    return ICD_OK;
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
    hipStream_t st = (hipStream_t)stream;
    const int G = crop / patch;
    PreK p;
    const int rc = resample_h("icd_clip_preprocess", 2.0, images, B, Axis{h_first, h_count, h_coef, h_taps, W, resized_w, (resized_w - crop) / 2},
                              Axis{v_first, v_count, v_coef, v_taps, H, resized_h, (resized_h - crop) / 2}, crop, patch, ldo, mean, stdv, tmp, out,
                              (long long)B * G, st, p);
    if (rc != ICD_OK) return rc;
    hipLaunchKernelGGL(clip_resample_v_kernel, dim3((unsigned)(B * G)), dim3(256), (size_t)patch * crop * 3, st, p);
    ICD_CHECK_LAUNCH("icd_clip_preprocess (vertical)");
    return ICD_OK;
}

extern "C" int icd_image_resize_norm(const void* images, int32_t B, int32_t H, int32_t W, int32_t S, const int32_t* h_first,
                                     const int32_t* h_count, const int32_t* h_coef, int32_t h_taps, const int32_t* v_first,
                                     const int32_t* v_count, const int32_t* v_coef, int32_t v_taps, const float* mean, const float* stdv,
                                     void* tmp, void* out, void* stream) {
    ICD_CHECK_ARG(images && tmp && out && mean && stdv, "icd_image_resize_norm: null pointer");
    ICD_CHECK_ARG(h_first && h_count && h_coef && v_first && v_count && v_coef, "icd_image_resize_norm: null coefficient table");
    ICD_CHECK_ARG(B > 0, "icd_image_resize_norm: B must be positive (got %d)", B);
    ICD_CHECK_ARG(H > 0 && W > 0, "icd_image_resize_norm: image sizes must be positive (got %d x %d)", H, W);
    ICD_CHECK_ARG(S > 0 && S % 4 == 0 && S <= 4096, "icd_image_resize_norm: S must be a positive multiple of 4, <= 4096 (got %d)", S);
    hipStream_t st = (hipStream_t)stream;
    const long long vblocks = ((long long)B * S * S + 255) / 256;
    PreK p;
    const int rc = resample_h("icd_image_resize_norm", 2.0, images, B, Axis{h_first, h_count, h_coef, h_taps, W, S, 0},
                              Axis{v_first, v_count, v_coef, v_taps, H, S, 0}, S, 1, 8, mean, stdv, tmp, out, vblocks, st, p);
    if (rc != ICD_OK) return rc;
    hipLaunchKernelGGL(resample_v_pixel_kernel<StoreNormalised>, dim3((unsigned)vblocks), dim3(256), 0, st, p, StoreNormalised{});
    ICD_CHECK_LAUNCH("icd_image_resize_norm (vertical)");
    return ICD_OK;
}

extern "C" int icd_fid_ingest(const void* images, int32_t B, int32_t H, int32_t W, int32_t resized_h, int32_t resized_w, int32_t top, int32_t left,
                              int32_t S, int32_t R, const int32_t* h_first, const int32_t* h_count, const int32_t* h_coef, int32_t h_taps, const int32_t* v_first,
                              const int32_t* v_count, const int32_t* v_coef, int32_t v_taps, void* tmp, void* mid, void* out, void* stream) {
    ICD_CHECK_ARG(images && out, "icd_fid_ingest: null pointer");
    ICD_CHECK_ARG(B > 0, "icd_fid_ingest: B must be positive (got %d)", B);
    ICD_CHECK_ARG(H > 0 && W > 0 && S > 0 && R > 0 && S <= 4096 && R <= 4096, "icd_fid_ingest: sizes must be positive, S and R at most 4096");
    ICD_CHECK_ARG(((uintptr_t)out & 15) == 0, "icd_fid_ingest: out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long opix = (long long)B * R * R;
    ICD_CHECK_ARG((opix + 255) / 256 <= 0x7fffffffLL, "icd_fid_ingest: the batch exceeds the grid limit");
    const unsigned char* src = (const unsigned char*)images;
    if (h_first || v_first) {
        ICD_CHECK_ARG(h_first && h_count && h_coef && v_first && v_count && v_coef, "icd_fid_ingest: null coefficient table");
        ICD_CHECK_ARG(tmp && mid, "icd_fid_ingest: the resize needs tmp and mid");
        ICD_CHECK_ARG(S % 4 == 0, "icd_fid_ingest: S must be a multiple of 4 (got %d)", S);
        const long long vblocks = ((long long)B * S * S + 255) / 256;
        const float mean[3] = {0.f, 0.f, 0.f}, stdv[3] = {1.f, 1.f, 1.f};       // the bytes leave as they are
        PreK p;
        const int rc = resample_h("icd_fid_ingest", 3.0, images, B, Axis{h_first, h_count, h_coef, h_taps, W, resized_w, left},
                                  Axis{v_first, v_count, v_coef, v_taps, H, resized_h, top}, S, 1, 8, mean, stdv, tmp, out, vblocks, st, p);
        if (rc != ICD_OK) return rc;
        hipLaunchKernelGGL(resample_v_pixel_kernel<StoreBytes>, dim3((unsigned)vblocks), dim3(256), 0, st, p, StoreBytes{(unsigned char*)mid});
        ICD_CHECK_LAUNCH("icd_fid_ingest (vertical)");
        src = (const unsigned char*)mid;
    } else {
        ICD_CHECK_ARG(H == S && W == S, "icd_fid_ingest: without tables the images must be S x S already (got %d x %d, S %d)", H, W, S);
    }
    hipLaunchKernelGGL(fid_bilinear_kernel, dim3((unsigned)((opix + 255) / 256)), dim3(256), 0, st, src, (long long)B, S, R, (half_t*)out);
    ICD_CHECK_LAUNCH("icd_fid_ingest (bilinear)");
    return ICD_OK;
}

extern "C" int icd_vae_ingest(const void* images, int32_t B, int32_t H, int32_t W, int32_t S, const int32_t* h_first, const int32_t* h_count,
                              const int32_t* h_coef, int32_t h_taps, const int32_t* v_first, const int32_t* v_count, const int32_t* v_coef,
                              int32_t v_taps, void* tmp, void* out, void* bytes, void* stream) {
    ICD_CHECK_ARG(images && tmp && out, "icd_vae_ingest: null pointer");
    ICD_CHECK_ARG(h_first && h_count && h_coef && v_first && v_count && v_coef, "icd_vae_ingest: null coefficient table");
    ICD_CHECK_ARG(B > 0, "icd_vae_ingest: B must be positive (got %d)", B);
    ICD_CHECK_ARG(H > 0 && W > 0, "icd_vae_ingest: image sizes must be positive (got %d x %d)", H, W);
    ICD_CHECK_ARG(S > 0 && S % 8 == 0 && S <= 4096, "icd_vae_ingest: S must be a positive multiple of 8, <= 4096 (got %d)", S);
    hipStream_t st = (hipStream_t)stream;
    const long long vblocks = ((long long)B * S * S + 255) / 256;
    const float mean[3] = {0.f, 0.f, 0.f}, stdv[3] = {1.f, 1.f, 1.f};           // unused: StoreVae spells its own arithmetic out
    PreK p;
    const int rc = resample_h("icd_vae_ingest", 2.0, images, B, Axis{h_first, h_count, h_coef, h_taps, W, S, 0},
                              Axis{v_first, v_count, v_coef, v_taps, H, S, 0}, S, 1, 8, mean, stdv, tmp, out, vblocks, st, p);
    if (rc != ICD_OK) return rc;
    hipLaunchKernelGGL(resample_v_pixel_kernel<StoreVae>, dim3((unsigned)vblocks), dim3(256), 0, st, p, StoreVae{(unsigned char*)bytes});
    ICD_CHECK_LAUNCH("icd_vae_ingest (vertical)");
    return ICD_OK;
}

extern "C" int icd_vae_ingest_f32(const void* images, int32_t B, int32_t H, int32_t W, int32_t S, const int32_t* h_first, const int32_t* h_count,
                                  const int32_t* h_coef, int32_t h_taps, const int32_t* v_first, const int32_t* v_count, const int32_t* v_coef,
                                  int32_t v_taps, void* tmp, void* out, void* bytes, void* stream) {
    ICD_CHECK_ARG(images && tmp && out, "icd_vae_ingest_f32: null pointer");
    ICD_CHECK_ARG(h_first && h_count && h_coef && v_first && v_count && v_coef, "icd_vae_ingest_f32: null coefficient table");
    ICD_CHECK_ARG(B > 0, "icd_vae_ingest_f32: B must be positive (got %d)", B);
    ICD_CHECK_ARG(H > 0 && W > 0, "icd_vae_ingest_f32: image sizes must be positive (got %d x %d)", H, W);
    ICD_CHECK_ARG(S > 0 && S % 8 == 0 && S <= 4096, "icd_vae_ingest_f32: S must be a positive multiple of 8, <= 4096 (got %d)", S);
    hipStream_t st = (hipStream_t)stream;
    const long long vblocks = ((long long)B * S * S + 255) / 256;
    const float mean[3] = {0.f, 0.f, 0.f}, stdv[3] = {1.f, 1.f, 1.f};           // unused: StoreVaeF32 spells its own arithmetic out
    PreK p;
    const int rc = resample_h("icd_vae_ingest_f32", 2.0, images, B, Axis{h_first, h_count, h_coef, h_taps, W, S, 0},
                              Axis{v_first, v_count, v_coef, v_taps, H, S, 0}, S, 1, 24, mean, stdv, tmp, out, vblocks, st, p);
    if (rc != ICD_OK) return rc;
    hipLaunchKernelGGL(resample_v_pixel_kernel<StoreVaeF32>, dim3((unsigned)vblocks), dim3(256), 0, st, p, StoreVaeF32{(unsigned char*)bytes});
    ICD_CHECK_LAUNCH("icd_vae_ingest_f32 (vertical)");
    return ICD_OK;
}

namespace {
// What the two output entries share, for the exported function `fn`: the checks and the launch of image_to_u8_kernel<T, ROUND>.
template <bool ROUND>
int image_to_u8(const char* fn, const void* x, int32_t is_f32, int32_t B, int32_t H, int32_t W, void* out, void* stream) {
    ICD_CHECK_ARG(x && out, "%s: null pointer", fn);
    ICD_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B, H, W must be positive (got %d, %d, %d)", fn, B, H, W);
    ICD_CHECK_ARG(((uintptr_t)x & (is_f32 ? 3 : 1)) == 0 && ((uintptr_t)out & 3) == 0,
                  "%s: x must be aligned to its element, out 4-byte aligned", fn);
    const long long HW = (long long)H * W, npix = (long long)B * HW;
    const long long blocks = ((npix + 3) / 4 + 255) / 256;
    ICD_CHECK_ARG(blocks <= 0x7fffffffLL, "%s: the batch exceeds the grid limit", fn);
    hipStream_t st = (hipStream_t)stream;
    if (is_f32) hipLaunchKernelGGL((image_to_u8_kernel<float, ROUND>), dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, npix, HW, (unsigned char*)out);
    else hipLaunchKernelGGL((image_to_u8_kernel<half_t, ROUND>), dim3((unsigned)blocks), dim3(256), 0, st, (const half_t*)x, npix, HW, (unsigned char*)out);
    ICD_CHECK_LAUNCH(fn);
    return ICD_OK;
}
}  // namespace

extern "C" int icd_image_to_u8(const void* x, int32_t is_f32, int32_t B, int32_t H, int32_t W, void* out, void* stream) {
    return image_to_u8<false>("icd_image_to_u8", x, is_f32, B, H, W, out, stream);
}

extern "C" int icd_image_to_u8_round(const void* x, int32_t is_f32, int32_t B, int32_t H, int32_t W, void* out, void* stream) {
    return image_to_u8<true>("icd_image_to_u8_round", x, is_f32, B, H, W, out, stream);
}
