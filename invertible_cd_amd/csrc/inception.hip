// FID on the device (invertible_cd_amd/inception.py, metrics.calculate_fid): what the FID Inception-v3 needs and nothing else here does.
//   icd_conv2d          implicit-GEMM convolution over NHWC fp16 for any (kh, kw), stride 1 / 2, padding (ph, pw), on
//                       v_mfma_f32_16x16x32_f16; fp32 bias and ReLU in the epilogue; writes a column slice of a wider row (the concat)
//   icd_pool3x3         the three 3 x 3 poolings of the network, into a column slice as well
//   icd_global_avgpool  fp16 [B, HW, C] -> fp32 [B, C]
//   icd_moments_f64     streaming sum x and sum x x^T in float64
// 64-bit row offsets everywhere; no atomics: every sum has a fixed order and no result depends on a sample's position in the batch.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------- convolution
constexpr int BM = 128, BN = 64, BK = 32;      // block tile: 128 output pixels x 64 output channels, 32 of K per step

struct ConvP {
    const half_t* x;
    const half_t* w;
    const float* bias;
    half_t* out;                               // already at the slice's first column
    long long M;                               // B * Ho * Wo
    int ldx, H, W, Cin, N, K, kw, stride, ph, pw, Ho, Wo, relu, ldo;
};

// 256 threads = 4 waves.  K runs tap-major, channel-minor; Cin % 8 == 0, so a 16-byte chunk of K is 8 channels of ONE tap of one pixel: a
// chunk is either a plain 16-byte load or (tap outside the image, row past M, chunk past K) zeros - nothing outside the sample's own
// rows is ever addressed.  Thread t owns K-chunk t & 3 of rows t >> 2 and 64 + (t >> 2) of the activation tile and of row t >> 2 of the
// weight tile; the next step's chunks are fetched into registers while the MFMAs of this step run from LDS.  Wave v owns rows
// 32 v .. 32 v + 31 of the tile and all 64 columns: 2 x 4 accumulators.  The weights are the MFMA's first operand, so an accumulator
// holds 4 consecutive output CHANNELS of one pixel per lane: one 8-byte store.  LDS rows are 64 bytes and unpadded on purpose: the 64
// lanes of a fragment read (16 rows x 4 chunks) and of a staging write (thread t at byte 16 t) each cover 1024 CONTIGUOUS bytes, which
// is the conflict-free pattern for 16-byte accesses; a padded row would only break it.  (Not yet here: icd_gemm's ping-pong schedule.)
__global__ __launch_bounds__(256) void conv2d_kernel(ConvP p) {
    __shared__ __attribute__((aligned(16))) half_t sA[BM * BK];
    __shared__ __attribute__((aligned(16))) half_t sB[BN * BK];
    const int tid = threadIdx.x, q = tid & 3, r = tid >> 2;
    const long long m0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    long long rowbase[2];                                       // b * H
    int yb[2], xb[2];
    bool live[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + r + 64 * i;
        live[i] = m < p.M;
        const long long mm = live[i] ? m : 0;
        const long long by = mm / p.Wo;
        const int xo = (int)(mm - by * p.Wo);
        const long long b = by / p.Ho;
        const int yo = (int)(by - b * p.Ho);
        rowbase[i] = b * p.H;
        yb[i] = yo * p.stride - p.ph;
        xb[i] = xo * p.stride - p.pw;
    }
    const bool wlive = n0 + r < p.N;
    const half_t* wrow = p.w + (long long)(wlive ? n0 + r : 0) * p.K;

    // this thread's chunk of the current K step: its offset in K, and the tap (ky, kx) and channel it falls on.  The walk advances by BK
    // per step with additions only (the divisions run once, here).
    int kc = q * 8;
    int ky, kx, c;
    {
        const int tap = kc / p.Cin;
        c = kc - tap * p.Cin;
        ky = tap / p.kw;
        kx = tap - ky * p.kw;
    }
    f16x8 ra[2], rb;
    auto fetch = [&]() {                                        // the chunk at kc into registers, then on to the next step's chunk
        ra[0] = ra[1] = rb = zero;
        if (kc < p.K) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int yi = yb[i] + ky, xi = xb[i] + kx;
                if (live[i] && yi >= 0 && yi < p.H && xi >= 0 && xi < p.W)
                    ra[i] = *reinterpret_cast<const f16x8*>(p.x + ((rowbase[i] + yi) * p.W + xi) * (long long)p.ldx + c);
            }
            if (wlive) rb = *reinterpret_cast<const f16x8*>(wrow + kc);
        }
        kc += BK;
        c += BK;
        while (c >= p.Cin) {
            c -= p.Cin;
            if (++kx == p.kw) { kx = 0; ++ky; }
        }
    };

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wv = tid >> 6, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
    fetch();
    for (int k0 = 0; k0 < p.K; k0 += BK) {
        *reinterpret_cast<f16x8*>(sA + r * BK + q * 8) = ra[0];
        *reinterpret_cast<f16x8*>(sA + (r + 64) * BK + q * 8) = ra[1];
        *reinterpret_cast<f16x8*>(sB + r * BK + q * 8) = rb;
        __syncthreads();
        if (k0 + BK < p.K) fetch();
        f16x8 fa[2], fb[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f16x8*>(sA + (wv * 32 + i * 16 + lr) * BK + lq * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const f16x8*>(sB + (j * 16 + lr) * BK + lq * 8);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        __syncthreads();
    }

    // accumulator (i, j): pixel m0 + 32 wv + 16 i + lr, channels n0 + 16 j + 4 lq .. + 3
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + wv * 32 + i * 16 + lr;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + j * 16 + lq * 4;
            if (n >= p.N) continue;                             // N % 8 == 0: a group of 4 is inside or outside as a whole
            f32x4 v = acc[i][j];
            if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + n);
            f16x4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) h[e] = (half_t)(p.relu ? fmaxf(v[e], 0.f) : v[e]);
            *reinterpret_cast<f16x4*>(p.out + m * p.ldo + n) = h;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ pooling
// One thread owns 8 channels of one output pixel.  mode 0: max, stride 2, no padding (floor); 1: max, stride 1, padding 1 (a tap
// outside the image never wins); 2: average, stride 1, padding 1, over the taps inside the image (count_include_pad = False).
__global__ __launch_bounds__(256) void pool3x3_kernel(const half_t* x, int ldx, long long total, int H, int W, int Ho, int Wo, int vpr,
                                                      int mode, half_t* out, int ldo) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= total) return;
    const long long pix = it / vpr;
    const int c8 = (int)(it - pix * vpr) * 8;
    const long long by = pix / Wo;
    const int xo = (int)(pix - by * Wo);
    const long long b = by / Ho;
    const int yo = (int)(by - b * Ho);
    const int s = mode == 0 ? 2 : 1, pad = mode == 0 ? 0 : 1;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = mode == 2 ? 0.f : -INFINITY;
    int cnt = 0;
    for (int dy = 0; dy < 3; ++dy) {
        const int yi = yo * s - pad + dy;
        if (yi < 0 || yi >= H) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int xi = xo * s - pad + dx;
            if (xi < 0 || xi >= W) continue;
            const f16x8 v = *reinterpret_cast<const f16x8*>(x + ((b * H + yi) * W + xi) * (long long)ldx + c8);
            ++cnt;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = mode == 2 ? acc[j] + (float)v[j] : fmaxf(acc[j], (float)v[j]);
        }
    }
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)(mode == 2 ? acc[j] / (float)cnt : acc[j]);
    *reinterpret_cast<f16x8*>(out + pix * ldo + c8) = o;
}

// One thread owns 8 channels of one sample and walks its pixels in index order; the sum is kept in double and rounded once.  That is
// B * C / 8 threads with a serial loop over HW: right for the network's 8 x 8 final map (64 steps, 0.5 MB per 2 samples), not a kernel
// for large maps.
__global__ __launch_bounds__(256) void global_avgpool_kernel(const half_t* x, long long total, int HW, int vpr, float* out) {
    const long long it = (long long)blockIdx.x * 256 + threadIdx.x;
    if (it >= total) return;
    const long long b = it / vpr;
    const int c8 = (int)(it - b * vpr) * 8;
    const long long C = (long long)vpr * 8;
    const half_t* src = x + b * HW * C + c8;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < HW; ++i) {
        const f16x8 v = *reinterpret_cast<const f16x8*>(src + i * C);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (double)(float)v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) out[b * C + c8 + j] = (float)(acc[j] / (double)HW);
}

// ------------------------------------------------------------------------------------------------------------------------ moments
// outer[a][b] += sum_i x[i][a] x[i][b] in double.  A thread owns a 4 x 4 patch of `outer`, starts from the value that is there and adds
// the rows in index order (the product of two floats is exact in double): two calls give the bits of one call on the concatenation.
__global__ __launch_bounds__(256) void moments_outer_kernel(const float* x, int n, int D, double* outer) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int a0 = (blockIdx.y * 16 + ty) * 4, b0 = (blockIdx.x * 16 + tx) * 4;
    if (a0 >= D || b0 >= D) return;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = outer[(long long)(a0 + r) * D + b0 + c];
    for (int i = 0; i < n; ++i) {
        const f32x4 xa = *reinterpret_cast<const f32x4*>(x + (long long)i * D + a0);
        const f32x4 xb = *reinterpret_cast<const f32x4*>(x + (long long)i * D + b0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] += (double)xa[r] * (double)xb[c];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) outer[(long long)(a0 + r) * D + b0 + c] = acc[r][c];
}

__global__ __launch_bounds__(256) void moments_sum_kernel(const float* x, int n, int D, double* sum) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double acc = sum[d];
    for (int i = 0; i < n; ++i) acc += (double)x[(long long)i * D + d];
    sum[d] = acc;
}

}  // namespace

extern "C" int icd_conv2d(const void* x, int32_t ldx, int32_t B, int32_t H, int32_t W, int32_t Cin, const void* w, const float* bias,
                          int32_t N, int32_t kh, int32_t kw, int32_t stride, int32_t ph, int32_t pw, int32_t relu, void* out, int32_t ldo,
                          int32_t col_off, void* stream) {
    ICD_CHECK_ARG(x && w && out, "icd_conv2d: null pointer");
    ICD_CHECK_ARG(B > 0 && H > 0 && W > 0, "icd_conv2d: B, H, W must be positive (got %d, %d, %d)", B, H, W);
    ICD_CHECK_ARG(Cin > 0 && Cin % 8 == 0, "icd_conv2d: Cin must be a positive multiple of 8 (got %d)", Cin);
    ICD_CHECK_ARG(N > 0 && N % 8 == 0, "icd_conv2d: N must be a positive multiple of 8 (got %d)", N);
    ICD_CHECK_ARG(kh >= 1 && kw >= 1 && kh <= 15 && kw <= 15, "icd_conv2d: kernel sizes must be in 1 .. 15 (got %d x %d)", kh, kw);
    ICD_CHECK_ARG(stride == 1 || stride == 2, "icd_conv2d: stride must be 1 or 2 (got %d)", stride);
    ICD_CHECK_ARG(ph >= 0 && pw >= 0 && ph < kh && pw < kw, "icd_conv2d: padding must be in 0 .. kernel size - 1 (got %d, %d)", ph, pw);
    ICD_CHECK_ARG(H + 2 * ph >= kh && W + 2 * pw >= kw, "icd_conv2d: the %d x %d kernel does not fit the padded %d x %d image", kh, kw, H, W);
    ICD_CHECK_ARG(ldx >= Cin && ldx % 8 == 0, "icd_conv2d: ldx must be a multiple of 8, >= Cin (got %d, Cin %d)", ldx, Cin);
    ICD_CHECK_ARG(col_off >= 0 && col_off % 8 == 0 && ldo % 8 == 0 && (long long)col_off + N <= ldo,
                  "icd_conv2d: ldo and col_off must be multiples of 8 with col_off + N <= ldo (got %d, %d, N %d)", ldo, col_off, N);
    ICD_CHECK_ARG(relu == 0 || relu == 1, "icd_conv2d: relu must be 0 or 1");
    ICD_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias) & 15) == 0, "icd_conv2d: pointers must be 16-byte aligned");
    const long long K = (long long)kh * kw * Cin;
    ICD_CHECK_ARG(K <= 0x7fffffffLL - BK, "icd_conv2d: K = %lld is too large", K);
    ConvP p;
    p.x = (const half_t*)x; p.w = (const half_t*)w; p.bias = bias; p.out = (half_t*)out + col_off;
    p.ldx = ldx; p.H = H; p.W = W; p.Cin = Cin; p.N = N; p.K = (int)K; p.kw = kw; p.stride = stride; p.ph = ph; p.pw = pw;
    p.Ho = (H + 2 * ph - kh) / stride + 1; p.Wo = (W + 2 * pw - kw) / stride + 1; p.relu = relu; p.ldo = ldo;
    p.M = (long long)B * p.Ho * p.Wo;
    const long long gm = (p.M + BM - 1) / BM;
    const int gn = (N + BN - 1) / BN;
    ICD_CHECK_ARG(gm <= 0x7fffffffLL && gn <= 65535, "icd_conv2d: %lld x %d blocks exceed the grid limit", gm, gn);
    hipLaunchKernelGGL(conv2d_kernel, dim3((unsigned)gm, (unsigned)gn), dim3(256), 0, (hipStream_t)stream, p);
    ICD_CHECK_LAUNCH("icd_conv2d");
    return ICD_OK;
}

extern "C" int icd_pool3x3(const void* x, int32_t ldx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mode, void* out, int32_t ldo,
                           int32_t col_off, void* stream) {
    ICD_CHECK_ARG(x && out, "icd_pool3x3: null pointer");
    ICD_CHECK_ARG(B > 0, "icd_pool3x3: B must be positive (got %d)", B);
    ICD_CHECK_ARG(mode >= 0 && mode <= 2, "icd_pool3x3: mode must be ICD_POOL_MAX_S2, ICD_POOL_MAX_S1P1 or ICD_POOL_AVG_S1P1 (got %d)", mode);
    ICD_CHECK_ARG(H >= (mode == 0 ? 3 : 1) && W >= (mode == 0 ? 3 : 1), "icd_pool3x3: the image %d x %d is too small for this mode", H, W);
    ICD_CHECK_ARG(C > 0 && C % 8 == 0, "icd_pool3x3: C must be a positive multiple of 8 (got %d)", C);
    ICD_CHECK_ARG(ldx >= C && ldx % 8 == 0, "icd_pool3x3: ldx must be a multiple of 8, >= C (got %d, C %d)", ldx, C);
    ICD_CHECK_ARG(col_off >= 0 && col_off % 8 == 0 && ldo % 8 == 0 && (long long)col_off + C <= ldo,
                  "icd_pool3x3: ldo and col_off must be multiples of 8 with col_off + C <= ldo (got %d, %d, C %d)", ldo, col_off, C);
    ICD_CHECK_ARG((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "icd_pool3x3: pointers must be 16-byte aligned");
    ICD_CHECK_ARG(x != out, "icd_pool3x3: in-place pooling is not supported");
    const int Ho = mode == 0 ? (H - 3) / 2 + 1 : H, Wo = mode == 0 ? (W - 3) / 2 + 1 : W, vpr = C / 8;
    const long long total = (long long)B * Ho * Wo * vpr, blocks = (total + 255) / 256;
    ICD_CHECK_ARG(blocks <= 0x7fffffffLL, "icd_pool3x3: %lld blocks exceed the grid limit", blocks);
    hipLaunchKernelGGL(pool3x3_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, ldx, total, H, W, Ho, Wo,
                       vpr, mode, (half_t*)out + col_off, ldo);
    ICD_CHECK_LAUNCH("icd_pool3x3");
    return ICD_OK;
}

extern "C" int icd_global_avgpool(const void* x, int32_t B, int32_t HW, int32_t C, float* out, void* stream) {
    ICD_CHECK_ARG(x && out, "icd_global_avgpool: null pointer");
    ICD_CHECK_ARG(B > 0 && HW > 0, "icd_global_avgpool: B and HW must be positive (got %d, %d)", B, HW);
    ICD_CHECK_ARG(C > 0 && C % 8 == 0, "icd_global_avgpool: C must be a positive multiple of 8 (got %d)", C);
    ICD_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0, "icd_global_avgpool: x must be 16-byte aligned, out 4-byte aligned");
    const int vpr = C / 8;
    const long long total = (long long)B * vpr, blocks = (total + 255) / 256;
    ICD_CHECK_ARG(blocks <= 0x7fffffffLL, "icd_global_avgpool: %lld blocks exceed the grid limit", blocks);
    hipLaunchKernelGGL(global_avgpool_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, total, HW, vpr, out);
    ICD_CHECK_LAUNCH("icd_global_avgpool");
    return ICD_OK;
}

extern "C" int icd_moments_f64(const float* x, int32_t n, int32_t D, double* sum, double* outer, void* stream) {
    ICD_CHECK_ARG(x && sum && outer, "icd_moments_f64: null pointer");
    ICD_CHECK_ARG(n > 0, "icd_moments_f64: n must be positive (got %d)", n);
    ICD_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 32768, "icd_moments_f64: D must be a positive multiple of 4, at most 32768 (got %d)", D);
    ICD_CHECK_ARG(((uintptr_t)x & 15) == 0 && (((uintptr_t)sum | (uintptr_t)outer) & 7) == 0,
                  "icd_moments_f64: x must be 16-byte aligned, sum and outer 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned g = (unsigned)((D / 4 + 15) / 16);
    hipLaunchKernelGGL(moments_sum_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, st, x, n, D, sum);
    ICD_CHECK_LAUNCH("icd_moments_f64 (sum)");
    hipLaunchKernelGGL(moments_outer_kernel, dim3(g, g), dim3(256), 0, st, x, n, D, outer);
    ICD_CHECK_LAUNCH("icd_moments_f64 (outer)");
    return ICD_OK;
}
