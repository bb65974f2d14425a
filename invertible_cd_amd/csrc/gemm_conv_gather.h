// gemm_conv_gather.h - the implicit-GEMM conv A gather of the big tiles: what a GEMM row and a k-tile mean in terms of source pixels.
// Used by gemm_big.hip.  gemm_pp.hip and gemm_pp320.hip carry the same code as copies of their own - a change here has to be made there
// too: through these helpers the conv kernels of gemm_pp320.hip spill more (profiles/r13_gemm_gather_isa.txt) and those of gemm_pp.hip
// ran 1 - 4 % slower on the M = 8192 layers (profiles/r13_gemm_gather_bench.txt).  gemm.hip's 128-wide kernel has its own pointer-based loader.
//
// The A operand comes through a BUFFER descriptor (buffer_load_dwordx4 ... offen lds) with 32-bit byte offsets.  Per 16-B chunk a lane
// keeps the source pixel of its row's tap (0, 0) (a_pix), the byte offset of that pixel's chunk in the source being read (a_off, redone
// by the kernel's set_source when the k loop crosses from the first concat source to the second) and the complement of a 9-bit
// tap-validity mask (a_nmsk: zero padding, rows past the limit).  Per k-tile the offset to issue is a_off + a wave-uniform tap / channel
// term, with bit 31 set where the tap is invalid - out of the descriptor's range (sources < 2 GiB on this path, checked on the host), so
// the DMA writes zeros: 3 VALU issues per chunk and k-tile (add, bfe, lshl_or), no zero-page pointer select, no per-tap recompute of
// (y, x, pixel).  That economy is what makes the CHUNK-major K order affordable (k-tile = chunk * taps + tap: the nine taps of a
// 64-channel chunk back to back, the nine uses of a [rows + halo] x 64-channel slab inside nine consecutive k-tiles: L2 hits instead of 9
// fabric reads per line; weights stay tap-major in memory).  The tap-major order it replaced was measured against it in
// profiles/r04_conv_korder.txt.
//
// Everything here is __forceinline__ and works on scalars: the kernels keep their own array shapes (indexed by unrolled constants only)
// and their own way of turning a position into loads.
#pragma once
#include "gemm_common.h"

namespace icd_gemm_detail {

// what conv_row needs of the geometry beyond GemmK's own fields (wave-uniform; a kernel builds it once, ahead of its loader loops)
struct ConvGeom {
    int ntaps, pad, Hu, Wu;                      // taps of the geometry (9 or 1), low-side zero padding, the (upsampled) input map
    __device__ __forceinline__ explicit ConvGeom(const GemmK& p)
        : ntaps(p.ksize * p.ksize), pad((p.flags & ICD_GEMM_PAD_HI) ? 0 : p.ksize >> 1), Hu(p.Hin << p.upsample), Wu(p.Win << p.upsample) {}
};

// GEMM row m (a row >= m_lim reads nothing) -> a_pix, the source pixel of its tap (0, 0), and a_nmsk: bits 0..8 = tap INVALID,
// bits 9 / 10 = row / column parity of the tap-(0, 0) position in the upsampled map.  The one place that knows the padding
// (ICD_GEMM_PAD_HI: bottom / right only), the stride and the nearest-2x upsampling of the loader.
__device__ __forceinline__ void conv_row(const GemmK& p, const ConvGeom& g, int m, int m_lim, int& a_pix, unsigned& a_nmsk) {
    a_pix = 0; a_nmsk = 0x1ff;
    if (m < m_lim) {
        const int hw = p.Hout * p.Wout;
        const int b = m / hw, rem = m - b * hw;
        const int y = rem / p.Wout, x = rem - y * p.Wout;
        const int yu0 = y * p.stride - g.pad, xu0 = x * p.stride - g.pad;
        unsigned nm = 0x1ff;
        for (int t = 0; t < g.ntaps; ++t) {
            const int dy = g.ntaps == 9 ? t / 3 : 0, dx = g.ntaps == 9 ? t - dy * 3 : 0;
            if ((unsigned)(yu0 + dy) < (unsigned)g.Hu && (unsigned)(xu0 + dx) < (unsigned)g.Wu) nm &= ~(1u << t);
        }
        if (p.upsample) nm |= ((unsigned)(yu0 & 1) << 9) | ((unsigned)(xu0 & 1) << 10);
        a_nmsk = nm;
        a_pix = b * p.Hin * p.Win + (yu0 >> p.upsample) * p.Win + (xu0 >> p.upsample);
    }
}

// a_off of a chunk: byte offset of logical 16-B chunk lc of pixel a_pix in a source of Cs channels (the body of a kernel's set_source)
__device__ __forceinline__ unsigned conv_src_off(int a_pix, int Cs, int lc) { return ((unsigned)a_pix * (unsigned)Cs + (unsigned)(lc * 8)) * 2u; }

// pixels addressable in a conv source (its descriptor covers src_px * channels * 2 bytes)
__device__ __forceinline__ unsigned conv_src_px(const GemmK& p) {
    const int nb = (p.M + p.Hout * p.Wout - 1) / (p.Hout * p.Wout);
    return (unsigned)nb * (unsigned)(p.Hin * p.Win);
}

// a k-tile of the conv, decoded (wave-uniform): its tap in the 3 x 3 geometry, the concat source it reads and where
struct ConvKTile {
    int t3, dy, dx;                              // tap of the 3 x 3 geometry, (0, 0) for a 1 x 1 conv
    bool first;                                  // reads the first concat source (p.a0, C0 channels), else the second (p.a1, C1)
    int Cs, cc;                                  // channels of that source, first channel of the 64-channel chunk inside it
    unsigned s_tap;                              // byte offset of (tap, chunk) from the tap-(0, 0) pixel's chunk (no upsample)
};

// position in the chunk-major K order, from the split's first k-tile on
struct ConvKPos {
    int u_tap, u_c;                              // iterated tap (0 .. ktaps - 1), first channel of the chunk in the concatenated input
    __device__ __forceinline__ void start(int kt_begin, int ktaps) { const int ch = kt_begin / ktaps; u_tap = kt_begin - ch * ktaps; u_c = ch * BK; }
    __device__ __forceinline__ int w_k(int Cin) const { return u_tap * Cin + u_c; }      // k of the tile in the (tap-major) weight rows
    __device__ __forceinline__ ConvKTile decode(const GemmK& p) const {
        ConvKTile k;
        k.t3 = (int)((p.tapmap >> (4 * u_tap)) & 15u);       // iterated tap -> tap of the 3 x 3 geometry (one 64-bit scalar shift)
        k.dy = (k.t3 * 11) >> 5; k.dx = k.t3 - k.dy * 3;
        k.first = u_c < p.C0;
        k.Cs = k.first ? p.C0 : p.C1; k.cc = k.first ? u_c : u_c - p.C0;
        k.s_tap = (unsigned)(((k.dy * p.Win + k.dx) * k.Cs + k.cc) * 2);
        return k;
    }
    __device__ __forceinline__ bool step(int ktaps) {        // to the next k-tile; true when that is the first tap of the next chunk
        if (++u_tap != ktaps) return false;
        u_tap = 0; u_c += BK;
        return true;
    }
};

// offset to issue for one chunk in k-tile k: bit 31 ("outside": the DMA writes zeros) where the row's tap is invalid.  With the
// upsampling in the loader the tap's source pixel depends on the parity of the row's position (a_nmsk bits 9 / 10).
__device__ __forceinline__ unsigned conv_chunk_off(const GemmK& p, const ConvKTile& k, unsigned a_off, unsigned a_nmsk) {
    unsigned off = a_off + k.s_tap;
    if (p.upsample) {
        const int doff = (int)((((a_nmsk >> 9) & 1) + k.dy) >> 1) * p.Win + (int)((((a_nmsk >> 10) & 1) + k.dx) >> 1);
        off = a_off + (unsigned)((doff * k.Cs + k.cc) * 2);
    }
    return off | (__builtin_amdgcn_ubfe(a_nmsk, (unsigned)k.t3, 1u) << 31);
}

}  // namespace icd_gemm_detail
