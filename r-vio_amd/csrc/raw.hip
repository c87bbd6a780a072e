// raw.hip — T(-1) for raw sensor data: the gray conversion cv_bridge::toCvShare(msg, MONO8) runs in front of Tracker::track (rvio_mono.cc:64) for
// 16-bit samples (mono16, rgb16, bgr16, rgba16, bgra16) and Bayer mosaics (8 and 16 bit), for handles whose image format is one of them
// (rvio_hip_set_image_format).  HBM streaming like gray.hip, and the same geometry: a WAVE owns 256 adjacent pixels of one row, a workgroup four
// rows, "is this row inside the image" is wave-uniform, the instance is blockIdx.z.  No load is predicated: a lane past the row's end reads a
// clamped address inside the image and only its store is predicated.  The arithmetic is raw.h's.
//
// Per-pixel formats (16-bit samples, host byte order):
//   raw16_kernel4<CH>  wide form: a lane converts four adjacent pixels from the 2 CH aligned dwords that hold them (2 / 6 / 8 dwords, all issued
//                      before the first use), one dword store.  Needs base, row stride, instance stride and W to be multiples of 4.
//   raw16_kernel<CH>   plain form for everything else: a lane converts the pixels lane + 64 j, j < 4, with 16-bit loads (the ABI refuses an odd
//                      address or stride for a 16-bit format).
//
// Bayer mosaics (T = uint8_t | uint16_t): a 3 x 3 stencil with replicated borders.  Output (x, y) is the interior formula at
// (clamp(x, 1, W - 2), clamp(y, 1, H - 2)): at the first and last row the whole 3-row window moves (yc is wave-uniform), at the first and last
// column the output copies its neighbour.
//   bayer_kernel4<T>   wide form: a lane owns four adjacent pixels and loads their group (one or two aligned dwords) of the rows yc - 1, yc, yc + 1
//                      DIRECTLY — three row loads in flight per lane, 768 / 1536 contiguous bytes per wave.  The rows a wave shares with the waves
//                      above and below it (same workgroup: rows y - 1 .. y + 4 serve four outputs rows) and with the next workgroup are served by
//                      the CU's vector cache and L2; HBM delivers every row once.  The sample left and right of a lane's group comes from the
//                      neighbouring LANE (a cross-lane shift of the group's last / first sample, no LDS allocation, no barrier); the two samples
//                      outside the wave's segment come from one more unpredicated load per row in which the lower half-wave reads the sample left
//                      of the segment and the upper half the one right of it (two addresses per wave, clamped into the row).
//   bayer_kernel<T>    plain form (odd widths, a stride or base that is no multiple of 4): a lane computes the pixels lane + 64 j, each from
//                      nine loads at clamped addresses; consecutive lanes read consecutive samples and the cache absorbs the reuse.
#pragma once
#include "raw.h"

template <int CH>
__global__ __launch_bounds__(256) void raw16_kernel4(const uint8_t* __restrict__ src, int w, int h, int stride, int bgr, uint8_t* __restrict__ dst,
                                                     size_t src_bs, size_t bs) {
    src = zoff(src, src_bs); dst = zoff(dst, bs);
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const int x0 = blockIdx.x * 256;
    const GrayW wt = gray_weights(bgr);
    const int g = min(x0 / 4 + lane, w / 4 - 1);   // lanes past the row's end read its last group again
    const uint32_t* in = (const uint32_t*)(src + (size_t)y * stride) + (size_t)g * (2 * CH);
    uint32_t v[2 * CH];
#pragma unroll
    for (int k = 0; k < 2 * CH; ++k) v[k] = in[k];
    if (x0 + 4 * lane < w) ((uint32_t*)(dst + (size_t)y * w))[x0 / 4 + lane] = raw16_4<CH>(v, wt);
}

template <int CH>
__global__ __launch_bounds__(256) void raw16_kernel(const uint8_t* __restrict__ src, int w, int h, int stride, int bgr, uint8_t* __restrict__ dst,
                                                    size_t src_bs, size_t bs) {
    src = zoff(src, src_bs); dst = zoff(dst, bs);
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const int x0 = blockIdx.x * 256;
    const GrayW wt = gray_weights(bgr);
    const uint16_t* row = (const uint16_t*)(src + (size_t)y * stride);
    uint8_t* out = dst + (size_t)y * w + x0 + lane;
    constexpr int NS = CH == 1 ? 1 : 3;   // samples of a pixel that count (alpha is ignored)
    uint32_t c[4][NS];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = min(x0 + lane + 64 * j, w - 1);
#pragma unroll
        for (int k = 0; k < NS; ++k) c[j][k] = row[(size_t)x * CH + k];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x0 + lane + 64 * j < w) out[64 * j] = (uint8_t)(CH == 1 ? raw_depth8(c[j][0]) : raw16_px(c[j][0], c[j][NS > 1 ? 1 : 0], c[j][NS > 1 ? 2 : 0], wt));
}

template <typename T>
__global__ __launch_bounds__(256) void bayer_kernel4(const uint8_t* __restrict__ src, int w, int h, int stride, int pat, uint8_t* __restrict__ dst,
                                                     size_t src_bs, size_t bs) {
    constexpr int ND = sizeof(T);   // dwords that hold four samples
    src = zoff(src, src_bs); dst = zoff(dst, bs);
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;             // (wave-uniform: every lane of a wave takes part in the shifts below)
    const int x0 = blockIdx.x * 256;
    const BayerP bp = bayer_pattern(pat);
    const int yc = raw_clampi(y, 1, h - 2);
    const int g = min(x0 / 4 + lane, w / 4 - 1);
    const int xh = lane < 32 ? max(x0 - 1, 0) : min(x0 + 256, w - 1);   // the sample outside the segment: left for lane 0, right for lane 63
    uint32_t d[3][ND], e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint8_t* row = src + (size_t)(yc - 1 + r) * stride;
#pragma unroll
        for (int i = 0; i < ND; ++i) d[r][i] = ((const uint32_t*)row)[(size_t)g * ND + i];
        e[r] = ((const T*)row)[xh];
    }
    uint32_t s[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[r][k + 1] = ND == 1 ? gray_byte(d[r], k) : raw_half(d[r], k);
        const uint32_t up = __shfl_up(s[r][4], 1), dn = __shfl_down(s[r][1], 1);
        s[r][0] = lane == 0 ? e[r] : up;
        s[r][5] = lane == 63 ? e[r] : dn;
    }
    if (x0 + 4 * lane < w) ((uint32_t*)(dst + (size_t)y * w))[x0 / 4 + lane] = bayer4(s, x0 + 4 * lane, yc, w, bp, ND == 2);
}

template <typename T>
__global__ __launch_bounds__(256) void bayer_kernel(const uint8_t* __restrict__ src, int w, int h, int stride, int pat, uint8_t* __restrict__ dst,
                                                    size_t src_bs, size_t bs) {
    src = zoff(src, src_bs); dst = zoff(dst, bs);
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const int x0 = blockIdx.x * 256;
    const BayerP bp = bayer_pattern(pat);
    uint8_t* out = dst + (size_t)y * w + x0 + lane;
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bayer_at<T>((const T*)src, (size_t)stride / sizeof(T), w, h, min(x0 + lane + 64 * j, w - 1), y, bp);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (x0 + lane + 64 * j < w) out[64 * j] = (uint8_t)o[j];
}
