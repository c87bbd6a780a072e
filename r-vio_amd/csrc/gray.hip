// gray.hip — T(-1): the gray conversion in front of everything else Tracker::track does (Tracker.cc:182-196), for handles whose image
// format is a colour one (rvio_hip_set_image_format).  Pure HBM streaming: B interleaved images (3 or 4 bytes per pixel, row stride and
// instance stride in bytes) in, B packed W x H gray images out; the arithmetic is gray.h's.  Instance = blockIdx.z like every image kernel.
//
// Geometry of both forms: a WAVE owns 256 adjacent pixels of one row (workgroup = 4 rows), so "is this segment whole" and "is this row
// inside the image" are wave-uniform: the body of a whole segment has no per-lane predicate on its loads, the row tail is a branch of its own.
//   gray_kernel4  wide form: a lane converts four adjacent pixels — CH aligned dword loads (12 / 16 contiguous bytes per lane, the wave reads
//                 768 / 1024 contiguous bytes), all issued before the first use, one dword store.  Needs base, row stride, instance stride
//                 and W to be multiples of 4 (host-checked, like clahe_interp_kernel4).
//   gray_kernel   byte form for everything else (odd widths, a padded stride that is no multiple of 4): a lane converts the pixels
//                 lane + 64 j, j < 4 — 4 CH byte loads in flight, consecutive lanes on consecutive pixels, four byte stores.
#pragma once
#include "gray.h"

template <int CH>
__global__ __launch_bounds__(256) void gray_kernel4(const uint8_t* __restrict__ src, int w, int h, int stride, int bgr, uint8_t* __restrict__ dst,
                                                    size_t src_bs, size_t bs) {
    src = zoff(src, src_bs); dst = zoff(dst, bs);
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const int x0 = blockIdx.x * 256;
    const GrayW wt = gray_weights(bgr);
    const uint32_t* in = (const uint32_t*)(src + (size_t)y * stride) + (size_t)(x0 / 4 + lane) * CH;
    uint32_t* out = (uint32_t*)(dst + (size_t)y * w) + x0 / 4 + lane;
    uint32_t v[CH];
    if (x0 + 256 <= w) {
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = in[k];
        *out = gray4<CH>(v, wt);
    } else if (x0 + 4 * lane < w) {   // row tail (w % 4 == 0: whole groups of four)
#pragma unroll
        for (int k = 0; k < CH; ++k) v[k] = in[k];
        *out = gray4<CH>(v, wt);
    }
}

template <int CH>
__global__ __launch_bounds__(256) void gray_kernel(const uint8_t* __restrict__ src, int w, int h, int stride, int bgr, uint8_t* __restrict__ dst,
                                                   size_t src_bs, size_t bs) {
    src = zoff(src, src_bs); dst = zoff(dst, bs);
    const int lane = threadIdx.x & 63, y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= h) return;
    const int x0 = blockIdx.x * 256;
    const GrayW wt = gray_weights(bgr);
    const uint8_t* in = src + (size_t)y * stride + (size_t)(x0 + lane) * CH;
    uint8_t* out = dst + (size_t)y * w + x0 + lane;
    uint32_t c[4][3];
    if (x0 + 256 <= w) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) c[j][k] = in[64 * j * CH + k];
#pragma unroll
        for (int j = 0; j < 4; ++j) out[64 * j] = (uint8_t)gray_px(c[j][0], c[j][1], c[j][2], wt);
    } else {                          // row tail: loads of the lanes past the end go to the row's last pixel instead of being predicated, only the stores are
        const uint8_t* row = src + (size_t)y * stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + lane + 64 * j < w ? x0 + lane + 64 * j : w - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[j][k] = row[(size_t)x * CH + k];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) if (x0 + lane + 64 * j < w) out[64 * j] = (uint8_t)gray_px(c[j][0], c[j][1], c[j][2], wt);
    }
}
