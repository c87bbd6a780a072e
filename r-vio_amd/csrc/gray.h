// gray.h — "Convert to gray scale" at the head of Tracker::track (Tracker.cc:182-196): cv::cvtColor with CV_RGB2GRAY / CV_BGR2GRAY (three
// channels) or CV_RGBA2GRAY / CV_BGRA2GRAY (four), chosen by Camera.RGB.  OpenCV's 8-bit path is fixed point (imgproc color_yuv: R2Y = 4899,
// G2Y = 9617, B2Y = 1868, yuv_shift = 14, rounded): Y = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14 — the coefficients sum to 1 << 14, so
// Y <= 255 without a clamp.  Alpha is ignored; the channel order only says which byte of a pixel is R and which is B.
//
// The per-pixel arithmetic of gray_kernel / gray_kernel4 (gray.hip) lives here so that the very same code can be compiled with g++
// (tests/test_gray_arith.py walks all 2^24 (R, G, B) triples through both forms on the CPU, before any GPU sees it).
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#define GRAY_FN __host__ __device__ __forceinline__
#else
#define GRAY_FN static inline
#endif

#define GRAY_R2Y 4899u
#define GRAY_G2Y 9617u
#define GRAY_B2Y 1868u

// Weights of the first and third byte of a pixel in memory order; bgr != 0: the first byte is B (Camera.RGB: 0).  The channel order only
// swaps two weights of an integer sum, so a kernel selects them once per launch and its per-pixel code has no branch.
struct GrayW { uint32_t k0, k2; };
GRAY_FN GrayW gray_weights(int bgr) { GrayW w; w.k0 = bgr ? GRAY_B2Y : GRAY_R2Y; w.k2 = bgr ? GRAY_R2Y : GRAY_B2Y; return w; }

// one pixel whose first three bytes are c0 c1 c2 in memory order
GRAY_FN uint32_t gray_px(uint32_t c0, uint32_t c1, uint32_t c2, GrayW w) { return (c0 * w.k0 + c1 * GRAY_G2Y + c2 * w.k2 + 8192u) >> 14; }

GRAY_FN uint32_t gray_byte(const uint32_t* v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 255u; }

// four adjacent pixels as the CH dwords that hold them (little endian: byte i of the group is bits 8 (i % 4) .. of dword i / 4) -> four gray
// bytes packed the same way
template <int CH>
GRAY_FN uint32_t gray4(const uint32_t* v, GrayW w) {
    uint32_t out = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) out |= gray_px(gray_byte(v, CH * k), gray_byte(v, CH * k + 1), gray_byte(v, CH * k + 2), w) << (8 * k);
    return out;
}
